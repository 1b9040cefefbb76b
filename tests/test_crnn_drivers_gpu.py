"""The CRNN warm-up trainer and the evaluation drivers on the MI355X HIP path: a warm-up step against the fp64 oracle, the shapes
only these drivers reach (any validation batch, a document's strip count), the warm-up -> checkpoint -> area trainer / EvalCRNN
workflow, --graph against the eager loop, and EvalPrep against a direct loop over the same kernels."""
import os

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


def _crnn_args(tmp, *argv, **over):
    from train_crnn import build_parser
    a = build_parser().parse_args(["--crnn_model_path", str(tmp / "crnn" / "model"), *argv])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _oracle_crnn_grads(sc, x, labels, bn_training, dtype):
    from oracle import model_oracle as mo
    from oracle import step_oracle as so
    P, Bf = mo.split_state({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sc.items()})
    lp = mo.crnn_forward(P, Bf, x.to(dtype), bn_training=bn_training)
    y, ysz = H.encode(labels)
    loss = so.ctc_mean(lp, y, ysz)
    loss.backward()
    return {k: p.grad for k, p in P.items()}, lp.detach(), loss.item()


def _check_step_vs_oracle(crnn_grads, lp, loss, sc, x, labels):
    """The suite's rule (test_models_gpu.py::test_phase_b_vs_oracle): every gradient within max(1e-4, 3 x the conditioning of the
    problem) of the fp64 oracle, the conditioning being the fp32 oracle's deviation and the movement under a 4e-6 input perturbation."""
    g64, lp64, loss64 = _oracle_crnn_grads(sc, x, labels, True, torch.float64)
    g32, _, _ = _oracle_crnn_grads(sc, x, labels, True, torch.float32)
    xp = x * (1 + 4e-6 * torch.randn(x.shape, generator=torch.Generator().manual_seed(99)))
    gp, _, _ = _oracle_crnn_grads(sc, xp, labels, True, torch.float64)
    assert (lp.detach().cpu().double() - lp64).abs().max().item() < 2e-4
    assert abs(loss - loss64) < 1e-4 * abs(loss64)
    bad = {}
    for name, g in crnn_grads.items():
        r64 = g64[name].double()
        den = max(r64.norm().item(), 1e-300)
        dev = (g32[name].double() - r64).norm().item() / den
        cond = (gp[name].double() - r64).norm().item() / den
        err, _ = H.robust_rel_err(g, r64)
        if err > max(1e-4, 3 * max(dev, cond)):
            bad[name] = (err, dev, cond)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]


@pytest.mark.parametrize("B", [8, 17, 1])
def test_warmup_step_matches_the_oracle(tmp_path, B):
    """One TrainCRNN step (batch-statistic BatchNorm, CTC mean, backward with the NaN scrub) at the trainers' B = 8 and at odd B that
    only a warm-up reaches: loss, log-probs and every gradient against the fp64 oracle.  --std 0 without --random_std makes the
    jitter's sigma 1e-13, so the oracle may take the clean batch."""
    from datasets.synthetic import SyntheticTextAreas
    from oracle import model_oracle as mo
    from train_crnn import TrainCRNN
    x = H.synth_images(B, 40 + B)
    labels = H.synth_labels(B, 50 + B, 1, 10)
    sc = mo.seeded_state(mo.crnn_state_shapes(), 7)
    t = TrainCRNN(_crnn_args(tmp_path, "--std", "0", "--random_std"), train_set=SyntheticTextAreas(1), val_set=SyntheticTextAreas(1))
    assert t.device.type == "cuda" and type(t.model).__module__ == "models.model_crnn"
    t.model.load_state_dict(sc)
    t.model.train()
    seen = {}
    call = t._call_model
    t._call_model = lambda images, lab: seen.setdefault("out", call(images, lab))
    loss = t.train_step(x, labels)
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in t.model.named_parameters()}
    _check_step_vs_oracle(grads, seen["out"][0], loss.item(), sc, x, labels)


def _warmup(tmp_path):
    from train_crnn import TrainCRNN
    t = TrainCRNN(_crnn_args(tmp_path, "--synthetic_size", "256", "--epoch", "2", "--lr", "0.001"))
    losses = []
    step = t.train_step
    t.train_step = lambda images, labels: losses.append(step(images, labels).item()) or torch.tensor(losses[-1])
    best = t.train()
    return t, losses, best


def test_warmup_checkpoint_area_trainer_and_eval_crnn(tmp_path):
    """The README workflow on one GPU: a 2-epoch warm-up at B = 32 on synthetic strips lowers the training loss; its checkpoint loads
    through area_cli's --crnn_model and runs a trainer step; EvalCRNN of it on the validation strips reproduces the warm-up's final
    validation accuracy and CER exactly (same data, same eval-mode forward, same decode)."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_crnn import EvalCRNN
    from eval_crnn import build_parser as eval_parser
    from qea.cli_flags import build_parser
    from train_nn_area import TrainNNPrep
    t, losses, best = _warmup(tmp_path)
    assert len(losses) == 16 and all(l == l for l in losses)
    assert sum(losses[8:]) < sum(losses[:8]) and losses[-1] < losses[0]
    ckpt = "model_1_%.2f" % (t.last_val_accuracy * 100)
    assert ckpt in os.listdir(tmp_path / "crnn")
    # --crnn_model of the area trainer
    a = build_parser("a", "").parse_args(["--exp_base_path", str(tmp_path / "exp"), "--ocr", "stub", "--epoch", "1", "--batch_size", "8",
                                          "--inner_limit", "1", "--crnn_model", str(tmp_path / "crnn" / ckpt)])
    tr = TrainNNPrep(a, train_set=SyntheticTextAreas(8, seed=1, include_name=True, include_index=True),
                     val_set=SyntheticTextAreas(8, seed=2, include_name=True))
    assert type(tr.crnn_model).__name__ == "CRNN"
    for (k, v), (_, w) in zip(tr.crnn_model.state_dict().items(), t.model.state_dict().items()):
        assert torch.equal(v.cpu(), w.cpu()), k
    tr.train()
    c1 = torch.cat([p.detach().flatten() for p in tr.crnn_model.parameters()])
    c0 = torch.cat([p.detach().flatten() for p in t.model.parameters()])
    assert torch.isfinite(c1).all() and (c1 - c0).abs().max().item() > 0
    # EvalCRNN on the warm-up's validation strips
    ev = eval_parser().parse_args(["--crnn_path", str(tmp_path / "crnn"), "--crnn_model_name", ckpt, "--dataset", "vgg", "--batch_size", "32",
                                   "--ocr", "stub"])
    res = EvalCRNN(ev, dataset=t.loader_validation.dataset).eval()
    assert res["count"] == t.val_set_size and res["crnn_accuracy"] == t.last_val_accuracy and res["crnn_cer"] == t.last_val_cer


@pytest.mark.parametrize("B", [1, 3, 17, 33])
def test_eval_forward_and_decode_at_any_batch(B):
    """The validation loader keeps its last batch (no drop_last) and the pos flow's batch is a document's strip count: the eval-mode
    CRNN (one-launch BiLSTM, MFMA tiles) and the device decode at B in {1, 3, 17, 33} against the fp64 oracle — log-probs within the
    suite's 2e-4, decoded strings equal wherever the oracle's top-1 margin is not tiny."""
    from models.model_crnn import CRNN
    from oracle import model_oracle as mo
    from utils import pred_to_string
    sc = mo.seeded_state(mo.crnn_state_shapes(), 9)
    net = CRNN(95, False)
    net.load_state_dict(sc)
    net = net.cuda().eval()
    x = H.synth_images(B, 60 + B)
    with torch.no_grad():
        lp = net(x.cuda())
    P, Bf = mo.split_state({k: (v.double() if v.is_floating_point() else v) for k, v in sc.items()}, requires_grad=False)
    lp64 = mo.crnn_forward(P, Bf, x.double(), bn_training=False)
    assert lp.shape == (31, B, 95)
    assert (lp.cpu().double() - lp64).abs().max().item() < 2e-4
    got = pred_to_string(lp, [""] * B, H.I2C)
    ref = pred_to_string(lp64, [""] * B, H.I2C)
    top2 = lp64.topk(2, dim=2).values
    margin = (top2[..., 0] - top2[..., 1]).min(dim=0).values                     # [B]
    clear = [b for b in range(B) if margin[b] > 1e-3]
    assert len(clear) >= B // 2
    assert [got[b] for b in clear] == [ref[b] for b in clear]


def test_graph_warmup_equals_eager_and_relearns_the_lr(tmp_path, capsys):
    """--graph: the warm-up step as one hipGraph replay per (batch, width, target cap, lr).  Five steps at B = 32 (two eager, the
    capture, two replays) leave the same CRNN weights as the eager loop, bit for bit in the default split_f16 mode; a StepLR change
    between epochs records a second graph with the new lr instead of replaying the old one, and the weights still follow the eager run."""
    from train_crnn import TrainCRNN
    res = {}
    for flag in (False, True):
        args = _crnn_args(tmp_path / str(flag), "--synthetic_size", "160", "--epoch", "2", "--lr", "0.001", graph=flag)
        t = TrainCRNN(args)
        t.scheduler = torch.optim.lr_scheduler.StepLR(t.optimizer, step_size=1, gamma=0.5)
        snaps = []
        step = t.train_step

        def spy(images, labels, step=step, snaps=snaps, t=t):
            loss = step(images, labels)
            snaps.append(torch.cat([p.detach().flatten().clone() for p in t.model.parameters()]))
            return loss
        t.train_step = spy
        t.train()
        if flag:
            lrs = sorted({k[-1] for k in t.graphs.graphs})
            assert lrs == [0.0005, 0.001], t.graphs.graphs.keys()
        res[flag] = snaps
    assert len(res[True]) == len(res[False]) == 10
    d5 = (res[True][4] - res[False][4]).abs().max().item()
    d10 = (res[True][9] - res[False][9]).abs().max().item()
    with capsys.disabled():
        print(f"\n--graph vs eager after 5 steps: max |dw| = {d5:.3e} (bit-identical: {d5 == 0}); after 10 steps (lr halved at step 6): {d10:.3e}")
    from qea import ops
    if ops.mfma_mode() == "split_f16":                       # the default mode: the replay launches the eager step's kernels bit for bit
        assert d5 == 0 and d10 == 0
    assert d5 <= 5e-6 and d10 <= 1e-5                         # other modes (split_bf16's replay identity is flaky): Adam ulps


def _synthetic_docs(n):
    from datasets.synthetic import SyntheticPatches
    return SyntheticPatches(n, seed=5, strips=(3, 9))


def test_eval_prep_patch_and_area_flows_equal_a_direct_loop(tmp_path):
    """EvalPrep with --ocr stub: on synthetic patch_dataset documents its (accuracy, cer) equal a direct loop over the same HIP UNet
    outputs, device crops and the stub; the vgg area flow likewise, with --show_orig (the original strips' numbers divided once)."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_prep import EvalPrep, build_parser
    from models.model_unet import UNet
    from ocr_helper.stub_helper import StubHelper
    from oracle import model_oracle as mo
    from utils import compare_labels, get_text_stack
    prep = UNet()
    prep.load_state_dict(mo.seeded_state(mo.unet_state_shapes(), 13))
    prep = prep.cuda().eval()
    torch.save(prep, tmp_path / "prep")
    docs = _synthetic_docs(3)
    args = build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--ocr", "stub", "--show_orig"])
    acc, cer = EvalPrep(args, dataset=docs).eval()
    stub, n, c, e = StubHelper(), 0, 0, 0.0
    with torch.no_grad():
        for i in range(len(docs)):
            image, boxes, _ = docs[i]
            pred = prep(image[None].cuda())[0]
            crops, labels = get_text_stack(pred, boxes, (32, 128))
            ci, ei = compare_labels(stub.get_labels(crops.cpu()), labels)
            n, c, e = n + len(labels), c + ci, e + ei
    assert (acc, cer) == (c / n, e / n)
    strips = SyntheticTextAreas(37, seed=6)
    args = build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--ocr", "stub", "--show_orig", "--dataset", "vgg",
                                      "--batch_size", "16"])
    ev = EvalPrep(args, dataset=strips)
    acc, cer = ev.eval()
    c, e, oc, oe = 0, 0.0, 0, 0.0
    with torch.no_grad():
        for b0 in range(0, 37, 16):
            imgs = torch.stack([strips[i][0] for i in range(b0, min(37, b0 + 16))])
            labels = [strips[i][1] for i in range(b0, min(37, b0 + 16))]
            ci, ei = compare_labels(stub.get_labels(prep(imgs.cuda()).cpu()), labels)
            oci, oei = compare_labels(stub.get_labels(imgs), labels)
            c, e, oc, oe = c + ci, e + ei, oc + oci, oe + oei
    assert (acc, cer) == (c / 37, e / 37) and ev.orig_result == (oc / 37, oe / 37)


def test_eval_prep_names_an_oversized_document(tmp_path):
    """A document whose size is no multiple of 16 is refused by the UNet with its file named, not padded silently."""
    from eval_prep import EvalPrep, build_parser
    from models.model_unet import UNet
    torch.save(UNet().cuda(), tmp_path / "prep")
    img = torch.ones(1, 410, 512)
    docs = [(img, [dict(label="ab", x_min=0, y_min=0, x_max=40, y_max=20)], "odd/doc.png")]
    args = build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--ocr", "stub"])
    with pytest.raises(ValueError, match="odd/doc.png"):
        EvalPrep(args, dataset=docs).eval()
