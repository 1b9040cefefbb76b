"""The CRNN warm-up trainer (train_crnn.py) and the two evaluation drivers (eval_crnn.py, eval_prep.py) on CPU: their command-line
surfaces against the reference's (tests/golden/cli_reference_flags.json), and their host logic with the CPU oracle INJECTED as the
arithmetic backend — against a hand-written copy of the reference's loop (train_crnn.py:146-214)."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import helpers as H

torch.set_num_threads(4)


def oracle_backend():
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    return Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)


def _crnn_args(tmp, *argv, **over):
    from train_crnn import build_parser
    a = build_parser().parse_args(["--crnn_model_path", str(tmp / "crnn" / "model"), *argv])
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("script,tag", [("train_crnn", "c"), ("eval_crnn", "e"), ("eval_prep", "v")])
def test_cli_surfaces_match_the_reference(golden_dir, script, tag):
    from qea.cli_flags import build_parser
    ref = json.load(open(os.path.join(golden_dir, "cli_reference_flags.json")))[script]
    ap = build_parser(tag, "")
    args = vars(ap.parse_args([]))
    acts = {a.option_strings[0]: a for a in ap._actions if a.option_strings and a.option_strings[0] != "-h"}
    for f in ref:
        a = acts[f["flag"]]
        assert args[a.dest] == f["default"], f
        assert (a.type.__name__ if a.type else None) == f["type"], f
        if f["action"] == "store_false":
            assert a.const is False and a.default is True, f
        if f["action"] == "store_true":
            assert a.const is True and a.default is False, f
    extra = set(acts) - {f["flag"] for f in ref}
    assert all(acts[n].help.startswith("[new]") for n in extra), extra
    # the front ends parse through the same data
    mod = __import__(script)
    assert vars(mod.build_parser().parse_args([])) == args


def test_train_crnn_defaults():
    from qea.cli_flags import build_parser
    c = build_parser("c", "").parse_args([])
    assert c.random_std is True and c.start_epoch == -1 and c.ocr is None and c.dataset == "pos" and c.graph is False
    assert build_parser("c", "").parse_args(["--random_std"]).random_std is False
    # the trainers' surfaces are untouched by the new tags
    p, a = build_parser("p", "").parse_args([]), build_parser("a", "").parse_args([])
    assert p.start_epoch == 0 and a.start_epoch == 0 and p.ocr == "Tesseract" and not hasattr(a, "lr") and not hasattr(p, "ckpt_path")


class _Noisy(torch.utils.data.Dataset):
    """The reference's noisy_transform as a loader-side transform: AddGaussianNoice on every item as it is fetched."""

    def __init__(self, ds, noiser):
        self.ds, self.noiser = ds, noiser

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        item = self.ds[i]
        return (self.noiser(item[0]),) + tuple(item[1:])


def _reference_loop(train_set, val_set, batch_size, lr, epochs, seed, std):
    """train_crnn.py:25-214 written out on the CPU oracle: loader-side noise, torch CTC / Adam / StepLR."""
    from oracle.modules import OracleCRNN
    from transform_helper import AddGaussianNoice
    from utils import compare_labels, pred_to_string
    torch.manual_seed(seed)
    np.random.seed(torch.initial_seed())
    random.seed(torch.initial_seed())
    model = OracleCRNN(95, False)
    model.register_backward_hook(model.backward_hook)
    loader_train = torch.utils.data.DataLoader(_Noisy(train_set, AddGaussianNoice(std=std, is_stochastic=True)), batch_size=batch_size,
                                               drop_last=True, shuffle=True)
    loader_val = torch.utils.data.DataLoader(val_set, batch_size=batch_size)
    ctc = torch.nn.CTCLoss()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.8)
    losses, accs = [], []
    for _ in range(epochs):
        model.train()
        for images, labels, _names in loader_train:
            model.zero_grad()
            scores = model(images)
            y, ysz = H.encode(list(labels))
            loss = ctc(scores, y, torch.tensor([scores.shape[0]] * images.shape[0], dtype=torch.int), ysz)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        model.eval()
        correct = 0
        with torch.no_grad():
            for images, labels, _names in loader_val:
                correct += compare_labels(pred_to_string(model(images), list(labels), H.I2C), list(labels))[0]
        accs.append(correct / len(val_set))
        sched.step()
    return model, losses, accs


def test_train_crnn_is_the_reference_loop(tmp_path):
    """Two epochs on synthetic strips (3 steps each, a validation set of 5 = batches of 2, 2 and 1): the same optimiser steps (loss by
    loss), the same weights and the same validation accuracy as the reference's loop, with the noise drawn in the loader."""
    from datasets.synthetic import SyntheticTextAreas
    from train_crnn import TrainCRNN
    tr, va = SyntheticTextAreas(7, seed=1), SyntheticTextAreas(5, seed=2)
    args = _crnn_args(tmp_path, "--batch_size", "2", "--epoch", "2", "--lr", "0.001")
    t = TrainCRNN(args, backend=oracle_backend(), train_set=tr, val_set=va)
    seen, accs = [], []
    step = t.train_step
    t.train_step = lambda images, labels: seen.append(step(images, labels).item()) or torch.tensor(seen[-1])
    validate = t.validate
    t.validate = lambda: accs.append(validate()) or accs[-1]
    best = t.train()
    ref_model, ref_losses, ref_accs = _reference_loop(tr, va, 2, 1e-3, 2, 42, 5)
    assert len(seen) == 6 and np.allclose(seen, ref_losses, rtol=1e-6, atol=0)
    for (k, a), (_, b) in zip(t.model.state_dict().items(), ref_model.state_dict().items()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), k
    assert [c / len(va) for _, c, _ in accs] == ref_accs
    assert best[0] == max(ref_accs)


def test_train_crnn_step_lr_and_checkpoint_names(tmp_path):
    """StepLR(10, 0.8), stepped after every validation: epochs 0-9 run at lr, epoch 10 at 0.8 lr.  The last epoch writes
    `{crnn_model_path}_{epoch}_{acc*100:.2f}`, a whole-module pickle."""
    from datasets.synthetic import SyntheticTextAreas
    from train_crnn import TrainCRNN
    args = _crnn_args(tmp_path, "--batch_size", "2", "--epoch", "11")
    t = TrainCRNN(args, backend=oracle_backend(), train_set=SyntheticTextAreas(2, seed=1), val_set=SyntheticTextAreas(1, seed=2))
    lrs = []
    step = t.train_step
    t.train_step = lambda images, labels: lrs.append(t.optimizer.param_groups[0]["lr"]) or step(images, labels)
    t.train()
    assert lrs[:10] == [1e-4] * 10 and lrs[10] == pytest.approx(0.8e-4, rel=1e-12)
    files = os.listdir(tmp_path / "crnn")
    assert "model_10_%.2f" % (t.last_val_accuracy * 100) in files and all(re.fullmatch(r"model_\d+_\d+\.\d\d", f) for f in files)
    m = torch.load(tmp_path / "crnn" / ("model_10_%.2f" % (t.last_val_accuracy * 100)), weights_only=False)
    assert m.state_dict().keys() == t.model.state_dict().keys()


def _write_strips(d, labels, seed):
    from PIL import Image
    d.mkdir(parents=True)
    rng = np.random.RandomState(seed)
    for i, lab in enumerate(labels):
        Image.fromarray((rng.rand(20, 60 + 5 * i) * 255).astype(np.uint8)).save(d / f"{i}_{lab}_w.png")


def test_train_crnn_ground_truth_subsets_from_files(tmp_path):
    """--ocr absent with --train_subset / --val_subset: the reference crashes (ImgDataset has no num_subset); here the first N samples
    are used, the validation loader keeps its short last batch, and the epoch still checkpoints."""
    from train_crnn import TrainCRNN
    _write_strips(tmp_path / "data" / "vgg_train", ["ab", "Cd", "x1", "hello", "yes", "No"], 0)
    _write_strips(tmp_path / "data" / "vgg_dev", ["a", "b", "cc", "dd"], 1)
    args = _crnn_args(tmp_path, "--dataset", "vgg", "--data_base_path", str(tmp_path / "data"), "--batch_size", "2", "--epoch", "1",
                      "--train_subset", "4", "--val_subset", "3")
    t = TrainCRNN(args, backend=oracle_backend())
    assert t.train_set_size == 4 and t.val_set_size == 3
    assert [len(b[0]) for b in t.loader_validation] == [2, 1]
    t.train()
    assert any(f.startswith("model_0_") for f in os.listdir(tmp_path / "crnn"))


def test_train_crnn_ocr_labels(tmp_path):
    """--ocr stub: the training labels are the OCR's labels of the noisy batch, the validation labels its labels of the clean strips."""
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from train_crnn import TrainCRNN
    ocr = StubHelper()
    args = _crnn_args(tmp_path, "--batch_size", "2", "--epoch", "1", "--ocr", "stub")
    va = SyntheticTextAreas(3, seed=2)
    t = TrainCRNN(args, backend=oracle_backend(), train_set=SyntheticTextAreas(4, seed=1), val_set=va, ocr=ocr)
    got = []
    call = t._call_model
    t._call_model = lambda images, labels: got.append(list(labels)) or call(images, labels)
    t.train()
    assert ocr.count_calls == 4 + 3
    assert got[2:] == [StubHelper().get_labels(torch.stack([va[0][0], va[1][0]])), StubHelper().get_labels(va[2][0][None])]


def test_eval_crnn_area_and_patch_flows(tmp_path):
    """EvalCRNN on the oracle: the returned numbers are the decode of the loaded model against the labels, CER averaged over the
    strips (the pos flow included: the reference's per-document rounding of the running sum is not repeated)."""
    from datasets.synthetic import SyntheticPatches, SyntheticTextAreas
    from eval_crnn import EvalCRNN, build_parser
    from ocr_helper.stub_helper import StubHelper
    from oracle.modules import OracleCRNN
    from utils import compare_labels, get_text_stack, pred_to_string
    model = OracleCRNN(95, False, seed=3).eval()
    torch.save(model, tmp_path / "crnn_ckpt")
    va = SyntheticTextAreas(5, seed=2)
    args = build_parser().parse_args(["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--dataset", "vgg", "--batch_size", "2",
                                      "--ocr", "stub", "--show_orig", "--show_txt"])
    res = EvalCRNN(args, backend=oracle_backend(), dataset=va).eval()
    imgs = torch.stack([va[i][0] for i in range(5)])
    labels = [va[i][1] for i in range(5)]
    with torch.no_grad():
        preds = pred_to_string(model(imgs), labels, H.I2C)
    c, e = compare_labels(preds, labels)
    oc, oe = compare_labels(StubHelper().get_labels(imgs), labels)
    assert res["count"] == 5 and res["crnn_correct"] == c and res["crnn_cer"] == pytest.approx(e / 5)
    assert res["ocr_correct"] == oc and res["ocr_cer"] == pytest.approx(oe / 5)
    docs = SyntheticPatches(2, seed=4, strips=(2, 3), include_name=False)
    args.dataset = "pos"
    res = EvalCRNN(args, backend=oracle_backend(), dataset=docs).eval()
    n, cer = 0, 0.0
    for i in range(len(docs)):
        image, boxes = docs[i]
        crops, labels = get_text_stack(image, boxes, (32, 128))
        with torch.no_grad():
            cer += compare_labels(pred_to_string(model(crops), labels, H.I2C), labels)[1]
        n += len(labels)
    assert res["count"] == n and res["crnn_cer"] == pytest.approx(cer / n)


def test_eval_prep_area_flow_show_orig(tmp_path):
    """EvalPrep's area flow returns (accuracy, cer) of the cleaned strips (the reference returns None) and, with --show_orig, the
    original strips' CER divided once (the reference reads ori_lbl_cer before assigning it)."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_prep import EvalPrep, build_parser
    from ocr_helper.stub_helper import StubHelper
    from oracle.modules import OracleUNet
    from utils import compare_labels
    prep = OracleUNet(seed=5).eval()
    torch.save(prep, tmp_path / "prep")
    va = SyntheticTextAreas(3, seed=2)
    args = build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--dataset", "vgg", "--batch_size", "2", "--ocr", "stub",
                                      "--show_orig"])
    ev = EvalPrep(args, backend=oracle_backend(), dataset=va)
    acc, cer = ev.eval()
    imgs = torch.stack([va[i][0] for i in range(3)])
    labels = [va[i][1] for i in range(3)]
    with torch.no_grad():
        c, e = compare_labels(StubHelper().get_labels(prep(imgs)), labels)
    oc, oe = compare_labels(StubHelper().get_labels(imgs), labels)
    assert (acc, cer) == (pytest.approx(c / 3), pytest.approx(e / 3)) and ev.orig_result == (pytest.approx(oc / 3), pytest.approx(oe / 3))
