"""Host-side mirror of the reference interface (samplers, helpers, CLI flags, constants) on CPU."""
import json
import os

import numpy as np
import torch

import helpers as H


def test_properties_constants():
    import properties
    assert properties.char_set == H.CHAR_SET and properties.char_set[0] == "`"
    assert properties.input_size == (32, 128) and properties.max_char_len == 100 and properties.empty_char == " "
    assert properties.prep_crnn_ckpts == "ckpts" and properties.img_out == "img_out" and properties.param_path == "params.txt"
    assert properties.patch_dataset_train == "patch_dataset_train" and properties.vgg_text_dataset_dev == "vgg_dev"


def test_topk_sampler_matches_reference_cases(golden_dir):
    from selection_utils import datasampler_factory
    cases = json.load(open(os.path.join(golden_dir, "topk_cases.json")))["cases"]
    for c in cases:
        s = datasampler_factory("topKCER")(dict(c["cers"]))
        imgs = torch.arange(len(c["names"])).float().view(-1, 1)
        sel, labels, idx = s.query(imgs, list(c["names"]), c["k"], list(c["names"]))
        vals = np.float32([c["cers"][n] for n in c["names"] if n in c["cers"]])
        if "build-specific" in c["note"] or "real slice" in c["note"]:
            assert sorted(vals[idx].tolist()) == sorted(vals[c["idx"]].tolist())
        else:
            assert idx.tolist() == c["idx"], c["note"]
            if c["sel"] is not None:
                assert sel.view(-1).long().tolist() == c["sel"]
        assert labels == [c["names"][i] for i in idx.tolist()]


def test_sampler_protocol_and_factory_keys():
    from selection_utils import datasampler_factory
    for key in ("random", "topKCER", "uniformCERglobal", "randomglobal", "rangeCER", "uniformEntropy"):
        assert datasampler_factory(key)
    s = datasampler_factory("topKCER")({"a": 0.1})
    s.update_cer([0.5, 0.25], ["a", "b"])
    assert s.cers == {"a": 0.5, "b": 0.25} and s.all_cers == {"a": [0.5], "b": [0.25]}
    imgs = torch.arange(6).float().view(-1, 1)
    r = datasampler_factory("random")()
    sel, lab, idx = r.query(imgs, list("abcdef"), 3)
    assert sel.shape[0] == 3 and len(set(idx.tolist())) == 3
    rg = datasampler_factory("rangeCER")({n: i / 10 for i, n in enumerate("abcdef")})
    sel, lab, idx = rg.query(imgs, list("abcdef"), 2, list("abcdef"))
    assert len(set(idx.tolist())) == 2
    g = datasampler_factory("uniformCERglobal")({n: i / 10 for i, n in enumerate("abcdef")}, 2)
    g.select_samples()
    sel, lab, idx = g.query(imgs, list("abcdef"), names=list("abcdef"))
    assert len(idx) == 2


def test_utils_helpers_match_reference_fixtures(tmp_path):
    import utils
    fx = H.golden("helpers.npz")
    c2i, i2c, n = utils.get_char_maps(H.CHAR_SET)
    assert n == 95 and c2i["`"] == 0 and i2c[94] == "/"
    assert utils.pred_to_string(torch.from_numpy(fx["dec|scores"]), [""] * 6, i2c) == [str(s) for s in fx["dec|strings"]]
    boxes = [dict(label=str(i), x_min=int(b[0]), y_min=int(b[1]), x_max=int(b[2]), y_max=int(b[3])) for i, b in enumerate(fx["crop|boxes"])]
    stack, labels = utils.get_text_stack(torch.from_numpy(fx["crop|page"]), boxes, (32, 128))
    assert np.array_equal(stack.numpy(), fx["crop|stack"]) and labels == ["0", "1", "2", "3"]
    assert utils.compare_labels(["kitten", "abc"], ["sitting", "abc"]) == (1, 3 / 7)
    bn = torch.nn.BatchNorm2d(3).train()
    utils.set_bn_eval(bn)
    assert not bn.training

    class T:
        pass
    t, args = T(), type("A", (), dict(crnn_model=None, prep_model=None, data_base_path=".", exp_base_path=str(tmp_path / "exp")))()
    utils.create_dirs(t, args)
    for d in ("ckpts", "img_out", "cers", "tracked_labels", "selected_samples"):
        assert os.path.isdir(tmp_path / "exp" / d)
    utils.save_img(torch.rand(3, 1, 8, 16), "grid", str(tmp_path), 2)
    assert os.path.exists(tmp_path / "grid.png")


def test_add_gaussian_noice_call_semantics():
    from oracle import path_oracle as po
    from transform_helper import AddGaussianNoice
    fx = H.golden("helpers.npz")
    img = torch.from_numpy(fx["jit|img"])
    for stochastic, tag in ((False, "jit0"), (True, "jit1")):
        torch.manual_seed(123)
        out, noise = AddGaussianNoice(std=5, is_stochastic=stochastic, return_noise=True)(img.clone())
        assert np.array_equal(noise.numpy(), fx[f"{tag}|noise"]) and np.array_equal(out.numpy(), fx[f"{tag}|out"])
    torch.manual_seed(123)
    out = AddGaussianNoice(std=3)(img.clone(), noise_coef=0.5)
    assert np.array_equal(out.numpy(), po.jitter(img.numpy(), fx["jitc|noise"], 0.5))


def test_tracking_utils_and_stub_ocr():
    import tracking_utils as tu
    from label_tracking.tracking_methods import weightgenerator_factory
    from ocr_helper.stub_helper import StubHelper

    class T:
        window_size, weightgen_method, char_to_index = 3, "decaying", H.C2I
        tracked_labels = {"a": ["x", "yy"], "b": ["z"], "c": []}
    t = T()
    tu.add_labels_to_history(t, ["a", "c"], ["new", "cc"])
    assert t.tracked_labels["a"][-1] == "new" and t.tracked_labels["c"] == ["cc"]
    batches = tu.generate_ctc_target_batches(t, ["a", "b", "c"])
    assert [b[2] for b in batches] == [[0, 1, 2], [0], [0]]
    assert batches[0][1].tolist() == [3, 1, 2]
    args = type("A", (), dict(decay_factor=0.5, window_size=3))()
    w = weightgenerator_factory("decaying")(args, "cpu").gen_weights(None, None)
    assert w.tolist() == [1.0, 0.5, 0.25]
    ocr = StubHelper()
    imgs = H.synth_images(5, 3)
    a, b = ocr.get_labels(imgs), ocr.get_labels(imgs)
    assert a == b and ocr.count_calls == 10 and all(set(l) <= set(H.CHAR_SET) and 0 < len(l) <= 100 for l in a)


def test_cli_flag_surface():
    from qea.cli_flags import build_parser
    p = build_parser("p", "").parse_args([])
    assert (p.lr_crnn, p.lr_prep, p.epoch, p.std, p.inner_limit, p.weight_decay, p.minibatch_subset_prop) == (1e-4, 5e-5, 25, 5, 2, 5e-4, 0.5)
    assert p.random_std is True and p.ocr == "Tesseract" and p.weightgen_method == "decaying" and p.decay_factor == 0.7
    a = build_parser("a", "").parse_args(["--minibatch_subset", "topKCER", "--random_std", "--lr_scheduler", "cosine"])
    assert a.batch_size == 32 and a.epoch == 50 and a.random_std is False and not hasattr(a, "weight_decay")


def test_file_datasets_roundtrip(tmp_path):
    """on-disk formats of the reference's datasets (datasets/img_dataset.py, patch_dataset.py)."""
    from PIL import Image
    from datasets._io import to_tensor
    from datasets.img_dataset import ImgDataset
    from datasets.patch_dataset import PatchDataset
    from transform_helper import PadWhite
    d = tmp_path / "vgg_train"
    d.mkdir()
    rng = np.random.RandomState(0)
    for i, lab in enumerate(["hello", "A1", "x" * 101]):
        Image.fromarray((rng.rand(20, 60) * 255).astype(np.uint8)).save(d / f"{i}_{lab}_w.png")
    ds = ImgDataset(str(d), transform=lambda im: to_tensor(PadWhite((32, 128))(im)), include_name=True, include_index=True)
    assert len(ds) == 2                                   # the 101-char label is dropped
    img, label, name, idx = ds[0]
    assert img.shape == (1, 32, 128) and label in ("hello", "A1") and name.endswith("_w.png") and idx == 0
    assert img[0, 0, 0] == 1.0 and img.min() < 1.0        # white padding around the strip
    p = tmp_path / "patch_dataset_train" / "folderA"
    p.mkdir(parents=True)
    Image.fromarray((rng.rand(100, 300) * 255).astype(np.uint8)).save(p / "doc1.png")
    boxes = [dict(label="ab", x_min=10, y_min=5, x_max=90, y_max=30), dict(label="wide", x_min=0, y_min=0, x_max=200, y_max=20)]
    json.dump(boxes, open(p / "doc1.json", "w"))
    pd = PatchDataset(str(tmp_path / "patch_dataset_train"), pad=True, include_name=True)
    image, labels, name = pd[0]
    assert image.shape == (1, 400, 512) and len(labels) == 1 and labels[0]["label"] == "ab"
    assert (labels[0]["x_min"], labels[0]["y_min"]) == (10 + 106, 5 + 150)      # centred on the 400x512 canvas
    batch = PatchDataset.collate([pd[0]])
    assert batch[0].shape == (1, 1, 400, 512) and batch[2][0].endswith("doc1.png")


def test_levenshtein_and_attention_weight_generators():
    from label_tracking.tracking_methods import weightgenerator_factory
    args = type("A", (), dict(decay_factor=0.5, window_size=3, query_dim=8, emb_dim=16, attn_activation="sigmoid"))()
    hist = {"a": ["cat", "cat", "cut", "cat"], "b": ["x"], "c": []}
    lev = weightgenerator_factory("levenshtein")(args, "cpu")
    w = lev.gen_weights(hist, ["a", "b", "c", "missing"])
    assert w.shape == (4, 4) and w[:, 0].tolist() == [1, 1, 1, 1]
    # "a": window = [cat, cut, cat] (most recent first); cat vs {cut, cat}: mean 0.5 -> 0.5*(1-0.5/3)
    assert abs(w[0, 1].item() - 0.5 * (1 - 0.5 / 3)) < 1e-6 and abs(w[0, 2].item() - 0.5 * (1 - 1 / 3)) < 1e-6
    assert abs(w[1, 1].item() - 0.5) < 1e-6 and w[2, 1:].abs().sum() == 0 and w[3, 1:].abs().sum() == 0
    torch.manual_seed(0)
    att = weightgenerator_factory("self_attention")(args, "cpu", H.C2I)
    wa = att.gen_weights(hist, ["a", "b", "c"])
    assert wa.shape == (3, 4) and (wa[0, 1:] > 0).all() and (wa[0, 1:] < 1).all() and wa[1, 2:].abs().sum() == 0
    assert set(att.attention_model.state_dict().keys()) == {"positional_encodings", "embedding", "Wq.weight", "Wq.bias",
                                                            "loss_coef_layer.weight", "loss_coef_layer.bias"}


def test_global_topk_reports_the_picked_count_when_the_minibatch_is_smaller_than_k():
    """with fewer rows than k_global every row is picked and k is that number on every path (share = world * n / k)."""
    from qea import dist as qdist
    order, k = qdist.global_topk([0.3, 0.9], 5)
    assert order.tolist() == [1, 0] and k == 2
    order, k, counts = qdist.global_topk([0.3, 0.9], 5, with_counts=True)
    assert k == 2 and counts == [2] and k == sum(counts)
    order, k = qdist.global_topk([0.1, 0.5, 0.4], 2)
    assert order.tolist() == [1, 2] and k == 2


def test_f16_split_contract_in_numpy():
    """csrc/common.h: qea_f16_scale / qea_split2_f16 emulated with numpy float16 casts.  For magnitudes spanning 2^-30 ... 1 of the bound
    m (bounds just above / below a power of two, at gradient scale, near both ends of the supported range, and a bound 2^20 above the
    data): |x - (h + l) / s| <= max(SPLIT_REL |x|, SPLIT_ABS m) for EVERY element — the relative part alone down to 2^-16 of m — and
    both figures are reached (a 2^-24 relative / 2^-40 m absolute contract, as the comment once read, does not hold).  The derived
    gates of tests/test_operand_scale_gpu.py rest on these two constants; an all-zero tensor gets scale 1."""
    SPLIT_ABS, SPLIT_REL = H.SPLIT_ABS, H.SPLIT_REL

    def f16_scale(m):
        m = np.float32(m)
        e = int((m.view(np.uint32) >> 23) & 0xFF)
        se = 0 if (m == 0 or e == 0) else min(126, max(-126, 14 - (e - 127)))
        return np.float32(2.0) ** np.float32(se)

    def split2(x, s):
        xs = x * s                                              # fp32
        h = xs.astype(np.float16)
        l = (xs - h.astype(np.float32)).astype(np.float16)
        return h, l

    assert f16_scale(0.0) == 1.0 and f16_scale(1e-45) == 1.0
    rng = np.random.default_rng(0)
    worst_rel = worst_abs = 0.0
    for m in (1.0, np.nextafter(np.float32(2.0), np.float32(0)), 1.5, 4.7, 3e-9, 1.3 * 2.0 ** -100, 2.0 ** 100, 2.0 ** -112):
        m = float(np.float32(m))
        s = f16_scale(m)
        assert 2.0 ** 14 <= m * float(s) < 2.0 ** 15
        for top in (0.0, -20.0):                                 # data up to the bound / a bound 2^20 above the data
            mag = 2.0 ** rng.uniform(-30.0, top, 400_000)
            x = (mag * m * rng.choice([-1.0, 1.0], mag.size)).astype(np.float32)
            x[:4] = np.float32([m, -m, 0.0, m * 2.0 ** -16]) if top == 0.0 else 0.0
            h, l = split2(x, s)
            assert np.isfinite(h).all() and np.isfinite(l).all()
            err = np.abs((h.astype(np.float64) + l.astype(np.float64)) / float(s) - x.astype(np.float64))
            ax = np.abs(x.astype(np.float64))
            assert (err <= np.maximum(SPLIT_REL * ax, SPLIT_ABS * m)).all()
            big = ax >= 2.0 ** -16 * m
            if big.any():
                assert (err[big] <= SPLIT_REL * ax[big]).all()
                worst_rel = max(worst_rel, float((err[big] / ax[big]).max()))
            worst_abs = max(worst_abs, float(err[~big].max()) / m)
    assert worst_rel > 2.0 ** -24 and worst_abs > 2.0 ** -40      # the bounds are tight to a factor of two, not loose
    # the element-level probe of tests/test_operand_scale_gpu.py (an operand through an identity filter), emulated: the right scale is
    # inside helpers.split_element_gate, a scale one bit short (se = 13 - ...) is outside it — the mutation that every gate on a sum of
    # many terms is blind to
    x = H.split_probe_values(16384, 3).numpy()
    for se_base, inside in ((14, True), (13, False)):
        s = np.float32(2.0) ** np.float32(se_base)                # the bound is max |x| = 1.0
        h, l = split2(x, s)
        y = ((h.astype(np.float32) * s + l.astype(np.float32) * s) / s / s).astype(np.float32)   # hh + lh in an fp32 accumulator, un-scaled
        err = np.abs(y.astype(np.float64) - x.astype(np.float64))
        assert bool((err <= H.split_element_gate(torch.from_numpy(x), 1.0).numpy()).all()) == inside, se_base
    # below the supported range (m < 2^-112) the scale stops at 2^126: the planes lose bits against m, silently
    assert f16_scale(2.0 ** -120) == np.float32(2.0) ** 126


def test_colreduce_workspace_answers_equal_the_pinned_ones(golden_dir):
    """qea_colreduce_workspace_bytes(M, C) = (blocks * 2 + 3) * C doubles is a function of col_geom(M, C) alone: the block count that fixes
    the order of every fp64 column reduction.  Pinned (tests/golden/colreduce_workspace.json, written by
    tools/colreduce_workspace_queries.py) before the three BatchNorm backward entry points were made to share one pipeline."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import colreduce_workspace_queries as Q
    finally:
        sys.path.pop(0)
    pinned = json.load(open(os.path.join(golden_dir, "colreduce_workspace.json")))
    assert pinned["axes"] == Q.AXES, "the grid changed: regenerate the golden file from the commit that pinned it"
    got, want = Q.answers(), pinned["answers"]
    assert len(want) == 8 and all(len(row) == 9 for row in want)
    bad = [(m, c, want[i][j], got[i][j]) for i, m in enumerate(Q.AXES["M"]) for j, c in enumerate(Q.AXES["C"]) if want[i][j] != got[i][j]]
    assert not bad, f"{len(bad)} answers moved (M, C, pinned, got): {bad[:5]}"
    assert all(row[-1] == 0 for row in want) and all(v > 0 for row in want for v in row[:-1])      # C = 6: no multiple of 4


def test_batchnorm_partition():
    """qea.batchnorm.partition: the (first sample, samples) list of equal and of ragged statistics groups, and what it refuses."""
    import pytest
    from qea.batchnorm import partition
    assert partition(3, 12) == [(0, 4), (4, 4), (8, 4)]
    assert partition([3, 3, 5, 5, 2], 18) == [(0, 3), (3, 3), (6, 5), (11, 5), (16, 2)]
    assert partition((3, 1, 2), 6) == [(0, 3), (3, 1), (4, 2)]
    assert partition(1, 7) == [(0, 7)] and partition([7], 7) == [(0, 7)]
    for bad in (5, [3, 3], [4, 0, 3], [8, -1], 0, -2):           # not a multiple, another sum, a zero / negative size, groups < 1
        with pytest.raises(ValueError):
            partition(bad, 7)


def test_lstm_seq_timeout_index_lies_in_front_of_the_exchange_area():
    """qea_lstm_seq_timeout_index(B, backward) names the word a one-launch BiLSTM pass sets when a bounded spin runs out (read by
    qea.ops.lstm_seq_timed_out).  The workspace is [arrival counter per group][the timeout word][padding to a multiple of 64 words]
    [exchange area: parity 2 x direction 2 x row blocks of 32 (padded to the workgroup's rows) x bytes per row block]; a group is
    (workgroup's row block, direction), the workgroup has 128 rows above 512 (forward) / 1024 (backward) rows and 32 up to there.
    The index must be the group count of its own pass and lie below the 64-word-aligned start of the exchange area, and
    qea_lstm_seq_workspace_bytes must hold the larger of the two passes' layouts: restated here from csrc/lstm_seq.hip."""
    from qea import _lib
    L = _lib.lib()
    XRB = {0: 16 * 2048, 1: 64 * 2048 + 8 * 128}              # bytes of one row block: forward (h fragments) / backward (+ inverse scales)
    for B in (1, 32, 33, 512, 513, 1024, 1025, 2048):
        need = []
        for bwd in (0, 1):
            rows = 128 if B > (1024 if bwd else 512) else 32
            groups = -(-B // rows) * 2
            idx = L.qea_lstm_seq_timeout_index(B, bwd)
            assert idx == groups, (B, bwd)
            xch_start_words = (groups + 1 + 63) // 64 * 64     # the counters, then the timeout word, then the exchange area on a 256-byte line
            assert 0 <= idx < xch_start_words and idx >= groups, (B, bwd)
            need.append(xch_start_words * 4 + 2 * 2 * (-(-B // rows) * (rows // 32)) * XRB[bwd])
        assert L.qea_lstm_seq_workspace_bytes(B) == max(need), B
    assert L.qea_lstm_seq_timeout_index(0, 0) == -1 and L.qea_lstm_seq_timeout_index(-3, 1) == -1
