"""The binarisation baselines on the host: the statement (tests/binarize_spec.py) against the textbook formula and against exact rational
arithmetic, the product's host path (qea/binarize.py) bit for bit against the statement, every refusal, the flags of the two front ends,
and eval_prep.py --baseline / clean_cli.py --method on the host backend with the stub OCR."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import binarize_spec as spec

torch.set_num_threads(4)


def block_page(h=140, w=150):
    """seeded noise around a 130 x 130 all-255 block: a 127 x 127 window inside it holds the largest S1 and S2 there are"""
    page = torch.randint(0, 256, (h, w), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    page[5:135, 10:140] = 255
    return page


def structured_pages():
    g = np.random.default_rng(7)
    flat = np.zeros((40, 56), np.uint8)
    flat[:, 14:28], flat[:, 28:42], flat[:, 42:] = 1, 128, 255          # flat blocks of 0, 1, 128, 255, each wider than a 9-window
    checker = np.where((np.add.outer(np.arange(40), np.arange(56)) // 4) % 2, 200, 40).astype(np.uint8)
    ramp = np.tile(np.linspace(0, 255, 56).astype(np.uint8), (40, 1))
    return {"random": g.integers(0, 256, (40, 56), dtype=np.uint8), "random2": g.integers(0, 256, (33, 47), dtype=np.uint8),
            "flat": flat, "checker": checker, "ramp": ramp}


@pytest.mark.parametrize("win,k", [(9, 0.2), (25, 0.5), (3, 0.34)])
def test_the_statement_is_the_textbook_formula(win, k):
    """Decisions differ from v <= m (1 + k (s / R - 1)), evaluated with sqrt and division in fp64, only where |v - T| < 1e-9, and such
    pixels are at most 1 in 1000; the array-wide statement is the per-pixel brute force; flat regions: v > 0 background, v = 0 foreground."""
    near = total = 0
    for name, page in structured_pages().items():
        got = spec.sauvola(page, win, k, 128.0) == 0
        T, v = spec.sauvola_textbook(page, win, k, 128.0)
        differ = got != (v <= T)
        close = np.abs(v - T) < 1e-9
        assert not (differ & ~close).any(), name
        near += int((differ & close).sum())
        total += page.size
        n, S1, S2 = spec.window_sums(page, win)
        for y in range(0, page.shape[0], 3):
            for x in range(0, page.shape[1], 5):
                assert (int(n[y, x]), int(S1[y, x]), int(S2[y, x])) == spec.window_sums_at(page, y, x, win)
                assert spec.sauvola_at(page, y, x, win, k, 128.0) == bool(got[y, x]), (name, y, x)
    assert near * 1000 <= total
    r = win // 2
    flat = spec.sauvola(structured_pages()["flat"], win, k, 128.0)
    for x0, v in ((0, 0), (14, 1), (28, 128), (42, 255)):
        if 14 - 2 * r > 0:
            inner = flat[:, x0 + r:x0 + 14 - r]                 # windows that see one grey level only
            assert (inner == (0 if v == 0 else 255)).all(), v


def exact_otsu(hist):
    """t* by exact rational between-class scores d^2 / (w0 w1), ties to the smaller t"""
    hist = [int(c) for c in hist]
    N, S = sum(hist), sum(v * c for v, c in enumerate(hist))
    best, score = -1, None
    for t in range(255):
        w0, s0 = sum(hist[:t + 1]), sum(v * hist[v] for v in range(t + 1))
        if w0 == 0 or w0 == N:
            continue
        sc = Fraction((s0 * N - S * w0) ** 2, w0 * (N - w0))
        if score is None or sc > score:
            best, score = t, sc
    return best


def otsu_pages():
    g = np.random.default_rng(3)
    bimodal = np.clip(np.where(g.random((60, 70)) < 0.3, g.normal(60, 12, (60, 70)), g.normal(190, 20, (60, 70))), 0, 255).astype(np.uint8)
    spikes = np.full((20, 30), 50, np.uint8)
    spikes[:, 15:] = 180                                      # two equal spikes: every t in 50..179 scores alike
    ends = np.where(g.random((25, 25)) < 0.4, 0, 255).astype(np.uint8)
    return {"bimodal": (bimodal, None), "single": (np.full((9, 11), 77, np.uint8), -1), "spikes": (spikes, 50), "ends": (ends, 0)}


@pytest.mark.parametrize("name", sorted(otsu_pages()))
def test_otsu_threshold_against_exact_rationals(name):
    page, known = otsu_pages()[name]
    want = exact_otsu(np.bincount(page.reshape(-1), minlength=256))
    out, t = spec.otsu(page)
    assert t == want and (known is None or t == known)
    assert np.array_equal(out, np.where(page.astype(int) <= t, 0, 255))
    if name == "single":
        assert (out == 255).all()
    if name == "bimodal":
        assert 90 <= t <= 160
    from qea.binarize import binarize_pages, otsu_thresholds
    assert int(otsu_thresholds([torch.from_numpy(page)])[0]) == want
    assert np.array_equal(binarize_pages([torch.from_numpy(page)], "otsu", out="u8")[0].numpy(), out)


def host_pages():
    g = torch.Generator().manual_seed(2)
    f = torch.rand(17, 33, generator=g) * 1.5 - 0.25          # floats outside [0, 1]
    f[3, 4], f[0, 0], f[16, 32] = float("nan"), float("inf"), -float("inf")
    return {"1x1": torch.full((1, 1), 9, dtype=torch.uint8), "17x33": torch.randint(0, 256, (17, 33), generator=g, dtype=torch.uint8),
            "block": block_page(), "float": f, "float3": (block_page().float() / 255)[None]}


@pytest.mark.parametrize("name", sorted(host_pages()))
def test_host_path_is_the_statement(name):
    """torch.equal with the statement for both methods and both output forms; windows 3, 25, 127 (larger than the 1 x 1 and 17 x 33 pages)"""
    from qea.binarize import binarize_pages, otsu_thresholds
    page = host_pages()[name]
    flat = (page[0] if page.dim() == 3 else page).numpy()
    for out in ("u8", "float"):
        for win in (3, 25, 127):
            got = binarize_pages([page], "sauvola", window=win, k=0.2, R=128.0, out=out)[0]
            assert got.shape == page.shape and got.dtype == (torch.uint8 if out == "u8" else torch.float32)
            assert torch.equal(got.reshape(flat.shape), torch.from_numpy(spec.sauvola(flat, win, 0.2, 128.0, out=out))), (out, win)
        want, t = spec.otsu(flat, out=out)
        assert torch.equal(binarize_pages([page], "otsu", out=out)[0].reshape(flat.shape), torch.from_numpy(want))
        assert otsu_thresholds([page]).tolist() == [t]
    if name == "float3":                                      # float32(p) / 255 reads back as p
        assert np.array_equal(spec.to_u8(flat), block_page().numpy())
        a = binarize_pages([page], "sauvola", window=127, out="u8")[0][0]
        assert torch.equal(a, binarize_pages([block_page()], "sauvola", window=127, out="u8")[0])
    if name == "block":                                       # the largest sums occur: a whole 127-window of 255s
        assert spec.window_sums_at(flat, 69, 74, 127) == (127 * 127, 127 * 127 * 255, 127 * 127 * 65025)


def test_several_pages_of_mixed_sizes_in_one_call():
    from qea.binarize import binarize_pages
    pages = [host_pages()[n] for n in ("1x1", "17x33", "block")]
    for method in ("otsu", "sauvola"):
        together = binarize_pages(pages, method, window=25, out="u8")
        for p, b in zip(pages, together):
            assert torch.equal(b, binarize_pages([p], method, window=25, out="u8")[0])


def test_refusals_of_the_product_module():
    from qea._lib import QeaError
    from qea.binarize import binarize_pages, otsu_thresholds
    page = [torch.zeros(4, 4, dtype=torch.uint8)]
    for bad in (dict(method="niblack"), dict(window=24), dict(window=1), dict(window=129), dict(window=25.5), dict(k=0.0), dict(k=1.0),
                dict(k=float("nan")), dict(R=0.0), dict(R=-1.0), dict(R=float("inf")), dict(R=float("nan")), dict(out="png")):
        with pytest.raises(ValueError):
            binarize_pages(page, **bad)
    with pytest.raises(ValueError):
        binarize_pages([torch.zeros(0, 4, dtype=torch.uint8)])                       # an empty page
    with pytest.raises(ValueError):
        binarize_pages([])
    huge = torch.zeros(1, dtype=torch.uint8).expand(1 << 14, (1 << 13) + 1)          # over 2^27 pixels, no memory behind it
    for call in (lambda: binarize_pages([huge], "otsu"), lambda: binarize_pages([huge]), lambda: otsu_thresholds([huge])):
        with pytest.raises(QeaError, match="2\\^27"):
            call()


def test_library_refuses_bad_arguments_before_any_launch():
    """the three entry points: negative codes and a qea_last_error text; nothing but host_h / host_w is dereferenced on the host"""
    from qea import _lib
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    assert len(protos["qea_binarize_sauvola"]) == 16 and len(protos["qea_otsu_histogram"]) == 12 and len(protos["qea_binarize_otsu"]) == 15
    L = _lib.lib()
    assert L.qea_version() == 9
    one, odd = C.c_void_p(256), C.c_void_p(258)
    hh, ww = (C.c_int32 * 1)(4), (C.c_int32 * 1)(4)

    def sauvola(store=one, f32=0, elems=16, off=one, h=one, w=one, n=1, host_h=hh, host_w=ww, first=one, win=25, k=0.2, R=128.0, of=None, ou=one):
        return L.qea_binarize_sauvola(store, f32, elems, off, h, w, n, host_h, host_w, first, win, k, R, of, ou, None)
    bad = [dict(store=None), dict(off=None), dict(h=None), dict(w=None), dict(host_h=None), dict(host_w=None), dict(first=None), dict(f32=2),
           dict(n=0), dict(elems=0), dict(win=24), dict(win=1), dict(win=129), dict(k=0.0), dict(k=1.0), dict(k=float("nan")), dict(R=0.0),
           dict(R=float("inf")), dict(R=float("nan")), dict(ou=None), dict(of=odd), dict(store=odd, f32=1),
           dict(host_h=(C.c_int32 * 1)(0)), dict(host_w=(C.c_int32 * 1)(-3)),
           dict(host_h=(C.c_int32 * 1)(1 << 14), host_w=(C.c_int32 * 1)((1 << 13) + 1))]
    for kw in bad:
        assert sauvola(**kw) < 0, kw
        assert b"qea_binarize_sauvola" in L.qea_last_error(), kw
    assert b"2^27" in L.qea_last_error()
    hist, thr = one, one
    assert L.qea_otsu_histogram(one, 0, 16, one, one, one, 1, hh, ww, one, None, None) < 0                    # no table
    assert L.qea_otsu_histogram(one, 0, 16, one, one, one, 1, hh, ww, one, odd, None) < 0                     # misaligned table
    assert L.qea_otsu_histogram(one, 0, 16, one, one, one, 1, (C.c_int32 * 1)(0), ww, one, hist, None) < 0    # an empty page
    assert L.qea_otsu_histogram(None, 0, 16, one, one, one, 1, hh, ww, one, hist, None) < 0
    assert b"qea_otsu_histogram" in L.qea_last_error()
    big_h, big_w = (C.c_int32 * 2)(4, 1 << 14), (C.c_int32 * 2)(4, (1 << 13) + 1)
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 2, big_h, big_w, one, hist, None, one, thr, None) < 0   # page 1 over 2^27 pixels
    assert b"page 1" in L.qea_last_error()
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 1, hh, ww, one, hist, None, None, thr, None) < 0    # no output
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 1, hh, ww, one, hist, odd, None, thr, None) < 0     # out_f32 misaligned
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 1, hh, ww, one, None, None, one, thr, None) < 0     # no histogram
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 1, hh, ww, one, hist, None, one, None, None) < 0    # no thresholds
    assert L.qea_binarize_otsu(one, 0, 16, one, one, one, 1, hh, ww, one, hist, None, one, odd, None) < 0     # thresholds misaligned
    assert b"qea_binarize_otsu" in L.qea_last_error()


def test_ops_need_a_device():
    from qea import _lib, ops
    assert set(ops.BINARIZE_LAUNCHES) == {"sauvola", "histogram", "otsu"}
    with pytest.raises(_lib.QeaError):
        ops.page_table(np.zeros(1, np.int64), np.ones(1, np.int32), np.ones(1, np.int32), torch.device("cpu"))


def test_flags_of_the_two_front_ends():
    import clean_cli
    import eval_prep
    from qea.cli_flags import build_parser
    v = eval_prep.build_parser()
    a = v.parse_args([])
    assert a.baseline is None and a.baseline_window == 25 and a.baseline_k == 0.2
    a = v.parse_args(["--baseline", "sauvola", "--baseline_window", "51", "--baseline_k", "0.34"])
    assert (a.baseline, a.baseline_window, a.baseline_k) == ("sauvola", 51, 0.34)
    assert v.parse_args(["--baseline", "otsu"]).baseline == "otsu"
    with pytest.raises(SystemExit):
        v.parse_args(["--baseline", "niblack"])
    n = clean_cli.build_parser()
    a = n.parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert (a.method, a.window, a.k) == ("unet", 25, 0.2)
    a = n.parse_args(["--in_dir", "a", "--out_dir", "b", "--method", "sauvola", "--window", "15", "--k", "0.5"])
    assert (a.method, a.window, a.k) == ("sauvola", 15, 0.5)
    with pytest.raises(SystemExit):
        n.parse_args(["--in_dir", "a", "--out_dir", "b", "--method", "wolf"])
    new = {"v": ["--baseline", "--baseline_window", "--baseline_k"], "n": ["--method", "--window", "--k"]}
    for tag, flags in new.items():
        acts = {s: act for act in build_parser(tag, "")._actions for s in act.option_strings}
        assert all(acts[f].help.startswith("[new]") for f in flags)
    for tag in "pacer":
        got = build_parser(tag, "").parse_args([] if tag != "r" else ["--cers_tess_path", "x"])
        assert not hasattr(got, "baseline") and not hasattr(got, "method")


def host_backend():
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    return Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False), OracleUNet


def baseline_docs():
    g = torch.Generator().manual_seed(4)
    boxes = [dict(label="ab", x_min=3, y_min=5, x_max=90, y_max=30), dict(label="cde", x_min=20, y_min=40, x_max=140, y_max=64)]
    return [(torch.rand(1, 80, 160, generator=g), boxes, "first.png"), (torch.rand(1, 64, 144, generator=g), boxes[:1], "second.png")]


def expected_patch_result(docs, method, **kw):
    """the evaluation of the STATEMENT's images: each document binarised whole by tests/binarize_spec.py, cut, read by the stub OCR"""
    import properties
    from ocr_helper.stub_helper import StubHelper
    from utils import compare_labels, get_text_stack
    ocr, correct, cer, count = StubHelper(is_eval=True), 0, 0.0, 0
    for image, boxes, _ in docs:
        flat = image[0].numpy()
        b = spec.otsu(flat, out="float")[0] if method == "otsu" else spec.sauvola(flat, out="float", **kw)
        crops, labels = get_text_stack(torch.from_numpy(b)[None], boxes, properties.input_size)
        c, e = compare_labels(ocr.get_labels(crops), labels)
        correct, cer, count = correct + c, cer + e, count + len(labels)
    return correct / count, cer / count


@pytest.mark.parametrize("method", ["otsu", "sauvola"])
def test_eval_prep_baseline_on_the_host_backend(tmp_path, capsys, method):
    """--baseline on the oracle backend with the stub OCR: baseline_result is the evaluation of the statement's images in both flows, the
    new lines are printed, and the return value and the other prints are those of the run without the flag."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_prep import EvalPrep, build_parser
    from ocr_helper.stub_helper import StubHelper
    from utils import compare_labels
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep")
    base = ["--prep_path", str(tmp_path / "prep"), "--ocr", "stub"]
    flags = ["--baseline", method] + (["--baseline_window", "9", "--baseline_k", "0.3"] if method == "sauvola" else [])
    kw = dict(win=9, k=0.3, R=128.0) if method == "sauvola" else {}
    docs = baseline_docs()
    plain = EvalPrep(build_parser().parse_args(base), backend=backend, dataset=docs)
    plain_result = plain.eval()
    plain_out = capsys.readouterr().out
    assert plain.baseline_result is None and method not in plain_out
    ev = EvalPrep(build_parser().parse_args(base + flags), backend=backend, dataset=docs)
    assert ev.eval() == plain_result
    out = capsys.readouterr().out
    assert ev.baseline_result == expected_patch_result(docs, method, **kw)
    assert f"Correct count from {method} images: " in out and f"Average CER from {method} images: (" in out
    assert [l for l in out.splitlines() if method not in l] == plain_out.splitlines()
    # area flow: every strip of a batch is its own page
    va = SyntheticTextAreas(3, seed=2)
    area = base + ["--dataset", "vgg", "--batch_size", "2"]
    plain_result = EvalPrep(build_parser().parse_args(area), backend=backend, dataset=va).eval()
    ev = EvalPrep(build_parser().parse_args(area + flags), backend=backend, dataset=va)
    assert ev.eval() == plain_result
    ocr, correct, cer = StubHelper(is_eval=True), 0, 0.0
    for i in range(len(va)):
        strip, label = va[i][0], va[i][1]
        b = spec.otsu(strip[0].numpy(), out="float")[0] if method == "otsu" else spec.sauvola(strip[0].numpy(), out="float", **kw)
        c, e = compare_labels(ocr.get_labels(torch.from_numpy(b)[None, None]), [label])
        correct, cer = correct + c, cer + e
    assert ev.baseline_result == (correct / len(va), cer / len(va))
    assert f"Average CER from {method} images: " in capsys.readouterr().out
    with pytest.raises(ValueError):
        EvalPrep(build_parser().parse_args(base + ["--baseline", "sauvola", "--baseline_window", "10"]), backend=backend, dataset=docs)


@pytest.mark.parametrize("method", ["otsu", "sauvola"])
def test_clean_cli_method_on_the_host_backend(tmp_path, method):
    """--method otsu / sauvola: no checkpoint is read (the path does not exist), --tile is ignored, and the PNGs are the statement's bytes"""
    from PIL import Image
    import clean_cli
    backend, _ = host_backend()
    (tmp_path / "in").mkdir()
    g = torch.Generator().manual_seed(9)
    scans = {"a": torch.randint(0, 256, (21, 67), generator=g, dtype=torch.uint8), "b": torch.randint(0, 256, (35, 219), generator=g, dtype=torch.uint8),
             "c": torch.randint(0, 256, (50, 40), generator=g, dtype=torch.uint8)}
    for stem, px in scans.items():
        Image.fromarray(px.numpy()).save(tmp_path / "in" / f"{stem}.png")
    args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "no_such_checkpoint"), "--in_dir", str(tmp_path / "in"),
                                                "--out_dir", str(tmp_path / "out"), "--method", method, "--window", "15", "--k", "0.25",
                                                "--tile", "7", "7", "--batch_pages", "2"])
    written = clean_cli.CleanPages(args, backend=backend).run()
    assert [p.split("/")[-1] for p in written] == ["a.png", "b.png", "c.png"]
    for path, px in zip(written, scans.values()):
        want = spec.otsu(px.numpy())[0] if method == "otsu" else spec.sauvola(px.numpy(), 15, 0.25, 128.0)
        with Image.open(path) as img:
            assert img.mode == "L" and img.size == (px.shape[1], px.shape[0]) and np.array_equal(np.asarray(img), want)
