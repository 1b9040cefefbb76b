"""The binarisation baselines on the MI355X (csrc/binarize.hip): bit for bit the statement tests/binarize_spec.py over a ragged store, the
launch counts, no stray writes, the largest sums and the degenerate pages, and the front ends against their host-backend runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import binarize_spec as spec
from test_binarize_cpu import baseline_docs, block_page, host_backend

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (17, 33), (437, 531), (400, 512)]
WINDOWS = [3, 25, 127]
KS = [0.2, 0.5]


def _store(sizes, dtype, seed=11):
    """pages of `sizes` in one store with junk between them, every page at an ODD element offset (as tests/test_pages_gpu.py builds its
    store) -> (store, offset, h, w, pages)"""
    g = torch.Generator().manual_seed(seed)
    offset, off = [], 1
    for hh, ww in sizes:
        off += 1 - off % 2
        offset.append(off)
        off += hh * ww + 3
    if dtype == torch.uint8:
        store = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8)
    else:
        store = torch.rand(off, generator=g) * 1.5 - 0.25
    pages = [store[o:o + hh * ww].view(hh, ww) for o, (hh, ww) in zip(offset, sizes)]
    return store, np.asarray(offset, np.int64), np.asarray([s[0] for s in sizes], np.int32), np.asarray([s[1] for s in sizes], np.int32), pages


@pytest.fixture(scope="module")
def reference():
    """(dtype) -> the store and, computed once and never changed, the statement's window sums per (page, window) and Otsu results"""
    done = {}

    def get(dtype):
        if dtype not in done:
            store, offset, h, w, pages = _store(SIZES, dtype)
            v8 = [spec.to_u8(p.numpy()) for p in pages]
            sums = {(i, win): spec.window_sums(v, win) for i, v in enumerate(v8) for win in WINDOWS}
            done[dtype] = dict(store=store, offset=offset, h=h, w=w, pages=pages, v8=v8, sums=sums, otsu=[spec.otsu(v) for v in v8])
        return done[dtype]
    return get


def _inside(ref):
    inside = torch.zeros(ref["store"].numel(), dtype=torch.bool)
    for o, hh, ww in zip(ref["offset"], ref["h"], ref["w"]):
        inside[int(o):int(o) + int(hh) * int(ww)] = True
    return inside


def _outputs(n, out):
    """a prefilled output and its keyword: 0x5A / -7.0 are values no binariser writes"""
    if out == "u8":
        return torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda"), "out_u8"
    return torch.full((n,), -7.0, device="cuda"), "out_f32"


def _check(res, ref, want_pages, out, inside):
    """every page equals the statement; every element between the pages keeps its sentinel"""
    res = res.cpu()
    for o, hh, ww, want in zip(ref["offset"], ref["h"], ref["w"], want_pages):
        got = res[int(o):int(o) + int(hh) * int(ww)].view(int(hh), int(ww))
        assert torch.equal(got, torch.from_numpy(want)), (int(hh), int(ww))
    assert bool((res[~inside] == (0x5A if out == "u8" else -7.0)).all())


@pytest.mark.parametrize("out", ["u8", "float"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_sauvola_is_the_statement_bit_for_bit(reference, dtype, out):
    """Four pages (1x1, 17x33, 437x531, 400x512) at odd offsets with junk between them, ONE launch per (window, k) whatever the page
    count: torch.equal with the statement for windows 3, 25, 127 and k = 0.2, 0.5; the junk keeps its sentinel."""
    from qea import ops
    ref = reference(dtype)
    store = ref["store"].cuda()
    table = ops.page_table(ref["offset"], ref["h"], ref["w"], store.device)
    inside = _inside(ref)
    for win in WINDOWS:
        for k in KS:
            want = [spec.sauvola(v, win, k, 128.0, out=out, sums=ref["sums"][i, win]) for i, v in enumerate(ref["v8"])]
            assert all(bool((x == 0).any()) and bool((x != 0).any()) for x in want[1:])
            res, key = _outputs(store.numel(), out)
            before = dict(ops.BINARIZE_LAUNCHES)
            ops.binarize_sauvola(store, table, win, k, 128.0, **{key: res})
            assert sum(ops.BINARIZE_LAUNCHES.values()) == sum(before.values()) + 1 and ops.BINARIZE_LAUNCHES["sauvola"] == before["sauvola"] + 1
            _check(res, ref, want, out, inside)
    one = ops.page_table(ref["offset"][2:3], ref["h"][2:3], ref["w"][2:3], store.device)      # one page: one launch as well
    before = sum(ops.BINARIZE_LAUNCHES.values())
    res, key = _outputs(store.numel(), out)
    ops.binarize_sauvola(store, one, 25, 0.2, 128.0, **{key: res})
    assert sum(ops.BINARIZE_LAUNCHES.values()) == before + 1
    o, hh, ww = int(ref["offset"][2]), int(ref["h"][2]), int(ref["w"][2])
    assert torch.equal(res.cpu()[o:o + hh * ww].view(hh, ww), torch.from_numpy(spec.sauvola(ref["v8"][2], 25, 0.2, 128.0, out=out, sums=ref["sums"][2, 25])))


@pytest.mark.parametrize("out", ["u8", "float"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_otsu_is_the_statement_bit_for_bit(reference, dtype, out):
    """the same store: two launches whatever the page count, the histograms are the exact counts, t* per page and every pixel are the
    statement's; the junk keeps its sentinel."""
    from qea import ops
    ref = reference(dtype)
    store = ref["store"].cuda()
    table = ops.page_table(ref["offset"], ref["h"], ref["w"], store.device)
    res, key = _outputs(store.numel(), out)
    before = dict(ops.BINARIZE_LAUNCHES)
    hist = ops.otsu_histogram(store, table)
    thr = ops.binarize_otsu(store, table, hist, **{key: res})
    assert sum(ops.BINARIZE_LAUNCHES.values()) == sum(before.values()) + 2 and ops.BINARIZE_LAUNCHES["sauvola"] == before["sauvola"]
    for i, v in enumerate(ref["v8"]):
        assert np.array_equal(hist[i].cpu().numpy(), np.bincount(v.reshape(-1), minlength=256))
    assert thr.dtype == torch.int32 and thr.tolist() == [t for _, t in ref["otsu"]] and thr.tolist()[0] == -1
    want = [b if out == "u8" else spec.as_output(b == 0, "float") for b, _ in ref["otsu"]]
    _check(res, ref, want, out, _inside(ref))


def test_largest_sums_and_degenerate_pages():
    """the 130 x 130 all-255 block at window 127 (S2 = 127^2 * 65025, n * S2 beyond 32 bits), an all-zero page and a single-level page,
    through the product's device path, against the statement"""
    from qea.binarize import binarize_pages, otsu_thresholds
    pages = [block_page(), torch.zeros(70, 90, dtype=torch.uint8), torch.full((33, 65), 200, dtype=torch.uint8)]
    got = binarize_pages([p.cuda() for p in pages], "sauvola", window=127, out="u8")
    for p, b in zip(pages, got):
        assert b.is_cuda and torch.equal(b.cpu(), torch.from_numpy(spec.sauvola(p.numpy(), 127, 0.2, 128.0)))
    assert bool((got[1] == 0).all()) and bool((got[2] == 255).all())          # v = 0 is ink, a flat v > 0 is background
    got = binarize_pages(pages, "otsu", out="float", device="cuda")
    for p, b in zip(pages, got):
        assert torch.equal(b.cpu(), torch.from_numpy(spec.otsu(p.numpy(), out="float")[0]))
    assert otsu_thresholds(pages, device="cuda").tolist() == [spec.otsu_threshold(p.numpy()) for p in pages]
    assert otsu_thresholds(pages, device="cuda").tolist()[1:] == [-1, -1] and bool((got[1] == 1).all())


@pytest.mark.parametrize("method", ["otsu", "sauvola"])
def test_binarize_pages_on_the_device_is_its_host_path(method):
    """CUDA pages against the same call on CPU pages: mixed sizes, [1, h, w] float pages with values outside [0, 1] and NaN, both outputs"""
    from qea.binarize import binarize_pages
    g = torch.Generator().manual_seed(6)
    floats = [torch.rand(1, 45, 67, generator=g) * 1.5 - 0.25, torch.rand(1, 233, 219, generator=g), torch.rand(1, 1, 300, generator=g)]
    floats[0][0, 2, 3] = float("nan")
    bytes_ = [torch.randint(0, 256, (s, t), generator=g, dtype=torch.uint8) for s, t in ((64, 64), (65, 129), (31, 1))]
    for pages in (floats, bytes_):
        for out in ("u8", "float"):
            want = binarize_pages(pages, method, window=15, k=0.3, out=out)
            got = binarize_pages([p.cuda() for p in pages], method, window=15, k=0.3, out=out)
            assert all(g_.is_cuda and g_.shape == p.shape and torch.equal(g_.cpu(), w_) for g_, w_, p in zip(got, want, pages))


def test_eval_prep_baseline_on_the_device(tmp_path):
    """--baseline sauvola on the device gives the baseline_result of the host-backend run (the binarised images are bit-identical, so the
    stub OCR reads the same labels)"""
    from eval_prep import EvalPrep, build_parser
    from models.model_unet import UNet
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep_host")
    torch.save(UNet().cuda().eval(), tmp_path / "prep")
    flags = ["--ocr", "stub", "--baseline", "sauvola", "--baseline_window", "9", "--baseline_k", "0.3"]
    host = EvalPrep(build_parser().parse_args(["--prep_path", str(tmp_path / "prep_host")] + flags), backend=backend, dataset=baseline_docs())
    host.eval()
    dev = EvalPrep(build_parser().parse_args(["--prep_path", str(tmp_path / "prep")] + flags), dataset=baseline_docs())
    acc, cer = dev.eval()
    assert 0.0 <= acc <= 1.0 and cer >= 0.0
    assert dev.baseline_result == host.baseline_result and dev.baseline_result is not None


def test_clean_cli_otsu_on_the_device(tmp_path):
    """--method otsu on the device writes the PNGs of the host-backend run"""
    from PIL import Image
    import clean_cli
    backend, _ = host_backend()
    (tmp_path / "in").mkdir()
    g = torch.Generator().manual_seed(9)
    for stem, (hh, ww) in {"a": (45, 67), "b": (233, 219), "c": (50, 40)}.items():
        Image.fromarray(torch.randint(0, 256, (hh, ww), generator=g, dtype=torch.uint8).numpy()).save(tmp_path / "in" / f"{stem}.png")
    written = {}
    for name, be in (("host", backend), ("device", None)):
        args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"),
                                                    "--out_dir", str(tmp_path / name), "--method", "otsu", "--batch_pages", "2"])
        written[name] = clean_cli.CleanPages(args, backend=be).run()
    assert len(written["device"]) == 3
    for a, b in zip(written["host"], written["device"]):
        with Image.open(a) as x, Image.open(b) as y:
            assert y.mode == "L" and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y))


def test_library_refusals_launch_nothing():
    """the C ABI with real device buffers: every refusal returns a negative code, and the prefilled output is untouched afterwards"""
    from qea import _lib, ops
    L = _lib.lib()
    store = torch.randint(0, 256, (64,), dtype=torch.uint8, device="cuda")
    table = ops.page_table(np.zeros(1, np.int64), np.asarray([8], np.int32), np.asarray([8], np.int32), store.device)
    out = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    outf = torch.full((65,), -7.0, device="cuda")
    hist = torch.full((256,), 3, dtype=torch.int32, device="cuda")
    thr = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    hh, ww = table.host_h.ctypes.data, table.host_w.ctypes.data
    lead = (store.data_ptr(), 0, 64, table.offset, table.h, table.w, 1)

    def sauvola(win=25, k=0.2, R=128.0, host_h=hh, host_w=ww, of=None, ou=out.data_ptr(), first=table.tile_first):
        return L.qea_binarize_sauvola(*lead, host_h, host_w, first, win, k, R, of, ou, None)
    zero, big_h, big_w = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1 << 14), (C.c_int32 * 1)((1 << 13) + 1)
    for kw in (dict(win=24), dict(win=1), dict(win=129), dict(k=0.0), dict(k=1.5), dict(k=float("nan")), dict(R=0.0), dict(R=float("inf")),
               dict(host_h=zero), dict(host_h=big_h, host_w=big_w), dict(ou=None), dict(of=outf.data_ptr() + 2), dict(first=None)):
        assert sauvola(**kw) < 0, kw
    assert L.qea_otsu_histogram(*lead, zero, ww, table.chunk_first, hist.data_ptr(), None) < 0
    assert L.qea_otsu_histogram(*lead, hh, ww, table.chunk_first, None, None) < 0
    assert L.qea_binarize_otsu(*lead, big_h, big_w, table.chunk_first, hist.data_ptr(), None, out.data_ptr(), thr.data_ptr(), None) < 0
    assert L.qea_binarize_otsu(*lead, hh, ww, table.chunk_first, hist.data_ptr(), None, None, thr.data_ptr(), None) < 0
    assert L.qea_binarize_otsu(*lead, hh, ww, table.chunk_first, hist.data_ptr(), outf.data_ptr() + 2, None, thr.data_ptr(), None) < 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((outf == -7.0).all()) and bool((hist == 3).all()) and thr.item() == 77
    assert sauvola() == 0                                      # and the accepted call writes the page
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(8, 8), torch.from_numpy(spec.sauvola(store.cpu().view(8, 8).numpy(), 25, 0.2, 128.0)))
