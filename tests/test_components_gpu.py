"""Connected components on the MI355X (csrc/components.hip): labels, areas and despeckled pages bit for bit the statement
tests/components_spec.py over a ragged store with junk between the pages, the fixed launch sequence, the tile seams alone, the product's
device path against its host path, the front ends against their host-backend runs, and the refusals of the C ABI."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import components_spec as spec
from test_binarize_cpu import baseline_docs, host_backend
from test_components_cpu import NAMES, as_page, ink_pages, scans_with_words, statement_labels, words_page

pytestmark = pytest.mark.gpu

LABEL_SENTINEL, AREA_SENTINEL = -77, -55


def _store(dtype, seed=11):
    """every page of the issue in ONE store with junk between them, every page at an ODD element offset (as _store of
    tests/test_binarize_gpu.py): ink is any value that reads as <= 127, background any value that reads as more -> (store, offset, h, w)"""
    g = torch.Generator().manual_seed(seed)
    inks = [ink_pages()[n] for n in NAMES]
    offset, off = [], 1
    for ink in inks:
        off += 1 - off % 2
        offset.append(off)
        off += ink.size + 3
    if dtype == torch.uint8:
        store = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8)
        dark, light = torch.randint(0, 128, (off,), generator=g, dtype=torch.uint8), torch.randint(128, 256, (off,), generator=g, dtype=torch.uint8)
    else:
        store = torch.rand(off, generator=g) * 1.5 - 0.25
        dark, light = torch.rand(off, generator=g) * 0.74 - 0.25, torch.rand(off, generator=g) * 0.74 + 0.51       # read as <= 124 / >= 130
    for o, ink in zip(offset, inks):
        m = torch.from_numpy(ink.reshape(-1))
        store[o:o + ink.size] = torch.where(m, dark[o:o + ink.size], light[o:o + ink.size])
    return store, np.asarray(offset, np.int64), np.asarray([i.shape[0] for i in inks], np.int32), np.asarray([i.shape[1] for i in inks], np.int32)


def _inside(n, offset, h, w):
    inside = torch.zeros(n, dtype=torch.bool)
    for o, hh, ww in zip(offset, h, w):
        inside[int(o):int(o) + int(hh) * int(ww)] = True
    return inside


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_labels_areas_and_despeckle_are_the_statement_bit_for_bit(dtype, connectivity):
    from qea import ops
    store, offset, h, w = _store(dtype)
    for o, name in zip(offset, NAMES):                         # the store reads as the pages
        ink = ink_pages()[name]
        assert np.array_equal(spec.ink_of(store[int(o):int(o) + ink.size].view(ink.shape).numpy()), ink)
    n = store.numel()
    store = store.cuda()
    table = ops.page_table(offset, h, w, store.device)
    labels = torch.full((n,), LABEL_SENTINEL, dtype=torch.int32, device="cuda")
    area = torch.full((n,), AREA_SENTINEL, dtype=torch.int32, device="cuda")
    before = dict(ops.COMPONENT_LAUNCHES)
    ops.cc_label(store, table, connectivity, 127, labels=labels, area=area)
    ops.cc_stats(store, table, labels, area)
    outs = {"u8": torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda"), "float": torch.full((n,), -7.0, device="cuda")}
    ops.cc_despeckle(store, table, labels, area, 4, out_u8=outs["u8"])
    ops.cc_despeckle(store, table, labels, area, 4, out_f32=outs["float"])
    delta = {k: ops.COMPONENT_LAUNCHES[k] - before[k] for k in before}
    assert delta == {"tile": 1, "border": 1, "flatten": 1, "stats": 1, "despeckle": 2, "smear": 0, "boxes": 0}
    labels, area, outs = labels.cpu(), area.cpu(), {k: v.cpu() for k, v in outs.items()}
    for o, name in zip(offset, NAMES):
        want = statement_labels(name, connectivity)
        o, size = int(o), want.size
        assert np.array_equal(labels[o:o + size].view(want.shape).numpy(), want), name
        want_area = np.zeros(size, np.int32)
        roots, counts = np.unique(want[want >= 0], return_counts=True)
        want_area[roots] = counts
        assert np.array_equal(area[o:o + size].numpy(), want_area), name
        for out in ("u8", "float"):
            page = as_page(ink_pages()[name])
            assert np.array_equal(outs[out][o:o + size].view(want.shape).numpy(), spec.despeckle(page, 4, connectivity, out=out, lab=want)), (name, out)
    outside = ~_inside(n, offset, h, w)
    assert bool((labels[outside] == LABEL_SENTINEL).all()) and bool((area[outside] == AREA_SENTINEL).all())
    assert bool((outs["u8"][outside] == 0x5A).all()) and bool((outs["float"][outside] == -7.0).all())


def test_the_launch_sequence_is_fixed():
    from qea import ops
    from qea.binarize import binarize_pages
    from qea.components import despeckle_pages
    pages = {n: torch.from_numpy(as_page(ink_pages()[n])).cuda() for n in NAMES}

    def launches(fn):
        before = dict(ops.COMPONENT_LAUNCHES)
        fn()
        return {k: ops.COMPONENT_LAUNCHES[k] - before[k] for k in before}
    want = {"tile": 1, "border": 1, "flatten": 1, "stats": 1, "despeckle": 1, "smear": 0, "boxes": 0}
    assert launches(lambda: despeckle_pages([pages["rand45"]], 4)) == want
    assert launches(lambda: despeckle_pages(list(pages.values()), 4)) == want
    assert launches(lambda: despeckle_pages([pages["all_bg"]], 4)) == want
    assert launches(lambda: despeckle_pages([pages["serpentine"]], 4)) == want
    before = dict(ops.BINARIZE_LAUNCHES)
    assert launches(lambda: binarize_pages([pages["rand30"]], "sauvola", window=15, despeckle=0)) == dict.fromkeys(want, 0)
    assert {k: ops.BINARIZE_LAUNCHES[k] - before[k] for k in before} == {"sauvola": 1, "histogram": 0, "otsu": 0}
    before = dict(ops.BINARIZE_LAUNCHES)
    assert launches(lambda: binarize_pages([pages["rand30"]], "sauvola", window=15, despeckle=4)) == want
    assert {k: ops.BINARIZE_LAUNCHES[k] - before[k] for k in before} == {"sauvola": 1, "histogram": 0, "otsu": 0}


def seam_pages():
    """each alone: the diagonal through a tile corner, one-pixel lines beside the vertical seam at x = 63 | 64 and two of them four pixels
    apart across it, lines along the horizontal seam at y = 31 | 32, and a 33 x 65 page whose last tiles are one pixel wide and high"""
    def lines(xs=(), ys=(), shape=(100, 130)):
        ink = np.zeros(shape, bool)
        for x in xs:
            ink[:, x] = True
        for y in ys:
            ink[y, :] = True
        return ink
    return {"diagonal": ink_pages()["diagonal"], "x63": lines([63]), "x64": lines([64]), "x63_x64": lines([63, 64]), "x62_x66": lines([62, 66]),
            "y31": lines(ys=[31]), "y32": lines(ys=[32]), "y30_y33": lines(ys=[30, 33]), "cross": lines([64], [31]),
            "checker": ink_pages()["checker"], "full_33x65": np.ones((33, 65), bool)}


@pytest.mark.parametrize("name", sorted(seam_pages()))
def test_tile_seams_alone(name):
    from qea.components import label_pages, page_components
    ink = seam_pages()[name]
    page = torch.from_numpy(as_page(ink)).cuda()
    for connectivity in (4, 8):
        want = spec.labels_of_ink(ink, connectivity)
        assert np.array_equal(label_pages([page], connectivity)[0].cpu().numpy(), want), connectivity
        table = page_components([page], connectivity)[0]
        assert table.is_cuda and np.array_equal(table.cpu().numpy(), spec.table_fast(want)), connectivity
    counts = {"diagonal": (3, 1), "x63": (1, 1), "x64": (1, 1), "x63_x64": (1, 1), "x62_x66": (2, 2), "y31": (1, 1), "y32": (1, 1), "y30_y33": (2, 2),
              "cross": (1, 1), "checker": (1073, 1), "full_33x65": (1, 1)}[name]
    assert (len(spec.table_fast(spec.labels_of_ink(ink, 4))), len(spec.table_fast(spec.labels_of_ink(ink, 8)))) == counts


def test_the_device_path_is_the_host_path():
    """mixed page lists: [1, h, w] floats with values outside [0, 1] and a NaN, and uint8 pages 64 x 64, 65 x 129 and 31 x 1"""
    from qea.components import despeckle_pages, label_pages, page_components, word_boxes
    g = torch.Generator().manual_seed(6)
    floats = [torch.rand(1, 45, 67, generator=g) * 1.5 - 0.25, torch.rand(1, 233, 219, generator=g), torch.rand(1, 1, 300, generator=g)]
    floats[0][0, 2, 3] = float("nan")
    bytes_ = [torch.randint(0, 256, (s, t), generator=g, dtype=torch.uint8) for s, t in ((64, 64), (65, 129), (31, 1))]
    words = [torch.from_numpy(words_page(100, 300, (10, 40, 70), 1)[0]), torch.from_numpy(words_page(64, 129, (3, 33), 2)[0])]

    def same(got, want):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b)
    for pages in (floats, bytes_, words):
        dev = [p.cuda() for p in pages]
        for connectivity, ink_max in ((8, 127), (4, 90)):
            same(label_pages(dev, connectivity, ink_max), label_pages(pages, connectivity, ink_max))
            same(page_components(dev, connectivity, ink_max), page_components(pages, connectivity, ink_max))
            for out in ("u8", "float"):
                same(despeckle_pages(dev, 3, connectivity, ink_max, out=out), despeckle_pages(pages, 3, connectivity, ink_max, out=out))
        for gx, gy, a in ((8, 0, 16), (4, 0, 16), (3, 2, 2), (0, 5, 1), (0, 0, 1), (127, 127, 1)):
            same(word_boxes(dev, gx, gy, a), word_boxes(pages, gx, gy, a))
        same(word_boxes(pages, 4, 1, 4, device="cuda"), word_boxes(pages, 4, 1, 4))
    got = word_boxes([words[0].cuda()], gap_x=4, min_area=16)[0]
    assert np.array_equal(got.cpu().numpy(), words_page(100, 300, (10, 40, 70), 1)[1])


def test_binarize_pages_with_despeckle_on_the_device_is_its_host_run():
    from qea.binarize import binarize_pages
    g = torch.Generator().manual_seed(12)
    pages = [torch.randint(0, 256, (s, t), generator=g, dtype=torch.uint8) for s, t in ((233, 219), (65, 129), (31, 1))]
    for out in ("u8", "float"):
        want = binarize_pages(pages, "sauvola", window=15, despeckle=4, out=out)
        got = binarize_pages([p.cuda() for p in pages], "sauvola", window=15, despeckle=4, out=out)
        plain = binarize_pages(pages, "sauvola", window=15, out=out)
        assert any(not torch.equal(a, b) for a, b in zip(want, plain))
        assert all(a.is_cuda and torch.equal(a.cpu(), b) for a, b in zip(got, want))
    want = binarize_pages(pages, "otsu", despeckle=3, despeckle_connectivity=4, out="u8")
    got = binarize_pages(pages, "otsu", despeckle=3, despeckle_connectivity=4, out="u8", device="cuda")
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))


def test_eval_prep_baseline_despeckle_on_the_device(tmp_path):
    from eval_prep import EvalPrep, build_parser
    from models.model_unet import UNet
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep_host")
    torch.save(UNet().cuda().eval(), tmp_path / "prep")
    flags = ["--ocr", "stub", "--baseline", "sauvola", "--baseline_window", "9", "--baseline_k", "0.3", "--baseline_despeckle", "4"]
    host = EvalPrep(build_parser().parse_args(["--prep_path", str(tmp_path / "prep_host")] + flags), backend=backend, dataset=baseline_docs())
    host.eval()
    dev = EvalPrep(build_parser().parse_args(["--prep_path", str(tmp_path / "prep")] + flags), dataset=baseline_docs())
    dev.eval()
    assert dev.baseline_result == host.baseline_result and dev.baseline_result is not None and dev.baseline_name == "sauvola+despeckle4"


def test_clean_cli_despeckle_and_boxes_on_the_device(tmp_path):
    """--method otsu --despeckle 4 --boxes on the device writes the PNGs and the JSON of the host-backend run"""
    from PIL import Image
    import clean_cli
    backend, _ = host_backend()
    scans_with_words(tmp_path / "in")
    written = {}
    for name, be in (("host", backend), ("device", None)):
        args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"), "--out_dir",
                                                    str(tmp_path / name), "--method", "otsu", "--despeckle", "4", "--boxes", "--boxes_gap", "4",
                                                    "--batch_pages", "2"])
        written[name] = clean_cli.CleanPages(args, backend=be).run()
    assert len(written["device"]) == 3
    for a, b in zip(written["host"], written["device"]):
        with Image.open(a) as x, Image.open(b) as y:
            assert y.mode == "L" and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y))
        with open(a[:-4] + ".json") as x, open(b[:-4] + ".json") as y:
            rows = json.load(y)
            assert rows == json.load(x) and len(rows) > 0


def test_library_refusals_launch_nothing():
    """the C ABI with real device buffers: every refusal returns a negative code and leaves the prefilled buffers untouched; the accepted
    calls then write the page"""
    from qea import _lib, ops
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    page = torch.randint(0, 256, (8, 8), generator=g, dtype=torch.uint8)
    store = page.reshape(-1).cuda()
    table = ops.page_table(np.zeros(1, np.int64), np.asarray([8], np.int32), np.asarray([8], np.int32), store.device)
    labels = torch.full((64,), LABEL_SENTINEL, dtype=torch.int32, device="cuda")
    area = torch.full((64,), AREA_SENTINEL, dtype=torch.int32, device="cuda")
    out = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    outf = torch.full((65,), -7.0, device="cuda")
    mask = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    boxes = torch.full((4, 4), 123, dtype=torch.int32, device="cuda")
    roots = torch.zeros(4, dtype=torch.int32, device="cuda")
    first = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    hh, ww = table.host_h.ctypes.data, table.host_w.ctypes.data
    zero, big_h, big_w = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1 << 14), (C.c_int32 * 1)((1 << 13) + 1)
    sizes = [dict(host_h=zero), dict(host_h=big_h, host_w=big_w), dict(n=0)]

    def lead(n=1, host_h=hh, host_w=ww, tile_first=table.tile_first):
        return (store.data_ptr(), 0, 64, table.offset, table.h, table.w, n, host_h, host_w, tile_first)

    def label(ink_max=127, conn=8, lab=labels.data_ptr(), ar=area.data_ptr(), **kw):
        return L.qea_cc_label(*lead(**kw), None, ink_max, conn, lab, ar, None)

    def stats(lab=labels.data_ptr(), ar=area.data_ptr(), **kw):
        return L.qea_cc_stats(*lead(**kw), lab, ar, None)

    def despeckle(min_area=2, of=None, ou=out.data_ptr(), lab=labels.data_ptr(), ar=area.data_ptr(), **kw):
        return L.qea_cc_despeckle(*lead(**kw), lab, ar, min_area, of, ou, None)

    def smear(ink_max=127, gap=3, vertical=0, om=mask.data_ptr(), **kw):
        return L.qea_cc_smear(*lead(**kw), None, ink_max, gap, vertical, om, None)

    def box(n_roots=1, bx=boxes.data_ptr(), rt=roots.data_ptr(), rf=first.data_ptr(), lab=labels.data_ptr(), **kw):
        return L.qea_cc_boxes(*lead(**kw), lab, rt, rf, n_roots, bx, None)
    for kw in sizes + [dict(tile_first=None), dict(conn=6), dict(conn=0), dict(ink_max=-1), dict(ink_max=255), dict(lab=None),
                       dict(lab=labels.data_ptr() + 2), dict(ar=area.data_ptr() + 1)]:
        assert label(**kw) < 0, kw
    for kw in sizes + [dict(lab=None), dict(ar=None), dict(ar=area.data_ptr() + 2)]:
        assert stats(**kw) < 0, kw
    for kw in sizes + [dict(min_area=0), dict(min_area=-3), dict(ou=None), dict(of=outf.data_ptr() + 2), dict(lab=None), dict(ar=None)]:
        assert despeckle(**kw) < 0, kw
    for kw in sizes + [dict(gap=-1), dict(gap=128), dict(ink_max=255), dict(om=None), dict(vertical=2)]:
        assert smear(**kw) < 0, kw
    for kw in sizes + [dict(n_roots=-1), dict(bx=None), dict(bx=boxes.data_ptr() + 2), dict(rt=None), dict(rf=None), dict(lab=None)]:
        assert box(**kw) < 0, kw
    assert b"qea_cc_boxes" in L.qea_last_error()
    torch.cuda.synchronize()
    assert bool((labels == LABEL_SENTINEL).all()) and bool((area == AREA_SENTINEL).all()) and bool((out == 0x5A).all())
    assert bool((outf == -7.0).all()) and bool((mask == 9).all()) and bool((boxes == 123).all())
    # and the accepted calls write the page
    want = spec.labels(page.numpy(), 8)
    table6 = spec.table_fast(want)
    assert label() == 0 and stats() == 0 and despeckle() == 0 and smear() == 0
    roots = torch.from_numpy(table6[:4, 0].copy()).cuda()
    first = torch.tensor([0, len(roots)], dtype=torch.int32, device="cuda")
    boxes[:, :2], boxes[:, 2:] = 2 ** 31 - 1, -1
    assert box(n_roots=len(roots), rt=roots.data_ptr(), rf=first.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().view(8, 8).numpy(), want)
    assert np.array_equal(out.cpu().view(8, 8).numpy(), spec.despeckle(page.numpy(), 2, 8, lab=want))
    assert np.array_equal(mask.cpu().view(8, 8).numpy() != 0, spec.smear(spec.ink_of(page.numpy()), 3, 0))
    assert np.array_equal(boxes.cpu().numpy()[:len(roots)], table6[:len(roots), 2:])


def test_two_calls_give_the_same_labels():
    """the statement already implies it: no ordering leaks through"""
    from qea.components import label_pages
    page = torch.from_numpy(as_page(ink_pages()["rand45"])).cuda()
    a, b = label_pages([page])[0], label_pages([page])[0]
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), statement_labels("rand45", 8))
