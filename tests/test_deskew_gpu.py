"""Page skew estimation and deskew on the MI355X (csrc/deskew.hip): strip sums, scores, slopes and rotated pages bit for bit the statement
tests/deskew_spec.py over a ragged store with junk between the pages, the fixed launch sequence, the pick on hand-made scores, per-page
ink from the device's Otsu thresholds, the product's device path against its host path, the front end against its host-backend run, and
the refusals of the C ABI."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import binarize_spec as bspec
import deskew_spec as spec
from test_binarize_cpu import host_backend
from test_deskew_cpu import LARGE_A, NAMES, cli_args, float_pages, large_pages, large_statement, norm, score_rows, skewed_scans, statement, u8_pages

pytestmark = pytest.mark.gpu

C_SENTINEL, SCORE_SENTINEL, SLOPE_SENTINEL = 0xA5, -1234567, -77


def _store(kind, seed=11):
    """every page of the issue in ONE store with junk between them, every page at an ODD element offset, the last page ending with the
    store, and the store itself starting three elements into its allocation -> (store on the host, offset, h, w)"""
    g = torch.Generator().manual_seed(seed)
    pages = [(u8_pages() if kind == "u8" else float_pages())[n] for n in NAMES]
    offset, off = [], 1
    for px in pages:
        off += 1 - off % 2
        offset.append(off)
        off += px.size + 2
    off -= 2
    whole = torch.randint(0, 256, (off + 3,), generator=g, dtype=torch.uint8) if kind == "u8" else torch.rand(off + 3, generator=g) * 1.5 - 0.25
    store = whole[3:]
    for o, px in zip(offset, pages):
        store[o:o + px.size] = torch.from_numpy(px.reshape(-1))
    return store, np.asarray(offset, np.int64), np.asarray([p.shape[0] for p in pages], np.int32), np.asarray([p.shape[1] for p in pages], np.int32)


def _on_device(store):
    """a device copy that keeps the three-element lead, so that the store's first byte is not 16-byte aligned"""
    whole = torch.empty(store.numel() + 3, dtype=store.dtype).copy_(torch.cat([store[:3], store]))
    return whole.cuda()[3:]


def _launches(before):
    from qea import ops
    return {k: ops.DESKEW_LAUNCHES[k] - before[k] for k in before}


@pytest.mark.parametrize("A", [0, 100, 256])
@pytest.mark.parametrize("kind", ["u8", "float"])
def test_sums_scores_slopes_and_pages_are_the_statement_bit_for_bit(kind, A):
    from qea import ops
    from qea.deskew import rotation_table
    host, offset, h, w = _store(kind)
    pages = u8_pages() if kind == "u8" else float_pages()
    n = host.numel()
    store = _on_device(host)
    assert store.data_ptr() % 16 != 0 and store.is_contiguous()
    table = ops.page_table(offset, h, w, store.device)
    Cs = torch.full((n,), C_SENTINEL, dtype=torch.uint8, device="cuda")
    scores = torch.full((len(NAMES), 2 * A + 1), SCORE_SENTINEL, dtype=torch.int64, device="cuda")
    slopes = torch.full((len(NAMES),), SLOPE_SENTINEL, dtype=torch.int32, device="cuda")
    out_u8 = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    rot = torch.from_numpy(rotation_table(A)).cuda()
    before = dict(ops.DESKEW_LAUNCHES)
    ops.skew_strip_sums(store, table, 127, C=Cs)
    ops.skew_scores(Cs, table, A, scores=scores)
    ops.skew_pick(scores, 0, slopes=slopes)
    ops.deskew_rotate(store, table, slopes, rot, "bilinear", 255, out_u8=out_u8)
    assert _launches(before) == {"strip_sums": 1, "scores": 1, "pick": 1, "rotate": 1}
    out_f = torch.full((n,), -7.0, device="cuda")
    ops.deskew_rotate(store, table, slopes, rot, "nearest", 7, norm=torch.from_numpy(norm()).cuda(), out_f32=out_f)
    both_u8, both_f = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((n,), -7.0, device="cuda")
    ops.deskew_rotate(store, table, slopes, rot, "bilinear", 7, norm=torch.from_numpy(norm()).cuda(), out_f32=both_f, out_u8=both_u8)
    Cs, scores, slopes, out_u8, out_f, both_u8, both_f = (t.cpu() for t in (Cs, scores, slopes, out_u8, out_f, both_u8, both_f))
    rtable = spec.rotation_table(A)
    written_C, inside = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    for i, (o, name) in enumerate(zip(offset, NAMES)):
        o, px = int(o), pages[name]
        a, S, _ = statement(kind, name, A, 127)
        want_C = spec.strip_sums(px, 127)
        assert np.array_equal(Cs[o:o + want_C.size].view(want_C.shape).numpy(), want_C), name
        assert scores[i].tolist() == S, name
        assert int(slopes[i]) == a, name
        assert np.array_equal(out_u8[o:o + px.size].view(px.shape).numpy(), spec.rotate(px, a, rtable)), name
        assert np.array_equal(out_f[o:o + px.size].view(px.shape).numpy(), spec.rotate(px, a, rtable, "nearest", 7, "float", norm())), name
        want = spec.rotate(px, a, rtable, "bilinear", 7)
        assert np.array_equal(both_u8[o:o + px.size].view(px.shape).numpy(), want) and np.array_equal(both_f[o:o + px.size].view(px.shape).numpy(), norm()[want])
        written_C[o:o + want_C.size] = True
        inside[o:o + px.size] = True
    assert bool((Cs[~written_C] == C_SENTINEL).all())
    assert bool((out_u8[~inside] == 0x5A).all()) and bool((out_f[~inside] == -7.0).all())
    assert bool((both_u8[~inside] == 0x5A).all()) and bool((both_f[~inside] == -7.0).all())


def test_where_32_bits_overflow():
    """20011 columns or rows (X, Y past 2^31) and a score of 4.8e9, in one store, against the statement"""
    from qea import ops
    from qea.deskew import rotation_table
    from qea.pages import pack_pages
    names = sorted(large_pages())
    pk = pack_pages([torch.from_numpy(large_pages()[n]) for n in names])
    store = pk.store.cuda()
    table = ops.page_table(pk.offset, pk.h, pk.w, store.device)
    scores = ops.skew_scores(ops.skew_strip_sums(store, table, 127), table, LARGE_A)
    slopes = ops.skew_pick(scores)
    rot = torch.from_numpy(rotation_table(LARGE_A)).cuda()
    lo, hi = torch.empty_like(store), torch.empty_like(store)
    ops.deskew_rotate(store, table, torch.full((3,), -LARGE_A, dtype=torch.int32, device="cuda"), rot, "bilinear", 9, out_u8=lo)
    ops.deskew_rotate(store, table, torch.full((3,), LARGE_A, dtype=torch.int32, device="cuda"), rot, "nearest", 9, out_u8=hi)
    scores, slopes, lo, hi = scores.cpu(), slopes.cpu(), lo.cpu(), hi.cpu()
    for i, (o, n) in enumerate(zip(pk.offset, names)):
        a, S, want_lo, want_hi = large_statement(n)
        assert scores[i].tolist() == S and int(slopes[i]) == a, n
        o = int(o)
        assert np.array_equal(lo[o:o + want_lo.size].view(want_lo.shape).numpy(), want_lo), n
        assert np.array_equal(hi[o:o + want_hi.size].view(want_hi.shape).numpy(), want_hi), n
    assert max(large_statement("stripes_300x4000")[1]) > 2 ** 32


def test_pick_on_hand_made_scores():
    from qea import ops
    for g in sorted({g for _, g, _ in score_rows()}):
        rows = [(r, want) for r, gg, want in score_rows() if gg == g]
        before = dict(ops.DESKEW_LAUNCHES)
        got = ops.skew_pick(torch.tensor([r for r, _ in rows], dtype=torch.int64, device="cuda"), g)
        assert _launches(before) == {"strip_sums": 0, "scores": 0, "pick": 1, "rotate": 0}
        assert got.dtype == torch.int32 and got.cpu().tolist() == [want for _, want in rows], g
    # rows wider than a wave, few distinct values: ties everywhere, against the statement
    rng = np.random.default_rng(2)
    for A, g in ((100, 0), (256, 0), (256, 50), (40, 300)):
        rows = rng.integers(0, 4, (33, 2 * A + 1)) * 1000
        rows[0] = 5
        rows[1, 2 * A], rows[2, 0] = 9000, 9000
        got = ops.skew_pick(torch.from_numpy(rows).cuda(), g).cpu().tolist()
        assert got == [spec.pick(r.tolist(), g) for r in rows], (A, g)
        assert got[0] == 0 and (g or (got[1], got[2]) == (A, -A))


def test_per_page_ink_comes_from_the_device_otsu_thresholds():
    """the thresholds tensor qea_binarize_otsu wrote is the strip-sum kernel's ink_max: -1 for the page of one grey level"""
    from qea import ops
    for kind in ("u8", "float"):
        host, offset, h, w = _store(kind)
        pages = u8_pages() if kind == "u8" else float_pages()
        store = _on_device(host)
        table = ops.page_table(offset, h, w, store.device)
        scratch = torch.empty(host.numel(), dtype=torch.uint8, device="cuda")
        thresholds = ops.binarize_otsu(store, table, ops.otsu_histogram(store, table), out_u8=scratch)
        assert thresholds.is_cuda
        Cs = ops.skew_strip_sums(store, table, thresholds).cpu()
        want_t = [bspec.otsu_threshold(pages[n]) for n in NAMES]
        assert thresholds.cpu().tolist() == want_t and -1 in want_t and len(set(want_t)) > 3
        for o, name, t in zip(offset, NAMES, want_t):
            want = spec.strip_sums(pages[name], t)
            assert np.array_equal(Cs[int(o):int(o) + want.size].view(want.shape).numpy(), want), name


def test_the_device_path_is_the_host_path():
    """one 400 x 512 text page and the ragged list, uint8 and float pages, both outputs"""
    from qea import ops
    from qea.deskew import deskew_pages, estimate_skew
    text = torch.from_numpy(spec.sheared_text_page(-37, 1))
    lists = [[text], [torch.from_numpy(u8_pages()[n]) for n in NAMES],
             [torch.from_numpy(float_pages()[n][None] if i % 2 else float_pages()[n]) for i, n in enumerate(NAMES)]]
    for pages in lists:
        dev = [p.cuda() for p in pages]
        for kw in (dict(), dict(max_slope=256, ink=60, min_gain=3, interp="nearest", fill=0, out="float")):
            want, want_slopes = deskew_pages(pages, **kw)
            before = dict(ops.DESKEW_LAUNCHES)
            got, slopes = deskew_pages(dev, **kw)
            assert _launches(before) == {"strip_sums": 1, "scores": 1, "pick": 1, "rotate": 1}
            assert slopes.is_cuda and torch.equal(slopes.cpu(), want_slopes)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b)
        est = {k: v for k, v in kw.items() if k in ("max_slope", "ink", "min_gain")}
        for a, b in zip(estimate_skew(pages, device="cuda", **est), estimate_skew(pages, **est)):
            assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b)
        got, slopes = deskew_pages(pages, slopes=[5] * len(pages), device="cuda")
        want, _ = deskew_pages(pages, slopes=[5] * len(pages))
        assert slopes.cpu().tolist() == [5] * len(pages) and all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
    assert int(deskew_pages([text.cuda()])[1][0]) == spec.estimate(text.numpy(), 90, bspec.otsu_threshold(text.numpy()))[0] != 0


def test_clean_cli_deskew_on_the_device(tmp_path, capsys):
    """--method otsu --deskew --boxes on the device writes the PNGs, the JSON and the slope lines of the host-backend run"""
    from PIL import Image
    import clean_cli
    backend, _ = host_backend()
    skewed_scans(tmp_path / "in")
    written, printed = {}, {}
    for name, be in (("host", backend), ("device", None)):
        args = cli_args(tmp_path, name, "--method", "otsu", "--deskew", "--deskew_max_slope", "100", "--boxes", "--boxes_gap", "4")
        written[name] = clean_cli.CleanPages(args, backend=be).run()
        printed[name] = [l for l in capsys.readouterr().out.splitlines() if "slope" in l]
    assert len(written["device"]) == 3 and printed["device"] == printed["host"] and len(printed["host"]) == 3
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
    from qea.deskew import rotation_table
    L = _lib.lib()
    page = spec.sheared_text_page(61, 2, 40, 45)
    store = torch.from_numpy(page.reshape(-1)).cuda()
    n = store.numel()
    table = ops.page_table(np.zeros(1, np.int64), np.asarray([40], np.int32), np.asarray([45], np.int32), store.device)
    Cs = torch.full((n,), C_SENTINEL, dtype=torch.uint8, device="cuda")
    scores = torch.full((1, 181), SCORE_SENTINEL, dtype=torch.int64, device="cuda")
    slopes = torch.full((1,), SLOPE_SENTINEL, dtype=torch.int32, device="cuda")
    out = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    outf = torch.full((n + 1,), -7.0, device="cuda")
    rot, nrm = torch.from_numpy(rotation_table(90)).cuda(), torch.from_numpy(norm()).cuda()
    given = torch.tensor([61], dtype=torch.int32, device="cuda")
    hh, ww = table.host_h.ctypes.data, table.host_w.ctypes.data
    one = lambda v: (C.c_int32 * 1)(v)
    sizes = [dict(host_h=one(0)), dict(host_h=one(32768)), dict(host_w=one(32768)), dict(host_h=one(1 << 14), host_w=one((1 << 13) + 1)), dict(n=0)]

    def lead(n=1, host_h=hh, host_w=ww):
        return (store.data_ptr(), 0, store.numel(), table.offset, table.h, table.w, n, host_h, host_w)

    def sums(dev=None, ink_max=127, Cp=Cs.data_ptr(), **kw):
        return L.qea_skew_strip_sums(*lead(**kw), dev, ink_max, Cp, None)

    def score(A=90, Cp=Cs.data_ptr(), sc=scores.data_ptr(), **kw):
        return L.qea_skew_scores(Cp, *lead(**kw)[2:], A, sc, None)

    def pick(A=90, g=0, sc=scores.data_ptr(), sl=slopes.data_ptr(), n=1):
        return L.qea_skew_pick(sc, n, A, g, sl, None)

    def rotate(A=90, nearest=0, fill=255, sl=given.data_ptr(), tb=rot.data_ptr(), nm=nrm.data_ptr(), of=None, ou=out.data_ptr(),
               tile_first=table.tile_first, **kw):
        return L.qea_deskew_rotate(*lead(**kw), tile_first, sl, tb, A, nearest, fill, nm, of, ou, None)
    for kw in sizes + [dict(ink_max=-1), dict(ink_max=255), dict(Cp=None), dict(Cp=store.data_ptr()), dict(Cp=store.data_ptr() + n - 1)]:
        assert sums(**kw) < 0, kw
    for kw in sizes + [dict(A=-1), dict(A=257), dict(Cp=None), dict(sc=None), dict(sc=scores.data_ptr() + 4)]:
        assert score(**kw) < 0, kw
    for kw in [dict(A=-1), dict(A=257), dict(g=-1), dict(g=10001), dict(sc=None), dict(sl=None), dict(sl=slopes.data_ptr() + 2), dict(n=0)]:
        assert pick(**kw) < 0, kw
    for kw in sizes + [dict(A=257), dict(A=-1), dict(nearest=2), dict(fill=256), dict(fill=-1), dict(sl=None), dict(tb=None), dict(tile_first=None),
                       dict(ou=None), dict(ou=None, of=outf.data_ptr() + 2), dict(ou=None, of=outf.data_ptr(), nm=None),
                       dict(ou=store.data_ptr()), dict(ou=store.data_ptr() + n - 1), dict(ou=store.data_ptr() - n + 1)]:
        assert rotate(**kw) < 0, kw
    assert b"qea_deskew_rotate" in L.qea_last_error() and b"overlaps" in L.qea_last_error()
    torch.cuda.synchronize()
    assert bool((Cs == C_SENTINEL).all()) and bool((scores == SCORE_SENTINEL).all()) and bool((slopes == SLOPE_SENTINEL).all())
    assert bool((out == 0x5A).all()) and bool((outf == -7.0).all()) and np.array_equal(store.cpu().numpy().reshape(page.shape), page)
    # and the accepted calls write the page
    assert sums() == 0 and score() == 0 and pick() == 0
    assert rotate(sl=slopes.data_ptr()) == 0 and rotate(sl=slopes.data_ptr(), ou=None, of=outf.data_ptr(), nearest=1, fill=3) == 0
    torch.cuda.synchronize()
    a, S = spec.estimate(page, 90, 127)
    want_C = spec.strip_sums(page, 127)
    assert np.array_equal(Cs.cpu()[:want_C.size].view(want_C.shape).numpy(), want_C) and bool((Cs[want_C.size:] == C_SENTINEL).all())
    assert scores.cpu()[0].tolist() == S and slopes.cpu().tolist() == [a] and a != 0
    assert np.array_equal(out.cpu().view(page.shape).numpy(), spec.rotate(page, a, spec.rotation_table(90)))
    assert np.array_equal(outf.cpu()[:n].view(page.shape).numpy(), spec.rotate(page, a, spec.rotation_table(90), "nearest", 3, "float", norm()))
    assert float(outf[n]) == -7.0
