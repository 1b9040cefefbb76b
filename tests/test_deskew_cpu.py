"""Page skew estimation and deskew without a GPU: the product's host path (qea/deskew.py) against the statement tests/deskew_spec.py bit for
bit, the tie and gate rules on hand-made scores, the statement's recall on sheared text, the taps of the rotation one by one, the refusals,
the header and the clean_cli front end on the host backend."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import binarize_spec as bspec
import components_spec as cspec
import deskew_spec as spec
from test_binarize_cpu import host_backend

SIZES = [(1, 1), (1, 40), (2, 33), (37, 31), (64, 70), (96, 160), (130, 257)]


def u8_pages():
    """name -> uint8 page: every size of SIZES with text bars or noise, plus a page that is all ink and one of a single grey level"""
    rng = np.random.default_rng(17)
    pages = {f"noise_{h}x{w}": rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in SIZES}
    for (h, w), k, seed in (((37, 31), 61, 3), ((64, 70), -90, 4), ((96, 160), -37, 5), ((130, 257), 22, 6)):
        pages[f"text_{h}x{w}"] = spec.sheared_text_page(k, seed, h, w)
    pages["all_ink_37x31"] = np.zeros((37, 31), np.uint8)
    pages["no_ink_64x70"] = np.full((64, 70), 255, np.uint8)
    pages["dark_row_2x33"] = np.asarray([[0] * 33, [255] * 33], np.uint8)
    return pages


def float_pages():
    """the same pages as floats that read as other 8-bit values: noise outside [0, 1] and a NaN among them"""
    rng = np.random.default_rng(18)
    out = {}
    for name, px in u8_pages().items():
        f = (px.astype(np.float32) / np.float32(255) if "noise" not in name
             else (rng.random(px.shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)))
        if name == "noise_64x70":
            f[3, 5] = np.nan
        out[name] = f
    return out


NAMES = sorted(u8_pages())
_cache = {}


def statement(kind, name, A, ink):
    """(a*, scores, ink_max) of the statement for one page, computed once and shared by the tests (the GPU tests use it too)"""
    key = (kind, name, A, ink)
    if key not in _cache:
        page = (u8_pages() if kind == "u8" else float_pages())[name]
        ink_max = bspec.otsu_threshold(page) if ink == "otsu" else ink
        _cache[key] = spec.estimate(page, A, ink_max) + (ink_max,)
    return _cache[key]


def norm():
    from qea.pages import norm_table
    return norm_table().numpy()


def test_the_pages_cover_the_sizes_and_contents():
    pages = u8_pages()
    assert {p.shape for p in pages.values()} == set(SIZES)
    assert bspec.otsu_threshold(pages["no_ink_64x70"]) == -1 and statement("u8", "no_ink_64x70", 100, "otsu")[:2] == (0, [0] * 201)
    assert any(statement("u8", n, 100, 127)[0] != 0 for n in NAMES)
    assert np.isnan(float_pages()["noise_64x70"]).sum() == 1


@pytest.mark.parametrize("A", [0, 100, 256])
@pytest.mark.parametrize("ink", [127, 60, "otsu"])
@pytest.mark.parametrize("kind", ["u8", "float"])
def test_host_estimate_is_the_statement(kind, ink, A):
    """scalar ink_max and the per-page one of Otsu; all pages in ONE call"""
    from qea.deskew import estimate_skew
    pages = u8_pages() if kind == "u8" else float_pages()
    slopes, scores = estimate_skew([torch.from_numpy(pages[n]) for n in NAMES], A, ink)
    assert slopes.dtype == torch.int32 and scores.dtype == torch.int64 and scores.shape == (len(NAMES), 2 * A + 1)
    for i, n in enumerate(NAMES):
        a, S, _ = statement(kind, n, A, ink)
        assert scores[i].tolist() == S, n
        assert int(slopes[i]) == a, n


def test_host_strip_sums_are_the_statement():
    from qea.deskew import _strip_sums_host
    for n, px in u8_pages().items():
        for ink_max in (-1, 0, 127, 254):
            assert np.array_equal(_strip_sums_host(px, ink_max), spec.strip_sums(px, ink_max)), (n, ink_max)


@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
@pytest.mark.parametrize("kind", ["u8", "float"])
def test_host_rotation_is_the_statement(kind, interp):
    """estimated slopes, and given ones at both ends of the table, to both output kinds, with two fills"""
    from qea.deskew import deskew_pages
    pages = u8_pages() if kind == "u8" else float_pages()
    tensors = [torch.from_numpy(pages[n][None] if kind == "float" and i % 2 else pages[n]) for i, n in enumerate(NAMES)]
    for A, fill, out in ((100, 255, "u8"), (256, 7, "float")):
        table = spec.rotation_table(A)
        got, slopes = deskew_pages(tensors, A, 127, interp=interp, fill=fill, out=out)
        for i, n in enumerate(NAMES):
            a = statement(kind, n, A, 127)[0]
            assert int(slopes[i]) == a and got[i].shape == tensors[i].shape
            want = spec.rotate(pages[n], a, table, interp, fill, out, norm())
            assert got[i].dtype == (torch.uint8 if out == "u8" else torch.float32)
            assert np.array_equal(got[i].numpy().reshape(want.shape), want), (n, A)
        for given in (-A, A, 13):
            got, slopes = deskew_pages(tensors, A, interp=interp, fill=fill, out=out, slopes=[given] * len(NAMES))
            assert slopes.tolist() == [given] * len(NAMES)
            for i, n in enumerate(NAMES):
                want = spec.rotate(pages[n], given, table, interp, fill, out, norm())
                assert np.array_equal(got[i].numpy().reshape(want.shape), want), (n, given)


def large_pages():
    """the sizes at which 32 bits overflow: X and Y pass 2^31 from 16384 columns or rows on (65536 (w - 1) alone), and a score passes 2^32
    where full rows of ink alternate with empty ones on a wide page (h w^2 = 300 * 4000^2 = 4.8e9)"""
    rng = np.random.default_rng(23)
    stripes = np.full((300, 4000), 255, np.uint8)
    stripes[::2] = 0
    return {"wide_3x20011": rng.integers(0, 256, (3, 20011), dtype=np.uint8), "tall_20011x3": rng.integers(0, 256, (20011, 3), dtype=np.uint8),
            "stripes_300x4000": stripes}


LARGE_A = 20
_large = {}


def large_statement(name):
    """-> (a*, scores, the page rotated by -LARGE_A bilinearly and by LARGE_A to the nearest pixel), computed once"""
    if name not in _large:
        page, table = large_pages()[name], spec.rotation_table(LARGE_A)
        _large[name] = spec.estimate(page, LARGE_A, 127) + (spec.rotate(page, -LARGE_A, table, "bilinear", 9),
                                                            spec.rotate(page, LARGE_A, table, "nearest", 9))
    return _large[name]


def test_host_path_where_32_bits_overflow():
    from qea.deskew import deskew_pages, estimate_skew
    names = sorted(large_pages())
    pages = [torch.from_numpy(large_pages()[n]) for n in names]
    slopes, scores = estimate_skew(pages, LARGE_A, 127)
    lo, _ = deskew_pages(pages, LARGE_A, fill=9, slopes=[-LARGE_A] * 3)
    hi, _ = deskew_pages(pages, LARGE_A, interp="nearest", fill=9, slopes=[LARGE_A] * 3)
    for i, n in enumerate(names):
        a, S, want_lo, want_hi = large_statement(n)
        assert int(slopes[i]) == a and scores[i].tolist() == S, n
        assert np.array_equal(lo[i].numpy(), want_lo) and np.array_equal(hi[i].numpy(), want_hi), n
    assert max(large_statement("stripes_300x4000")[1]) == 299 * 4000 ** 2 > 2 ** 32 and large_statement("stripes_300x4000")[0] == 0
    assert 65536 * 20010 > 2 ** 30 and (large_statement("wide_3x20011")[2] != 9).any()


def test_rotation_table_is_the_statements():
    from qea.deskew import rotation_table
    for A in (0, 90, 256):
        t = rotation_table(A)
        assert t.dtype == np.int32 and np.array_equal(t, spec.rotation_table(A))
        assert t[A].tolist() == [65536, 0] and np.array_equal(t[::-1, 0], t[:, 0]) and np.array_equal(t[::-1, 1], -t[:, 1])
    t = spec.rotation_table(256)                               # tan = 1 / 4: cos = 4 / sqrt(17), sin = 1 / sqrt(17)
    assert t[512].tolist() == [round(65536 * 4 / 17 ** 0.5), round(65536 / 17 ** 0.5)]


def score_rows():
    """hand-made rows of 2 A + 1 = 7 scores, the gate g -> the pick"""
    return [
        ([5, 9, 1, 2, 1, 9, 5], 0, -2),            # equal maxima at -2 and +2: the negative one
        ([9, 5, 1, 2, 1, 9, 5], 0, 2),             # equal maxima at -3 and +2: the smaller |a|
        ([1, 9, 1, 9, 1, 9, 1], 0, 0),             # a maximum at 0 against equal ones elsewhere: 0
        ([0, 0, 0, 0, 0, 0, 0], 0, 0),             # no ink
        ([1, 2, 3, 4, 5, 6, 7], 0, 3),
        ([7, 2, 3, 4, 5, 6, 1], 0, -3),
        ([0, 0, 0, 200, 0, 250, 0], 25, 2),        # 100 (250 - 200) = 25 * 200: exactly at the boundary, kept
        ([0, 0, 0, 200, 0, 250, 0], 26, 0),        # one above it: dropped
        ([0, 0, 0, 200, 0, 249, 0], 25, 0),        # one score below the boundary: dropped
        ([0, 0, 0, 0, 0, 1, 0], 10000, 2),         # S_0 = 0: every gate passes
        ([0, 0, 0, 1 << 44, 0, 101 << 44, 0], 10000, 2),       # 100 (S - S_0) = g S_0 = 2^44 10^6: past 32 and 53 bits
        ([0, 0, 0, 1 << 44, 0, (101 << 44) - 1, 0], 10000, 0),
    ]


def test_tie_and_gate_rules_on_hand_made_scores():
    from qea.deskew import pick_slopes
    for row, g, want in score_rows():
        assert spec.pick(row, g) == want, (row, g)
        assert pick_slopes(np.asarray([row], np.int64), g).tolist() == [want], (row, g)
    assert spec.pick([4], 0) == 0 and pick_slopes(np.asarray([[4], [0]]), 5).tolist() == [0, 0]
    rows = np.asarray([r for r, g, _ in score_rows() if g == 0], np.int64)
    assert pick_slopes(rows).tolist() == [w for _, g, w in score_rows() if g == 0]
    assert pick_slopes(torch.from_numpy(rows)).dtype == np.int32


RECALL_SLOPES, RECALL_SEEDS = (-80, -37, -5, 0, 3, 22, 61, 90), (0, 1, 2)


def test_recall_of_the_statement_on_sheared_text():
    """400 x 512 pages of bars sheared per column by k / 1024: |a* - k| <= ceil(2048 / w) = 4, one pixel of shift at the page edge, and the
    same bound for the estimate on the rotated page; the seeds are fixed, the bound is the issue's"""
    h, w, A = 400, 512, 100
    bound = -(-2048 // w)
    table = spec.rotation_table(A)
    for seed in RECALL_SEEDS:
        for k in RECALL_SLOPES:
            page = spec.sheared_text_page(k, seed, h, w)
            a = spec.estimate(page, A, 127)[0]
            assert abs(a - k) <= bound, (seed, k, a)
            again = spec.estimate(spec.rotate(page, a, table), A, 127)[0]
            assert abs(again) <= bound, (seed, k, a, again)


def test_rotation_by_zero_is_the_identity():
    from qea.deskew import deskew_pages
    for kind, pages in (("u8", u8_pages()), ("float", float_pages())):
        for interp in ("bilinear", "nearest"):
            got, _ = deskew_pages([torch.from_numpy(pages[n]) for n in NAMES], 90, interp=interp, fill=3, slopes=[0] * len(NAMES))
            for n, g in zip(NAMES, got):
                assert np.array_equal(g.numpy(), spec.to_u8(pages[n])), (kind, n)
                assert np.array_equal(spec.rotate(pages[n], 0, spec.rotation_table(90), interp, 3), spec.to_u8(pages[n]))
    got, slopes = deskew_pages([torch.from_numpy(u8_pages()["text_130x257"])], max_slope=0)         # A = 0: only the identity is a candidate
    assert slopes.tolist() == [0] and np.array_equal(got[0].numpy(), u8_pages()["text_130x257"])


def rotate_by_hand(page, a, table, fill):
    """the bilinear rule pixel by pixel in Python integers -> (the image, which taps carried weight onto the page, and at which edges
    a tap with weight fell outside)"""
    h, w = page.shape
    A = len(table) // 2
    C16, S16 = int(table[a + A][0]), int(table[a + A][1])
    out, used, edges = np.zeros((h, w), np.uint8), set(), set()
    for y in range(h):
        for x in range(w):
            dx2, dy2 = 2 * x - (w - 1), 2 * y - (h - 1)
            X, Y = C16 * dx2 - S16 * dy2 + 65536 * (w - 1), S16 * dx2 + C16 * dy2 + 65536 * (h - 1)
            x0, y0, fx, fy = X >> 17, Y >> 17, (X >> 9) & 255, (Y >> 9) & 255
            acc = 32768
            for tap, (yy, xx, wgt) in enumerate(((y0, x0, (256 - fx) * (256 - fy)), (y0, x0 + 1, fx * (256 - fy)), (y0 + 1, x0, (256 - fx) * fy),
                                                 (y0 + 1, x0 + 1, fx * fy))):
                inside = 0 <= yy < h and 0 <= xx < w
                acc += wgt * (int(page[yy, xx]) if inside else fill)
                if wgt and inside and page[yy, xx] != fill:
                    used.add(tap)
                if wgt and not inside:
                    edges |= {e for e, c in (("left", xx < 0), ("right", xx >= w), ("top", yy < 0), ("bottom", yy >= h)) if c}
            out[y, x] = acc >> 16
    return out, used, edges


@pytest.mark.parametrize("a", [-256, 256, -90, 90])
def test_one_ink_pixel_lands_in_the_taps_the_statement_names(a):
    """one dark pixel on a page of the fill value: every output pixel is decided by the weight of the single tap that meets it; and an
    all-dark page against a light fill: the edges are decided by the taps that leave the page, at all four edges"""
    from qea.deskew import deskew_pages
    table = spec.rotation_table(256)
    for fill, ink in ((255, 0), (9, 200)):
        seen = set()
        for py, px in ((4, 5), (0, 0), (8, 10), (2, 9)):
            page = np.full((9, 11), fill, np.uint8)
            page[py, px] = ink
            want, used, _ = rotate_by_hand(page, a, table, fill)
            seen |= used
            assert np.array_equal(spec.rotate(page, a, table, "bilinear", fill), want)
            assert np.array_equal(deskew_pages([torch.from_numpy(page)], 256, fill=fill, slopes=[a])[0][0].numpy(), want)
            assert (py, px) != (4, 5) or (want != fill).sum() >= 1
        assert seen == {0, 1, 2, 3}
    page = np.full((9, 11), 30, np.uint8)
    want, _, edges = rotate_by_hand(page, a, table, 250)
    assert edges == {"left", "right", "top", "bottom"} and want[4, 5] == 30 and want.max() > 30
    assert np.array_equal(spec.rotate(page, a, table, "bilinear", 250), want)
    assert np.array_equal(deskew_pages([torch.from_numpy(page)], 256, fill=250, slopes=[a])[0][0].numpy(), want)


def test_shifts_floor_and_use_w_div_2():
    assert spec.shift(0, 3, 31) == (3 * 1 + 512) // 1024 == 0 and spec.shift(0, -90, 257) == (-90 * (16 - 128) + 512) // 1024 == 10
    assert spec.shift(0, 100, 257) == (100 * -112 + 512) // 1024 == -11        # a negative numerator: C's / would give -10
    assert int(-10688 / 1024) == -10
    assert spec.shift(8, 256, 257) == 36 and spec.shift(2, 1, 33) == 0 and spec.shift(1, 256, 33) == (256 * 32 + 512) // 1024 == 8


def test_refusals_of_the_product_module():
    from qea._lib import QeaError
    from qea.deskew import check_params, deskew_pages, estimate_skew, rotation_table
    page = torch.zeros(4, 4, dtype=torch.uint8)
    for kw in (dict(max_slope=-1), dict(max_slope=257), dict(max_slope=1.5), dict(max_slope=True), dict(ink=255), dict(ink=-1), dict(ink="sauvola"),
               dict(ink=12.0), dict(min_gain=-1), dict(min_gain=10001), dict(min_gain=0.5), dict(interp="cubic"), dict(fill=256), dict(fill=-1),
               dict(fill=1.0)):
        with pytest.raises(ValueError):
            check_params(**kw)
        with pytest.raises(ValueError):
            deskew_pages([page], **kw)
    check_params(256, 0, 10000, "nearest", 0)
    with pytest.raises(ValueError):
        estimate_skew([page], max_slope=300)
    with pytest.raises(ValueError):
        deskew_pages([page], out="int")
    with pytest.raises(ValueError):
        deskew_pages([])
    with pytest.raises(ValueError):
        rotation_table(257)
    for bad in ([91], [0, 0], [1.0], [-91]):
        with pytest.raises(ValueError):
            deskew_pages([page], 90, slopes=bad)
    with pytest.raises(QeaError, match="32767"):
        estimate_skew([torch.zeros(1, 1, dtype=torch.uint8).expand(2, 32768)])
    with pytest.raises(QeaError, match="2\\^27"):
        estimate_skew([torch.zeros(1, 1, dtype=torch.uint8).expand(1 << 14, (1 << 13) + 1)])


def test_abi_and_ops():
    """the four symbols are in the header and in the built library; the library refuses bad arguments before any launch"""
    from qea import _lib, ops
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    sizes = {"qea_skew_strip_sums": 13, "qea_skew_scores": 11, "qea_skew_pick": 6, "qea_deskew_rotate": 19}
    L = _lib.lib()
    for name, n in sizes.items():
        assert len(protos[name]) == n and hasattr(L, name), name
    assert L.qea_version() == 9
    assert set(ops.DESKEW_LAUNCHES) == {"strip_sums", "scores", "pick", "rotate"}
    assert (ops.DESKEW_MAX_SIDE, ops.DESKEW_MAX_SLOPE, ops.DESKEW_MAX_GAIN) == (spec.MAX_SIDE, spec.MAX_SLOPE, spec.MAX_GAIN)
    one, two, odd = C.c_void_p(256), C.c_void_p(1 << 20), C.c_void_p(258)
    hh, ww = (C.c_int32 * 1)(4), (C.c_int32 * 1)(4)

    def sums(store=one, n=1, host_h=hh, host_w=ww, dev=None, ink_max=127, Cp=two):
        return L.qea_skew_strip_sums(store, 0, 16, one, one, one, n, host_h, host_w, dev, ink_max, Cp, None)
    for kw in (dict(store=None), dict(n=0), dict(host_h=(C.c_int32 * 1)(0)), dict(ink_max=-1), dict(ink_max=255), dict(Cp=None), dict(Cp=one),
               dict(dev=odd), dict(host_w=(C.c_int32 * 1)(32768)), dict(host_h=(C.c_int32 * 1)(1 << 14), host_w=(C.c_int32 * 1)((1 << 13) + 1))):
        assert sums(**kw) < 0, kw
        assert b"qea_skew_strip_sums" in L.qea_last_error(), kw
    assert b"2^27" in L.qea_last_error()
    lead = (16, one, one, one, 1, hh, ww)
    assert L.qea_skew_scores(one, *lead, 257, two, None) < 0 and b"A=257" in L.qea_last_error()
    assert L.qea_skew_scores(one, *lead, -1, two, None) < 0 and L.qea_skew_scores(None, *lead, 90, two, None) < 0
    assert L.qea_skew_scores(one, *lead, 90, None, None) < 0 and L.qea_skew_scores(one, *lead, 90, C.c_void_p(260), None) < 0
    assert L.qea_skew_pick(one, 1, 90, 10001, two, None) < 0 and b"g=10001" in L.qea_last_error()
    assert L.qea_skew_pick(one, 1, 90, -1, two, None) < 0 and L.qea_skew_pick(one, 1, 257, 0, two, None) < 0
    assert L.qea_skew_pick(None, 1, 90, 0, two, None) < 0 and L.qea_skew_pick(one, 1, 90, 0, None, None) < 0 and L.qea_skew_pick(one, 0, 90, 0, two, None) < 0
    page = (one, 0, 16, one, one, one, 1, hh, ww, one)
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 255, None, None, None, None) < 0 and b"neither" in L.qea_last_error()
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 255, None, None, one, None) < 0 and b"overlaps" in L.qea_last_error()
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 255, None, None, C.c_void_p(256 + 15), None) < 0 and b"overlaps" in L.qea_last_error()
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 255, one, C.c_void_p(256 - 60), None, None) < 0 and b"overlaps" in L.qea_last_error()
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 255, None, two, None, None) < 0 and b"norm" in L.qea_last_error()
    assert L.qea_deskew_rotate(*page, one, one, 257, 0, 255, None, None, two, None) < 0 and L.qea_deskew_rotate(*page, one, one, 90, 2, 255, None, None, two, None) < 0
    assert L.qea_deskew_rotate(*page, one, one, 90, 0, 256, None, None, two, None) < 0 and L.qea_deskew_rotate(*page, None, one, 90, 0, 255, None, None, two, None) < 0
    assert L.qea_deskew_rotate(*page, one, None, 90, 0, 255, None, None, two, None) < 0 and b"qea_deskew_rotate" in L.qea_last_error()
    with pytest.raises(_lib.QeaError):
        ops.skew_strip_sums(torch.zeros(4, dtype=torch.uint8), None)


def test_flags_of_the_front_end():
    import clean_cli
    from qea.cli_flags import build_parser
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert (a.deskew, a.deskew_max_slope, a.deskew_min_gain, a.deskew_interp) == (False, 90, 0, "bilinear")
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--deskew", "--deskew_max_slope", "40", "--deskew_min_gain", "5",
                                             "--deskew_interp", "nearest"])
    assert (a.deskew, a.deskew_max_slope, a.deskew_min_gain, a.deskew_interp) == (True, 40, 5, "nearest")
    flags = ["--deskew", "--deskew_max_slope", "--deskew_min_gain", "--deskew_interp"]
    acts = {s: act for act in build_parser("n", "")._actions for s in act.option_strings}
    assert all(acts[f].help.startswith("[new]") for f in flags)
    for tag in "pacerv":
        assert not {s for act in build_parser(tag, "")._actions for s in act.option_strings} & set(flags)
    lead = ["--prep_path", "none", "--in_dir", ".", "--out_dir", "out", "--method", "otsu", "--deskew"]
    for bad in (["--deskew_max_slope", "257"], ["--deskew_min_gain", "-1"]):
        with pytest.raises(ValueError):
            clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + bad), backend=host_backend()[0])


def skewed_scans(folder):
    from PIL import Image
    folder.mkdir()
    scans = {"a": spec.sheared_text_page(40, 1, 120, 300), "b": spec.sheared_text_page(-37, 2, 96, 160), "c": spec.sheared_text_page(0, 3, 64, 129)}
    for stem, px in scans.items():
        Image.fromarray(px).save(folder / f"{stem}.png")
    return scans


def cli_args(tmp_path, out, *more):
    import clean_cli
    return clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"), "--out_dir",
                                                str(tmp_path / out), "--batch_pages", "2"] + list(more))


def test_clean_cli_deskew_on_the_host_backend(tmp_path, capsys):
    """--method sauvola --deskew --boxes: the PNGs are deskew_pages followed by the binariser (both by their statements), the JSON holds the
    boxes of the written page, a line per page names the slope; without --deskew the outputs are those of the binariser alone"""
    from PIL import Image
    import clean_cli
    backend, _ = host_backend()
    scans = skewed_scans(tmp_path / "in")
    method = ["--method", "sauvola", "--window", "15", "--boxes", "--boxes_gap", "4"]
    written = clean_cli.CleanPages(cli_args(tmp_path, "out", "--deskew", "--deskew_max_slope", "100", *method), backend=backend).run()
    printed = capsys.readouterr().out
    plain = clean_cli.CleanPages(cli_args(tmp_path, "plain", *method), backend=backend).run()
    assert "slope" not in capsys.readouterr().out
    table, slopes = spec.rotation_table(100), {}
    for path, before, (stem, px) in zip(written, plain, scans.items()):
        a = spec.estimate(px, 100, bspec.otsu_threshold(px))[0]
        slopes[stem] = a
        assert f"{stem}: slope {a}/1024\n" in printed
        want = bspec.sauvola(spec.rotate(px, a, table), win=15, out="u8")
        with Image.open(path) as img:
            assert img.mode == "L" and np.array_equal(np.asarray(img), want), stem
        with open(path[:-4] + ".json") as f:
            rows = json.load(f)
        boxes = cspec.word_boxes(want, gap_x=4, min_area=16)
        assert len(rows) == len(boxes) > 0
        assert [[r["x_min"], r["y_min"], r["x_max"], r["y_max"]] for r in rows] == (boxes + [0, 0, 1, 1]).tolist()
        with Image.open(before) as img:
            assert np.array_equal(np.asarray(img), bspec.sauvola(px, win=15, out="u8")), stem
        with open(before[:-4] + ".json") as f:
            assert [[r["x_min"], r["y_min"], r["x_max"], r["y_max"]] for r in json.load(f)] == \
                (cspec.word_boxes(bspec.sauvola(px, win=15, out="u8"), gap_x=4, min_area=16) + [0, 0, 1, 1]).tolist()
    assert abs(slopes["a"] - 40) <= 7 and abs(slopes["b"] + 37) <= 13 and slopes["a"] != 0 != slopes["b"]      # ceil(2048 / w)


def test_clean_cli_deskew_in_front_of_the_unet(tmp_path):
    """with the UNet of the host backend: the cleaner sees the deskewed page"""
    from PIL import Image
    import clean_cli
    from qea.deskew import deskew_pages
    from qea.pages import clean_pages
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "none")
    scans = skewed_scans(tmp_path / "in")
    written = clean_cli.CleanPages(cli_args(tmp_path, "out", "--deskew", "--deskew_interp", "nearest", "--tile", "208", "208"), backend=backend).run()
    model = torch.load(tmp_path / "none", weights_only=False).eval()
    pages, _ = deskew_pages([torch.from_numpy(px) for px in scans.values()], interp="nearest")
    for path, px, page in zip(written, scans.values(), pages):
        want = clean_pages(model, [page], tile=(208, 208), out="u8")[0]
        with Image.open(path) as img:
            assert np.array_equal(np.asarray(img), want.numpy())
    assert any(not torch.equal(p, torch.from_numpy(px)) for p, px in zip(pages, scans.values()))
