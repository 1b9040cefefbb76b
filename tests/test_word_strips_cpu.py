"""Word strips and read_pages on the host: the product's host path (qea/reading.py) bit for bit against the statement
(tests/word_strips_spec.py), the two facts that follow from the statement, one pixel worked by hand, equality with utils.get_text_stack
where nothing is resampled, strip_plan on hand-made tables, every refusal, the ABI, the flags of the front end, and clean_cli.py --read
on the host backend with the oracle CRNN."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import word_strips_spec as spec

torch.set_num_threads(4)

WIDTHS = (64, 128)


@functools.lru_cache(None)
def u8_pages():
    """about 70 x 200, 45 x 67 and 2100 x 40; column 5 of the long page is all 255, the largest S a 2049-row box can have.  And 3000 x 96 of
    250..255: on the 2100 x 40 page a pixel covers at most 2100 x 40 source pixels and 2 S + Area stays below 1.4e9; here it covers
    3000 x 93.75 and 2 S + Area passes 2^32"""
    g = np.random.default_rng(21)
    pages = [g.integers(0, 256, (70, 200), dtype=np.uint8), g.integers(0, 256, (45, 67), dtype=np.uint8),
             g.integers(0, 256, (2100, 40), dtype=np.uint8), g.integers(250, 256, (3000, 96), dtype=np.uint8)]
    pages[2][:, 5] = 255
    return pages


@functools.lru_cache(None)
def float_pages():
    """the same sizes in fp32, values from -0.25 to 1.25 with a few NaN: read as 8-bit by the project's rule"""
    g = np.random.default_rng(22)
    pages = [(g.random(p.shape) * 1.5 - 0.25).astype(np.float32) for p in u8_pages()]
    pages[0][3, 4] = pages[1][44, 66] = np.nan
    pages[2][:, 5] = 1.0
    pages[3] = (1 - g.random(pages[3].shape) * 0.015).astype(np.float32)                  # 251..255
    return pages


def pages_of(kind):
    return u8_pages() if kind == "u8" else float_pages()


def as_u8(kind):
    return u8_pages() if kind == "u8" else [spec.quantise(p) for p in float_pages()]


def boxes_for(OW):
    """(page, x0, y0, x1, y1), exclusive: every case of the issue; the comment names (cw, ch) after the clip"""
    big = 2 ** 31 - 1
    return np.asarray([
        (0, 10, 5, 50, 6),                    # ch = 1
        (0, 3, 2, 90, 33),                    # ch = 31
        (0, 0, 0, 200, 32),                   # ch = 32, the whole width: cut
        (0, 7, 1, 150, 34),                   # ch = 33: the smallest shrink
        (0, 20, 10, 180, 57),                 # ch = 47: no integer ratio
        (0, 0, 3, 200, 67),                   # ch = 64
        (0, 0, 0, 200, 70),                   # the whole page
        (2, 5, 10, 6, 2059),                  # ch = 2049, cw = 1, all 255: the first 64-bit case at its largest S
        (2, 0, 3, 40, 2052),                  # ch = 2049 over the whole width
        (2, 0, 0, 40, 2100),                  # the whole long page
        (2, 3, 40, 30, 2088),                 # ch = 2048: the last 32-bit case
        (2, 5, 0, 6, 2048),                   # ch = 2048, all 255: the largest sum of the 32-bit range
        (0, 100, 0, 101, 20),                 # cw = 1
        (1, 66, 0, 67, 45),                   # cw = 1, shrunk
        (0, 10, 0, 10 + OW, 30),              # sw == OW, copied
        (0, 10, 0, 11 + OW, 30),              # sw == OW + 1: the odd cut loses the left pixel
        (0, 10, 0, 12 + OW, 30),              # sw == OW + 2
        (0, 5, 0, 12 + OW, 30),               # sw > OW
        (0, 2, 4, 2 + OW * 5 // 4, 44),       # ch = 40: sw == OW
        (0, 2, 4, 3 + OW * 5 // 4, 44),       # ch = 40: sw == OW + 1
        (0, 1, 1, 199, 34),                   # ch = 33, cw = 198: sw > OW
        (0, -5, -3, 40, 20),                  # partly outside, top left
        (0, 180, 50, 230, 90),                # partly outside, bottom right
        (1, -10, -10, 100, 100),              # larger than its page: clipped to 45 x 67, shrunk
        (0, 300, 10, 340, 30),                # wholly outside
        (0, 10, -50, 40, -2),
        (0, 50, 40, 20, 10),                  # inverted
        (0, big, 0, -big - 1, 10),            # inverted at the ends of int32
        (0, -big - 1, -big - 1, big, big),    # everything: the whole page
        (3, 0, 0, 96, 3000),                  # 2 S + Area = 4.5e9: past 2^32
        (7, 0, 0, 10, 10),                    # no such page
        (-1, 0, 0, 10, 10),
        (1, 0, 0, 67, 45),
        (1, 5, 7, 60, 39),                    # ch = 32 on the second page
    ], np.int64).astype(np.int32)


@functools.lru_cache(None)
def statement(kind, OW):
    return spec.strips(as_u8(kind), boxes_for(OW), OW)


def tensors(kind):
    return [torch.from_numpy(p) for p in pages_of(kind)]


@pytest.mark.parametrize("OW", WIDTHS)
@pytest.mark.parametrize("kind", ["u8", "float"])
def test_the_host_path_is_the_statement_bit_for_bit(kind, OW):
    from qea.reading import word_strips
    got = word_strips(tensors(kind), boxes_for(OW), OW)
    want = statement(kind, OW)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(boxes_for(OW)), 1, 32, OW)
    for i, b in enumerate(boxes_for(OW)):
        assert np.array_equal(got[i].numpy(), want[i]), (i, b.tolist())
    white = [i for i, b in enumerate(boxes_for(OW)) if spec.clip(b, [p.shape for p in u8_pages()]) is None]
    assert len(white) == 6 and all(bool((got[i] == 1.0).all()) for i in white)
    if kind == "float":                                        # [1, h, w] pages and a box table given as a tensor
        again = word_strips([t[None] for t in tensors(kind)], torch.from_numpy(boxes_for(OW)), OW)
        assert torch.equal(again, got)


def test_the_cases_the_list_is_meant_to_hold():
    sizes = [p.shape for p in u8_pages()]
    for OW in WIDTHS:
        geo = [spec.clip(b, sizes) for b in boxes_for(OW)]
        chs = {g[4] for g in geo if g}
        assert {1, 31, 32, 33, 47, 64, 2048, 2049} <= chs
        sws = [spec.scaled_width(g[3], g[4]) for g in geo if g]
        copied = {spec.scaled_width(g[3], g[4]) for g in geo if g and g[4] <= 32}
        shrunk = {spec.scaled_width(g[3], g[4]) for g in geo if g and g[4] > 32}
        assert {OW, OW + 1} <= copied and {OW, OW + 1} <= shrunk and max(copied) > OW + 1 and max(shrunk) > OW + 1 and 1 in sws
    # the all-255 box of 2049 rows is as bright as a box gets; the sums that 32 bits cannot hold are on the fourth page
    q, S, area, taps = spec.area_pixel(u8_pages()[2].tolist(), 5, 10, 1, 2049, 7, 0)
    assert q == 255 and S == 255 * area and area == 2049 * 32 and len(taps) == 65      # source rows 448..512
    q, S, area, _ = spec.area_pixel(u8_pages()[3].tolist(), 0, 0, 96, 3000, 31, 0)
    assert 2 * S + area > 2 ** 32 and area == 3000 * 3000 and 250 <= q <= 255


def test_a_box_of_one_grey_level_reads_as_that_level_at_every_scale():
    from qea.reading import word_strips
    norm = spec.norm()
    for p in (0, 1, 77, 128, 254, 255):
        page = torch.full((2100, 300), p, dtype=torch.uint8)
        boxes = [(0, 0, 0, 300, ch) for ch in (33, 47, 64, 100, 1000, 2049)] + [(0, 3, 5, 3 + cw, 5 + ch) for cw, ch in ((1, 33), (7, 90), (299, 2095))]
        got = word_strips([page], boxes, 128).numpy()
        assert set(np.unique(got).tolist()) <= {float(norm[p]), 1.0}
        for i, b in enumerate(boxes):
            sw = spec.scaled_width(b[3] - b[1], b[4] - b[2])
            left = (128 - sw) // 2
            inside = got[i, 0, :, max(left, 0):min(left + sw, 128)]
            assert inside.size and bool((inside == norm[p]).all()), (p, b)


def test_at_64_rows_a_pixel_is_the_rounded_mean_of_its_2_x_2_block():
    from qea.reading import word_strips
    page = u8_pages()[0]
    x0, y0, cw = 6, 3, 100
    got = word_strips([torch.from_numpy(page)], [(0, x0, y0, x0 + cw, y0 + 64)], 64)[0, 0].numpy()
    block = page[y0:y0 + 64, x0:x0 + cw].astype(np.int64).reshape(32, 2, cw // 2, 2)
    want = (block.sum((1, 3)) + 2) // 4
    assert np.array_equal(got[:, 7:57], spec.norm()[want]) and bool((got[:, :7] == 1).all()) and bool((got[:, 57:] == 1).all())
    # an odd width: the last column is half covered and is the mean of its two pixels
    got = word_strips([torch.from_numpy(page)], [(0, x0, y0, x0 + 5, y0 + 64)], 64)[0, 0].numpy()
    last = page[y0:y0 + 64, x0 + 4].astype(np.int64).reshape(32, 2)
    assert np.array_equal(got[:, (64 - 3) // 2 + 2], spec.norm()[(2 * last.sum(1) + 2) // 4])


def test_one_pixel_at_48_rows_by_hand():
    """ch = 48: a scaled pixel is 1.5 source pixels wide and high.  Scaled pixel (oy 1, j 1) covers [48, 96) in both axes: source rows and
    columns 1 (by 16) and 2 (by 32).  The weights are 16 16, 16 32, 32 16, 32 32 and the area is 48 48."""
    from qea.reading import word_strips
    page = np.full((60, 20), 255, np.uint8)
    page[5 + 1, 2 + 1], page[5 + 1, 2 + 2], page[5 + 2, 2 + 1], page[5 + 2, 2 + 2] = 10, 200, 97, 33
    S = 16 * 16 * 10 + 16 * 32 * 200 + 32 * 16 * 97 + 32 * 32 * 33
    q = (2 * S + 2304) // 4608
    assert (S, q) == (188416, 82)                              # 81.78 rounds up
    got, _, area, taps = spec.area_pixel(page.tolist(), 2, 5, 9, 48, 1, 1)
    assert (got, area) == (q, 2304) and taps == [(1, 1, 16, 16), (1, 2, 16, 32), (2, 1, 32, 16), (2, 2, 32, 32)]
    strip = word_strips([torch.from_numpy(page)], [(0, 2, 5, 11, 53)], 64)[0, 0].numpy()       # cw = 9: sw = 6, left = 29
    assert strip[1, 29 + 1] == spec.norm()[q] and strip[1, 29 + 5] == 1.0 and strip[1, 28] == 1.0
    assert np.array_equal(strip, spec.strip([page], (0, 2, 5, 11, 53), 64))


@pytest.mark.parametrize("OW", WIDTHS)
def test_boxes_of_at_most_32_rows_are_get_text_stack(OW):
    """where nothing is resampled the strip is the crop + pad the CRNN was trained on.  A negative bound means something else to a Python
    slice, so the bounds are raised to 0 for it, as utils.get_text_stack's device path does with the near edges"""
    from qea.reading import word_strips
    from utils import get_text_stack
    sizes = [p.shape for p in u8_pages()]
    boxes = boxes_for(OW)
    got = word_strips(tensors("u8"), boxes, OW)
    seen = 0
    for p, page in enumerate(u8_pages()):
        rows = [i for i, b in enumerate(boxes.tolist()) if b[0] == p and min(b[4], sizes[p][0]) - max(b[2], 0) <= 32]
        image = torch.from_numpy(spec.norm()[page])[None]
        labels = [dict(zip(("x_min", "y_min", "x_max", "y_max"), (max(v, 0) for v in boxes[i, 1:].tolist())), label="") for i in rows]
        if rows:
            want, _ = get_text_stack(image, labels, (32, OW))
            assert torch.equal(got[rows], want), p
            seen += len(rows)
    assert seen >= 14


def test_strip_plan_on_hand_made_tables():
    from qea.reading import strip_plan
    hs, ws = [100, 3000], [1000, 700]
    boxes = [(0, 0, 0, 128, 20),        # sw 128 -> bucket 128
             (0, 0, 0, 129, 20),        # 129 -> 256
             (0, 0, 0, 600, 32),        # 600 -> 512, cut
             (1, 0, 0, 700, 64),        # ch 64: sw 350 -> 384
             (1, 0, 0, 100, 3000),      # sw = ceil(3200 / 3000) = 2 -> 128
             (0, 5, 5, 5, 50),          # empty: sw 0 -> 128
             (0, 0, 0, 512, 32),        # 512 -> 512, not cut
             (1, 0, 0, 700, 33),        # sw = ceil(22400 / 33) = 679 -> 512, cut
             (0, 900, 0, 1200, 10),     # clipped to cw 100 -> 128
             (7, 0, 0, 10, 10)]         # no such page: sw 0 -> 128
    plan = strip_plan(boxes, hs, ws)
    assert plan.sw.tolist() == [128, 129, 600, 350, 2, 0, 512, 679, 100, 0]
    assert plan.bucket.tolist() == [128, 256, 512, 384, 128, 128, 512, 512, 128, 128]
    assert plan.cut.tolist() == [False, False, True, False, False, False, False, True, False, False]
    assert [(OW, idx.tolist()) for OW, idx in plan.passes] == [(128, [0, 4, 5, 8, 9]), (256, [1]), (384, [3]), (512, [2, 6, 7])]
    plan = strip_plan(boxes, hs, ws, buckets=(64, 352), strip_pixels=128)
    assert plan.bucket.tolist() == [352, 352, 352, 352, 64, 64, 352, 352, 352, 64] and int(plan.cut.sum()) == 3
    assert [(OW, idx.tolist()) for OW, idx in plan.passes] == [(64, [4, 5]), (64, [9]), (352, [0]), (352, [1]), (352, [2]), (352, [3]), (352, [6]),
                                                              (352, [7]), (352, [8])]
    plan = strip_plan(boxes, hs, ws, strip_pixels=384)
    assert [(OW, idx.tolist()) for OW, idx in plan.passes] == [(128, [0, 4, 5]), (128, [8, 9]), (256, [1]), (384, [3]), (512, [2]), (512, [6]),
                                                              (512, [7])]
    empty = strip_plan(np.zeros((0, 5), np.int32), hs, ws)
    assert empty.passes == [] and empty.sw.shape == (0,)


def test_refusals_of_the_product_module():
    from qea._lib import QeaError
    from qea.reading import check_params, read_pages, strip_plan, word_strips
    page = torch.zeros(40, 40, dtype=torch.uint8)
    for kw in (dict(buckets=()), dict(buckets=(120,)), dict(buckets=(48,)), dict(buckets=(528,)), dict(buckets=(256, 128)), dict(buckets=(128, 128)),
               dict(buckets=(128.0,)), dict(buckets=128), dict(strip_pixels=0), dict(strip_pixels=1.5), dict(beam=-1), dict(beam=33), dict(beam=2.0),
               dict(nbest=0), dict(nbest=2), dict(beam=4, nbest=5)):
        with pytest.raises(ValueError):
            check_params(**kw)
    assert check_params() == (128, 256, 384, 512) and check_params([64, 512], 1, 8, 8) == (64, 512)
    for width in (60, 72, 48, 528, 128.0, True):
        with pytest.raises(ValueError):
            word_strips([page], [(0, 0, 0, 4, 4)], width)
    for boxes in ([(0, 0, 0, 4)], [(0.0, 0, 0, 4, 4)], [(0, 0, 0, 4, 2 ** 31)]):
        with pytest.raises(ValueError):
            word_strips([page], boxes, 64)
    with pytest.raises(ValueError):
        strip_plan([(0, 0, 0, 4, 4)], [40], [40], buckets=(100,))
    with pytest.raises(ValueError):
        word_strips([], [(0, 0, 0, 4, 4)], 64)
    with pytest.raises(QeaError, match="32767"):
        word_strips([torch.zeros(1, 1, dtype=torch.uint8).expand(2, 32768)], [(0, 0, 0, 4, 4)], 64)
    assert tuple(word_strips([page], [], 64).shape) == (0, 1, 32, 64)

    class Model(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("no pass may run")
    maps = {i: "a" for i in range(95)}
    with pytest.raises(ValueError, match="eval"):
        read_pages(Model().train(), [page], [[(0, 0, 4, 4)]], maps)
    with pytest.raises(ValueError):
        read_pages(Model().eval(), [page], [], maps)
    with pytest.raises(ValueError):
        read_pages(Model().eval(), [page], [[(0, 0, 4, 4)]], maps, buckets=(100,))
    with pytest.raises(QeaError):
        read_pages(Model().eval(), [page], [[(0, 0, 4, 4)]], maps, lm=object())
    with pytest.raises(QeaError):
        read_pages(Model().eval(), [page], [[(0, 0, 4, 4)]], maps, beam=4, lm=object(), lexicon=object())
    assert read_pages(Model().eval(), [page, page], [[], []], maps) == ([[], []], 0)


def test_abi_and_ops():
    """the symbol is in the header and in the built library; the library refuses bad arguments before any launch"""
    import inspect
    from qea import _lib, ops, reading
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    L = _lib.lib()
    assert len(protos["qea_word_strips"]) == 13 and hasattr(L, "qea_word_strips") and L.qea_version() == 9
    assert list(inspect.signature(ops.word_strips).parameters) == ["store", "table", "boxes", "OW", "norm", "out"]
    assert set(ops.WORD_STRIP_LAUNCHES) == {"strips"}
    assert (ops.WORD_STRIP_H, ops.WORD_STRIP_MIN_W, ops.WORD_STRIP_MAX_W, ops.WORD_STRIP_MAX_BOXES, ops.WORD_STRIP_MAX_SIDE) == \
        (reading.OH, reading.MIN_W, reading.MAX_W, reading.MAX_BOXES, reading.MAX_SIDE) == (32, 64, 512, 1 << 20, 32767)
    one, two = C.c_void_p(256), C.c_void_p(1 << 20)

    def call(store=one, f32=0, elems=16, offset=one, h=one, w=one, n_pages=1, boxes=one, n=1, OW=128, norm=one, out=two):
        return L.qea_word_strips(store, f32, elems, offset, h, w, n_pages, boxes, n, OW, norm, out, None)
    for kw in (dict(store=None), dict(offset=None), dict(h=None), dict(w=None), dict(boxes=None), dict(norm=None), dict(out=None), dict(f32=2),
               dict(store=C.c_void_p(258), f32=1), dict(elems=0), dict(n_pages=0), dict(n=-1), dict(n=(1 << 20) + 1), dict(OW=120), dict(OW=48),
               dict(OW=528), dict(OW=0), dict(out=C.c_void_p((1 << 20) + 8)), dict(boxes=C.c_void_p(258)), dict(offset=C.c_void_p(260))):
        assert call(**kw) < 0, kw
        assert b"qea_word_strips" in L.qea_last_error(), kw
    assert call(n=0) == 0                                      # nothing to write: accepted, and nothing is launched
    with pytest.raises(_lib.QeaError):
        ops.word_strips(torch.zeros(4, dtype=torch.uint8), None, torch.zeros(1, 5, dtype=torch.int32), 128, torch.zeros(256))


READ_FLAGS = ["--read", "--read_beam", "--read_lm", "--read_lm_weight", "--read_lm_bonus", "--read_lexicon", "--read_buckets"]


def host_backend():
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    return Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False), OracleCRNN


def test_flags_of_the_front_end(tmp_path):
    import clean_cli
    from qea.cli_flags import build_parser
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert (a.read, a.read_beam, a.read_lm, a.read_lm_weight, a.read_lm_bonus, a.read_lexicon, a.read_buckets) == (None, 0, None, 1.0, 0.0, None, None)
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--read", "ckpt", "--read_beam", "8", "--read_lm", "lm", "--read_lm_weight",
                                             "0.5", "--read_lm_bonus", "1.5", "--read_lexicon", "lex", "--read_buckets", "64", "256"])
    assert (a.read, a.read_beam, a.read_lm, a.read_lm_weight, a.read_lm_bonus, a.read_lexicon, a.read_buckets) == ("ckpt", 8, "lm", 0.5, 1.5, "lex", [64, 256])
    acts = {s: act for act in build_parser("n", "")._actions for s in act.option_strings}
    assert all(acts[f].help.startswith("[new]") for f in READ_FLAGS)
    for tag in "pacerv":
        assert not {s for act in build_parser(tag, "")._actions for s in act.option_strings} & set(READ_FLAGS)
    backend, OracleCRNN = host_backend()
    torch.save(OracleCRNN(95).eval(), tmp_path / "crnn")
    (tmp_path / "in").mkdir()
    lead = ["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--method", "otsu"]
    read = ["--read", str(tmp_path / "crnn")]
    for bad in (read + ["--read_lm", "x"], read + ["--read_lexicon", "x"], read + ["--read_beam", "4", "--read_lm", "x", "--read_lexicon", "y"],
                read + ["--read_beam", "33"], read + ["--read_beam", "-1"], read + ["--read_buckets", "100"], read + ["--read_buckets", "256", "128"],
                ["--read_beam", "4"], ["--read_buckets", "128"], ["--read_lm", "x"], ["--read_lexicon", "x"]):
        with pytest.raises(ValueError):
            clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + bad), backend=backend)
    ok = clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + read + ["--read_beam", "4", "--read_buckets", "64", "128"]), backend=backend)
    assert ok.boxes and ok.read_buckets == (64, 128) and ok.read_beam == 4 and not ok.read_model.training


def word_scans(folder):
    """three small scans with a few dark words each, one of them 40 rows high and one wider than the last bucket of the test"""
    from PIL import Image
    folder.mkdir()
    a = np.full((90, 220), 255, np.uint8)
    a[6:46, 10:70], a[10:22, 90:130], a[60:70, 12:60], a[58:82, 100:200] = 20, 40, 0, 30
    a[12:40:4, 14:66:3], a[62:68:2, 20:50:5] = 230, 200                     # light dots inside the words: the strips are not flat
    b = np.full((64, 150), 255, np.uint8)
    b[5:15, 4:146], b[30:50, 20:60] = 10, 50                                # 142 columns: wider than 128
    b[7:13:2, 10:140:7] = 220
    c = np.full((50, 70), 255, np.uint8)
    c[20:28, 10:40] = 0
    scans = {"a": a, "b": b, "c": c}
    for stem, px in scans.items():
        Image.fromarray(px).save(folder / f"{stem}.png")
    return scans


def cli_args(tmp_path, out, *more):
    import clean_cli
    return clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"), "--out_dir",
                                                str(tmp_path / out), "--batch_pages", "2", "--method", "otsu", "--boxes_gap", "2"] + list(more))


def test_clean_cli_read_on_the_host_backend(tmp_path, capsys):
    """--read with the oracle CRNN as the checkpoint: the labels of the JSON are read_pages of the written pages and their boxes, the boxes
    and the PNGs are those of the run without the flag, whose JSON bytes are what the front end wrote before it had the flag"""
    from PIL import Image
    import clean_cli
    import properties
    from qea.components import word_boxes
    from qea.reading import read_pages
    from utils import get_char_maps
    backend, OracleCRNN = host_backend()
    torch.save(OracleCRNN(95, seed=4).eval(), tmp_path / "crnn")
    scans = word_scans(tmp_path / "in")
    plain = clean_cli.CleanPages(cli_args(tmp_path, "plain", "--boxes"), backend=backend).run()
    assert "words read" not in capsys.readouterr().out
    read = ["--read", str(tmp_path / "crnn"), "--read_buckets", "64", "128"]
    greedy = clean_cli.CleanPages(cli_args(tmp_path, "greedy", *read), backend=backend).run()
    printed = capsys.readouterr().out
    beam = clean_cli.CleanPages(cli_args(tmp_path, "beam", "--read_beam", "3", *read), backend=backend).run()
    model = torch.load(tmp_path / "crnn", weights_only=False).eval()
    index_to_char = get_char_maps(properties.char_set)[1]
    pages = []
    for path in plain:
        with Image.open(path) as img:
            pages.append(torch.from_numpy(np.asarray(img).copy()))
    boxes = word_boxes(pages, gap_x=2, min_area=16)
    assert [len(b) for b in boxes] == [4, 2, 1]
    texts, btexts, bscores, cut = [], [], [], 0
    for group in (slice(0, 2), slice(2, 3)):                               # --batch_pages 2: the passes of the run, so the same tensors
        t, c = read_pages(model, pages[group], boxes[group], index_to_char, buckets=(64, 128))
        bt, bs, _ = read_pages(model, pages[group], boxes[group], index_to_char, buckets=(64, 128), beam=3)
        texts, btexts, bscores, cut = texts + t, btexts + bt, bscores + bs, cut + c
    assert cut == 1
    for i, (stem, p, g, b) in enumerate(zip(scans, plain, greedy, beam)):
        with open(p, "rb") as x, open(g, "rb") as y, open(b, "rb") as z:
            assert x.read() == y.read() == z.read()                        # the PNG bytes
        with open(p[:-4] + ".json") as f:
            raw = f.read()
        rows = json.loads(raw)
        want = [dict(label="", x_min=a, y_min=b_, x_max=c + 1, y_max=d + 1) for a, b_, c, d in boxes[i].tolist()]
        assert rows == want and raw == json.dumps(want)                    # the bytes of a run without --read
        with open(g[:-4] + ".json") as f:
            got = json.load(f)
        assert got == [dict(r, label=t) for r, t in zip(want, texts[i])]
        with open(b[:-4] + ".json") as f:
            got = json.load(f)
        assert got == [dict(r, label=t, score=s) for r, t, s in zip(want, btexts[i], bscores[i])]
        assert f"{stem}: {len(want)} words read, {int(stem == 'b')} cut\n" in printed
    assert any(t for page in texts for t in page)                          # the seeded CRNN reads something somewhere


def test_read_pages_follows_the_plan_with_an_injected_forward():
    """a recording forward: the passes are those of strip_plan, every pass holds the strips of its boxes at its width, and the strings are
    pred_to_string of the recorded scores scattered back into box order"""
    from qea.reading import box_table, read_pages, strip_plan, word_strips
    from utils import pred_to_string
    pages = tensors("u8")[:2]
    per_page = [torch.tensor([(0, 0, 199, 69), (10, 5, 49, 5), (3, 2, 89, 32), (0, 0, 199, 31), (7, 1, 149, 33)], dtype=torch.int32),
                torch.tensor([(0, 0, 66, 44), (5, 7, 59, 38)], dtype=torch.int32)]
    table = box_table(per_page)
    assert table.tolist()[0] == [0, 0, 0, 200, 70] and table.tolist()[-1] == [1, 5, 7, 60, 39]
    plan = strip_plan(table, [70, 45], [200, 67], (64, 128), strip_pixels=128)
    index_to_char = {i: chr(96 + i) for i in range(6)}
    seen = []

    class Model(torch.nn.Module):
        pass

    def forward(x):
        g = torch.Generator().manual_seed(len(seen))
        s = torch.log_softmax(torch.randn(x.shape[3] // 4 - 1, x.shape[0], 6, generator=g) * 3, 2)
        seen.append((x.clone(), s))
        return s
    texts, cut = read_pages(Model().eval(), pages, per_page, index_to_char, buckets=(64, 128), strip_pixels=128, forward=forward)
    assert cut == 2 and [len(t) for t in texts] == [5, 2]
    assert [(x.shape[3], x.shape[0]) for x, _ in seen] == [(OW, len(idx)) for OW, idx in plan.passes] and len(seen) >= 4
    flat = [None] * len(table)
    for (x, s), (OW, idx) in zip(seen, plan.passes):
        assert torch.equal(x, word_strips(pages, table[idx], OW))
        for i, t in zip(idx.tolist(), pred_to_string(s, [""] * len(idx), index_to_char)):
            flat[i] = t
    assert texts == [flat[:5], flat[5:]] and any(flat)
