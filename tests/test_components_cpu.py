"""Connected components on the host: the product's host path (qea/components.py) bit for bit against the statement
(tests/components_spec.py), the statement against scipy where scipy is installed, smearing by hand, word boxes of rendered words, every
refusal, the new flags, and eval_prep.py --baseline_despeckle / clean_cli.py --despeckle --boxes on the host backend."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import binarize_spec as bspec
import components_spec as spec
from test_binarize_cpu import baseline_docs, host_backend

torch.set_num_threads(4)

TILE_H, TILE_W = 32, 64


def as_page(ink):
    """bool ink -> the uint8 page that reads as it at any ink_max: ink 0, background 255"""
    return np.where(ink, 0, 255).astype(np.uint8)


def serpentine(h=131, w=257):
    """every even row all ink, the odd rows joined alternately at the last and the first column: one path through every tile border"""
    ink = np.zeros((h, w), bool)
    ink[0::2] = True
    ink[1::4, w - 1] = True
    ink[3::4, 0] = True
    return ink


def corner_diagonal():
    ink = np.zeros((70, 130), bool)
    ink[31, 63] = ink[32, 64] = ink[33, 65] = True
    return ink


def ink_pages():
    """name -> bool ink, the pages of the issue: built once"""
    if not _PAGES:
        g = np.random.default_rng(11)
        draws = [g.random((437, 531)) for _ in range(4)]
        _PAGES.update({
            "rand30": draws[1] < 0.30, "rand45": draws[3] < 0.45,
            "one_ink": np.ones((1, 1), bool), "one_bg": np.zeros((1, 1), bool),
            "row": g.random((1, 300)) < 0.5, "column": g.random((31, 1)) < 0.5,
            "all_ink": np.ones((70, 90), bool), "all_bg": np.zeros((70, 90), bool),
            "checker": np.add.outer(np.arange(33), np.arange(65)) % 2 == 0,
            "serpentine": serpentine(), "diagonal": corner_diagonal()})
    return _PAGES


_PAGES, _LABELS = {}, {}
NAMES = ["rand30", "rand45", "one_ink", "one_bg", "row", "column", "all_ink", "all_bg", "checker", "serpentine", "diagonal"]


def statement_labels(name, connectivity):
    """the statement's labels of a page, computed once and never changed (tests/test_components_gpu.py shares them)"""
    if (name, connectivity) not in _LABELS:
        lab = spec.labels_of_ink(ink_pages()[name], connectivity)
        lab.setflags(write=False)
        _LABELS[name, connectivity] = lab
    return _LABELS[name, connectivity]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_host_path_is_the_statement(name, connectivity):
    from qea.components import despeckle_pages, label_pages, page_components
    ink = ink_pages()[name]
    page = torch.from_numpy(as_page(ink))
    want = statement_labels(name, connectivity)
    got = label_pages([page], connectivity)[0]
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    table = spec.table_fast(want)
    if want.size < 10000:
        assert np.array_equal(table, spec.table_of_labels(want))
    got = page_components([page], connectivity)[0]
    assert got.dtype == torch.int32 and got.shape == table.shape and np.array_equal(got.numpy(), table)
    for out in ("u8", "float"):
        for min_area in (1, 4):
            got = despeckle_pages([page], min_area, connectivity, out=out)[0]
            assert np.array_equal(got.numpy(), spec.despeckle(page.numpy(), min_area, connectivity, out=out, lab=want)), (out, min_area)
    assert np.array_equal(despeckle_pages([page], 1, connectivity, out="u8")[0].numpy(), as_page(ink))      # min_area 1 only binarises


def test_the_random_pages_are_not_vacuous():
    """the counts the issue states for these pages at connectivity 8; despeckle(4) removes and keeps; the largest component crosses tiles"""
    t30, t45 = (spec.table_fast(statement_labels(n, 8)) for n in ("rand30", "rand45"))
    assert len(t30) == 11112 and int((t30[:, 1] < 4).sum()) == 6864 and int((t30[:, 1] >= 4).sum()) == 4248
    assert len(t45) == 1823 and int(t45[:, 1].max()) == 97638
    for name in ("rand30", "rand45"):
        ink = ink_pages()[name]
        kept = spec.despeckle(as_page(ink), 4, 8, lab=statement_labels(name, 8)) == 0
        assert kept.any() and (ink & ~kept).any()
    big = t45[np.argmax(t45[:, 1])]
    assert big[4] // TILE_W > big[2] // TILE_W + 1 and big[5] // TILE_H > big[3] // TILE_H + 1


def test_the_structured_pages_have_the_components_they_were_built_for():
    assert len(spec.table_fast(statement_labels("checker", 8))) == 1
    assert len(spec.table_fast(statement_labels("checker", 4))) == int(ink_pages()["checker"].sum()) == 1073
    for c in (4, 8):
        t = spec.table_fast(statement_labels("serpentine", c))
        assert t.tolist() == [[0, 17027, 0, 0, 256, 130]]
        assert (statement_labels("all_bg", c) == -1).all() and (statement_labels("all_ink", c) == 0).all()
    assert spec.table_fast(statement_labels("diagonal", 8)).tolist() == [[31 * 130 + 63, 3, 63, 31, 65, 33]]
    assert spec.table_fast(statement_labels("diagonal", 4))[:, 0].tolist() == [31 * 130 + 63, 32 * 130 + 64, 33 * 130 + 65]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_statement_against_scipy(connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for name in ("rand30", "rand45"):
        ink = ink_pages()[name]
        lab, n = nd.label(ink, structure=structure)
        first = np.full(n + 1, ink.size, np.int64)
        np.minimum.at(first, lab.reshape(-1), np.arange(ink.size))
        assert np.array_equal(np.where(ink, first[lab], -1), statement_labels(name, connectivity))


def _row(text):
    return np.asarray([[c == "#" for c in text]])


def test_smear_by_hand():
    from qea.components import _smear_host
    row = _row("..#.#..#...#....#.....#")
    cases = {0: "..#.#..#...#....#.....#", 1: "..###..#...#....#.....#", 3: "..##########....#.....#", 127: "..#####################"}
    for gx, want in cases.items():
        for f in (spec.smear, _smear_host):
            assert np.array_equal(f(row, gx, 0), _row(want)), (gx, f)
            assert np.array_equal(f(row.T.copy(), 0, gx), _row(want).T), (gx, f)
    for gx in (1, 3, 7, 127):                                  # a run of exactly gx is filled, one of gx + 1 is not; the edges never
        for run, filled in ((gx, True), (gx + 1, False)):
            row = np.zeros((1, run + 6), bool)
            row[0, 2] = row[0, 3 + run] = True
            for f in (spec.smear, _smear_host):
                got = f(row, gx, 0)
                assert bool(got[0, 3:3 + run].all()) == filled and not got[0, :2].any() and not got[0, 4 + run:].any()
                assert not filled or not (got ^ row)[0, [0, 1, 2, 3 + run, 4 + run, 5 + run]].any()
    # the vertical pass acts on the horizontal result: the bridge of row 0 and the pixel under it close the column gap
    page = np.zeros((3, 5), bool)
    page[0, 0] = page[0, 4] = page[2, 2] = True
    for f in (spec.smear, _smear_host):
        assert not f(page, 0, 1)[1].any() and f(page, 3, 0)[0].all()
        assert f(page, 3, 1).tolist() == [[True] * 5, [False, False, True, False, False], [False, False, True, False, False]]
    g = np.random.default_rng(3)
    for shape, gx, gy in (((40, 70), 2, 0), ((33, 65), 5, 3), ((70, 20), 0, 9), ((5, 300), 127, 127)):
        ink = g.random(shape) < 0.1
        assert np.array_equal(_smear_host(ink, gx, gy), spec.smear(ink, gx, gy)), (shape, gx, gy)


def words_page(h=100, w=300, lines=(10, 40, 70), seed=0):
    """rectangles as letters (5 x 9, 2 px apart) in words 12 px apart -> (uint8 page, the words' boxes in reading order, inclusive)"""
    g = np.random.default_rng(seed)
    page, boxes = np.full((h, w), 255, np.uint8), []
    for y in lines:
        x = 8
        while True:
            letters = int(g.integers(1, 6))
            end = x + letters * 5 + (letters - 1) * 2
            if end > w - 8:
                break
            for i in range(letters):
                page[y:y + 9, x + 7 * i:x + 7 * i + 5] = 0
            boxes.append([x, y, end - 1, y + 8])
            x = end + 12
    return page, np.asarray(boxes, np.int32)


def test_word_boxes_of_rendered_words():
    from qea.components import word_boxes
    page, want = words_page()
    assert len(want) > 12
    got = word_boxes([torch.from_numpy(page)], gap_x=4, gap_y=0, min_area=16)[0]
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want) and np.array_equal(spec.word_boxes(page, 4, 0, 16), want)
    letters = word_boxes([torch.from_numpy(page)], gap_x=1, gap_y=0, min_area=1)[0]
    assert len(letters) == int((page[10::30][:3, 1:] < page[10::30][:3, :-1]).sum())       # gap 1 < 2: every letter is its own box
    lines = word_boxes([torch.from_numpy(page)], gap_x=12, gap_y=0, min_area=1)[0]
    assert lines[:, 1].tolist() == [10, 40, 70]
    assert len(word_boxes([torch.from_numpy(page)], gap_x=4, min_area=46)[0]) == int(((want[:, 2] - want[:, 0] + 1) * 9 >= 46).sum())
    g = np.random.default_rng(8)
    noise = as_page(g.random((90, 140)) < 0.08)
    for gx, gy, a in ((3, 0, 1), (2, 2, 6), (0, 4, 2), (0, 0, 3)):
        assert np.array_equal(word_boxes([torch.from_numpy(noise)], gx, gy, a)[0].numpy(), spec.word_boxes(noise, gx, gy, a)), (gx, gy, a)


def test_mixed_page_lists_and_ink_max():
    """[1, h, w] floats with values outside [0, 1] and NaN, several sizes in one call, ink_max other than the default"""
    from qea.components import despeckle_pages, label_pages, page_components, word_boxes
    g = torch.Generator().manual_seed(6)
    floats = [torch.rand(1, 45, 67, generator=g) * 1.5 - 0.25, torch.rand(1, 33, 19, generator=g), torch.rand(1, 1, 300, generator=g)]
    floats[0][0, 2, 3] = float("nan")
    bytes_ = [torch.randint(0, 256, (s, t), generator=g, dtype=torch.uint8) for s, t in ((64, 64), (65, 129), (31, 1))]
    for pages in (floats, bytes_):
        for ink_max in (127, 60, 0, 254):
            labs = label_pages(pages, 8, ink_max)
            tabs = page_components(pages, 4, ink_max)
            outs = despeckle_pages(pages, 3, 8, ink_max, out="float")
            boxes = word_boxes(pages, 2, 1, 2, ink_max)
            for p, lab, tab, o, b in zip(pages, labs, tabs, outs, boxes):
                flat = p.reshape(p.shape[-2], p.shape[-1]).numpy()
                assert o.shape == p.shape and lab.shape == flat.shape
                assert np.array_equal(lab.numpy(), spec.labels(flat, 8, ink_max))
                assert np.array_equal(tab.numpy(), spec.table_fast(spec.labels(flat, 4, ink_max)))
                assert np.array_equal(o.reshape(flat.shape).numpy(), spec.despeckle(flat, 3, 8, ink_max, out="float"))
                assert np.array_equal(b.numpy(), spec.word_boxes(flat, 2, 1, 2, ink_max))
    assert (spec.to_u8(floats[0][0].numpy()) == bspec.to_u8(floats[0][0].numpy())).all()


def test_binarize_pages_despeckle_is_the_two_statements_in_a_row():
    from qea.binarize import binarize_pages
    g = torch.Generator().manual_seed(12)
    pages = [torch.randint(0, 256, (s, t), generator=g, dtype=torch.uint8) for s, t in ((50, 70), (33, 65))]
    for out in ("u8", "float"):
        for conn in (4, 8):
            got = binarize_pages(pages, "sauvola", window=15, out=out, despeckle=4, despeckle_connectivity=conn)
            for p, b in zip(pages, got):
                plain = bspec.sauvola(p.numpy(), 15, 0.2, 128.0)
                want = spec.despeckle(plain, 4, conn, out=out)
                assert (want != bspec.as_output(plain == 0, out)).any() and np.array_equal(b.numpy(), want)
    for p, a, b in zip(pages, binarize_pages(pages, "otsu", out="u8"), binarize_pages(pages, "otsu", out="u8", despeckle=0)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        binarize_pages(pages, "otsu", despeckle=3, despeckle_connectivity=6)
    with pytest.raises(ValueError):
        binarize_pages(pages, "otsu", despeckle=-1)


def test_refusals_of_the_product_module():
    from qea._lib import QeaError
    from qea.components import check_params, despeckle_pages, label_pages, page_components, word_boxes
    page = [torch.zeros(4, 4, dtype=torch.uint8)]
    check_params()
    check_params(4, 0, 1, 127, 127)
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(connectivity=8.0), dict(ink_max=-1), dict(ink_max=255), dict(ink_max=1.5),
                dict(min_area=0), dict(min_area=2.5), dict(gap_x=-1), dict(gap_x=128), dict(gap_y=128), dict(gap_y=0.5)):
        with pytest.raises(ValueError):
            check_params(**bad)
    for call in (lambda: label_pages(page, 5), lambda: label_pages(page, 8, 255), lambda: page_components(page, ink_max=-1),
                 lambda: despeckle_pages(page, 0), lambda: despeckle_pages(page, 2, out="png"), lambda: word_boxes(page, gap_x=200),
                 lambda: word_boxes(page, min_area=0), lambda: label_pages([]), lambda: label_pages([torch.zeros(0, 4, dtype=torch.uint8)])):
        with pytest.raises(ValueError):
            call()
    huge = torch.zeros(1, dtype=torch.uint8).expand(1 << 14, (1 << 13) + 1)
    with pytest.raises(QeaError, match="2\\^27"):
        label_pages([huge])


def test_abi_and_ops():
    """the five symbols are in the header and in the built library; the library refuses bad arguments before any launch"""
    from qea import _lib, ops
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    sizes = {"qea_cc_label": 16, "qea_cc_stats": 13, "qea_cc_despeckle": 16, "qea_cc_smear": 16, "qea_cc_boxes": 16}
    L = _lib.lib()
    for name, n in sizes.items():
        assert len(protos[name]) == n and hasattr(L, name), name
    assert L.qea_version() == 9
    assert set(ops.COMPONENT_LAUNCHES) == {"tile", "border", "flatten", "stats", "despeckle", "smear", "boxes"}
    assert set(ops.BINARIZE_LAUNCHES) == {"sauvola", "histogram", "otsu"}
    one, odd = C.c_void_p(256), C.c_void_p(258)
    hh, ww = (C.c_int32 * 1)(4), (C.c_int32 * 1)(4)

    def label(store=one, n=1, host_h=hh, host_w=ww, first=one, mask=None, ink_max=127, conn=8, labels=one, area=None):
        return L.qea_cc_label(store, 0, 16, one, one, one, n, host_h, host_w, first, mask, ink_max, conn, labels, area, None)
    for kw in (dict(store=None), dict(n=0), dict(first=None), dict(host_h=(C.c_int32 * 1)(0)), dict(ink_max=-1), dict(ink_max=255), dict(conn=6),
               dict(conn=0), dict(labels=None), dict(labels=odd), dict(area=odd),
               dict(host_h=(C.c_int32 * 1)(1 << 14), host_w=(C.c_int32 * 1)((1 << 13) + 1))):
        assert label(**kw) < 0, kw
        assert b"qea_cc_label" in L.qea_last_error(), kw
    assert b"2^27" in L.qea_last_error()
    lead = (one, 0, 16, one, one, one, 1, hh, ww, one)
    assert L.qea_cc_stats(*lead, None, one, None) < 0 and L.qea_cc_stats(*lead, one, None, None) < 0 and L.qea_cc_stats(*lead, one, odd, None) < 0
    assert L.qea_cc_despeckle(*lead, one, one, 0, None, one, None) < 0 and b"min_area" in L.qea_last_error()
    assert L.qea_cc_despeckle(*lead, one, one, 1, None, None, None) < 0 and L.qea_cc_despeckle(*lead, one, one, 1, odd, None, None) < 0
    assert L.qea_cc_despeckle(*lead, None, one, 1, None, one, None) < 0 and L.qea_cc_despeckle(*lead, one, odd, 1, None, one, None) < 0
    assert L.qea_cc_smear(*lead, None, 127, 128, 0, one, None) < 0 and b"gap" in L.qea_last_error()
    assert L.qea_cc_smear(*lead, None, 127, -1, 0, one, None) < 0 and L.qea_cc_smear(*lead, None, 127, 3, 0, None, None) < 0
    assert L.qea_cc_smear(*lead, None, 255, 3, 0, one, None) < 0 and L.qea_cc_smear(*lead, one, 127, 3, 1, one, None) < 0
    assert L.qea_cc_boxes(*lead, one, one, one, 1, None, None) < 0 and L.qea_cc_boxes(*lead, one, odd, one, 1, one, None) < 0
    assert L.qea_cc_boxes(*lead, one, one, one, -1, one, None) < 0 and L.qea_cc_boxes(*lead, None, one, one, 1, one, None) < 0
    assert b"qea_cc_boxes" in L.qea_last_error()
    with pytest.raises(_lib.QeaError):
        ops.cc_label(torch.zeros(4, dtype=torch.uint8), None)


def test_flags_of_the_two_front_ends():
    import clean_cli
    import eval_prep
    from qea.cli_flags import build_parser
    a = eval_prep.build_parser().parse_args([])
    assert a.baseline_despeckle == 0
    assert eval_prep.build_parser().parse_args(["--baseline", "sauvola", "--baseline_despeckle", "4"]).baseline_despeckle == 4
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert a.despeckle == 0 and a.boxes is False and a.boxes_gap == 8 and a.boxes_min_area == 16
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--despeckle", "5", "--boxes", "--boxes_gap", "3", "--boxes_min_area", "9"])
    assert (a.despeckle, a.boxes, a.boxes_gap, a.boxes_min_area) == (5, True, 3, 9)
    new = {"v": ["--baseline_despeckle"], "n": ["--despeckle", "--boxes", "--boxes_gap", "--boxes_min_area"]}
    for tag, flags in new.items():
        acts = {s: act for act in build_parser(tag, "")._actions for s in act.option_strings}
        assert all(acts[f].help.startswith("[new]") for f in flags)
        other = {s for act in build_parser("n" if tag == "v" else "v", "")._actions for s in act.option_strings}
        assert not other & set(flags)
    for tag in "pacer":
        got = build_parser(tag, "").parse_args([] if tag != "r" else ["--cers_tess_path", "x"])
        assert not any(hasattr(got, n) for n in ("baseline_despeckle", "despeckle", "boxes", "boxes_gap", "boxes_min_area"))


def test_front_ends_refuse_what_makes_no_sense(tmp_path):
    import clean_cli
    from eval_prep import EvalPrep, build_parser
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep")
    (tmp_path / "in").mkdir()
    lead = ["--prep_path", str(tmp_path / "prep"), "--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="grey"):
        clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--method", "unet", "--despeckle", "4"]), backend=backend)
    with pytest.raises(ValueError):
        clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--method", "otsu", "--despeckle", "-2"]), backend=backend)
    with pytest.raises(ValueError):
        clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--boxes", "--boxes_gap", "128"]), backend=backend)
    base = ["--prep_path", str(tmp_path / "prep"), "--ocr", "stub"]
    with pytest.raises(ValueError):
        EvalPrep(build_parser().parse_args(base + ["--baseline_despeckle", "4"]), backend=backend, dataset=baseline_docs())
    with pytest.raises(ValueError):
        EvalPrep(build_parser().parse_args(base + ["--baseline", "otsu", "--baseline_despeckle", "-1"]), backend=backend, dataset=baseline_docs())


def expected_despeckled_result(docs, min_area, **kw):
    """the evaluation of the STATEMENTS' images (the pattern of test_binarize_cpu.expected_patch_result): each document binarised whole by
    tests/binarize_spec.py, despeckled by tests/components_spec.py, cut, read by the stub OCR"""
    import properties
    from ocr_helper.stub_helper import StubHelper
    from utils import compare_labels, get_text_stack
    ocr, correct, cer, count, changed = StubHelper(is_eval=True), 0, 0.0, 0, 0
    for image, boxes, _ in docs:
        plain = bspec.sauvola(image[0].numpy(), out="u8", **kw)
        b = spec.despeckle(plain, min_area, 8, out="float")
        changed += int(((b == 0) != (plain == 0)).sum())
        crops, labels = get_text_stack(torch.from_numpy(b)[None], boxes, properties.input_size)
        c, e = compare_labels(ocr.get_labels(crops), labels)
        correct, cer, count = correct + c, cer + e, count + len(labels)
    assert changed > 0
    return correct / count, cer / count


def test_eval_prep_baseline_despeckle_on_the_host_backend(tmp_path, capsys):
    from eval_prep import EvalPrep, build_parser
    backend, OracleUNet = host_backend()
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep")
    base = ["--prep_path", str(tmp_path / "prep"), "--ocr", "stub", "--baseline", "sauvola", "--baseline_window", "9", "--baseline_k", "0.3"]
    docs = baseline_docs()
    plain = EvalPrep(build_parser().parse_args(base), backend=backend, dataset=docs)
    plain_result = plain.eval()
    plain_out = capsys.readouterr().out
    assert "despeckle" not in plain_out and "from sauvola images" in plain_out
    ev = EvalPrep(build_parser().parse_args(base + ["--baseline_despeckle", "4"]), backend=backend, dataset=docs)
    assert ev.eval() == plain_result
    out = capsys.readouterr().out
    assert ev.baseline_result == expected_despeckled_result(docs, 4, win=9, k=0.3, R=128.0)
    assert "Correct count from sauvola+despeckle4 images: " in out and "Average CER from sauvola+despeckle4 images: (" in out
    assert [l for l in out.splitlines() if "sauvola" not in l] == [l for l in plain_out.splitlines() if "sauvola" not in l]


def scans_with_words(folder):
    from PIL import Image
    folder.mkdir()
    scans = {"a": words_page(100, 300, (10, 40, 70), 1)[0], "b": words_page(64, 129, (3, 33), 2)[0], "c": words_page(45, 200, (20,), 3)[0]}
    speck = np.random.default_rng(5).random(scans["a"].shape) < 0.002        # isolated specks for --despeckle to remove
    scans["a"] = np.where(speck, 0, scans["a"]).astype(np.uint8)
    for stem, px in scans.items():
        Image.fromarray(px).save(folder / f"{stem}.png")
    return scans


def test_clean_cli_boxes_json_round_trip(tmp_path):
    """--method otsu --despeckle 4 --boxes on the host backend: the PNGs are the statements' bytes, the JSON loads through PatchDataset, and
    every crop, cut the way utils.get_text_stack cuts, holds all ink of its component"""
    from PIL import Image
    import clean_cli
    from datasets.patch_dataset import PatchDataset
    backend, _ = host_backend()
    scans = scans_with_words(tmp_path / "in")
    args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"), "--out_dir",
                                                str(tmp_path / "out"), "--method", "otsu", "--despeckle", "4", "--boxes", "--boxes_gap", "4",
                                                "--boxes_min_area", "16", "--batch_pages", "2"])
    written = clean_cli.CleanPages(args, backend=backend).run()
    assert [p.split("/")[-1] for p in written] == ["a.png", "b.png", "c.png"]
    ds = PatchDataset(str(tmp_path / "out"))
    assert len(ds) == 3
    for i, (path, px) in enumerate(zip(written, scans.values())):
        want = spec.despeckle(bspec.otsu(px)[0], 4, 8)
        with Image.open(path) as img:
            assert np.array_equal(np.asarray(img), want)
        if i == 0:
            assert (want != bspec.otsu(px)[0]).any()
        with open(path[:-4] + ".json") as f:
            rows = json.load(f)
        smeared = spec.labels_of_ink(spec.smear(want == 0, 4, 0), 8)
        table = spec.table_fast(smeared)
        table = table[table[:, 1] >= 16]
        assert len(rows) == len(table) > 0 and all(r["label"] == "" and set(r) == {"label", "x_min", "y_min", "x_max", "y_max"} for r in rows)
        image, boxes = ds[i]
        assert len(boxes) == len(table)                        # none dropped: every word is narrower than 128 and lower than 32
        for box, t in zip(boxes, table.tolist()):
            assert [box["x_min"], box["y_min"], box["x_max"], box["y_max"]] == [t[2], t[3], t[4] + 1, t[5] + 1]
            inside = np.zeros(want.shape, bool)
            inside[box["y_min"]:box["y_max"], box["x_min"]:box["x_max"]] = True
            assert inside[smeared == t[0]].all()
            crop = image[0, box["y_min"]:box["y_max"], box["x_min"]:box["x_max"]]
            assert int((crop == 0).sum()) >= int(((smeared == t[0]) & (want == 0)).sum()) > 0
