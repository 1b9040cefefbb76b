"""Text lines on the host (qea/lines.py): the numpy path against the statement tests/lines_spec.py bit for bit on every case the device
test runs and on hand-worked pages, the synthetic-text property the statement was chosen for, page_text, the flags of clean_cli.py and a
run of --lines --text --read on the host backend with the oracle CRNN, and the header."""
import json

import numpy as np
import pytest
import torch

import lines_spec as spec

KEYS = ("line", "pos", "order")


def host(boxes, params=spec.DEFAULTS):
    from qea.lines import group_host
    return group_host(np.array(boxes, np.int64).reshape(-1, 4), *params)


def assert_is_spec(got, want):
    for k in KEYS:
        assert got[k].dtype == np.int32 and got[k].tolist() == want[k], k
    assert got["line_boxes"].dtype == np.int32 and [tuple(r) for r in got["line_boxes"].tolist()] == want["line_boxes"]
    assert got["med"] == want["med"] and isinstance(got["med"], int)


def lines_of(r):
    """the lines as sets of box indices, in line order"""
    line = list(r["line"])
    return [{i for i, l in enumerate(line) if l == k} for k in range(max(line, default=-1) + 1)]


# ------------------------------------------------------------------------------------------------------------------ against the statement
@pytest.mark.parametrize("name", spec.CASE_NAMES)
def test_the_host_path_is_the_statement_bit_for_bit(name):
    boxes, params, want = spec.case(name)
    assert_is_spec(host(boxes, params), want)


def test_nine_pages_are_the_statement():
    for k, n in enumerate(spec.NINE_PAGES):
        boxes = spec.text_like(n, 100 + k)
        assert_is_spec(host(boxes), spec.group(boxes))


@pytest.mark.parametrize("name", [n for n in spec.CASE_NAMES if not n.startswith("stairs") and "/409" not in n])
def test_the_window_of_the_statement_loses_no_pair(name):
    """the statement's default looks at one window of the boxes sorted by y_min: the same result as trying every pair"""
    boxes, params, want = spec.case(name)
    assert spec.group(boxes, *params, prune=False) == want


def test_the_cases_are_not_vacuous():
    """the random pages hold what they were built to hold, and the parameter sets decide differently on them"""
    boxes, _, r = spec.case("count/4096/0")
    h = [b[3] - b[1] + 1 for b in boxes]
    assert sum(b[2] < b[0] or b[3] < b[1] for b in boxes) > 20 and sum(x <= 0 for x in h) > 2
    assert sum(x > 3 * r["med"] for x in h) > 20 and len(set(boxes)) < len(boxes)
    assert 60 < len(r["line_boxes"]) < 1500 and max(len(s) for s in lines_of(r)) > 10
    assert any(s is not None and spec.case("count/4096/0")[2]["pred"][s] != i for i, s in enumerate(r["succ"]))   # succ is not symmetric
    per_params = [len(spec.group(spec.text_like(257, 0), *p)["line_boxes"]) for p in spec.PARAMS]
    assert len(set(per_params)) == len(per_params)
    assert len(spec.case("stairs/0")[2]["line_boxes"]) == 1 and len(spec.case("stairs/1")[2]["line_boxes"]) == spec.MAX_BOXES
    assert spec.case("stairs/0")[2]["order"] == list(range(spec.MAX_BOXES))


# ------------------------------------------------------------------------------------------------------------------ by hand
def test_two_words_and_a_hyphen():
    boxes = [(65, 0, 110, 19), (55, 9, 60, 11), (0, 0, 50, 19)]
    r = host(boxes)
    assert r["med"] == 20 and r["line"].tolist() == [0, 0, 0] and r["order"].tolist() == [2, 1, 0] and r["pos"].tolist() == [2, 1, 0]
    assert r["line_boxes"].tolist() == [[0, 0, 110, 19]]
    assert_is_spec(r, spec.group(boxes))
    # the hyphen hangs too low for the left word but not for the right one: succ(left) is the right word, whose pred is the hyphen
    low = [(65, 4, 110, 23), (55, 18, 60, 23), (0, 0, 50, 19)]
    s = spec.group(low)
    assert (s["succ"][2], s["pred"][0], s["pred"][1], s["succ"][1]) == (0, 1, None, 0) and s["line"] == [0, 0, 0]
    assert_is_spec(host(low), s)


def test_a_tall_rule_through_three_lines_is_a_line_of_its_own():
    words = [(x, y, x + 40, y + 19) for y in (0, 40, 80) for x in (0, 60, 140, 200)]
    rule = (110, 0, 112, 99)                                   # 100 rows > 3 * 20: never links, so it cannot bridge the three lines
    r = host(words + [rule])
    assert r["med"] == 20
    assert lines_of(r) == [{0, 1, 2, 3}, {4, 5, 6, 7}, {12}, {8, 9, 10, 11}]       # y_min + y_max = 19, 99, 99 (the rule: x_min 110 after 0), 179
    assert r["line_boxes"].tolist() == [[0, 0, 240, 19], [0, 40, 240, 59], [110, 0, 112, 99], [0, 80, 240, 99]]
    assert r["order"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 12, 8, 9, 10, 11]
    assert_is_spec(r, spec.group(words + [rule]))
    bridged = host(words + [rule], (50, 64, 0))                # allowed to link, the rule joins all three
    assert len(bridged["line_boxes"]) == 1


def test_the_band_threshold_is_met_exactly_or_missed_by_one_row():
    at = [(0, 0, 10, 19), (20, 10, 30, 29)]                    # ov = 10: 100 * 10 == 50 * 20
    short = [(0, 0, 10, 19), (20, 11, 30, 30)]                 # ov = 9
    assert host(at)["line"].tolist() == [0, 0] and host(short)["line"].tolist() == [0, 1]
    assert host(at, (51, 3, 0))["line"].tolist() == [0, 1] and host(short, (45, 3, 0))["line"].tolist() == [0, 0]
    uneven = [(0, 0, 10, 29), (20, 27, 30, 32)]                # heights 30 and 6, ov = 3: 300 == 50 * 6
    assert host(uneven, (50, 5, 0))["line"].tolist() == [0, 0] and host(uneven, (51, 5, 0))["line"].tolist() == [0, 1]
    assert host(uneven, (50, 4, 0))["line"].tolist() == [0, 1]             # med = 6: at tall = 4 the box of 30 rows never links
    for boxes in (at, short, uneven):
        assert_is_spec(host(boxes, (50, 5, 0)), spec.group(boxes, 50, 5, 0))


def test_the_gap_threshold_is_met_exactly_or_missed_by_one_column():
    at = [(0, 0, 10, 19), (51, 0, 70, 19)]                     # 51 - 10 - 1 = 40 == 2 * 20
    far = [(0, 0, 10, 19), (52, 0, 70, 19)]
    assert host(at, (50, 3, 2))["line"].tolist() == [0, 0] and host(far, (50, 3, 2))["line"].tolist() == [0, 1]
    assert host(far, (50, 3, 0))["line"].tolist() == [0, 0] and host(far, (50, 3, 3))["line"].tolist() == [0, 0]
    overlapping = [(0, 0, 100, 19), (5, 0, 20, 19)]            # a negative gap links at any positive limit
    assert host(overlapping, (50, 3, 1))["line"].tolist() == [0, 0]
    for boxes in (at, far, overlapping):
        assert_is_spec(host(boxes, (50, 3, 2)), spec.group(boxes, 50, 3, 2))


def test_ties_identical_nested_empty_and_extreme_boxes():
    boxes, _, r = spec.case("hand/equal_x_min")
    assert r["succ"][:3] == [1, 2, 3] and r["pred"][:3] == [None, 0, 1]       # the keys (10, 0) < (10, 1) < (10, 2) < (50, 3)
    assert r["line"] == [0] * 4 and r["order"] == [0, 2, 1, 3]               # within the line by (x_min, y_min, index)
    r = host(spec.case("hand/identical")[0])
    assert r["line"].tolist() == [0] * 9 and r["order"].tolist() == list(range(9)) and r["line_boxes"].tolist() == [[5, 5, 40, 24]]
    r = host(spec.case("hand/nested")[0])
    assert r["med"] == 30 and r["line"].tolist() == [0] * 5 and r["order"].tolist() == [0, 1, 2, 3, 4]
    boxes = spec.case("hand/empty_boxes")[0]
    r = host(boxes)
    assert r["med"] == 20 and lines_of(r) == [{6}, {5}, {3}, {0, 2, 4}, {1}]      # y_min + y_max = -1, 9, 9, 19, 19, then x_min
    assert [list(boxes[i]) in r["line_boxes"].tolist() for i in (1, 3, 5, 6)] == [True] * 4      # an empty box's line box is its own
    r = host(spec.case("hand/all_empty")[0])
    assert r["med"] == 0 and sorted(r["line"].tolist()) == [0, 1]
    boxes, params, want = spec.case("hand/extremes_huge")
    # heights 2^32, 2^32 - 1, 2^31, 2^32: med is a height that no int32 holds, and only boxes 1 and 2 are linkable at tall = 1; their
    # overlap is 2^31 - 1 rows, 100 times which is >= 50 * 2^31, and box 2 starts left of box 1: a negative gap links
    assert want["med"] == 2 ** 32 - 1 and want["succ"] == [None, None, 1, None] and want["line"][1] == want["line"][2]
    assert len(want["line_boxes"]) == 3 and host(boxes, params)["med"] == 2 ** 32 - 1


def test_no_box_and_one_box():
    r = host([])
    assert all(r[k].shape == (0,) for k in KEYS) and r["line_boxes"].shape == (0, 4) and r["med"] == 0
    r = host([(3, 4, 9, 8)])
    assert [r[k].tolist() for k in KEYS] == [[0]] * 3 and r["line_boxes"].tolist() == [[3, 4, 9, 8]] and r["med"] == 5


# ------------------------------------------------------------------------------------------------------------------ the property
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("slope", [0, 0.01, 0.03])
def test_synthetic_text_gives_the_true_lines_in_reading_order(slope, gap):
    """12 lines across 2000 columns, x-height 20, ascenders and descenders, pitch 34, shuffled, seeds 0..19: the lines are the true lines,
    numbered top to bottom, and the order reads each of them left to right"""
    for seed in range(20):
        boxes, truth = spec.synthetic_page(seed, slope)
        assert len(boxes) > 150 and len(set(truth)) == 12
        r = host(boxes, (50, 3, gap))
        assert r["line"].tolist() == truth, (seed, slope, gap)
        read = r["order"].tolist()
        assert [truth[i] for i in read] == sorted(truth)
        assert all(boxes[a][0] < boxes[b][0] for a, b in zip(read, read[1:]) if truth[a] == truth[b])
        if seed < 2:
            assert_is_spec(r, spec.group(boxes, 50, 3, gap))


# ------------------------------------------------------------------------------------------------------------------ the interface
def test_group_lines_and_its_refusals(monkeypatch):
    from qea import lines
    pages = [spec.text_like(n, 5) for n in (0, 7, 64)]
    tensors = [torch.tensor(p, dtype=torch.int32).reshape(-1, 4) for p in pages]
    for env in (None, "host"):
        if env:
            monkeypatch.setenv("QEA_LINES", env)
        got = lines.group_lines(tensors, 34, 2, 3)
        for p, (order, line, line_boxes) in zip(pages, got):
            want = spec.group(p, 34, 2, 3)
            assert order.dtype == line.dtype == line_boxes.dtype == torch.int32 and order.device.type == "cpu"
            assert (order.tolist(), line.tolist(), [tuple(r) for r in line_boxes.tolist()]) == (want["order"], want["line"], want["line_boxes"])
    assert lines.group_lines([]) == []
    for bad in (dict(overlap=0), dict(overlap=101), dict(tall=0), dict(tall=65), dict(gap=-1), dict(gap=1025), dict(overlap=50.0), dict(tall=True)):
        with pytest.raises(ValueError):
            lines.check_params(**bad)
        with pytest.raises(ValueError):
            lines.group_lines(tensors, **bad)
    lines.check_params(1, 64, 1024)
    with pytest.raises(ValueError, match="4096"):
        lines.group_lines([torch.zeros(4097, 4, dtype=torch.int32)])
    with pytest.raises(ValueError, match="4096"):
        lines.group_host(np.zeros((4097, 4), np.int64))


def test_page_text_by_hand():
    from qea.lines import page_text
    texts = ["world", "hello", "", "line", "second", ""]
    order, line = [1, 0, 2, 4, 3, 5], [0, 0, 0, 2, 2, 1]
    assert page_text(texts, order, line) == "hello world\nsecond line"          # the empty word is skipped, line 1 has no word left
    assert page_text(texts, torch.tensor(order), torch.tensor(line)) == "hello world\nsecond line"
    assert page_text([], [], []) == "" and page_text(["", ""], [1, 0], [0, 1]) == ""
    assert page_text(["a b", "c"], [1, 0], [1, 0]) == "c\na b"
    with pytest.raises(ValueError):
        page_text(["a"], [0, 1], [0, 0])


# ------------------------------------------------------------------------------------------------------------------ the front end
LINE_FLAGS = ["--lines", "--lines_overlap", "--lines_tall", "--lines_gap", "--text"]


def test_flags_of_the_front_end(tmp_path):
    import clean_cli
    import test_word_strips_cpu as W
    from qea.cli_flags import build_parser
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert (a.lines, a.lines_overlap, a.lines_tall, a.lines_gap, a.text) == (False, None, None, None, False)
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--lines", "--lines_overlap", "34", "--lines_tall", "2", "--lines_gap",
                                             "3", "--text"])
    assert (a.lines, a.lines_overlap, a.lines_tall, a.lines_gap, a.text) == (True, 34, 2, 3, True)
    acts = {s: act for act in build_parser("n", "")._actions for s in act.option_strings}
    assert all(acts[f].help.startswith("[new]") for f in LINE_FLAGS)
    for tag in "pacerv":
        assert not {s for act in build_parser(tag, "")._actions for s in act.option_strings} & set(LINE_FLAGS)
    backend, OracleCRNN = W.host_backend()
    torch.save(OracleCRNN(95).eval(), tmp_path / "crnn")
    (tmp_path / "in").mkdir()
    lead = ["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--method", "otsu"]
    read = ["--read", str(tmp_path / "crnn")]
    for bad in (["--lines_overlap", "50"], ["--lines_tall", "3"], ["--lines_gap", "0"], ["--boxes", "--lines_gap", "2"]):
        with pytest.raises(ValueError, match="--lines"):
            clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + bad), backend=backend)
    for bad in (["--text"], ["--text", "--lines"]):
        with pytest.raises(ValueError, match="--text"):
            clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + bad), backend=backend)
    for bad in (["--lines_overlap", "0"], ["--lines_overlap", "101"], ["--lines_tall", "65"], ["--lines_gap", "1025"], ["--lines_gap", "-1"]):
        with pytest.raises(ValueError):
            clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--lines"] + bad), backend=backend)
    ok = clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--lines"]), backend=backend)
    assert ok.boxes and ok.lines and not ok.text and ok.lines_params == (50, 3, 0)
    ok = clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + read + ["--text", "--lines_gap", "4", "--lines_overlap", "1"]), backend=backend)
    assert ok.boxes and ok.lines and ok.text and ok.lines_params == (1, 3, 4)
    plain = clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--boxes"]), backend=backend)
    assert not plain.lines and not plain.text


def test_clean_cli_lines_and_text_on_the_host_backend(tmp_path, capsys):
    """--read --lines --text with the oracle CRNN: the JSON rows are those of the run without --lines, in the statement's reading order
    and with their line; the .txt is page_text of the labels; without --lines the files are what they were"""
    import clean_cli
    import test_word_strips_cpu as W
    from datasets.patch_dataset import PatchDataset
    from qea.components import word_boxes
    from qea.lines import page_text
    from PIL import Image
    backend, OracleCRNN = W.host_backend()
    torch.save(OracleCRNN(95, seed=4).eval(), tmp_path / "crnn")
    scans = W.word_scans(tmp_path / "in")
    read = ["--read", str(tmp_path / "crnn"), "--read_buckets", "64", "128"]
    boxes_only = clean_cli.CleanPages(W.cli_args(tmp_path, "boxes", "--boxes"), backend=backend).run()
    plain = clean_cli.CleanPages(W.cli_args(tmp_path, "plain", *read), backend=backend).run()
    assert " lines\n" not in capsys.readouterr().out
    grouped = clean_cli.CleanPages(W.cli_args(tmp_path, "grouped", "--lines"), backend=backend).run()
    text = clean_cli.CleanPages(W.cli_args(tmp_path, "text", "--text", *read), backend=backend).run()
    printed = capsys.readouterr().out
    reordered = 0
    for stem, b, p, g, t in zip(scans, boxes_only, plain, grouped, text):
        with open(b, "rb") as f0, open(p, "rb") as f1, open(g, "rb") as f2, open(t, "rb") as f3:
            assert f0.read() == f1.read() == f2.read() == f3.read()                 # the PNG bytes
        with Image.open(b) as img:
            (found,) = word_boxes([torch.from_numpy(np.asarray(img).copy())], gap_x=2, min_area=16)
        before = [dict(label="", x_min=x0, y_min=y0, x_max=x1 + 1, y_max=y1 + 1) for x0, y0, x1, y1 in found.tolist()]
        with open(b[:-4] + ".json") as f:
            assert f.read() == json.dumps(before)                                  # without --lines: the bytes of the format before it
        want = spec.group(found.tolist())
        rows, with_labels, read_rows = (json.load(open(path[:-4] + ".json")) for path in (g, p, t))
        assert rows == [dict(before[i], line=want["line"][i]) for i in want["order"]]
        assert [r["line"] for r in rows] == sorted(r["line"] for r in rows)
        assert read_rows == [dict(with_labels[i], line=want["line"][i]) for i in want["order"]]    # read in the order read_pages was given
        assert not any(path.endswith(".txt") for path in map(str, (tmp_path / "grouped").iterdir()))
        with open(t[:-4] + ".txt") as f:
            got = f.read()
        assert got == page_text([r["label"] for r in with_labels], want["order"], want["line"])
        assert got.split() == " ".join(r["label"] for r in read_rows).split()
        assert f"{stem}: {len(want['line_boxes'])} lines\n" in printed
        reordered += want["order"] != sorted(want["order"])
    assert reordered >= 1                                                          # page a: the tall word sorts first by root, second by line
    for folder in ("grouped", "text"):
        ds = PatchDataset(str(tmp_path / folder), pad=True)
        assert len(ds) == 3
        ds[0]


def test_the_header_declares_the_entry_point():
    import inspect
    from qea import _lib, lines, ops
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    assert len(protos["qea_line_group"]) == 15 and hasattr(_lib.lib(), "qea_line_group") and _lib.lib().qea_version() == 9
    text = open(_lib.HEADER_PATH).read()
    assert "#define QEA_LINE_MAX_BOXES 4096" in text and "#define QEA_LINE_MAX_TALL 64" in text and "#define QEA_LINE_MAX_GAP 1024" in text
    assert (ops.LINE_MAX_BOXES, ops.LINE_MAX_TALL, ops.LINE_MAX_GAP) == (lines.MAX_BOXES, lines.MAX_TALL, lines.MAX_GAP) == (4096, 64, 1024)
    assert set(ops.LINE_LAUNCHES) == {"group"}
    assert list(inspect.signature(ops.line_group).parameters) == ["boxes", "box_first", "max_boxes", "overlap", "tall", "gap"]
