"""Text lines on the MI355X (csrc/lines.hip): line, pos, order, the line boxes and med bit for bit the statement tests/lines_spec.py over
the boundary counts at four parameter sets, nine pages in one call, the longest chain there is, the hand cases, a page over the caller's
cap, the product interface against its host path, and the refusals of the C ABI.  Every call goes through buffers with guard words
before and after each output, which must come back intact."""
import ctypes as C

import numpy as np
import pytest
import torch

import lines_spec as spec
from test_binarize_cpu import host_backend
from test_components_cpu import scans_with_words, words_page

pytestmark = pytest.mark.gpu

GUARD, MARK = 64, -7777                     # guard elements on either side of every output, and what they hold
OUTPUTS = ("line", "pos", "order", "line_box", "n_lines", "med")


def run(pages, params=spec.DEFAULTS, max_boxes=None):
    """one call of qea_line_group over `pages` (lists of boxes) -> dict of numpy arrays, after checking every guard word"""
    from qea import _lib
    counts = [len(p) for p in pages]
    N, P = sum(counts), len(pages)
    flat = [b for p in pages for b in p]
    boxes = torch.tensor(flat, dtype=torch.int64).reshape(-1, 4).to(torch.int32).cuda()
    first = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    shapes = dict(line=(N, torch.int32), pos=(N, torch.int32), order=(N, torch.int32), line_box=(4 * N, torch.int32), n_lines=(P, torch.int32),
                  med=(P, torch.int64))
    bufs = {k: torch.full((n + 2 * GUARD,), MARK, dtype=dt, device="cuda") for k, (n, dt) in shapes.items()}
    ptr = {k: bufs[k].data_ptr() + GUARD * bufs[k].element_size() for k in bufs}
    rc = _lib.lib().qea_line_group(boxes.data_ptr() if N else None, first.data_ptr(), P, N, max(counts, default=0) if max_boxes is None else max_boxes,
                                   *params, *(ptr[k] for k in OUTPUTS), None)
    assert rc == 0, _lib.lib().qea_last_error()
    torch.cuda.synchronize()
    out = {}
    for k, (n, _) in shapes.items():
        host = bufs[k].cpu().numpy()
        assert (host[:GUARD] == MARK).all() and (host[GUARD + n:] == MARK).all(), f"{k}: a guard word was written"
        out[k] = host[GUARD:GUARD + n]
    out["line_box"] = out["line_box"].reshape(-1, 4)
    return out, np.concatenate([[0], np.cumsum(counts)]).tolist()


def assert_pages(out, first, wants):
    """every page of a call against the statement; a `want` of None is a page that must hold -1 throughout"""
    for p, (a, b, want) in enumerate(zip(first[:-1], first[1:], wants)):
        if want is None:
            assert all((out[k][a:b] == -1).all() for k in ("line", "pos", "order", "line_box")) and out["n_lines"][p] == out["med"][p] == -1
            continue
        L = len(want["line_boxes"])
        for k in ("line", "pos", "order"):
            assert out[k][a:b].tolist() == want[k], (p, k)
        assert [tuple(r) for r in out["line_box"][a:a + L].tolist()] == want["line_boxes"] and (out["line_box"][a + L:b] == -1).all(), p
        assert out["n_lines"][p] == L and out["med"][p] == want["med"], p


@pytest.mark.parametrize("name", spec.CASE_NAMES)
def test_every_output_is_the_statement_bit_for_bit(name):
    """the boundary counts at the four parameter sets, the two staircases of 4096 boxes and the hand cases, a page per call"""
    boxes, params, want = spec.case(name)
    out, first = run([boxes], params)
    assert_pages(out, first, [want])


def test_nine_pages_in_one_call():
    """empty pages first, last and in the middle; the pages do not see each other"""
    pages = [spec.text_like(n, 100 + k) for k, n in enumerate(spec.NINE_PAGES)]
    out, first = run(pages)
    assert_pages(out, first, [spec.group(p) for p in pages])
    assert out["n_lines"].tolist()[0::3] == [0, 0, 0] and out["med"].tolist()[0::3] == [0, 0, 0]


def test_a_page_over_the_cap_is_marked_and_the_others_are_right():
    """max_boxes is the OTHER pages' maximum: the page of max_boxes + 1 boxes holds -1 throughout, nothing around it is touched"""
    counts = [5, 64, 65, 0, 33]
    pages = [spec.text_like(n, 200 + k) for k, n in enumerate(counts)]
    out, first = run(pages, max_boxes=64)
    assert_pages(out, first, [None if len(p) > 64 else spec.group(p) for p in pages])
    out, first = run(pages, (34, 2, 3), max_boxes=0)           # no table at all: only the empty page is within the cap
    assert_pages(out, first, [spec.group(p, 34, 2, 3) if not p else None for p in pages])


def test_group_lines_on_the_device_is_its_host_path(monkeypatch):
    from qea import lines, ops
    pages = [spec.text_like(n, 300 + k) for k, n in enumerate((70, 0, 1, 513))]
    cpu = [torch.tensor(p, dtype=torch.int32).reshape(-1, 4) for p in pages]
    before = dict(ops.LINE_LAUNCHES)
    got = lines.group_lines([t.cuda() for t in cpu], 34, 2, 3)
    assert {k: ops.LINE_LAUNCHES[k] - before[k] for k in before} == {"group": 1}        # one launch, whatever the pages hold
    on_host = lines.group_lines(cpu, 34, 2, 3)
    moved = lines.group_lines(cpu, 34, 2, 3, device="cuda")
    monkeypatch.setenv("QEA_LINES", "host")
    before = dict(ops.LINE_LAUNCHES)
    switched = lines.group_lines([t.cuda() for t in cpu], 34, 2, 3)
    assert ops.LINE_LAUNCHES == before
    for p, want in enumerate(on_host):
        for other in (got, moved, switched):
            assert all(o.is_cuda and o.dtype == torch.int32 and torch.equal(o.cpu(), w) for o, w in zip(other[p], want)), p
    assert [len(lb) for _, _, lb in got] == [len(spec.group(p, 34, 2, 3)["line_boxes"]) for p in pages]
    empty = lines.group_lines([torch.zeros(0, 4, dtype=torch.int32, device="cuda")] * 2)
    assert [tuple(t.shape) for page in empty for t in page] == [(0,), (0,), (0, 4)] * 2


def test_word_boxes_into_group_lines_on_rendered_words():
    """three rendered lines of words, boxes by word_boxes on the device in root order: the lines are the rendered lines, read left to right"""
    from qea.components import word_boxes
    from qea.lines import group_lines
    page, want = words_page(h=100, w=300, lines=(10, 40, 70), seed=3)
    tall, _ = words_page(h=130, w=500, lines=(6, 31, 57, 90, 112), seed=4)
    boxes = word_boxes([torch.from_numpy(page).cuda(), torch.from_numpy(tall).cuda()], gap_x=4, min_area=16)
    (order, line, line_boxes), (order2, line2, line_boxes2) = group_lines(boxes)
    assert boxes[0][order.long()].cpu().tolist() == want.tolist()              # words_page lists its words in reading order
    assert line_boxes[:, 1].tolist() == [10, 40, 70] and line_boxes2[:, 1].tolist() == [6, 31, 57, 90, 112]
    assert line[order.long()].tolist() == sorted(line.tolist()) and len(line2) == len(boxes[1]) > 40
    for b, got in zip(boxes, ((order, line, line_boxes), (order2, line2, line_boxes2))):
        s = spec.group(b.cpu().tolist())
        assert (got[0].tolist(), got[1].tolist(), [tuple(r) for r in got[2].tolist()]) == (s["order"], s["line"], s["line_boxes"])


def test_clean_cli_lines_on_the_device(tmp_path):
    """--boxes --lines on the device writes the JSON of the host-backend run"""
    import json
    import clean_cli
    backend, _ = host_backend()
    scans_with_words(tmp_path / "in")
    written = {}
    for name, be in (("host", backend), ("device", None)):
        args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "none"), "--in_dir", str(tmp_path / "in"), "--out_dir",
                                                    str(tmp_path / name), "--method", "otsu", "--lines", "--boxes_gap", "4", "--batch_pages", "2"])
        written[name] = clean_cli.CleanPages(args, backend=be).run()
    for a, b in zip(written["host"], written["device"]):
        with open(a[:-4] + ".json") as x, open(b[:-4] + ".json") as y:
            rows = json.load(y)
            assert rows == json.load(x) and len(rows) > 0 and all("line" in r for r in rows)


def test_library_refusals_launch_nothing():
    """the C ABI with real device buffers: every refusal returns a negative code and a text, and leaves the prefilled buffers untouched"""
    from qea import _lib
    L = _lib.lib()
    boxes = torch.tensor(spec.text_like(8, 1), dtype=torch.int32).cuda()
    first = torch.tensor([0, 8], dtype=torch.int32).cuda()
    outs = {k: torch.full((32,), MARK, dtype=torch.int64 if k == "med" else torch.int32, device="cuda") for k in OUTPUTS}

    def call(bx=boxes.data_ptr(), bf=first.data_ptr(), n_pages=1, n_boxes=8, max_boxes=8, overlap=50, tall=3, gap=0, **ptrs):
        p = {k: outs[k].data_ptr() for k in OUTPUTS}
        p.update(ptrs)
        return L.qea_line_group(bx, bf, n_pages, n_boxes, max_boxes, overlap, tall, gap, *(p[k] for k in OUTPUTS), None)
    bad = [dict(bx=None), dict(bf=None), dict(n_pages=-1), dict(n_boxes=-1), dict(max_boxes=-1), dict(max_boxes=4097), dict(overlap=0), dict(overlap=101),
           dict(tall=0), dict(tall=65), dict(gap=-1), dict(gap=1025), dict(n_pages=0), dict(bx=boxes.data_ptr() + 4), dict(bf=first.data_ptr() + 2),
           dict(line_box=outs["line_box"].data_ptr() + 8), dict(med=outs["med"].data_ptr() + 4), dict(pos=outs["pos"].data_ptr() + 1)]
    bad += [{k: None} for k in OUTPUTS]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert b"qea_line_group" in L.qea_last_error(), kw
    assert call(n_pages=0, n_boxes=0) == 0                     # no page: accepted, nothing happens
    torch.cuda.synchronize()
    assert all(bool((t == MARK).all()) for t in outs.values())
    assert call(n_pages=1, n_boxes=0, bx=None, line=None, pos=None, order=None, line_box=None) == 0      # no box: the counts are cleared
    torch.cuda.synchronize()
    assert outs["n_lines"][:2].tolist() == [0, MARK] and outs["med"][:2].tolist() == [0, MARK]
    assert all(bool((outs[k] == MARK).all()) for k in ("line", "pos", "order", "line_box"))
    assert call() == 0                                         # and the accepted call writes the page
    torch.cuda.synchronize()
    want = spec.group(boxes.cpu().tolist())
    assert outs["line"][:8].tolist() == want["line"] and outs["order"][:8].tolist() == want["order"] and int(outs["line"][8]) == MARK
