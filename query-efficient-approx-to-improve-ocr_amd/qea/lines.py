"""Word boxes grouped into text lines and put into reading order (csrc/lines.hip), and the plain text of a page: what turns the rows of
clean_cli.py's <stem>.json, which components.word_boxes returns by each component's first pixel, into lines one can read.

The statement (tests/lines_spec.py spells it out; DESIGN.md "Text lines" says why it is exact and total, why it terminates, and what it
does not do).  Per page: n boxes (x_min, y_min, x_max, y_max), inclusive, int32, in any order.  overlap (1..100, default 50) is the per
cent of vertical overlap that puts two boxes into one height band, tall (1..64, default 3) the number of median heights above which a
box never links, gap (0..1024, default 0 = no limit) the largest horizontal gap that links, in median heights.  All arithmetic is int64.
  * h = y_max - y_min + 1, w = x_max - x_min + 1; a box with h <= 0 or w <= 0 is empty and a line of its own.
  * med = the element of rank (m - 1) // 2 among the ascending heights of the m non-empty boxes (0 if there is none); a non-empty box is
    linkable iff h <= tall * med: a rule, a picture or a drop cap is a line of its own and cannot bridge two lines.
  * Two linkable boxes are in one band iff 100 * ov >= overlap * min(h_i, h_j), ov = min(y_max_i, y_max_j) - max(y_min_i, y_min_j) + 1.
  * Under the key (x_min_i, i), succ(i) is the box of i's band with the smallest key above i's, pred(i) the one with the largest key
    below it; i links to succ(i) iff gap == 0 or x_min_succ - x_max_i - 1 <= gap * med, and to pred(i) likewise.
  * A line is a connected component of the links; its box is the union of its members' boxes; lines are numbered ascending by
    (y_min + y_max, x_min, smallest member) of their boxes; a box's position is its rank under (line, x_min, y_min, index).
The rule is local, only neighbours along x link, so it is meant for pages that are level or deskewed (clean_cli.py --deskew leaves at
most about 1 / 1024).  All of it is integer work: the device, the host path below and the statement agree bit for bit.

CUDA tables (or a CUDA `device`) go through ONE launch for all pages of the call (qea.ops.line_group) and one read of the line counts,
which sizes the result.  CPU tables run the host path, numpy over blocks of rows so that a page of 4096 boxes never needs an n x n int64
matrix at once.  QEA_LINES=host sends CUDA tables through the host path too (an A/B switch like QEA_ALIGN=host).
"""
import os

import numpy as np
import torch

from .pages import is_int

MAX_BOXES, MAX_TALL, MAX_GAP = 4096, 64, 1024      # QEA_LINE_MAX_* of include/qea_hip.h
_BLOCK = 256                                       # rows of the pair matrices held at once: 256 x 4096 int64 = 8 MB each


def use_host():
    return os.environ.get("QEA_LINES", "device") == "host"


def check_params(overlap=50, tall=3, gap=0):
    """ValueError for parameters outside the statement's ranges, before any work"""
    if not is_int(overlap) or not 1 <= overlap <= 100:
        raise ValueError(f"overlap={overlap!r}: an integer in 1..100")
    if not is_int(tall) or not 1 <= tall <= MAX_TALL:
        raise ValueError(f"tall={tall!r}: an integer in 1..{MAX_TALL}")
    if not is_int(gap) or not 0 <= gap <= MAX_GAP:
        raise ValueError(f"gap={gap!r}: an integer in 0..{MAX_GAP}")


# ---------------------------------------------------------------------------------------------------------------- the host path
def group_host(boxes, overlap=50, tall=3, gap=0):
    """One page, int [n, 4] (numpy) -> dict(line, pos, order: int32 [n]; line_boxes: int32 [L, 4]; med: int)"""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    n = b.shape[0]
    if n > MAX_BOXES:
        raise ValueError(f"a page of {n} boxes: at most {MAX_BOXES}")
    x0, y0, x1, y1 = b.T
    h, w, idx = y1 - y0 + 1, x1 - x0 + 1, np.arange(n)
    some = (h > 0) & (w > 0)
    heights = np.sort(h[some])
    med = int(heights[(heights.size - 1) // 2]) if heights.size else 0
    ok = np.flatnonzero(some & (h <= tall * med))              # the linkable boxes
    # a key (x_min, i) as one integer: i < 4096 = 2^12, so x_min * 4096 + i keeps the lexicographic order, within int64
    key = x0[ok] * MAX_BOXES + ok
    far = np.int64(2) ** 62
    succ, pred = np.full(n, -1), np.full(n, -1)
    for a in range(0, ok.size, _BLOCK):
        i = ok[a:a + _BLOCK, None]
        ov = np.minimum(y1[i], y1[ok]) - np.maximum(y0[i], y0[ok]) + 1
        band = 100 * ov >= overlap * np.minimum(h[i], h[ok])
        after = np.where(band & (key > key[a:a + _BLOCK, None]), key, far)
        before = np.where(band & (key < key[a:a + _BLOCK, None]), key, -far)
        s, p = after.argmin(1), before.argmax(1)
        succ[i[:, 0]] = np.where(after[np.arange(i.size), s] < far, ok[s], -1)
        pred[i[:, 0]] = np.where(before[np.arange(i.size), p] > -far, ok[p], -1)
    linked = (succ >= 0) & ((gap == 0) | (x0[succ] - x1 - 1 <= gap * med))
    u, v = idx[linked], succ[linked]
    linked = (pred >= 0) & ((gap == 0) | (x0 - x1[pred] - 1 <= gap * med))
    u, v = np.concatenate([u, idx[linked]]), np.concatenate([v, pred[linked]])
    lab = idx.copy()
    while u.size:                                              # hook both ends and their labels to the smaller label, then jump; labels only fall
        m = np.minimum(lab[u], lab[v])
        new = lab.copy()
        for t in (u, v, lab[u], lab[v]):
            np.minimum.at(new, t, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    roots, inv = np.unique(lab, return_inverse=True)           # a label is the smallest index of its line
    lb = np.empty((roots.size, 4), np.int64)
    lb[:, :2], lb[:, 2:] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    np.minimum.at(lb[:, 0], inv, x0)
    np.minimum.at(lb[:, 1], inv, y0)
    np.maximum.at(lb[:, 2], inv, x1)
    np.maximum.at(lb[:, 3], inv, y1)
    by = np.lexsort((roots, lb[:, 0], lb[:, 1] + lb[:, 3]))    # the last key is the primary one
    number = np.empty(roots.size, np.int64)
    number[by] = np.arange(roots.size)
    line = number[inv.reshape(-1)]
    order = np.lexsort((idx, y0, x0, line))
    pos = np.empty(n, np.int64)
    pos[order] = idx
    return dict(line=line.astype(np.int32), pos=pos.astype(np.int32), order=order.astype(np.int32), line_boxes=lb[by].astype(np.int32),
                med=med)


# ---------------------------------------------------------------------------------------------------------------- the interface
def group_lines(boxes_per_page, overlap=50, tall=3, gap=0, device=None):
    """boxes_per_page: per page an int32 [n, 4] tensor = (x_min, y_min, x_max, y_max), inclusive, as components.word_boxes returns them
    -> per page (order, line, line_boxes): order int32 [n], the boxes' indices in reading order; line int32 [n], every box's line;
    line_boxes int32 [L, 4], the lines' boxes in line order; on `device` if given, else where the boxes are"""
    check_params(overlap, tall, gap)
    tables = [torch.as_tensor(t, dtype=torch.int32).reshape(-1, 4) for t in boxes_per_page]
    counts = [t.shape[0] for t in tables]
    if max(counts, default=0) > MAX_BOXES:
        raise ValueError(f"a page of {max(counts)} boxes: at most {MAX_BOXES}")
    dev = torch.device(device) if device is not None else (tables[0].device if tables else torch.device("cpu"))
    if dev.type != "cuda" or use_host():
        out = []
        for t in tables:
            r = group_host(t.cpu().numpy(), overlap, tall, gap)
            out.append(tuple(torch.from_numpy(r[k]).to(dev) for k in ("order", "line", "line_boxes")))
        return out
    if not tables:
        return []
    from . import ops
    first = np.concatenate([[0], np.cumsum(counts)]).tolist()
    table = torch.cat([t.to(dev) for t in tables])
    box_first = torch.tensor(first, dtype=torch.int32).to(dev)
    res = ops.line_group(table, box_first, max(counts), overlap, tall, gap)
    n_lines = res.n_lines.cpu().tolist()                       # the one read: sizes the result
    return [(res.order[a:b], res.line[a:b], res.line_box[a:a + L]) for a, b, L in zip(first[:-1], first[1:], n_lines)]


def page_text(texts, order, line):
    """texts: a page's strings in box order; order, line: what group_lines returned for the page -> the page as a str: the words of a
    line joined by one space, the lines by a newline; empty strings are skipped and a line with no word left is dropped"""
    order = order.tolist() if hasattr(order, "tolist") else list(order)
    line = line.tolist() if hasattr(line, "tolist") else list(line)
    if not len(texts) == len(order) == len(line):
        raise ValueError(f"{len(texts)} strings, {len(order)} positions and {len(line)} line numbers")
    rows = {}
    for i in order:
        if texts[i]:
            rows.setdefault(line[i], []).append(texts[i])
    return "\n".join(" ".join(rows[k]) for k in sorted(rows))
