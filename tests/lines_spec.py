"""The statement "Text lines"  in plain Python loops over Python integers: what csrc/lines.hip and the host path of
qea/lines.py are held to bit for bit.  Written for reading; it imports nothing of the library it checks.

Per page the input is n boxes (x_min, y_min, x_max, y_max), inclusive, any int32 values, in any order; the parameters are overlap
(1..100, per cent), tall (1..64) and gap (0..1024, 0 = no limit).  Python integers do not overflow, so the statement is total.
  1. h_i = y_max_i - y_min_i + 1, w_i = x_max_i - x_min_i + 1; a box with h_i <= 0 or w_i <= 0 is EMPTY: it never links.
  2. med = the element of rank (m - 1) // 2 among the ascending heights of the m non-empty boxes; 0 if m = 0.
  3. A non-empty box is LINKABLE iff h_i <= tall * med.
  4. Two linkable boxes i != j are in one height band, V(i, j), iff 100 * ov >= overlap * min(h_i, h_j) with
     ov = min(y_max_i, y_max_j) - max(y_min_i, y_min_j) + 1.
  5. The key of a box is (x_min_i, i).
  6. succ(i) = the j with V(i, j) and key_j > key_i of the smallest key; pred(i) = the j with V(i, j) and key_j < key_i of the largest.
  7. The link i - succ(i) exists iff gap == 0 or x_min_succ - x_max_i - 1 <= gap * med; the link i - pred(i) iff gap == 0 or
     x_min_i - x_max_pred - 1 <= gap * med.
  8. A line is a connected component of the links, its root its smallest index, its box the union of its members' boxes.
  9. Lines are numbered ascending by (y_min_L + y_max_L, x_min_L, root_L).
 10. pos_i = the rank of box i under (line_i, x_min_i, y_min_i, i); order is the inverse of pos.

group(..., prune=False) tries every pair.  The default looks only at the boxes that can be in i's band at all: V(i, j) needs ov >= 1
(overlap >= 1 and both heights >= 1 make its right side positive), that is y_min_j <= y_max_i and y_max_j >= y_min_i, and a linkable j
is at most H = the largest linkable height tall, so y_min_j >= y_min_i - H + 1: one window of the linkable boxes sorted by y_min.
tests/test_lines_cpu.py holds the two to each other on the small cases.
"""
import bisect
import functools
import math
import random

MAX_BOXES = 4096
DEFAULTS = (50, 3, 0)
PARAMS = [DEFAULTS, (1, 1, 1), (100, 64, 1024), (34, 2, 3)]
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096]
NINE_PAGES = [0, 1, 300, 0, 4096, 7, 0, 64, 0]
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def group(boxes, overlap=50, tall=3, gap=0, prune=True):
    """-> dict(line, pos, order, line_boxes, med, succ, pred): lists of Python ints, line_boxes a list of 4-tuples in line order;
    succ / pred hold the NEIGHBOURS of step 6 (None where there is none), whether or not step 7 links them"""
    assert 1 <= overlap <= 100 and 1 <= tall <= 64 and 0 <= gap <= 1024
    boxes = [tuple(int(v) for v in b) for b in boxes]
    n = len(boxes)
    h = [b[3] - b[1] + 1 for b in boxes]
    w = [b[2] - b[0] + 1 for b in boxes]
    some = [h[i] > 0 and w[i] > 0 for i in range(n)]
    heights = sorted(h[i] for i in range(n) if some[i])
    med = heights[(len(heights) - 1) // 2] if heights else 0
    linkable = [some[i] and h[i] <= tall * med for i in range(n)]

    def V(i, j):
        ov = min(boxes[i][3], boxes[j][3]) - max(boxes[i][1], boxes[j][1]) + 1
        return 100 * ov >= overlap * min(h[i], h[j])

    links = [i for i in range(n) if linkable[i]]
    if prune:
        by_y = sorted(links, key=lambda i: boxes[i][1])
        y_of = [boxes[i][1] for i in by_y]
        H = max((h[i] for i in links), default=0)
    succ, pred = [None] * n, [None] * n
    for i in links:
        near = by_y[bisect.bisect_left(y_of, boxes[i][1] - H + 1):bisect.bisect_right(y_of, boxes[i][3])] if prune else links
        key_i = (boxes[i][0], i)
        for j in near:
            if j == i or not V(i, j):
                continue
            key_j = (boxes[j][0], j)
            if key_j > key_i and (succ[i] is None or key_j < (boxes[succ[i]][0], succ[i])):
                succ[i] = j
            if key_j < key_i and (pred[i] is None or key_j > (boxes[pred[i]][0], pred[i])):
                pred[i] = j
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def link(a, b):
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)                         # the root is the smallest index of the component
    for i in range(n):
        if succ[i] is not None and (gap == 0 or boxes[succ[i]][0] - boxes[i][2] - 1 <= gap * med):
            link(i, succ[i])
        if pred[i] is not None and (gap == 0 or boxes[i][0] - boxes[pred[i]][2] - 1 <= gap * med):
            link(i, pred[i])
    root = [find(i) for i in range(n)]
    box_of = {}
    for i in range(n):
        a = box_of.get(root[i])
        b = boxes[i]
        box_of[root[i]] = b if a is None else (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))
    roots = sorted(box_of, key=lambda r: (box_of[r][1] + box_of[r][3], box_of[r][0], r))
    number = {r: k for k, r in enumerate(roots)}
    line = [number[root[i]] for i in range(n)]
    order = sorted(range(n), key=lambda i: (line[i], boxes[i][0], boxes[i][1], i))
    pos = [0] * n
    for k, i in enumerate(order):
        pos[i] = k
    return dict(line=line, pos=pos, order=order, line_boxes=[box_of[r] for r in roots], med=med, succ=succ, pred=pred)


# ------------------------------------------------------------------------------------------------------------------ the generators
def text_like(n, seed, width=3000):
    """n boxes of random text-like geometry, shuffled: words of 10..34 rows on lines 40 rows apart across `width` columns, and among them
    a few rules and pictures far taller than a word, small marks, empty boxes and exact copies"""
    rng = random.Random(seed * 7919 + n)
    out, y, x = [], 20, rng.randrange(0, 60)
    while len(out) < n:
        kind = rng.randrange(50)
        if kind == 0:                                          # a rule or a picture through several lines
            out.append((x, y - rng.randrange(0, 90), x + rng.randrange(2, 200), y + rng.randrange(60, 200)))
        elif kind == 1:                                        # empty, in one direction or both
            out.append((x, y, x - rng.randrange(1, 3), y + rng.randrange(-3, 20)))
        elif kind == 2 and out:                                # a copy of an earlier box
            out.append(out[rng.randrange(len(out))])
        elif kind == 3:                                        # a mark below the baseline
            out.append((x, y + 18, x + 3, y + 18 + rng.randrange(2, 8)))
        else:
            ww, top, bottom = rng.randrange(12, 140), rng.randrange(0, 8), rng.randrange(0, 7)
            out.append((x, y - top, x + ww - 1, y + 19 + bottom))
            x += ww + rng.randrange(6, 25)
        if x > width:
            x, y = rng.randrange(0, 60), y + 40
    rng.shuffle(out)
    return out


def synthetic_page(seed, slope, lines=12, width=2000, x_height=20, pitch=34):
    """-> (boxes, true line of every box): `lines` text lines `pitch` rows apart across `width` columns; a word is 30..139 columns wide,
    x_height rows high plus an ascender of 7 or 0 and a descender of 6 or 0 rows, 10..24 columns from the next; every word is shifted
    down by floor(slope * its x_min); the boxes are shuffled"""
    rng = random.Random(seed)
    words = []
    for k in range(lines):
        x, y = rng.randrange(0, 40), 60 + pitch * k
        while True:
            ww = rng.randrange(30, 140)
            if x + ww > width:
                break
            dy = math.floor(slope * x)
            words.append(((x, y - rng.choice((7, 0)) + dy, x + ww - 1, y + x_height - 1 + rng.choice((6, 0)) + dy), k))
            x += ww + rng.randrange(10, 25)
    rng.shuffle(words)
    return [b for b, _ in words], [k for _, k in words]


def staircase(n, short, h=20, overlap=50):
    """n boxes of h rows, each one step to the right of and below the one before and overlapping it by exactly overlap per cent of h
    rows (short = 0: one line, the longest chain of links there is) or by one row less (short = 1: n lines)"""
    step = h - overlap * h // 100 + short
    assert (overlap * h) % 100 == 0
    return [(30 * i, step * i, 30 * i + 24, step * i + h - 1) for i in range(n)]


def hand_cases():
    """name -> (boxes, (overlap, tall, gap)): the cases both test files run"""
    M = INT_MAX
    return {
        "equal_x_min": ([(10, 0, 30, 19), (10, 2, 40, 21), (10, 1, 20, 20), (50, 0, 60, 19)], DEFAULTS),
        "identical": ([(5, 5, 40, 24)] * 9, DEFAULTS),
        "nested": ([(0, 0, 100, 39), (10, 10, 20, 19), (30, 5, 60, 34), (35, 12, 40, 15), (120, 0, 130, 39)], DEFAULTS),
        "empty_boxes": ([(0, 0, 20, 19), (30, 0, 29, 19), (40, 0, 60, 19), (70, 5, 90, 4), (100, 0, 120, 19), (5, 5, 4, 4), (0, 0, -1, -1)],
                        DEFAULTS),
        "all_empty": ([(3, 3, 2, 9), (0, 0, 5, -1)], DEFAULTS),
        "extremes": ([(-M - 1, -M - 1, M, M), (-M - 1, -M - 1, -M - 1, -M - 1), (M, M, M, M), (-M - 1, 0, M, 19), (0, -M - 1, 19, M),
                      (-M, -M, M - 1, M - 1), (M, -M - 1, -M - 1, M), (0, 0, 9, 19), (20, 0, 29, 19)], (50, 64, 1024)),
        # every height near 2^32, so med = 2^32 - 1: tall * med, gap * med and 100 * ov leave int32 by far
        "extremes_huge": ([(-M - 1, -M - 1, -1, M), (0, -M - 1, M, M - 1), (-M - 1, 0, M, M), (M, -M - 1, M, M)], (50, 1, 1)),
        "extremes_huge_all": ([(-M - 1, -M - 1, -1, M), (0, -M - 1, M, M - 1), (-M - 1, 0, M, M), (M, -M - 1, M, M)], (100, 64, 1024)),
        "extremes_tall_1": ([(-M - 1, -M - 1, M, M), (-M - 1, -M - 1, M, M), (-M - 1, M - 1, M, M), (M - 5, -M - 1, M, -M)], (100, 1, 1)),
    }


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (boxes, params, group(boxes, *params)), computed once per process.  Names: 'count/<n>/<k>' (text_like(n, seed k) at PARAMS[k]),
    'stairs/<short>', 'hand/<name>'"""
    kind, *rest = name.split("/")
    if kind == "count":
        n, k = int(rest[0]), int(rest[1])
        boxes, params = text_like(n, k), PARAMS[k]
    elif kind == "stairs":
        boxes, params = staircase(MAX_BOXES, int(rest[0])), DEFAULTS
    else:
        boxes, params = hand_cases()[rest[0]]
    return boxes, params, group(boxes, *params)


CASE_NAMES = ([f"count/{n}/{k}" for k in range(len(PARAMS)) for n in COUNTS] + ["stairs/0", "stairs/1"]
              + [f"hand/{name}" for name in hand_cases()])
