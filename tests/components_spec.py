"""The statement of the connected-component features (csrc/components.hip, qea/components.py), in plain numpy and Python, written for
reading.  It imports nothing from the library; the device kernels and the product's host path reproduce it bit for bit.

Ink.  A page is [h, w] uint8, or a floating page, which is first read as the 8-bit image the OCR engine would see (to_u8 below, the rule
of tests/binarize_spec.py).  A pixel is ink iff v8 <= ink_max, an integer in 0..254 (default 127).

Labels.  Two ink pixels are neighbours when they differ by one step along a row or a column (connectivity 4) or also along a diagonal
(connectivity 8); a component is a maximal set of ink pixels joined by chains of neighbours.  The label of an ink pixel is the smallest
row-major index y * w + x of its page over the pixels of its component, as int32 (a page has at most 2^27 pixels); background is -1.
This names one labelling: no order of visiting the pixels enters it.

Component table.  int32 [n, 6] = (root, area, x_min, y_min, x_max, y_max), coordinates inclusive, rows ascending by root, which is reading
order by each component's first pixel.

Despeckle.  A pixel is 0 iff it is ink and its component has at least min_area (>= 1) pixels, else 255 (out="u8") or 1.0 (out="float").

Smear.  Horizontal pass, gap gx: a background pixel becomes ink iff its row has ink at distance a >= 1 to its left and b >= 1 to its right
with a + b - 1 <= gx, i.e. background runs of at most gx pixels between two ink pixels are filled; what touches the page edge is not
between ink.  The vertical pass, gap gy, does the same along columns on the result of the horizontal pass.  A gap of 0 skips its pass;
gaps are 0..127.

Word boxes.  int32 [n, 4] = (x_min, y_min, x_max, y_max), inclusive, of the connectivity-8 components of the smeared page whose smeared
area is >= min_area, ascending by root of the smeared page.
"""
import numpy as np

MAX_PAGE_PIXELS = 1 << 27
MAX_GAP = 127


def to_u8(page):
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page
    x = page.astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)        # the cast truncates


def ink_of(page, ink_max=127):
    assert isinstance(ink_max, int) and 0 <= ink_max <= 254
    v = to_u8(page)
    assert v.ndim == 2 and 0 < v.size <= MAX_PAGE_PIXELS
    return v.astype(np.int64) <= ink_max


def labels_of_ink(ink, connectivity=8):
    """bool [h, w] -> int32 [h, w].  Breadth first from every still unlabelled ink pixel in row-major order: the pixel a search starts at is
    the first pixel of its component in that order, hence its smallest index."""
    assert connectivity in (4, 8)
    h, w = ink.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    grid = ink.tolist()
    labels = [[-1] * w for _ in range(h)]
    for y0, x0 in zip(*(a.tolist() for a in np.nonzero(ink))):
        if labels[y0][x0] >= 0:
            continue
        root = y0 * w + x0
        labels[y0][x0] = root
        todo = [(y0, x0)]
        while todo:
            y, x = todo.pop()
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < h and 0 <= u < w and grid[v][u] and labels[v][u] < 0:
                    labels[v][u] = root
                    todo.append((v, u))
    return np.asarray(labels, np.int32).reshape(h, w)


def labels(page, connectivity=8, ink_max=127):
    return labels_of_ink(ink_of(page, ink_max), connectivity)


def table_of_labels(lab):
    """int32 labels -> int32 [n, 6] = (root, area, x_min, y_min, x_max, y_max), ascending by root"""
    rows = []
    for root in np.unique(lab[lab >= 0]).tolist():
        ys, xs = np.nonzero(lab == root)
        rows.append((root, ys.size, xs.min(), ys.min(), xs.max(), ys.max()))
    return np.asarray(rows, np.int32).reshape(-1, 6)


def table_fast(lab):
    """the same table from per-label reductions, for pages with thousands of components (equal to table_of_labels; the tests check that)"""
    h, w = lab.shape
    ys, xs = np.nonzero(lab >= 0)
    roots, inv = np.unique(lab[ys, xs], return_inverse=True)
    t = np.zeros((roots.size, 6), np.int64)
    t[:, 0] = roots
    t[:, 1] = np.bincount(inv, minlength=roots.size)
    for col, vals, pick in ((2, xs, np.minimum), (3, ys, np.minimum), (4, xs, np.maximum), (5, ys, np.maximum)):
        t[:, col] = max(h, w) if pick is np.minimum else -1
        pick.at(t[:, col], inv, vals)
    return t.astype(np.int32)


def as_output(keep, out="u8"):
    return np.where(keep, 0, 255).astype(np.uint8) if out == "u8" else np.where(keep, 0.0, 1.0).astype(np.float32)


def despeckle(page, min_area, connectivity=8, ink_max=127, out="u8", lab=None):
    assert isinstance(min_area, int) and min_area >= 1
    lab = labels(page, connectivity, ink_max) if lab is None else lab
    area = np.bincount(lab[lab >= 0], minlength=lab.size)
    return as_output((lab >= 0) & (area[np.maximum(lab, 0)] >= min_area), out)


def smear_rows(ink, gap):
    """one pass along rows, by the distances of the definition"""
    assert isinstance(gap, int) and 0 <= gap <= MAX_GAP
    if gap == 0:
        return ink.copy()
    h, w = ink.shape
    far = 4 * (w + MAX_GAP)
    x = np.arange(w)[None, :]
    left = np.maximum.accumulate(np.where(ink, x, -far), axis=1)             # the last ink position at or before x
    right = np.minimum.accumulate(np.where(ink, x, far)[:, ::-1], axis=1)[:, ::-1]      # the first at or after x
    a, b = x - left, right - x
    return ink | (~ink & (a + b - 1 <= gap))


def smear(ink, gap_x, gap_y):
    return smear_rows(smear_rows(ink, gap_x).T, gap_y).T


def word_boxes(page, gap_x=8, gap_y=0, min_area=16, ink_max=127):
    t = table_fast(labels_of_ink(smear(ink_of(page, ink_max), gap_x, gap_y), 8))
    return np.ascontiguousarray(t[t[:, 1] >= min_area, 2:])
