"""The statement of page skew estimation and deskew (csrc/deskew.hip, qea/deskew.py), in plain numpy and Python, written for reading.
It imports nothing from the library; the device kernels and the product's host path reproduce it bit for bit.  Every value is an integer
(Python ints or int64), so nothing depends on an order of summation or a rounding mode.

A page is [h, w] uint8, or a floating page, which is first read as the 8-bit image the OCR engine would see (to_u8 below, the rule of
tests/binarize_spec.py).  Limits: h, w <= 32767 and h w <= 2^27.

1. Strip sums.  Ink is v <= ink_max; ink_max is 0..254, or -1 for "no ink" where it comes from Otsu (a page of a single grey level).
   Strip j covers the columns [32 j, 32 j + 32) cut to w, ns = ceil(w / 32).  C[j][y] = the ink pixels of row y inside strip j (<= 32).
2. Scores.  The candidates are the slopes a / 1024, a = -A..A, A in 0..256.  Strip j is shifted by
   d(j, a) = floor((a (32 j + 16 - w div 2) + 512) / 1024), a true floor; P_a[r] = sum_j C[j][r + d(j, a)], rows outside [0, h) count 0;
   S_a = sum_{r = 0}^{h - 2} (P_a[r + 1] - P_a[r])^2: the differential projection profile under a shear of whole strips.
3. Pick.  a* = the candidate of the largest S_a, ties to the smallest |a|, then to the negative one; kept only if
   100 (S_a* - S_0) >= g S_0 for the gain gate g in 0..10000, else 0.
4. Rotate about the page centre by the slope a, output size = input size, through the table (C16, S16) of rotation_table: see rotate.
"""
import math

import numpy as np

MAX_SIDE, MAX_PAGE_PIXELS, MAX_SLOPE, MAX_GAIN = 32767, 1 << 27, 256, 10000


def to_u8(page):
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page
    x = page.astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)        # the cast truncates


def _page(page):
    v = to_u8(page)
    assert v.ndim == 2 and v.size > 0 and max(v.shape) <= MAX_SIDE and v.size <= MAX_PAGE_PIXELS
    return v


def strip_sums(page, ink_max=127):
    """-> uint8 [ns, h]"""
    assert isinstance(ink_max, int) and -1 <= ink_max <= 254
    v = _page(page)
    h, w = v.shape
    ink = v.astype(np.int64) <= ink_max
    return np.stack([ink[:, 32 * j:32 * j + 32].sum(1) for j in range((w + 31) // 32)]).astype(np.uint8)


def shift(j, a, w):
    return (a * (32 * j + 16 - w // 2) + 512) // 1024           # Python's // is the floor for negative numerators too


def scores(C, w, A):
    """C: strip_sums of a page of width w -> a list of 2 A + 1 Python ints, S_a at index a + A"""
    assert isinstance(A, int) and 0 <= A <= MAX_SLOPE
    ns, h = C.shape
    assert ns == (w + 31) // 32
    out = []
    for a in range(-A, A + 1):
        P = np.zeros(h, np.int64)
        for j in range(ns):
            d = shift(j, a, w)
            lo, hi = max(0, -d), min(h, h - d)                  # the rows r with 0 <= r + d < h
            if lo < hi:
                P[lo:hi] += C[j, lo + d:hi + d]
        out.append(int((np.diff(P) ** 2).sum()))
    return out


def pick(S, g=0):
    """S: 2 A + 1 integers -> a*"""
    assert isinstance(g, int) and 0 <= g <= MAX_GAIN and len(S) % 2 == 1
    A = len(S) // 2
    S = [int(s) for s in S]
    best = min(range(-A, A + 1), key=lambda a: (-S[a + A], abs(a), a))
    return best if 100 * (S[best + A] - S[A]) >= g * S[A] else 0


def estimate(page, A=90, ink_max=127, g=0):
    """-> (a*, the scores)"""
    v = _page(page)
    S = scores(strip_sums(v, ink_max), v.shape[1], A)
    return pick(S, g), S


def rotation_table(A):
    """-> int64 [2 A + 1, 2]: row a + A = (C16, S16) = (round(65536 / n), round(65536 t / n)), t = a / 1024, n = sqrt(1 + t t), in fp64 as
    written.  The table is data: the kernel and rotate() below read it, neither recomputes it."""
    rows = []
    for a in range(-A, A + 1):
        t = a / 1024
        n = math.sqrt(1 + t * t)
        rows.append((round(65536 / n), round(65536 * t / n)))
    return np.asarray(rows, np.int64).reshape(-1, 2)


def rotate(page, a, table, interp="bilinear", fill=255, out="u8", norm=None):
    """The page rotated about its centre by the slope a / 1024 (a within the table's range).  All of it in int64; >> on a negative numpy
    int64 is arithmetic.  out="float" needs `norm`, the 256 fp32 values of qea.pages.norm_table()."""
    assert interp in ("bilinear", "nearest") and isinstance(fill, int) and 0 <= fill <= 255
    v = _page(page).astype(np.int64)
    h, w = v.shape
    A = len(table) // 2
    assert -A <= a <= A
    C16, S16 = int(table[a + A][0]), int(table[a + A][1])
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    dx2, dy2 = 2 * x - (w - 1), 2 * y - (h - 1)
    X = C16 * dx2 - S16 * dy2 + 65536 * (w - 1)
    Y = S16 * dx2 + C16 * dy2 + 65536 * (h - 1)

    def p(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside, v[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], fill)
    if interp == "nearest":
        res = p((Y + 65536) >> 17, (X + 65536) >> 17)
    else:
        x0, y0, fx, fy = X >> 17, Y >> 17, (X >> 9) & 255, (Y >> 9) & 255
        res = ((256 - fx) * (256 - fy) * p(y0, x0) + fx * (256 - fy) * p(y0, x0 + 1) + (256 - fx) * fy * p(y0 + 1, x0) +
               fx * fy * p(y0 + 1, x0 + 1) + 32768) >> 16
    res = res.astype(np.uint8)
    return res if out == "u8" else np.asarray(norm, np.float32)[res]


def sheared_text_page(k, seed, h=400, w=512):
    """The recall generator: about 20 lines of dark bars, 6 to 9 pixels high and 8 to 60 long, on white, every column x then moved down by
    floor((k (x - w div 2) + 512) / 1024) -> uint8 [h, w]"""
    rng = np.random.default_rng(seed)
    flat = np.full((h, w), 255, np.uint8)
    y = 12
    while y + 9 < h - 8:
        bar = int(rng.integers(6, 10))
        x = int(rng.integers(4, 20))
        while x < w - 8:
            n = int(rng.integers(8, 61))
            flat[y:y + bar, x:min(x + n, w - 4)] = int(rng.integers(0, 60))
            x += n + int(rng.integers(5, 14))
        y += bar + int(rng.integers(9, 13))
    out = np.full((h, w), 255, np.uint8)
    for x in range(w):
        d = (k * (x - w // 2) + 512) // 1024
        lo, hi = max(0, d), min(h, h + d)                       # out[r] = flat[r - d]
        if lo < hi:
            out[lo:hi, x] = flat[lo - d:hi - d, x]
    return out
