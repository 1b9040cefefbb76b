"""The statement of the two binarisation baselines (csrc/binarize.hip, qea/binarize.py), in plain numpy and Python, written for reading.
It imports nothing from the library; the device kernels and the product's host path reproduce it bit for bit.

A page is [h, w] uint8, or a floating page, which is first read as the 8-bit image the OCR engine would see: (uint8)(clamp(x, 0, 1) *
255) in fp32, truncated, NaN as 0 (to_u8 below; qea.pages.quantise_u8 is the same rule).  Ink is foreground.  The result is 0 for a
foreground pixel and 255 for a background pixel (as_output(..., "u8")), or 0.0 / 1.0 in fp32 (as_output(..., "float")).

Why it is exact: pixels are integers 0..255, so every histogram count and every window sum is an exact integer whatever the order of
summation, and both decisions are written with fp64 products and one subtraction only — no sqrt, no division, no fused multiply-add —
which IEEE arithmetic rounds the same way everywhere.

Otsu, per page: hist[256], N = h * w <= 2^27 (so that 255 * N^2 < 2^63), S = sum v * hist[v].  For t = 0..254 ascending, with
w0 = sum hist[:t + 1], s0 = sum v * hist[v] over v <= t, w1 = N - w0: skip t when w0 == 0 or w1 == 0; d = s0 * N - S * w0 (an exact
integer below 2^63), num = double(d) * double(d), den = double(w0) * double(w1).  The first valid t starts the chain; a later t replaces
the best iff num * den_best > num_best * den.  Ties therefore keep the smaller t.  (num / den is N^2 times the between-class variance
w0 w1 (mu0 - mu1)^2.)  A pixel is foreground iff v <= t*; a page of a single grey level has no valid t, t* = -1, and is all background.

Sauvola, per pixel: window side win odd in 3..127, fp64 0 < k < 1 and R > 0.  The window is centred on the pixel and clipped to the
page; n is its pixel count, S1 = sum v, S2 = sum v^2, Q = n * S2 - S1^2 (exact integers; Q needs 64 bits).  With v the pixel:
    A = double(n * v) - double(S1) * (1.0 - k);      A <= 0: foreground
    L = A * (R * double(n)),  G = k * double(S1);    otherwise foreground iff L * L <= (G * G) * double(Q)
This is the textbook v <= m * (1 + k * (s / R - 1)) with m = S1 / n and s^2 = S2 / n - m^2: multiply by n to get
n v - S1 (1 - k) <= k S1 s / R, whose right side is >= 0; with s = sqrt(Q) / n, multiply by R n and square.
"""
import numpy as np

MAX_PAGE_PIXELS = 1 << 27
MAX_WINDOW = 127


def to_u8(page):
    """[h, w] uint8 as it is; a floating page through the 8-bit rule"""
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page
    x = page.astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)        # the cast truncates


def as_output(foreground, out="u8"):
    """bool [h, w] -> 0 / 255 uint8 (out="u8") or 0.0 / 1.0 float32 (out="float")"""
    return np.where(foreground, 0, 255).astype(np.uint8) if out == "u8" else np.where(foreground, 0.0, 1.0).astype(np.float32)


def check_page(page):
    if page.ndim != 2 or page.size == 0 or page.size > MAX_PAGE_PIXELS:
        raise ValueError(f"a page is [h, w] with 1..2^27 pixels, not {page.shape}")


def otsu_threshold_of_hist(hist):
    """256 exact counts (Python ints) -> t*, or -1"""
    hist = [int(c) for c in hist]
    N = sum(hist)
    S = sum(v * c for v, c in enumerate(hist))
    best, num_best, den_best = -1, 0.0, 0.0
    w0 = s0 = 0
    for t in range(255):
        w0 += hist[t]
        s0 += t * hist[t]
        w1 = N - w0
        if w0 == 0 or w1 == 0:
            continue
        d = s0 * N - S * w0
        assert abs(d) < 2 ** 63
        num = float(d) * float(d)
        den = float(w0) * float(w1)
        if best < 0 or num * den_best > num_best * den:
            best, num_best, den_best = t, num, den
    return best


def otsu_threshold(page):
    v = to_u8(page)
    check_page(v)
    return otsu_threshold_of_hist(np.bincount(v.reshape(-1), minlength=256))


def otsu(page, out="u8"):
    """-> (binarised page, t*)"""
    t = otsu_threshold(page)
    return as_output(to_u8(page).astype(np.int64) <= t, out), t


def check_sauvola(win, k, R):
    if int(win) != win or win % 2 != 1 or not 3 <= win <= MAX_WINDOW:
        raise ValueError(f"window {win}: odd, 3..{MAX_WINDOW}")
    if not 0.0 < k < 1.0:
        raise ValueError(f"k = {k}: strictly between 0 and 1")
    if not 0.0 < R < float("inf"):
        raise ValueError(f"R = {R}: positive and finite")


def window_sums_at(v, y, x, win):
    """(n, S1, S2) of the window centred on (y, x) and clipped to the page, as Python ints: the definition, one pixel at a time"""
    r = win // 2
    box = v[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].astype(np.int64)
    return int(box.size), int(box.sum()), int((box * box).sum())


def sauvola_decision(n, v, S1, S2, k, R):
    """the rule on exact integers n, v, S1, S2 and Python floats (IEEE fp64, each operation rounded once)"""
    Q = n * S2 - S1 * S1
    A = float(n * v) - float(S1) * (1.0 - k)
    if A <= 0.0:
        return True
    L = A * (R * float(n))
    G = k * float(S1)
    return L * L <= (G * G) * float(Q)


def sauvola_at(page, y, x, win=25, k=0.2, R=128.0):
    """is pixel (y, x) foreground?  The statement, brute force."""
    v = to_u8(page)
    n, S1, S2 = window_sums_at(v, y, x, win)
    return sauvola_decision(n, int(v[y, x]), S1, S2, float(k), float(R))


def window_sums(v, win):
    """(n, S1, S2) int64 [h, w] of every pixel's clipped window, summed one window offset at a time, first along the rows, then along the
    columns.  Integer sums: the order is immaterial, and window_sums_at gives the same numbers (tests/test_binarize_cpu.py compares them)."""
    r = win // 2
    h, w = v.shape

    def along(a, axis):
        a = np.moveaxis(a, axis, 0)
        pad = np.zeros((r,) + a.shape[1:], np.int64)
        p = np.concatenate([pad, a, pad])
        s = np.zeros_like(a)
        for o in range(win):
            s += p[o:o + a.shape[0]]
        return np.moveaxis(s, 0, axis)
    v = v.astype(np.int64)
    return tuple(along(along(a, 1), 0) for a in (np.ones((h, w), np.int64), v, v * v))


def sauvola(page, win=25, k=0.2, R=128.0, out="u8", sums=None):
    """The whole page by the same statement, array-wide: numpy's fp64 multiplies and subtracts round exactly as Python's, and an
    int64 -> float64 conversion rounds to nearest like float(int).  `sums` = window_sums(to_u8(page), win), to share between calls."""
    check_sauvola(win, k, R)
    v = to_u8(page)
    check_page(v)
    k, R = np.float64(k), np.float64(R)
    n, S1, S2 = sums if sums is not None else window_sums(v, win)
    Q = n * S2 - S1 * S1
    A = (n * v.astype(np.int64)).astype(np.float64) - S1.astype(np.float64) * (np.float64(1.0) - k)
    L = A * (R * n.astype(np.float64))
    G = k * S1.astype(np.float64)
    return as_output((A <= 0.0) | (L * L <= (G * G) * Q.astype(np.float64)), out)


def sauvola_textbook(page, win=25, k=0.2, R=128.0):
    """-> (T, v): the threshold of the textbook formula with sqrt and division, m * (1 + k * (s / R - 1)), and the 8-bit page; a pixel is
    foreground iff v <= T.  The yardstick of the statement, not part of it."""
    v = to_u8(page)
    n, S1, S2 = (a.astype(np.float64) for a in window_sums(v, win))
    m = S1 / n
    s = np.sqrt(np.maximum(S2 / n - m * m, 0.0))
    return m * (1.0 + k * (s / R - 1.0)), v
