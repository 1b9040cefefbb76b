"""Page skew estimation and deskew over the ragged page lists of qea/pages.py (csrc/deskew.hip): the first stage of the page pipeline,
in front of binarize_pages, the components and the word boxes, which all assume horizontal text lines.

The statement (tests/deskew_spec.py spells it out; DESIGN.md "Deskew" says why it is exact).  A page is read as 8-bit grey exactly as
binarize_pages reads it; h, w <= 32767 and h w <= 2^27.
  * Strip sums: ink is v <= ink_max; C[j][y] = the ink pixels of row y in the columns [32 j, 32 j + 32) cut to w.
  * Scores of the slopes a / 1024, a = -A..A (A = max_slope, 0..256): strip j shifted by d(j, a) = floor((a (32 j + 16 - w div 2) + 512) /
    1024), P_a[r] = sum_j C[j][r + d(j, a)] with rows outside the page counting 0, S_a = sum_r (P_a[r + 1] - P_a[r])^2 in int64: the
    differential projection profile with whole strips sheared, so that one pass over the pixels serves all candidates.
  * Pick: the a of the largest S_a, ties to the smallest |a|, then to the negative one; kept only if 100 (S_a - S_0) >= min_gain S_0
    (min_gain 0..10000), else 0.  a is the baselines' dy / dx in 1024ths, y pointing down.
  * Rotate about the page centre, same size out: 16.16 fixed-point coordinates from a table (round(65536 / n), round(65536 t / n)),
    t = a / 1024, n = sqrt(1 + t t), 8-bit bilinear weights (or the nearest pixel), `fill` for every tap outside the page.  a = 0 is the
    identity.  u8 out is the value, float out norm_table()[value].
All of it is integer work: the device, the host path below and the statement agree bit for bit.

CUDA pages (or a CUDA `device`) run the kernels over the packed store: strip sums, scores, pick, rotate, one launch each, a fixed
sequence whatever the pages hold; the slopes stay on the device between pick and rotate.  CPU tensors run the host path: the same
statement vectorised in numpy over all candidates at once.
"""
import math

import numpy as np
import torch

from .pages import _check_out, host_pages, is_int, norm_table, open_store, pack_host, packed_result, unpack_pages

MAX_SIDE, MAX_PAGE_PIXELS, MAX_SLOPE, MAX_GAIN = 32767, 1 << 27, 256, 10000
INTERPS = ("bilinear", "nearest")


def check_params(max_slope=90, ink="otsu", min_gain=0, interp="bilinear", fill=255):
    """ValueError for parameters outside the statement's ranges, before any work"""
    if not is_int(max_slope) or not 0 <= max_slope <= MAX_SLOPE:
        raise ValueError(f"max_slope={max_slope!r}: an integer in 0..{MAX_SLOPE} (1024ths)")
    if ink != "otsu" and (not is_int(ink) or not 0 <= ink <= 254):
        raise ValueError(f"ink={ink!r}: 'otsu' or an integer in 0..254")
    if not is_int(min_gain) or not 0 <= min_gain <= MAX_GAIN:
        raise ValueError(f"min_gain={min_gain!r}: an integer in 0..{MAX_GAIN} (per cent)")
    if interp not in INTERPS:
        raise ValueError(f"interp={interp!r}: one of {INTERPS}")
    if not is_int(fill) or not 0 <= fill <= 255:
        raise ValueError(f"fill={fill!r}: an integer in 0..255")


def rotation_table(A):
    """-> int32 numpy [2 A + 1, 2]: row a + A = (C16, S16) = (round(65536 / n), round(65536 t / n)), t = a / 1024, n = sqrt(1 + t t) in
    fp64.  The kernel and the host path read it as data."""
    if not is_int(A) or not 0 <= A <= MAX_SLOPE:
        raise ValueError(f"A={A!r}: an integer in 0..{MAX_SLOPE}")
    rows = []
    for a in range(-A, A + 1):
        t = a / 1024
        n = math.sqrt(1 + t * t)
        rows.append((round(65536 / n), round(65536 * t / n)))
    return np.asarray(rows, np.int32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------- the host path
def _strip_sums_host(v, ink_max):
    """uint8 [h, w] -> uint8 [ns, h]"""
    h, w = v.shape
    ns = (w + 31) // 32
    ink = np.zeros((h, ns * 32), np.uint8)
    ink[:, :w] = v.astype(np.int16) <= ink_max
    return np.ascontiguousarray(ink.reshape(h, ns, 32).sum(2, dtype=np.uint8).T)


def _scores_host(C, w, A):
    """-> int64 [2 A + 1]: all candidates at once, one gather per strip out of the strip's column padded with zeros by the largest shift"""
    ns, h = C.shape
    a = np.arange(-A, A + 1, dtype=np.int64)
    centre = 32 * np.arange(ns, dtype=np.int64) + 16 - w // 2
    d = (a[:, None] * centre[None, :] + 512) >> 10                             # [2 A + 1, ns]; >> floors
    D = int(np.abs(d).max())
    S = np.zeros(2 * A + 1, np.int64)
    r = np.arange(h, dtype=np.int64)[None, :] + D
    padded = np.zeros((ns, h + 2 * D), np.int32)
    padded[:, D:D + h] = C
    step = max(1, (1 << 22) // h)                                              # candidates per block: the gathers stay a few MB
    for k in range(0, 2 * A + 1, step):
        P = np.zeros((min(step, 2 * A + 1 - k), h), np.int32)
        for j in range(ns):
            P += padded[j][r + d[k:k + step, j, None]]
        S[k:k + step] = (np.diff(P.astype(np.int64), axis=1) ** 2).sum(1)
    return S


def pick_slopes(scores, min_gain=0):
    """int64 [n, 2 A + 1] (numpy or CPU tensor, any values) -> int32 numpy [n]: the pick of the statement, rows at once"""
    S = np.asarray(scores, np.int64)
    S = S.reshape(-1, S.shape[-1])
    if S.shape[1] % 2 != 1:
        raise ValueError(f"scores {S.shape}: rows of 2 A + 1 values")
    A = S.shape[1] // 2
    # candidates in the order of preference among equals: 0, -1, 1, -2, 2, ...: the first maximum in that order is the pick
    order = np.asarray(sorted(range(-A, A + 1), key=lambda a: (abs(a), a)), np.int64)
    best = order[np.argmax(S[:, order + A], axis=1)]
    top, zero = S[np.arange(len(S)), best + A], S[:, A]
    return np.where(100 * (top - zero) >= int(min_gain) * zero, best, 0).astype(np.int32)


def _rotate_host(v, a, table, interp, fill, rows=256):
    """uint8 [h, w] -> uint8 [h, w], band after band of `rows` output rows"""
    h, w = v.shape
    A = len(table) // 2
    C16, S16 = int(table[a + A][0]), int(table[a + A][1])
    flat = np.concatenate([v.reshape(-1), np.asarray([fill], np.uint8)]).astype(np.int32)      # one more element: the fill
    out = np.empty((h, w), np.uint8)
    dx2 = 2 * np.arange(w, dtype=np.int64)[None, :] - (w - 1)

    def p(yy, xx):
        return flat[np.where((yy >= 0) & (yy < h) & (xx >= 0) & (xx < w), yy * w + xx, h * w)]
    for y in range(0, h, rows):
        dy2 = 2 * np.arange(y, min(y + rows, h), dtype=np.int64)[:, None] - (h - 1)
        X = C16 * dx2 - S16 * dy2 + 65536 * (w - 1)
        Y = S16 * dx2 + C16 * dy2 + 65536 * (h - 1)
        if interp == "nearest":
            res = p((Y + 65536) >> 17, (X + 65536) >> 17)
        else:
            x0, y0 = X >> 17, Y >> 17
            fx, fy = ((X >> 9) & 255).astype(np.int32), ((Y >> 9) & 255).astype(np.int32)
            res = ((256 - fx) * (256 - fy) * p(y0, x0) + fx * (256 - fy) * p(y0, x0 + 1) + (256 - fx) * fy * p(y0 + 1, x0)
                   + fx * fy * p(y0 + 1, x0 + 1) + 32768) >> 16
        out[y:y + rows] = res
    return out


def _estimate_host(pk, A, ink, g):
    from .binarize import otsu_threshold_of_hist
    scores = np.zeros((len(pk.h), 2 * A + 1), np.int64)
    for i, v in enumerate(host_pages(pk)):
        ink_max = otsu_threshold_of_hist(np.bincount(v.reshape(-1), minlength=256)) if ink == "otsu" else ink
        scores[i] = _scores_host(_strip_sums_host(v, ink_max), v.shape[1], A)
    return pick_slopes(scores, g), scores


def _rotate_pages_host(pk, slopes, A, interp, fill, out):
    table = rotation_table(A)
    res = pack_host(pk, (_rotate_host(v, int(a), table, interp, fill) for a, v in zip(slopes, host_pages(pk))), torch.uint8)
    return res if out == "u8" else norm_table()[res.long()]


# ---------------------------------------------------------------------------------------------------------------- the device path
def _estimate_device(store, table, A, ink, g):
    """three launches of csrc/deskew.hip (after Otsu's two for ink="otsu") -> (slopes, scores) on the device; nothing is read back"""
    from . import ops
    if ink == "otsu":                                          # t* per page stays on the device; the binarised image is scratch
        scratch = torch.empty(store.numel(), dtype=torch.uint8, device=store.device)
        ink = ops.binarize_otsu(store, table, ops.otsu_histogram(store, table), out_u8=scratch)
    scores = ops.skew_scores(ops.skew_strip_sums(store, table, ink), table, A)
    return ops.skew_pick(scores, g), scores


def _rotate_device(store, table, slopes, A, interp, fill, out):
    from . import ops
    res, outs = packed_result(store.numel(), out, store.device)
    rot = torch.from_numpy(rotation_table(A)).to(store.device)
    ops.deskew_rotate(store, table, slopes, rot, interp, fill, norm=None if out == "u8" else norm_table().to(store.device), **outs)
    return res


def _given_slopes(slopes, n, A):
    s = slopes.detach().cpu().numpy() if torch.is_tensor(slopes) else np.asarray(slopes)
    if s.shape != (n,) or s.dtype.kind not in "iu" or (np.abs(s.astype(np.int64)) > A).any():
        raise ValueError(f"slopes: {n} integers within +-max_slope = {A}, one per page")
    return s.astype(np.int32)


def _open(pages, device):
    return open_store(pages, device, MAX_SIDE, MAX_PAGE_PIXELS)


def estimate_skew(pages, max_slope=90, ink="otsu", min_gain=0, device=None):
    """pages: a list of [h, w] uint8 tensors or of [h, w] / [1, h, w] floating tensors, of any sizes (as for binarize_pages) ->
    (slopes int32 [n], scores int64 [n, 2 max_slope + 1]), on `device` if given, else where the pages are.  slopes[i] / 1024 is the dy / dx
    of page i's text baselines, y pointing down.  ink: an integer 0..254 (ink is v <= ink), or "otsu": every page's own Otsu threshold by
    the path of qea/binarize.py (on the device its two launches run first and t* is read by the strip-sum kernel there; the binarised
    image that path also writes is discarded).  A page of a single grey level has no ink and gets slope 0."""
    check_params(max_slope, ink, min_gain)
    pk, dev, store, table = _open(pages, device)
    if dev.type == "cuda":
        return _estimate_device(store, table, int(max_slope), ink, int(min_gain))
    slopes, scores = _estimate_host(pk, int(max_slope), ink, int(min_gain))
    return torch.from_numpy(slopes), torch.from_numpy(scores)


def deskew_pages(pages, max_slope=90, ink="otsu", min_gain=0, interp="bilinear", fill=255, out="u8", device=None, slopes=None):
    """pages as for estimate_skew -> (the pages rotated about their centres by their slopes, same sizes: uint8 for out="u8", fp32
    norm_table()[value] for out="float"; slopes int32 [n]), on `device` if given, else where the pages are.  The slopes are those of
    estimate_skew(pages, max_slope, ink, min_gain) unless `slopes` gives them (n integers within +-max_slope; ink and min_gain are then
    unused).  On a CUDA device: four launches, and the slopes go from the pick to the rotation without visiting the host."""
    _check_out(out)
    check_params(max_slope, ink, min_gain, interp, fill)
    A = int(max_slope)
    pk, dev, store, table = _open(pages, device)
    if slopes is not None:
        slopes = torch.from_numpy(_given_slopes(slopes, len(pk.h), A))
    if dev.type == "cuda":
        slopes = _estimate_device(store, table, A, ink, int(min_gain))[0] if slopes is None else slopes.to(dev)
        res = _rotate_device(store, table, slopes, A, interp, int(fill), out)
    else:
        if slopes is None:
            slopes = torch.from_numpy(_estimate_host(pk, A, ink, int(min_gain))[0])
        res = _rotate_pages_host(pk, slopes.numpy(), A, interp, int(fill), out)
    return unpack_pages(res, pk), slopes
