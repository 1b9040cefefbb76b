"""Classic binarisation baselines, Otsu and Sauvola, over the ragged page lists of qea/pages.py (csrc/binarize.hip).

The question they answer: is the trained cleaner better than a classic binariser in front of the same OCR engine?  eval_prep.py
--baseline and clean_cli.py --method send the same images through binarize_pages instead of the UNet.

The statement (tests/binarize_spec.py spells it out; DESIGN.md "Binarisation baselines" says why it is exact).  A page is read as 8-bit
grey — a floating page through quantise_u8, the image the OCR engine would see — and ink is foreground: 0 / 0.0 out, background 255 / 1.0.
  * Otsu, per page: from the 256-bin histogram, for t = 0..254 ascending with both classes non-empty, d = s0 N - S w0 (int64; pages are
    capped at 2^27 pixels so that 255 N^2 < 2^63), num = double(d)^2, den = double(w0) double(w1); t replaces the best iff
    num * den_best > num_best * den.  Foreground iff v <= t*; one grey level: t* = -1, all background.
  * Sauvola, per pixel, over the window x window box centred on it and clipped to the page (n pixels, S1 = sum v, S2 = sum v^2,
    Q = n S2 - S1^2): A = double(n v) - double(S1) (1.0 - k); foreground iff A <= 0 or L L <= (G G) double(Q), L = A (R double(n)),
    G = k double(S1) — the textbook v <= m (1 + k (s / R - 1)) without sqrt or division.
Integer sums and fp64 products rounded as written: the device and the host agree bit for bit, with no tolerance.

CUDA pages (or a CUDA `device`) run the kernels: the pages packed into one store, ONE launch for Sauvola, two for Otsu (histograms, then
threshold-and-apply; t* never visits the host).  CPU tensors run the host path below — integral images for the same integer sums, the same
fp64 statements in numpy — which is to binarize_pages what clean_pages_spec is to clean_pages.
"""
import math

import numpy as np
import torch

from .pages import _check_out, host_pages, open_store, pack_ink_host, packed_result, unpack_pages

METHODS = ("otsu", "sauvola")
MAX_WINDOW, MAX_PAGE_PIXELS = 127, 1 << 27


def check_params(method, window=25, k=0.2, R=128.0):
    """ValueError for an unknown method or parameters outside the statement's ranges, before any work"""
    if method not in METHODS:
        raise ValueError(f"method={method!r}: one of {METHODS}")
    if method == "sauvola":
        if isinstance(window, bool) or int(window) != window or window % 2 != 1 or not 3 <= window <= MAX_WINDOW:
            raise ValueError(f"window={window!r}: an odd integer in 3..{MAX_WINDOW}")
        if not (isinstance(k, (int, float)) and 0.0 < k < 1.0):
            raise ValueError(f"k={k!r}: strictly between 0 and 1")
        if not (isinstance(R, (int, float)) and 0.0 < R < math.inf):
            raise ValueError(f"R={R!r}: positive and finite")


def otsu_threshold_of_hist(hist):
    """256 counts -> t* or -1: the statement's chain over int64 prefix sums (exact: |d| <= 255 N^2 < 2^63) and Python floats"""
    hist = np.asarray(hist, np.int64)
    w0, s0 = np.cumsum(hist), np.cumsum(hist * np.arange(256))
    N, S = int(w0[-1]), int(s0[-1])
    best, num_best, den_best = -1, 0.0, 0.0
    for t in range(255):
        a, b = int(w0[t]), N - int(w0[t])
        if a == 0 or b == 0:
            continue
        d = float(int(s0[t]) * N - S * a)
        num, den = d * d, float(a) * float(b)
        if best < 0 or num * den_best > num_best * den:
            best, num_best, den_best = t, num, den
    return best


def _box_sums(a, r):
    """int64 [h, w] -> the sum over each pixel's (2r + 1)^2 box clipped to the page, from one integral image"""
    h, w = a.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    np.cumsum(np.cumsum(a, 0), 1, out=ii[1:, 1:])
    y0, y1 = np.maximum(np.arange(h) - r, 0)[:, None], np.minimum(np.arange(h) + r + 1, h)[:, None]
    x0, x1 = np.maximum(np.arange(w) - r, 0)[None, :], np.minimum(np.arange(w) + r + 1, w)[None, :]
    return ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]


def _sauvola_host(v, window, k, R):
    """uint8 [h, w] numpy -> bool foreground"""
    r = window // 2
    h, w = v.shape
    v = v.astype(np.int64)
    n = (np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1)[:, None] * \
        (np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1)[None, :]
    S1, S2 = _box_sums(v, r), _box_sums(v * v, r)
    k, R = np.float64(k), np.float64(R)
    Q = n * S2 - S1 * S1
    A = (n * v).astype(np.float64) - S1.astype(np.float64) * (np.float64(1.0) - k)
    L = A * (R * n.astype(np.float64))
    G = k * S1.astype(np.float64)
    return (A <= 0.0) | (L * L <= (G * G) * Q.astype(np.float64))


def _host(pk, method, window, k, R, out):
    """The host path over a packed store -> (packed result, thresholds or None)"""
    thresholds, inks = [], []
    for v in host_pages(pk):
        if method == "otsu":
            thresholds.append(otsu_threshold_of_hist(np.bincount(v.reshape(-1), minlength=256)))
            inks.append(v.astype(np.int64) <= thresholds[-1])
        else:
            inks.append(_sauvola_host(v, window, k, R))
    return pack_ink_host(pk, inks, out), (torch.tensor(thresholds, dtype=torch.int32) if method == "otsu" else None)


def _device(store, table, method, window, k, R, out):
    from . import ops
    res, outs = packed_result(store.numel(), out, store.device)
    if method == "sauvola":
        ops.binarize_sauvola(store, table, window, k, R, **outs)
        return res, None
    return res, ops.binarize_otsu(store, table, ops.otsu_histogram(store, table), **outs)


def _run(pages, method, window, k, R, out, device, despeckle=0, despeckle_connectivity=8):
    _check_out(out)
    check_params(method, window, k, R)
    if despeckle:
        from . import components
        components.check_params(despeckle_connectivity, min_area=despeckle)
    pk, dev, store, table = open_store(pages, device, max_pixels=MAX_PAGE_PIXELS)   # the bound that keeps Otsu's integers below 2^63
    if dev.type == "cuda":
        res, thr = _device(store, table, method, int(window), float(k), float(R), out)
        if despeckle:                                          # the packed result is the next store: nothing is unpacked or copied
            res = components.despeckle_store(res, table, despeckle, despeckle_connectivity, out=out)
    else:
        res, thr = _host(pk, method, int(window), float(k), float(R), out)
        if despeckle:
            res = components.despeckle_store_host(pk._replace(store=res), despeckle, despeckle_connectivity, out=out)
    return unpack_pages(res, pk), thr


def binarize_pages(pages, method="sauvola", window=25, k=0.2, R=128.0, out="float", device=None, despeckle=0, despeckle_connectivity=8):
    """pages: a list of [h, w] uint8 tensors or of [h, w] / [1, h, w] floating tensors, of any sizes (as for clean_pages) -> a list of the
    same sizes: 0.0 / 1.0 fp32 for out="float", 0 / 255 uint8 for out="u8", ink = 0.  method "otsu" (window, k, R unused) or "sauvola".
    The result lives on `device` if given, else where the pages are; a CUDA device runs the kernels, the host runs the same statement
    in numpy.  despeckle = N > 0 also turns the ink of connected components (despeckle_connectivity 4 or 8) of fewer than N pixels into
    background (qea/components.py: the binarised store goes through label, stats and apply where it is); 0 changes nothing."""
    return _run(pages, method, window, k, R, out, device, despeckle, despeckle_connectivity)[0]


def otsu_thresholds(pages, device=None):
    """-> int32 [len(pages)]: Otsu's t* per page (-1 for a page of a single grey level), on `device` / where the pages are"""
    return _run(pages, "otsu", 25, 0.2, 128.0, "u8", device)[1]
