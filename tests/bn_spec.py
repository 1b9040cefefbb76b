"""Plain numpy statements, fp64, of the BatchNorm, pool-fused and column kernels of csrc/norm_pool.hip (batch statistics, eval
coefficients, apply (+ ReLU) (+ max-pool), the backward in all its forms, column sums, 2-D transpose), of qea_absmax (csrc/misc.hip) and
of qea_filter_flip_transpose.  Written for reading, not for speed; nothing of the library is imported.  tests/test_bn_spec_cpu.py holds
the statements to torch in double precision; tests/test_bn_kernels_gpu.py holds the kernels to them.

Layouts are the library's: rows [M][C] (NHWC with M = B * H * W), per-channel vectors [C], partial rows [blocks][C][2].

Every statement that is gated returns, beside its value, the gate: a count of roundings (fp32: 2^-24, fp64: 2^-53, as the kernel's
code has them) times the magnitudes they act on, with the conditioning term where a difference cancels.  Each derivation stands next to
its gate ("BatchNorm, pool-fused and column kernels").  No gate is taken from what a kernel gives.

The second half of the file mirrors the launch arithmetic of the entry points.  The mirrors only PROVE (tests/test_bn_spec_cpu.py) that
each entry of the shape tables reaches the branch it is named for; no expected value is computed from them."""
import collections
import math

import numpy as np

from c1_spec import amax, f64, gate_ratio, pool, pool_bwd  # noqa: F401  (one pool rule and one gate_ratio for all spec files)

EPS32 = 2.0 ** -24                                       # one fp32 rounding, relative
EPS64 = 2.0 ** -53                                       # one fp64 rounding, relative


def f32(a):
    return np.asarray(a, dtype=np.float32)


def col_fsum(a):
    """correctly rounded fp64 column sums of a [M][C] fp64 array (math.fsum); above 2^21 elements numpy's sum, which the callers use
    on exactly summable data only (any order gives the same bits)"""
    a = f64(a)
    if a.size > 1 << 21:
        return a.sum(0)
    return np.array([math.fsum(col) for col in a.T], dtype=np.float64)


def sum_depth(M):
    """An upper bound on the number of fp64 additions any one addend passes through in the column reductions, from the kernels'
    structure: a thread adds its rows one after the other (16 by design, ceil(M / 1024) + 1 once the 1024-block cap holds), the LDS
    rows of a block are added in sequence (at most 256), a lane of the finalize wave adds at most 1024 / 64 partial rows and the
    butterfly has 6 levels.  17 + 256 + 16 + 6 <= 320.  A sum of n terms in ANY order with depth D errs by at most D u sum|term|."""
    return 320 + M // 1024


# ----------------------------------------------------------------------------- forward statistics
Stats = collections.namedtuple("Stats", "s q mean var invstd unbiased mean_out invstd_out scale shift running_mean running_var "
                                        "g_mean g_var g_invstd g_mean_out g_invstd_out g_scale g_shift g_running_mean g_running_var")


def _stats_from_sums(s, q, a1, M, gamma, beta, eps, momentum, running_mean, running_var, depth):
    """everything bn_stats_finalize_kernel derives from s = sum x and q = sum x^2 (a1 = sum |x|), with the gates

    mean = s / M:       the device's s errs by depth u64 sum|x|, the division rounds once:     g_mean = (depth + 1) u64 sum|x| / M
    var = q / M - mean^2 (ONE pass):  q errs by depth u64 q and the division by u64 q / M; mean^2 by 2 |mean| g_mean + u64 mean^2; the
                        subtraction by u64 |var|; the statement's own fp64 evaluation of the same expression by 4 u64 q / M.  With
                        |mean| sum|x| / M <= q / M (Cauchy-Schwarz) all of it is <= c u64 E[x^2], c = 3 depth + 10:
                                                                                                g_var = (3 depth + 10) u64 q / M
                        THE CONDITIONING TERM: relative to var it is c u64 E[x^2] / var, large on a channel of large mean.
    invstd = (var + eps)^-1/2: d invstd / invstd = -0.5 d var / (var + eps) to first order (factor 1.1 for g_var <= 0.1 (var + eps),
                        which the CPU test asserts on every builder) + sqrt, division, addition and the fp32 eps taken to fp64:
                                                                      g_invstd = invstd (0.55 g_var / (var + eps) + 4 u64)
    mean_out, invstd_out: one cast to fp32 more:                      g + u32 |value|
    scale = g * (float)invstd: cast and product:                      |scale| (g_invstd / invstd + 2 u32)
    shift = b - (float)mean * g * invstd: casts of mean and invstd, two products, the subtraction (5 u32 on the product, 1 on the
                        result) and the errors of mean and invstd:     T (g_invstd / invstd + 5 u32) + |g invstd| g_mean + u32 |shift|,
                                                                      T = |mean g invstd|
    running = (1 - m) * old + m * new in fp32: 1 - m, the cast of new, two products, the sum (4 u32 on each term):
                                                                      4 u32 (|(1 - m) old| + |m new|) + m g_new
    eps and momentum enter as the fp32 values the ABI passes."""
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    C = len(s)
    g = np.ones(C) if gamma is None else f64(gamma)
    b = np.zeros(C) if beta is None else f64(beta)
    mean = s / M
    var = np.maximum(q / M - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    unb = var * M / (M - 1) if M > 1 else var
    scale, shift = g * invstd, b - mean * g * invstd
    g_mean = (depth + 1) * EPS64 * a1 / M
    g_var = (3 * depth + 10) * EPS64 * q / M
    r_is = 0.55 * g_var / (var + eps) + 4 * EPS64
    T = np.abs(mean * g * invstd)
    rm = rv = g_rm = g_rv = None
    if running_mean is not None:
        om, ov = f64(running_mean), f64(running_var)
        rm, rv = (1 - mom) * om + mom * mean, (1 - mom) * ov + mom * unb
        g_rm = 4 * EPS32 * (np.abs((1 - mom) * om) + np.abs(mom * mean)) + mom * g_mean
        g_rv = 4 * EPS32 * (np.abs((1 - mom) * ov) + np.abs(mom * unb)) + mom * g_var * (M / (M - 1) if M > 1 else 1)
    return Stats(s, q, mean, var, invstd, unb, mean, invstd, scale, shift, rm, rv,
                 g_mean, g_var, invstd * r_is, g_mean + EPS32 * np.abs(mean), invstd * (r_is + EPS32), np.abs(scale) * (r_is + 2 * EPS32),
                 T * (r_is + 5 * EPS32) + np.abs(g * invstd) * g_mean + EPS32 * np.abs(shift), g_rm, g_rv)


def train_stats(x, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """qea_bn_train_stats on x [M][C]: exact s and q, then `_stats_from_sums`"""
    x = f64(x)
    M = x.shape[0]
    return _stats_from_sums(col_fsum(x), col_fsum(x * x), col_fsum(np.abs(x)), M, gamma, beta, eps, momentum, running_mean, running_var,
                            sum_depth(M))


def train_stats_from_partials(partials, M, a1, **kw):
    """qea_bn_train_stats_from_partials: the same from [blocks][C][2] partial rows (a1 = sum |x| behind them, for the gates); a lane
    adds at most `blocks` rows"""
    p = f64(partials)
    return _stats_from_sums(col_fsum(p[:, :, 0]), col_fsum(p[:, :, 1]), a1, M, kw.get("gamma"), kw.get("beta"), kw.get("eps", 1e-5),
                            kw.get("momentum", 0.1), kw.get("running_mean"), kw.get("running_var"), len(p) + 30)


def two_pass_var(x):
    """the biased variance as sum (x - mean)^2 / M, mean = s / M: no cancellation, relative error ~ M u64 whatever the mean.  What
    the one-pass formula of the kernel loses is |two_pass_var - var|; its bound is Stats.g_var."""
    x = f64(x)
    d = x - col_fsum(x) / x.shape[0]
    return col_fsum(d * d) / x.shape[0]


EvalCoeff = collections.namedtuple("EvalCoeff", "mean invstd scale shift g_invstd g_scale g_shift")


def eval_coeff(gamma, beta, running_mean, running_var, eps, conv_bias=None):
    """qea_bn_eval_coeff, all in fp32 on the device: invstd = 1 / sqrtf(rvar + eps) (addition, sqrt, division: 3 u32; the library is
    built without fast-math, each is correctly rounded), scale = g * invstd (1 more), shift = b + (bias - rmean) * g * invstd: the
    difference rounds once (u32 |bias - rmean|, no cancellation beyond that: both are inputs), two products and invstd's 3 roundings
    act on the product P = |(bias - rmean) g invstd| (6 u32), the final sum rounds once.  mean_out is rmean itself."""
    rm, rv = f64(running_mean), f64(running_var)
    C = len(rm)
    g = np.ones(C) if gamma is None else f64(gamma)
    b = np.zeros(C) if beta is None else f64(beta)
    cb = np.zeros(C) if conv_bias is None else f64(conv_bias)
    invstd = 1.0 / np.sqrt(rv + float(np.float32(eps)))
    scale = g * invstd
    P = (cb - rm) * g * invstd
    shift = b + P
    return EvalCoeff(rm, invstd, scale, shift, 3 * EPS32 * invstd, 4 * EPS32 * np.abs(scale), 6 * EPS32 * np.abs(P) + EPS32 * np.abs(shift))


# ----------------------------------------------------------------------------- apply (+ ReLU) (+ pool)
def fma32(y, scale, shift):
    """float32 of the EXACT y * scale + shift, one rounding: what __fmaf_rn stores.  The fp64 product of two fp32 values is exact (48
    bits); the fp64 sum rounds, and rounding that to fp32 again could land on the wrong side of a tie.  So the sum is rounded TO ODD
    first (TwoSum gives the sum's error exactly; an inexact sum with an even last bit moves one fp64 step towards the error): with
    53 >= 24 + 2 bits, rounding the odd-rounded value to fp32 is the single correct rounding of the exact value."""
    p = f64(y) * f64(scale)
    h = np.broadcast_to(f64(shift), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + h
        bb = s - p
        e = (p - (s - bb)) + (h - bb)                                  # TwoSum: s + e == p + h exactly
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)   # the exact value lies on e's side of s
        return s.astype(np.float32)


def relu32(v):
    """fmaxf(v, 0): a NaN becomes 0"""
    return np.fmax(v, np.float32(0))


def mask_f64(y, scale, shift):
    """float64(y) * float64(scale) + float64(shift) > 0.  The product is exact and an fp64 sum of two fp32-ranged terms is zero only
    when the exact sum is and has the exact sum's sign otherwise (rounding is monotone and 0 is representable), so this IS the sign of
    the fused multiply-add for every element: none is ambiguous.  (tests/test_bn_spec_cpu.py shows it in rational arithmetic.)"""
    with np.errstate(invalid="ignore"):
        return f64(y) * f64(scale) + f64(shift) > 0


def bn_apply(y, scale, shift, relu):
    """qea_bn_apply on y [M][C] -> a, float32, to the bit.  Without the ReLU a NaN stays one."""
    z = fma32(y, scale, shift)
    return relu32(z) if relu else z


def bn_apply_pool(y, scale, shift, relu, B, H, W, kh, kw):
    """qea_bn_apply_pool -> (a [M][C], pooled [B*OH*OW][C], arg): bn_apply, then c1_spec.pool (first maximum in scan order, NaN wins)"""
    a = bn_apply(y, scale, shift, relu)
    C = a.shape[-1]
    m, arg = pool(a.reshape(B, H, W, C), kh, kw)
    return a, m.reshape(-1, C), arg


# ----------------------------------------------------------------------------- backward
Bwd = collections.namedtuple("Bwd", "dz s q dbeta dgamma dbeta_f32 dgamma_f32 g_dbeta g_dgamma k0 k1 k2 dy g_dy")


def masked_dz(da, y, mask, pool_args=None):
    """dz [M][C] float32.  mask: None (no ReLU), ("a", a) (a > 0), ("remask", scale, shift) (mask_f64).  pool_args = (dpool, B, H, W,
    kw): dpool is routed to the winner of each 2 x kw window of a = relu(fma32(y, scale, shift)) and ADDED IN FP32 to da (da None: to
    zero), as qea_maxpool_bwd(accumulate) leaves it; the mask is a > 0."""
    y = f32(y)
    if pool_args is not None:
        dpool, B, H, W, kw = pool_args
        C = y.shape[-1]
        a = relu32(fma32(y, mask[1], mask[2]))
        routed = f32(pool_bwd(a.reshape(B, H, W, C), f32(dpool).reshape(B, H // 2, W // kw, C), 2, kw, False)).reshape(-1, C)
        d = routed + (np.zeros_like(routed) if da is None else f32(da))
        return np.where(a > 0, d, np.float32(0))
    da = f32(da)
    if mask is None:
        return da
    on = f32(mask[1]) > 0 if mask[0] == "a" else mask_f64(y, mask[1], mask[2])
    return np.where(on, da, np.float32(0))


def bn_bwd(dz, y, gamma, mu, invstd, training, old=None, partials=None):
    """What follows dz in qea_bn_bwd / qea_bn_bwd_pool / qea_bn_bwd_from_partials.  mu, invstd: fp64 [C], the stat64 halves or the
    fp32 vectors.  old = (dgamma0, dbeta0): accumulate.  partials [blocks][C][2]: s and q are THEIR column sums, not dz's.

    s = sum dz, q = sum dz xhat, xhat = (y - mu) invstd evaluated in fp64 as the kernel does (difference, product, product: 3 u64 per
    term), summed exactly here; the device's sums err by depth u64 sum|term|:
        g_s = depth u64 sum|dz|,  g_q = (depth + 3) u64 sum|dz xhat|
    dbeta = (float)s, dgamma = (float)q: + u32 |value|; accumulating: one fp32 addition more, + u32 |old + value|.  (dbeta_f32 /
        dgamma_f32 are the same in fp32 arithmetic: on exactly summable data the device must give these bits.)
    k0 = g is, k1 = -g is^2 m1, k2 = g is (mu is m1 - m0), m0 = s / M, m1 = q / M (0 in eval mode), all fp64:
        g_m0 = g_s / M + u64 |m0|,  g_m1 = g_q / M + u64 |m1|
    dy = (float)(k0 dz + (k1 y + k2)): one fp32 rounding of an fp64 value whose error is at most
        e64 = 5 u64 (|k0 dz| + |k1 y| + |k2| + |g is| (|mu is m1| + |m0|))          roundings of the k's and of the polynomial; the
                                                                                     last term conditions k2's inner difference
            + |g is^2| g_m1 |y| + |g is| (|mu is| g_m1 + g_m0)                      the sums' errors carried through k1 and k2
        g_dy = u32 (|dy| + e64) + e64"""
    dz32 = f32(dz)
    dzd, yd, mu, invstd = f64(dz32), f64(f32(y)), f64(mu), f64(invstd)
    M, C = dzd.shape
    g = np.ones(C) if gamma is None else f64(gamma)
    with np.errstate(invalid="ignore"):
        term = dzd * ((yd - mu) * invstd)
    if partials is None:
        s, q, depth = col_fsum(dzd), col_fsum(term), sum_depth(M)
    else:
        p = f64(partials)
        s, q, depth = col_fsum(p[:, :, 0]), col_fsum(p[:, :, 1]), len(p) + 30
    g_s = depth * EPS64 * col_fsum(np.abs(dzd))
    g_q = (depth + 3) * EPS64 * col_fsum(np.abs(term))
    dbeta, dgamma = s.copy(), q.copy()
    dbeta_f32, dgamma_f32 = s.astype(np.float32), q.astype(np.float32)
    g_db, g_dg = g_s + EPS32 * np.abs(s), g_q + EPS32 * np.abs(q)
    if old is not None:
        dgamma, dbeta = f64(old[0]) + q, f64(old[1]) + s
        dgamma_f32, dbeta_f32 = f32(old[0]) + dgamma_f32, f32(old[1]) + dbeta_f32
        g_db, g_dg = g_db + EPS32 * np.abs(dbeta), g_dg + EPS32 * np.abs(dgamma)
    m0, m1 = (s / M, q / M) if training else (np.zeros(C), np.zeros(C))
    g_m0 = (g_s / M + EPS64 * np.abs(m0)) if training else np.zeros(C)
    g_m1 = (g_q / M + EPS64 * np.abs(m1)) if training else np.zeros(C)
    k0, k1, k2 = g * invstd, -g * invstd * invstd * m1, g * invstd * (mu * invstd * m1 - m0)
    dy = k0 * dzd + (k1 * yd + k2)
    e64 = 5 * EPS64 * (np.abs(k0 * dzd) + np.abs(k1 * yd) + np.abs(k2) + np.abs(g * invstd) * (np.abs(mu * invstd * m1) + np.abs(m0)))
    e64 = e64 + np.abs(g * invstd * invstd) * g_m1 * np.abs(yd) + np.abs(g * invstd) * (np.abs(mu * invstd) * g_m1 + g_m0)
    return Bwd(dz32, s, q, dbeta, dgamma, dbeta_f32, dgamma_f32, g_db, g_dg, k0, k1, k2, dy, EPS32 * (np.abs(dy) + e64) + e64)


def partial_rows(dz, y, mu, invstd, blocks):
    """[blocks][C][2] partial rows as a producer would leave them: row r of dz goes to block r % blocks (fp64 sums in row order)"""
    dzd, yd = f64(f32(dz)), f64(f32(y))
    term = np.stack([dzd, dzd * ((yd - f64(mu)) * f64(invstd))], axis=-1)
    P = np.zeros((blocks,) + term.shape[1:])
    np.add.at(P, np.arange(len(dzd)) % blocks, term)
    return P


# ----------------------------------------------------------------------------- column and layout kernels
def colsum(x, old=None):
    """qea_colsum -> (value fp64, the same in fp32 arithmetic, gate): (float)sum x, + old in fp32 when accumulating.
    gate = sum_depth u64 sum|x| + u32 |sum| (+ u32 |old + sum|)"""
    x = f64(x)
    s = col_fsum(x)
    gate = sum_depth(x.shape[0]) * EPS64 * col_fsum(np.abs(x)) + EPS32 * np.abs(s)
    if old is None:
        return s, s.astype(np.float32), gate
    return f64(old) + s, f32(old) + s.astype(np.float32), gate + EPS32 * np.abs(f64(old) + s)


def absmax(x):
    """qea_absmax over the [M][C] columns the caller selected: float32 of the largest finite |x|, 0 when there is none"""
    return np.float32(amax(x))


def transpose2d(a):
    return np.ascontiguousarray(np.asarray(a).T)


def filter_flip_transpose(w):
    """w [Co][KH][KW][Ci] -> [Ci][KH][KW][Co] with both filter axes reversed (the filter of the input-gradient convolution)"""
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


# ----------------------------------------------------------------------------- launch arithmetic (mirrors; proofs only)
RED_THREADS = 256
SCRATCH_ROWS = 256                                       # QEA_BN_PARTIAL_SCRATCH_ROWS
ColGeom = collections.namedtuple("ColGeom", "cols rt want grid rows_per_block")
ApplyGeom = collections.namedtuple("ApplyGeom", "want grid per_block")


def cdiv(a, b):
    return -(-a // b)


def col_geom(M, C):
    """col_geom of norm_pool.hip; `want` is the block count BEFORE the 1024 cap"""
    cols = C // 4
    rt = max(RED_THREADS // cols, 1)
    want = cdiv(M, rt * 16)
    grid = min(max(want, 1), 1024)
    rpb = cdiv(M, grid)
    return ColGeom(cols, rt, want, cdiv(M, rpb), rpb)


def apply_geom(items, rt, per_thread):
    want = cdiv(items, rt * per_thread)
    grid = min(max(want, 1), 4096)
    per = cdiv(items, grid)
    return ApplyGeom(want, cdiv(items, per), per)


def grid_for(n, cap=4096):
    """qea_grid_for: 256-thread blocks, capped -> (grid, trips of the grid-stride loop the busiest thread makes)"""
    grid = min(max(cdiv(n, 256), 1), cap)
    return grid, cdiv(n, grid * 256)


def absmax_grid(M, C):
    n = M * (C // 4)
    want = n // 256 // 8
    return min(max(want, 1), 2048), want


def colreduce_ws_bytes(M, C):
    return (col_geom(M, C).grid * 2 + 3) * C * 8


def rows_per_thread(per_block, rt_n, block_rows=None):
    """rows each of the rt_n row-threads of a block walks when the block holds block_rows (default per_block) rows"""
    n = per_block if block_rows is None else block_rows
    return [len(range(rt, n, rt_n)) for rt in range(rt_n)]


def bwd_pool_geom(B, H, W, C, kw):
    """the window-block geometry of qea_bn_bwd_pool -> (gm, reduction grid, windows per block, ApplyGeom of the elementwise kernel)"""
    M = B * H * W
    nwin = M // (2 * kw)
    gm = col_geom(M, C)
    wpb = max(cdiv(gm.rows_per_block, 2 * kw), 1)
    return gm, cdiv(nwin, wpb), wpb, apply_geom(nwin, gm.rt, 4)


def fold(blocks):
    """fold_partials -> (folded?, rows the finalize kernel reads, partial rows per scratch row)"""
    if blocks <= 2 * SCRATCH_ROWS:
        return False, blocks, 0
    per = cdiv(blocks, SCRATCH_ROWS)
    return True, cdiv(blocks, per), per


# ----------------------------------------------------------------------------- shape tables
# (C, M) of the reductions and of bn_bwd, each with the branch it reaches (asserted by test_bn_spec_cpu.py)
RED = ((12, 130),      # cols = 3: 85 row-threads, thread 255 idle
       (64, 5),        # fewer rows than row-threads
       (1024, 7),      # one row-thread per block
       (1024, 33),     # 3 blocks of 11 rows
       (32, 8197),     # 17 blocks, ragged last; bn_bwd_apply_kernel: threads with an odd and with an even number of rows
       (96, 1))        # M == 1: the unbiased variance is the biased one
RED_BIG = (1024, 16400)                                  # want = 1025 > 1024: the cap (64 MB per tensor; exact data only)
APPLY_BIG = (32, 131080)                                 # M C / 4 = 4096 * 256 + 64: a second grid-stride trip of bn_apply
# apply_geom's 4096-block cap needs M > 4096 * 8 rows at rt = 1 (C = 1024): 128 MB per tensor.  Not reached here; the full-size model
# tests run through it.
POOL = tuple((3, H, W, C, 2, kw) for kw in (1, 2) for H in (2, 8) for W in (4, 16) for C in (12, 64, 1024))   # (B, H, W, C, kh, kw)
POOL_APPLY_BIG = (1, 2, 131080, 32, 2, 1)                # 131080 windows x 8 columns > 4096 * 256
POOL_BWD_RAGGED = (3, 8, 172, 32, 2, 2)                  # 9 window blocks of 115, the last with 112
PART_BLOCKS = (1, 3, 512, 513, 700)                      # 512: at the fold threshold; 513, 700: folded, 700 with a ragged last range
PART_C = (12, 384, 1024)                                 # 384: partials_reduce_kernel's second column pass is 128 wide
PART_M = 130
ABSMAX = ((1, 4, 4), (3, 12, 20))                        # (M, C, ld)
ABSMAX_BIG = (16400, 1024, 1024)                         # 4,198,400 float4 > 2048 * 256 * 8: the grid cap (67 MB)
TRANSPOSE = ((1, 1), (32, 32), (33, 31), (100, 70), (7, 2048))
FLIP = ((12, 20, 3, 3), (5, 33, 2, 2), (7, 3, 1, 1))     # (Co, Ci, KH, KW)


def strides(C):
    """(ld, column offset): alone, the second half of a 2C concat buffer, C + 8"""
    return ((C, 0), (2 * C, C), (C + 8, 0))


# ----------------------------------------------------------------------------- data
CONST_CH, BIG_CH = 1, 2                                  # real data: the constant channel and the mean-10^3, spread-10^-2 channel
CONST_VALUE = 2.75
_MEANS = (0.0, 0.7, -3.0, 30.0, 0.1)
_SPREADS = (1.0, 2.0, 0.05, 4.0)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def exact_rows(M, C, *key):
    """multiples of 2^-6 in [-4, 4], float32.  Sums of them, of their squares (units of 2^-12) and, with mean = 0.5 and invstd = 2,
    of dz xhat (units of 2^-11) are exact in fp64 in any order while the number of units stays below 2^53 (`exact_units`)."""
    return (_rng(M, C, *key).integers(-256, 257, size=(M, C)) / 64.0).astype(np.float32)


def exact_units(M):
    """the largest sum of |units| a table shape can reach: M rows of |x|^2 <= 16 in units of 2^-12 (the finest of the three)"""
    return M * 16 * 2 ** 12


def real_rows(M, C, *key):
    """seeded normal data, channel c with mean _MEANS[c % 5] and spread _SPREADS[c % 4]; channel CONST_CH constant, channel BIG_CH
    with mean 10^3 and spread 10^-2"""
    r = _rng(M, C, 7, *key)
    x = r.standard_normal((M, C)) * np.array([_SPREADS[c % 4] for c in range(C)]) + np.array([_MEANS[c % 5] for c in range(C)])
    x[:, CONST_CH] = CONST_VALUE
    x[:, BIG_CH] = 1e3 + 1e-2 * r.standard_normal(M)
    return x.astype(np.float32)


def vectors(C, *key):
    """gamma (both signs, away from 0), beta, running_mean, running_var (> 0.5), conv_bias: float32 [C]"""
    r = _rng(C, 11, *key)
    gamma = (r.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 0, -1.0, 1.0)).astype(np.float32)
    return gamma, f32(r.standard_normal(C) * 0.3), f32(r.standard_normal(C)), f32(r.uniform(0.5, 1.5, C)), f32(r.standard_normal(C))


def exact_vectors(C, *key):
    """gamma, beta as multiples of 2^-4 (gamma != 0): with mean 0.5 and invstd 2, scale and shift are exact too"""
    r = _rng(C, 13, *key)
    gamma = r.integers(4, 25, C) / 16.0 * np.where(np.arange(C) % 3 == 0, -1.0, 1.0)
    return f32(gamma), f32(r.integers(-8, 9, C) / 16.0)


FORCED_MEAN, FORCED_INVSTD = 0.5, 2.0


def forced_stats(C):
    """mean = 0.5, invstd = 2 -> (mean32, invstd32, stat64 [2][C])"""
    m, i = np.full(C, FORCED_MEAN), np.full(C, FORCED_INVSTD)
    return f32(m), f32(i), np.stack([m, i])


def pool_rows(B, H, W, C, kw, kind, *key):
    """y [B*H*W][C] for the pool cases: exact or real rows with a tie across and down a window (first in scan order wins) and a window
    whose activations are all zero under the ReLU"""
    M = B * H * W
    y = (exact_rows if kind == "exact" else real_rows)(M, C, 3, *key).reshape(B, H, W, C)
    y[0, 0, 0:2, :8] = 0.25
    y[0, 0:2, 2, :8] = 0.25
    y[1, H - 2:H, 0:2, 8:12] = -3.0
    return y.reshape(M, C)


# ----------------------------------------------------------------------------- abs-max positions
def amax_rows(C, M, per_block, rt_n):
    """{name: (row, column)} where the largest stored magnitude is planted in turn for a row kernel over [M][C] whose blocks hold
    per_block rows walked by rt_n row-threads: first and last element, the last row of the (ragged) last block, the last column
    (next to the idle lane at C = 12), and a row that a thread with an odd row count reaches last (bn_bwd_apply_kernel's odd tail)"""
    out = {"first": (0, 0), "last": (M - 1, C - 1), "last_row_first_col": (M - 1, 0), "last_col": (M // 2, C - 1)}
    counts = rows_per_thread(per_block, rt_n, min(per_block, M))
    odd = [rt for rt, n in enumerate(counts) if n % 2 == 1]
    if odd:
        rt = odd[-1]
        out["odd_tail"] = (rt + (counts[rt] - 1) * rt_n, C // 2)
    return out


AMAX_POOL = ((3, 8, 16, 12, 2, 2), (3, 2, 4, 64, 2, 1), POOL_BWD_RAGGED)     # the pool cases of the abs-max positions


def amax_pool_rows(B, H, W, C, kw):
    """{name: (row, column)} for the pool kernels: the last element of the last window, that window's first element, the very first"""
    M = B * H * W
    return {"last": (M - 1, C - 1), "last_window_first": (M - 1 - W - (kw - 1), 0), "first": (0, 0)}


def plant(rows, where, value):
    """a copy of `rows` with `value` at `where`"""
    out = np.array(rows, dtype=np.float32, copy=True)
    out[where] = value
    return out


def unique_finite_max_at(out):
    """the (row, column) of the single largest finite |out|, or None when it is not unique or there is none"""
    a = np.abs(f64(out))
    a = np.where(np.isfinite(a), a, -1.0)
    top = a.max()
    if top <= 0 or int((a == top).sum()) != 1:
        return None
    return tuple(int(i) for i in np.unravel_index(int(a.argmax()), a.shape))
