"""Plain numpy statements, fp64, of the single-channel kernels of csrc/conv_c1.hip (3x3 pad-1 convolution with C_in = 1: forward,
forward + 2x2 max-pool, weight / bias gradient, input gradient, the whole backward from the pooled gradient; the UNet head) and of the
two max-pool kernels of csrc/norm_pool.hip.  Each is written for reading, not for speed, and imports nothing of the library it checks.
tests/test_c1_spec_cpu.py holds them to torch in double precision; tests/test_c1_kernels_gpu.py holds the kernels to them.

Layouts are the library's: x [B][H][W], activations NHWC [B][H][W][C], filter [Co][9] (tap = kh * 3 + kw), head rows [M][C].

Beside each value the statements return `cond`, the sum of the magnitudes of the terms the value is a sum of: a gate is a number of
fp32 roundings x 2^-24 x cond ("Single-channel kernels").  The shape tables and input builders at the end are shared by
the two test files, so that the CPU tests speak about the very data the device sees."""
import collections
import zlib

import numpy as np

EPS32 = 2.0 ** -24                                       # half an ulp of fp32, relative: one rounding


def gate_ratio(got, ref, gate):
    """largest |got - ref| / gate over the elements where ref is no NaN (0 / 0 counts as 0, x / 0 as inf): <= 1 passes"""
    got, ref, gate = (np.asarray(a, dtype=np.float64) for a in (got, ref, gate))
    ok = ~np.isnan(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(ok & (got != ref), np.abs(got - ref), 0.0)       # equal infinities agree
        r = np.where(err == 0, 0.0, err / gate)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------- 3x3 convolution, C_in = 1
def taps(x):
    """x [B][H][W] -> [B*H*W][9]: column kh * 3 + kw holds x[b][h + kh - 1][w + kw - 1], zero outside the image"""
    x = f64(x)
    B, H, W = x.shape
    xp = np.zeros((B, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    return np.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], axis=-1).reshape(B * H * W, 9)


def relu(v):
    """max(v, 0) as fmaxf has it: a NaN becomes 0 (torch.relu keeps the NaN; the kernels' ReLU does not)"""
    return np.fmax(v, 0.0)


def conv_fwd(x, w, bias, relu_on):
    """y[b][h][w][c] = bias[c] + sum_tap w[c][tap] x[b][h + kh - 1][w + kw - 1] (ReLU: `relu`) -> (y, cond) both [B][H][W][Co],
    cond = |bias[c]| + sum_tap |w x|"""
    B, H, W = np.shape(x)
    X, w = taps(x), f64(w)
    b = np.zeros(len(w)) if bias is None else f64(bias)
    with np.errstate(invalid="ignore"):
        y = X @ w.T + b
        cond = np.abs(X) @ np.abs(w).T + np.abs(b)
    if relu_on:
        y = relu(y)
    return y.reshape(B, H, W, -1), cond.reshape(B, H, W, -1)


def conv_wgrad(x, dy):
    """dw[c][tap] = sum_p dy[p][c] x[p + tap], db[c] = sum_p dy[p][c] -> (dw [Co][9], db [Co], cond_w, cond_b): the sums of magnitudes"""
    X, g = taps(x), f64(dy).reshape(-1, np.shape(dy)[-1])
    return g.T @ X, g.sum(0), np.abs(g).T @ np.abs(X), np.abs(g).sum(0)


def conv_dgrad(dy, w):
    """dx[b][h][w] = sum_{kh, kw, c} dy[b][h + 1 - kh][w + 1 - kw][c] w[c][kh * 3 + kw] -> (dx, cond) both [B][H][W]"""
    B, H, W, Co = np.shape(dy)
    g, w = f64(dy).reshape(-1, Co), f64(w)
    out = []
    for T in (g @ w, np.abs(g) @ np.abs(w)):                            # T[p][tap] = sum_c dy[p][c] w[c][tap]
        Tp = np.zeros((B, H + 2, W + 2, 9))
        Tp[:, 1:-1, 1:-1] = T.reshape(B, H, W, 9)
        out.append(sum(Tp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, kh * 3 + kw] for kh in range(3) for kw in range(3)))
    return out[0], out[1]


# ----------------------------------------------------------------------------- max-pool, window == stride
def _windows(x, kh, kw):
    """[B][H][W][C] -> [B][H/kh][W/kw][kh*kw][C], the window's elements in row-major scan order"""
    B, H, W, C = x.shape
    return x.reshape(B, H // kh, kh, W // kw, kw, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // kh, W // kw, kh * kw, C)


def _unwindows(xw, kh, kw):
    B, OH, OW, _, C = xw.shape
    return xw.reshape(B, OH, OW, kh, kw, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, OH * kh, OW * kw, C)


def pool(x, kh, kw):
    """-> (pooled, arg) [B][H/kh][W/kw][C].  The scan starts from (-inf, position 0) and takes an element v over the running m when
    `v > m or v != v` (pool_take): the first maximum in scan order wins, -0.0 and +0.0 tie and the first is kept, a NaN wins and no
    number replaces it (of several NaNs the last is the winner).  The value keeps the dtype of x, so a float32 x gives the bits."""
    xw = _windows(np.asarray(x), kh, kw)
    m = np.full_like(xw[:, :, :, 0], -np.inf)
    arg = np.zeros(m.shape, dtype=np.int64)
    for k in range(kh * kw):
        v = xw[:, :, :, k]
        with np.errstate(invalid="ignore"):
            take = (v > m) | (v != v)
        m, arg = np.where(take, v, m), np.where(take, k, arg)
    return m, arg


def pool_bwd(x, dy, kh, kw, relu_mask):
    """dy [B][H/kh][W/kw][C] routed to each window's winner -> [B][H][W][C], zero elsewhere.  relu_mask: a window whose winner is not
    > 0 routes nothing (the pool of a ReLU output; a NaN winner is not > 0)."""
    m, arg = pool(x, kh, kw)
    dy = np.asarray(dy)
    if relu_mask:
        with np.errstate(invalid="ignore"):
            dy = np.where(m > 0, dy, np.zeros_like(dy))
    out = np.stack([np.where(arg == k, dy, np.zeros_like(dy)) for k in range(kh * kw)], axis=3)
    return _unwindows(out, kh, kw)


def amax(t):
    """the largest finite |t| (0 when there is none): NaN and inf are skipped, as in qea_amax_acc"""
    a = np.abs(f64(t)).ravel()
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


# ----------------------------------------------------------------------------- conv -> ReLU -> pool(2, 2), backward from the pooled gradient
PoolBwd = collections.namedtuple("PoolBwd", "masked dw db dx cond_w cond_b cond_x pre cond_pre")


def conv_pool_bwd(x, w, bias, dpool):
    """conv_fwd(relu) -> pool(2, 2) -> pool_bwd(relu_mask) -> conv_wgrad / conv_dgrad.  masked = dpool where the window's maximum
    is > 0, else 0 (what the kernel leaves in dpool); pre / cond_pre: the pre-activations and their cond, for `undecided`."""
    pre, cond_pre = conv_fwd(x, w, bias, False)
    y = relu(pre)
    m, _ = pool(y, 2, 2)
    dpool = f64(dpool)
    G = pool_bwd(y, dpool, 2, 2, True)
    dw, db, cw, cb = conv_wgrad(x, G)
    dx, cx = conv_dgrad(G, w)
    return PoolBwd(np.where(m > 0, dpool, 0.0), dw, db, dx, cw, cb, cx, pre, cond_pre)


FWD_ROUNDINGS = 10                                       # bias + nine products: any order of a 10-term fp32 sum


def undecided(pre, cond_pre, kh=2, kw=2):
    """[B][H/kh][W/kw][C] bool: the windows of relu(pre) whose winner or ReLU mask an fp32 evaluation within the forward gate
    g = 10 x 2^-24 x cond may decide otherwise.  With s the statement's winner: (a) another element j with pre_j != pre_s whose
    interval relu(pre_j +- g_j) reaches that of s above zero; (b) pre_s within g_s of zero without being zero.  Exact ties (equal
    pre-activations: equal operands in the same order, on any implementation) and elements decidedly below zero are decided."""
    g = FWD_ROUNDINGS * EPS32 * cond_pre
    _, arg = pool(relu(pre), kh, kw)
    P, G = _windows(pre, kh, kw), _windows(g, kh, kw)
    idx = arg[:, :, :, None, :]
    ps, gs = np.take_along_axis(P, idx, 3), np.take_along_axis(G, idx, 3)
    lo_s, hi_s = relu(ps - gs), relu(ps + gs)
    hi = relu(P + G)
    a = ((P != ps) & (hi >= lo_s) & (np.maximum(hi, hi_s) > 0)).any(axis=3)
    b = ((np.abs(ps) <= gs) & (ps != 0))[:, :, :, 0]
    return a | b


def undecided_slack(x, w, dpool, und):
    """What the undecided windows may move -> (slack_w [Co][9], slack_b [Co], slack_x [B][H][W]).  Such a window sends its gradient g
    to another of its four positions or nowhere: db[c] moves by at most |g|, dw[c][tap] by at most 2 |g| max|x| over the window's
    4 x 4 input patch, and the dx of that patch by at most 2 |g| max_tap |w[c][tap]|."""
    x, w, dpool = f64(x), f64(w), f64(dpool)
    B, H, W = x.shape
    sw, sb, sx = np.zeros(w.shape), np.zeros(len(w)), np.zeros(x.shape)
    for b, oh, ow, c in np.argwhere(und):
        g = abs(dpool[b, oh, ow, c])
        r0, r1, c0, c1 = max(2 * oh - 1, 0), min(2 * oh + 3, H), max(2 * ow - 1, 0), min(2 * ow + 3, W)
        sb[c] += g
        sw[c] += 2 * g * np.abs(x[b, r0:r1, c0:c1]).max()
        sx[b, r0:r1, c0:c1] += 2 * g * np.abs(w[c]).max()
    return sw, sb, sx


# ----------------------------------------------------------------------------- UNet head: 1x1 conv C -> 1, sigmoid
def head_fwd(x, w, b):
    """y[m] = sigmoid(sum_c x[m][c] w[c] + b) -> (y, gate).  gate = y (1 - y) (C + 1) 2^-24 (sum |x w| + |b|) + 4 x 2^-24 y: the
    C products and additions of z (and the add of b) reach y through sigmoid'(z) = y (1 - y); expf, the add of 1 and the divide give
    the second term (expf of the ROCm device library: 1 ulp = 2 x 2^-24, documented in the HIP math API's accuracy table).  Below
    the smallest normal fp32 number a result has no relative precision (expf(-z) overflows from z < -88.7, where y < 2^-126, and
    the kernel then returns 0): the gate has that number, 2^-126, as its floor."""
    x, w = f64(x), f64(w)
    z = x @ w + float(b)
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-z))
    cond = np.abs(x) @ np.abs(w) + abs(float(b))
    return y, y * (1 - y) * (x.shape[1] + 1) * EPS32 * cond + 4 * EPS32 * y + 2.0 ** -126


HeadBwd = collections.namedtuple("HeadBwd", "dx dw db cond_w cond_b")


def head_bwd(x, y32, dyy, w):
    """dz = dyy y (1 - y) from the fp32 y the device was given; dx[m][c] = dz[m] w[c], dw[c] = sum_m dz[m] x[m][c], db = sum_m dz[m]"""
    x, y, dyy, w = f64(x), f64(y32), f64(dyy), f64(w)
    dz = dyy * y * (1 - y)
    return HeadBwd(dz[:, None] * w[None, :], dz @ x, dz.sum(), np.abs(dz) @ np.abs(x), np.abs(dz).sum())


# ----------------------------------------------------------------------------- launch geometry, restated from csrc/conv_c1.hip
def c1_wgrad_geom(M, Co):
    """-> (rt_n, rows_per_thread, blocks) of qea_conv_c1_wgrad: rt_n = 256 / (Co / 4) pixel rows per block and step,
    rows_per_thread = M / (rt_n * 4096) clamped to 32 .. 128.  A thread adds rows_per_thread multiply-adds in fp32, the block's LDS
    sum adds rt_n such partials in fp32, the blocks are folded in fp64: the longest fp32 chain is rows_per_thread + rt_n."""
    rt_n = 256 // (Co // 4)
    rpt = min(max(M // (rt_n * 4096), 32), 128)
    return rt_n, rpt, -(-M // (rt_n * rpt))


def wgrad_chain(M, Co):
    rt_n, rpt, _ = c1_wgrad_geom(M, Co)
    return rpt + rt_n


def c1pb_win_per_wave(NW):
    """windows per wave of c1_pool_wgrad_kernel: about 2048 blocks of four waves, at least 16, whole groups of four.  A wave adds four
    multiply-adds per window (one per position, three of them zeros) in fp32: a chain of 4 x win_per_wave; the waves are folded in fp64."""
    return (max(-(-NW // (4 * 2048)), 16) + 3) // 4 * 4


FWD4_PIXELS_PER_TRIP = 16384 * (256 // 32) * 4            # Co = 128: 16384 blocks x 8 groups x 4 pixels = 524,288
FWD1_PIXELS_PER_TRIP = 8192 * 256 // 32                   # Co = 128: 8192 blocks x 256 threads / 32 columns = 65,536
WGRAD_BLOCK_PIXELS = 512                                  # rt_n * 32 at Co = 64
DGRAD_TILE = (8, 64)

# ----------------------------------------------------------------------------- shape tables (B, H, W, Co): the branch each entry reaches
FWD4 = (                                                  # conv_c1_fwd4_kernel: W % 4 == 0 and Co in {32, 64, 128}
    (2, 1, 4, 32),                                        # one group per image: both row neighbours are padding
    (1, 2, 8, 64),                                        # two groups per row, first and last image row
    (3, 5, 12, 128),                                      # interior rows, three images
)
FWD4_BIG = (65, 32, 256, 128)                             # 532,480 pixels > 524,288: the grid-stride second trip
FWD1 = (                                                  # conv_c1_fwd_kernel: W % 4 != 0 or Co outside {32, 64, 128}
    (1, 1, 1, 32),                                        # all eight neighbours are padding
    (2, 3, 5, 64),                                        # W % 4 != 0
    (2, 4, 8, 48),                                        # W % 4 == 0, Co outside the set
    (2, 4, 8, 4),                                         # one float4 column
)
FWD1_BIG = (9, 32, 230, 128)                              # 66,240 pixels > 65,536: the second trip
FWD_POOL = ((1, 2, 4, 32), (2, 6, 12, 64), (3, 4, 8, 128))
WGRAD = (
    (1, 1, 1, 32),                                        # one pixel, one block
    (40, 3, 5, 32),                                       # H * W = 15 < rt_n = 32: a step crosses whole images (ph % H)
    (1, 9, 57, 64),                                       # 513 pixels: one more than a block's 512
    (3, 4, 8, 48),                                        # rt_n = 21: threads 252 .. 255 idle
    (1, 16, 200, 128),                                    # rt_n = 8, W > rt_n
)
WGRAD_BIG = (9, 32, 4096, 128)                            # 1,179,648 pixels: rows_per_thread = 36, 4096 blocks
DGRAD = (
    (1, 1, 1, 32),
    (2, 8, 64, 64),                                       # one exact 8 x 64 tile per image
    (2, 9, 65, 64),                                       # one row and one column past it: four tiles per image
    (3, 7, 63, 128),                                      # one short of it
    (1, 17, 130, 32),                                     # 3 x 3 tiles, the last ones two columns / one row wide
)
POOL_BWD = (                                              # (B, H, W), Co = 64
    (1, 2, 8),                                            # 4 windows: one wave does a quarter of its 16, three waves are empty
    (1, 6, 24),                                           # 36 windows: waves of 16, 16 and 4
    (2, 4, 40),                                           # 80 windows: the second block holds 16
)
POOL_BWD_BIG = (129, 32, 128)                             # 132,096 windows: win_per_wave = 20: waves start mid-row and cross images
HEAD_C = (32, 64)
HEAD_M = (1, 63, 64 * 1024 + 5)                           # the last: the backward's 1024-block grid wraps (C = 64: 4097 blocks of work)
POOL_WINDOWS = ((2, 2), (2, 1), (1, 2), (3, 2))
POOL_SHAPES = ((1, 6, 4, 4), (3, 6, 8, 64), (2, 12, 6, 512))          # (B, H, W, C)
REAL_SCALES = (1.0, 2.0 ** -12)


# ----------------------------------------------------------------------------- shared inputs
def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


Data = collections.namedtuple("Data", "x w bias dy")


def int_data(B, H, W, Co, tag=""):
    """x in {0 .. 3}, w and bias in {-2 .. 2}, dy in {-1, 0, 1} (int8: the large shapes): every partial sum of every summation order
    is an integer below 2^24 (`int_bounds`), so an fp32 kernel must equal the statement exactly"""
    r = _rng("int", B, H, W, Co, tag)
    return Data(r.randint(0, 4, (B, H, W)).astype(np.float32), r.randint(-2, 3, (Co, 9)).astype(np.float32),
                r.randint(-2, 3, Co).astype(np.float32), r.randint(-1, 2, (B, H, W, Co)).astype(np.int8))


def int_bounds(B, H, W, Co):
    """the largest magnitude any partial sum of the int kind can reach: (forward, weight gradient, input gradient)"""
    return 2 + 9 * 2 * 3, 3 * B * H * W, 9 * Co * 2


def real_data(B, H, W, Co, scale, tag=""):
    """x = rand x scale, w = randn, bias and dy = randn x scale, all fp32.  Planted (Co >= 8): channel 1 has a zero filter and a
    positive bias (every window an exact four-way tie), channel 2 a non-positive filter and a negative bias (every window all-negative:
    four zeros after the ReLU), and where the image has room the 4 x 4 patch x[0][1:5][1:5] is constant (window (1, 1) of every channel
    an exact tie)."""
    r = _rng("real", B, H, W, Co, scale, tag)
    s = np.float32(scale)
    x = r.rand(B, H, W).astype(np.float32) * s
    w = r.randn(Co, 9).astype(np.float32)
    bias = r.randn(Co).astype(np.float32) * s
    dy = r.randn(B, H, W, Co).astype(np.float32) * s
    if Co >= 8:
        w[1], bias[1] = 0, abs(bias[1]) + s
        w[2], bias[2] = -np.abs(w[2]), -abs(bias[2]) - s
    if H >= 5 and W >= 5:
        x[0, 1:5, 1:5] = np.float32(0.375) * s
    return Data(x, w, bias, dy)


def pool_dpool(B, H, W, Co, kind, scale=1.0):
    """the pooled tensor's gradient [B][H/2][W/2][Co] of the conv -> ReLU -> pool backward"""
    r = _rng("dpool", B, H, W, Co, kind, scale)
    if kind == "int":
        return r.randint(-1, 2, (B, H // 2, W // 2, Co)).astype(np.float32)
    return r.randn(B, H // 2, W // 2, Co).astype(np.float32) * np.float32(scale)


def pool_data(B, H, W, C, kh, kw):
    """x [B][H][W][C] fp32 for the max-pool kernels and dy [B][H/kh][W/kw][C]: a ReLU'd randn (ties at zero, all-zero windows), some
    of the zeros negative (-0.0 before and after +0.0), positive ties between the two diagonals of every 2 x 2 block of image 0, and a
    NaN, two NaNs in one window, a +inf, a -inf and a NaN beside a +inf at fixed places of the last image"""
    r = _rng("pool", B, H, W, C, kh, kw)
    x = np.maximum(r.randn(B, H, W, C), 0).astype(np.float32)
    x[(x == 0) & (r.rand(B, H, W, C) < 0.5)] = np.float32(-0.0)
    x[0, ::2, ::2] = x[0, 1::2, 1::2]
    b = B - 1
    x[b, 0, 0, 0] = np.nan
    x[b, 0, 0, 1] = x[b, kh - 1, kw - 1, 1] = np.nan                    # first and last element of window (0, 0)
    x[b, kh - 1, kw - 1, 2] = np.inf
    x[b, 0, 0, 3] = -np.inf
    x[b, H - 1, W - 1, 0] = np.inf
    x[b, H - kh, W - kw, 0] = np.nan                                    # the same window: the NaN wins over the +inf
    x[b, H - 1, 0, 3] = np.float32(-1.5)                                # a window of negative numbers
    x[b, H - kh, 0, 3] = np.float32(-2.5)
    if kh * kw > 2:
        x[b, H - 1, 1, 3] = x[b, H - kh, 1, 3] = np.float32(-2.0)
    dy = (r.randn(B, H // kh, W // kw, C) + 0.25).astype(np.float32)
    dy[0, 0, 0, 0] = np.inf                                             # an abs-max must skip it
    return x, dy


def head_data(M, C, kind, scale=1.0):
    """-> (x [M][C], w [C], b, dyy [M], y32 or None).  int: x in {0 .. 3}, w in {-2 .. 2}, b = 1, dyy in {-4, 0, 4} and the backward is
    given y = 0.5, so dz = dyy y (1 - y) is -1, 0 or 1 exactly and dx, dw, db are integers below 2^24.  real: randn, x and dyy x scale."""
    r = _rng("head", M, C, kind, scale)
    if kind == "int":
        return (r.randint(0, 4, (M, C)).astype(np.float32), r.randint(-2, 3, C).astype(np.float32), np.float32(1.0),
                (4 * r.randint(-1, 2, M)).astype(np.float32), np.full(M, 0.5, dtype=np.float32))
    s = np.float32(scale)
    return r.randn(M, C).astype(np.float32) * s, r.randn(C).astype(np.float32), np.float32(r.randn()), r.randn(M).astype(np.float32) * s, None
