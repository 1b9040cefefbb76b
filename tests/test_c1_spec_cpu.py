"""The statements of tests/c1_spec.py held to torch in double precision (F.conv2d, F.max_pool2d, torch.sigmoid, autograd) and to a
direct loop, on the very inputs tests/test_c1_kernels_gpu.py gives the device; the NaN and tie rules on hand-written windows; the
integer bounds of the `int` kind; and the arithmetic behind every comment of the shape tables, so that an edit of a table cannot
silently leave the branch its entry is there for.  No GPU, nothing of the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import c1_spec as S

def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


SMALL_CONV = S.FWD4 + S.FWD1 + S.FWD_POOL + S.WGRAD[:4] + ((2, 9, 65, 64), (1, 17, 130, 32))


# ----------------------------------------------------------------------------- convolution against torch
@pytest.mark.parametrize("shape", SMALL_CONV)
@pytest.mark.parametrize("scale", S.REAL_SCALES)
def test_conv_statements_match_torch_double(shape, scale):
    B, H, W, Co = shape
    d = S.real_data(B, H, W, Co, scale)
    x = t64(d.x).reshape(B, 1, H, W).requires_grad_()
    w = t64(d.w).reshape(Co, 1, 3, 3).requires_grad_()
    b = t64(d.bias).requires_grad_()
    pre = F.conv2d(x, w, b, padding=1)
    pre.backward(t64(d.dy).permute(0, 3, 1, 2))
    y, cond = S.conv_fwd(d.x, d.w, d.bias, False)
    assert close(y, pre.detach().permute(0, 2, 3, 1)) and (cond >= np.abs(y) - 1e-12).all()
    assert close(S.conv_fwd(d.x, d.w, d.bias, True)[0], pre.detach().relu().permute(0, 2, 3, 1))
    assert close(S.conv_fwd(d.x, d.w, None, False)[0], F.conv2d(x, w, None, padding=1).detach().permute(0, 2, 3, 1))
    dw, db, cw, cb = S.conv_wgrad(d.x, d.dy)
    assert close(dw, w.grad.reshape(Co, 9)) and close(db, b.grad)
    assert (cw >= np.abs(dw) - 1e-12).all() and (cb >= np.abs(db) - 1e-12).all()
    dx, cx = S.conv_dgrad(d.dy, d.w)
    assert close(dx, x.grad.reshape(B, H, W)) and (cx >= np.abs(dx) - 1e-12).all()


def test_conv_statements_match_a_direct_loop_on_the_int_kind():
    B, H, W, Co = 2, 3, 5, 4
    d = S.int_data(B, H, W, Co)
    y = np.zeros((B, H, W, Co))
    dw, dx = np.zeros((Co, 9)), np.zeros((B, H, W))
    for b in range(B):
        for h in range(H):
            for w_ in range(W):
                for c in range(Co):
                    acc = float(d.bias[c])
                    for kh in range(3):
                        for kw in range(3):
                            ih, iw = h + kh - 1, w_ + kw - 1
                            if 0 <= ih < H and 0 <= iw < W:
                                acc += float(d.w[c, kh * 3 + kw]) * float(d.x[b, ih, iw])
                                dw[c, kh * 3 + kw] += float(d.dy[b, h, w_, c]) * float(d.x[b, ih, iw])
                                dx[b, ih, iw] += float(d.dy[b, h, w_, c]) * float(d.w[c, kh * 3 + kw])
                    y[b, h, w_, c] = acc
    assert np.array_equal(S.conv_fwd(d.x, d.w, d.bias, False)[0], y)
    assert np.array_equal(S.conv_wgrad(d.x, d.dy)[0], dw) and np.array_equal(S.conv_wgrad(d.x, d.dy)[1], d.dy.sum((0, 1, 2)))
    assert np.array_equal(S.conv_dgrad(d.dy, d.w)[0], dx)
    assert np.array_equal(S.relu(np.array([np.nan, -1.0, 2.0])), [0.0, 0.0, 2.0])          # fmaxf's rule, not torch.relu's


# ----------------------------------------------------------------------------- pool
def test_pool_rules_on_hand_written_windows():
    nan, inf = np.nan, np.inf

    def one(vals, kh=2, kw=2):
        m, arg = S.pool(np.asarray(vals, dtype=np.float32).reshape(1, kh, kw, 1), kh, kw)
        return m[0, 0, 0, 0], int(arg[0, 0, 0, 0])

    assert one([1, 3, 3, 2]) == (3, 1)                                  # the first maximum
    assert one([0, 0, 0, 0]) == (0, 0)
    m, a = one([-0.0, 0.0, 0.0, -0.0])                                  # zeros tie: the first is kept, sign and all
    assert a == 0 and np.signbit(m)
    m, a = one([0.0, -0.0, 0.0, 0.0])
    assert a == 0 and not np.signbit(m)
    m, a = one([1, nan, 5, inf])                                        # a NaN wins and stays, also against +inf
    assert np.isnan(m) and a == 1
    m, a = one([nan, 2, nan, 7])                                        # of several NaNs the last
    assert np.isnan(m) and a == 2
    assert one([-inf, -inf, -inf, -inf]) == (-inf, 0)
    assert one([-3, -inf, -2, -2]) == (-2, 2)
    assert one([1, 2, 3, 4, 4, 0], 3, 2) == (4, 3)                      # scan order is row-major
    # the backward: to the winner; relu_mask: nothing where the winner is not > 0 (zero, negative, NaN)
    for vals, masked in (([1, 3, 3, 2], False), ([0, 0, 0, 0], True), ([-1, -2, -1, -3], True), ([1, nan, 5, 2], True)):
        x = np.asarray(vals, dtype=np.float32).reshape(1, 2, 2, 1)
        dy = np.full((1, 1, 1, 1), 7.0, dtype=np.float32)
        _, arg = S.pool(x, 2, 2)
        want = np.zeros(4)
        want[int(arg.ravel()[0])] = 7.0
        assert np.array_equal(S.pool_bwd(x, dy, 2, 2, False).ravel(), want)
        assert np.array_equal(S.pool_bwd(x, dy, 2, 2, True).ravel(), np.zeros(4) if masked else want)
    assert S.amax([1.0, -3.0, np.inf, np.nan, -np.inf]) == 3.0 and S.amax([np.nan, np.inf]) == 0.0 and S.amax([]) == 0.0


@pytest.mark.parametrize("window", S.POOL_WINDOWS)
@pytest.mark.parametrize("shape", S.POOL_SHAPES[:2])
def test_pool_statements_match_torch_double(window, shape):
    """On the device's own data with the NaNs taken out and the ties broken (torch's forward agrees on ties; its CPU backward's
    choice among equal maxima is not the statement's business): pooled values, winners through autograd, and the ReLU mask."""
    (kh, kw), (B, H, W, C) = window, shape
    x, dy = S.pool_data(B, H, W, C, kh, kw)
    assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and np.signbit(x[x == 0]).any()
    m, _ = S.pool(x, kh, kw)
    tm = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), (kh, kw)).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(np.isnan(m), np.isnan(tm)) and np.array_equal(m[~np.isnan(m)], tm[~np.isnan(tm)])    # NaN rule is torch's
    xc = np.nan_to_num(x.astype(np.float64), nan=0.5, posinf=9.0, neginf=-9.0)
    xc = xc + np.random.RandomState(1).rand(*xc.shape) * 1e-3                                               # no ties left
    xt = t64(xc).permute(0, 3, 1, 2).requires_grad_()
    F.max_pool2d(xt, (kh, kw)).backward(t64(dy).permute(0, 3, 1, 2))
    assert np.array_equal(S.pool_bwd(xc, dy, kh, kw, False), xt.grad.permute(0, 2, 3, 1).numpy())
    xn = xc - 0.4                                                                                            # some windows all-negative
    xt = t64(xn).permute(0, 3, 1, 2).requires_grad_()
    F.max_pool2d(xt.relu(), (kh, kw)).backward(t64(dy).permute(0, 3, 1, 2))
    got = S.pool_bwd(S.relu(xn), dy, kh, kw, True)
    # torch routes a zero-valued winner's gradient to the ReLU, which stops it: the same zeros
    assert np.array_equal(got, xt.grad.permute(0, 2, 3, 1).numpy()) and (S.pool(S.relu(xn), kh, kw)[0] == 0).any()


# ----------------------------------------------------------------------------- conv -> ReLU -> pool backward
@pytest.mark.parametrize("shape", S.POOL_BWD + S.FWD_POOL)
@pytest.mark.parametrize("scale", S.REAL_SCALES)
def test_conv_pool_bwd_matches_autograd_and_few_windows_are_undecided(shape, scale):
    """autograd through conv2d -> relu -> max_pool2d in double, on the windows the statement calls decided and that hold no tie
    (torch's choice among ties is its own); at most 1 % of the windows of every `real` table entry are undecided: a condition on the
    seeds, which the statement alone decides"""
    B, H, W = shape[:3]
    Co = shape[3] if len(shape) == 4 else 64
    d = S.real_data(B, H, W, Co, scale)
    dpool = S.pool_dpool(B, H, W, Co, "real", scale)
    r = S.conv_pool_bwd(d.x, d.w, d.bias, dpool)
    und = S.undecided(r.pre, r.cond_pre)
    print(f"conv_pool_bwd {shape} x{scale:g}: {int(und.sum())} of {und.size} (window, channel) pairs undecided")
    assert und.mean() <= 0.01
    assert und[..., 1].sum() == 0 and und[..., 2].sum() == 0                      # the planted ties and all-negative windows are decided
    assert (S.pool(S.relu(r.pre), 2, 2)[1][..., 1] == 0).all() and not r.masked[..., 2].any() and r.masked[..., 1].all()
    # torch: break the planted ties by giving channel 1 a filter, and compare the channels that hold no tie
    x = t64(d.x).reshape(B, 1, H, W).requires_grad_()
    w = t64(d.w).reshape(Co, 1, 3, 3).requires_grad_()
    b = t64(d.bias).requires_grad_()
    a = F.conv2d(x, w, b, padding=1).relu()
    p = F.max_pool2d(a, 2)
    win = np.sort(S._windows(S.relu(r.pre), 2, 2), axis=3)
    sel = ~((win[:, :, :, -1] == win[:, :, :, -2]) & (win[:, :, :, -1] > 0))      # windows without a positive tie
    assert sel.mean() > 0.9
    g = dpool * sel
    p.backward(t64(g).permute(0, 3, 1, 2))
    r2 = S.conv_pool_bwd(d.x, d.w, d.bias, g)
    assert close(r2.dw, w.grad.reshape(Co, 9)) and close(r2.db, b.grad) and close(r2.dx, x.grad.reshape(B, H, W))
    assert np.array_equal(r2.masked, np.where((p.detach() > 0).permute(0, 2, 3, 1).numpy(), g, 0.0))


def test_undecided_flags_what_a_rounding_could_flip():
    pre = np.zeros((1, 2, 2, 4))
    cond = np.ones((1, 2, 2, 4))
    g = S.FWD_ROUNDINGS * S.EPS32
    pre[0, :, :, 0] = [[1.0, 1.0 - g], [0.2, 0.1]]                # second within the two gates of the best: undecided
    pre[0, :, :, 1] = [[1.0, 1.0], [0.2, 0.1]]                    # an exact tie: decided
    pre[0, :, :, 2] = [[g / 2, -1.0], [-1.0, -1.0]]               # the winner within its gate of zero: the mask is undecided
    pre[0, :, :, 3] = [[-1.0, -0.5], [-1.0, 1.0 - 3 * g]]         # clear
    assert S.undecided(pre, cond)[0, 0, 0].tolist() == [True, False, True, False]


# ----------------------------------------------------------------------------- head
@pytest.mark.parametrize("C", S.HEAD_C)
@pytest.mark.parametrize("M", S.HEAD_M[:2] + (517,))
def test_head_statements_match_torch_double(C, M):
    for scale in S.REAL_SCALES:
        x, w, b, dyy, _ = S.head_data(M, C, "real", scale)
        xt, wt, bt = t64(x).requires_grad_(), t64(w).requires_grad_(), t64(b).requires_grad_()
        y = torch.sigmoid(xt @ wt + bt)
        y.backward(t64(dyy))
        ys, gate = S.head_fwd(x, w, b)
        assert close(ys, y.detach()) and (gate > 0).all()
        # the backward takes an fp32 y: its own rounding of the statement's
        r = S.head_bwd(x, ys.astype(np.float32), dyy, w)
        tol = 4 * S.EPS32
        assert close(r.dx, xt.grad, tol) and close(r.dw, wt.grad, tol * M) and close(r.db, bt.grad, tol * M)
    x, w, b, dyy, y32 = S.head_data(M, C, "int")
    r = S.head_bwd(x, y32, dyy, w)
    assert np.array_equal(r.db, (dyy / 4).sum()) and np.array_equal(r.dw, (dyy / 4).astype(np.float64) @ x.astype(np.float64))
    assert set(np.unique(r.dx / np.where(w == 0, 1, w)[None, :])) <= {-1.0, 0.0, 1.0}


# ----------------------------------------------------------------------------- the int kind stays below 2^24
def test_int_kind_partial_sums_are_exact_in_fp32():
    tables = S.FWD4 + S.FWD1 + S.FWD_POOL + S.WGRAD + S.DGRAD + (S.FWD4_BIG, S.FWD1_BIG, S.WGRAD_BIG)
    tables += tuple(s + (64,) for s in S.POOL_BWD + (S.POOL_BWD_BIG,))
    worst = 0
    for B, H, W, Co in tables:
        fwd, wg, dg = S.int_bounds(B, H, W, Co)
        assert (wg, dg) == (3 * B * H * W, 9 * Co * 2)
        worst = max(worst, fwd, wg, dg)
    assert worst == 3 * 9 * 32 * 4096 < 2 ** 24
    d = S.int_data(2, 4, 8, 4)
    assert set(np.unique(d.x)) <= {0, 1, 2, 3} and set(np.unique(d.w)) <= {-2, -1, 0, 1, 2} and set(np.unique(d.dy)) <= {-1, 0, 1}
    assert set(np.unique(d.bias)) <= {-2, -1, 0, 1, 2}
    for C in S.HEAD_C:                                                  # head: |dz x| <= 3 per row, |dz w| <= 2
        assert 3 * max(S.HEAD_M) < 2 ** 24
    # the statements on the int kind give integers, so fp64 holds them exactly as well
    B, H, W, Co = S.WGRAD[1]
    d = S.int_data(B, H, W, Co)
    for a in S.conv_fwd(d.x, d.w, d.bias, True)[:1] + S.conv_wgrad(d.x, d.dy)[:2] + S.conv_dgrad(d.dy, d.w)[:1]:
        assert np.array_equal(a, np.round(a))


# ----------------------------------------------------------------------------- the tables reach the branches their comments name
def test_forward_tables_reach_both_kernels_and_their_second_trips():
    def fast(B, H, W, Co):                                              # qea_conv_c1_fwd's choice of the four-pixel kernel
        return W % 4 == 0 and Co in (32, 64, 128)

    assert all(fast(*s) for s in S.FWD4 + (S.FWD4_BIG,)) and not any(fast(*s) for s in S.FWD1 + (S.FWD1_BIG,))
    assert {s[3] for s in S.FWD4} == {32, 64, 128}
    assert [s[2] % 4 for s in S.FWD1] == [1, 1, 0, 0] and [s[3] for s in S.FWD1[2:]] == [48, 4]
    assert S.FWD1[0][:3] == (1, 1, 1) and S.FWD4[0][1] == 1
    B, H, W, Co = S.FWD4_BIG
    assert S.FWD4_PIXELS_PER_TRIP == 524288 and B * H * W == 532480 > S.FWD4_PIXELS_PER_TRIP and Co == 128
    B, H, W, Co = S.FWD1_BIG
    assert S.FWD1_PIXELS_PER_TRIP == 65536 and B * H * W == 66240 > S.FWD1_PIXELS_PER_TRIP and Co == 128 and W % 4
    for B, H, W, Co in S.FWD_POOL:                                      # ops.conv_c1_fwd_pool takes them
        assert H % 2 == 0 and W % 4 == 0 and Co in (32, 64, 128)
    assert {s[3] for s in S.FWD_POOL} == {32, 64, 128}


def test_wgrad_table_reaches_each_geometry_branch():
    geo = {s: S.c1_wgrad_geom(s[0] * s[1] * s[2], s[3]) for s in S.WGRAD + (S.WGRAD_BIG,)}
    assert geo[(1, 1, 1, 32)] == (32, 32, 1)
    rt_n, rpt, blocks = geo[(40, 3, 5, 32)]
    assert rt_n == 32 and 3 * 5 == 15 < rt_n and blocks == 1 and 40 * 15 > rt_n          # a step of rt_n pixels crosses two images
    rt_n, rpt, blocks = geo[(1, 9, 57, 64)]
    assert rt_n * rpt == S.WGRAD_BLOCK_PIXELS == 512 and 9 * 57 == 513 and blocks == 2
    rt_n, rpt, blocks = geo[(3, 4, 8, 48)]
    assert rt_n == 21 and rt_n * (48 // 4) == 252 < 256
    rt_n, rpt, blocks = geo[(1, 16, 200, 128)]
    assert rt_n == 8 and rpt == 32 and blocks == 13 and 16 * 200 % (rt_n * rpt) != 0
    assert geo[S.WGRAD_BIG] == (8, 36, 4096) and 9 * 32 * 4096 == 1179648
    assert all(g[1] == 32 for s, g in geo.items() if s != S.WGRAD_BIG)
    assert S.wgrad_chain(1179648, 128) == 44 and S.wgrad_chain(513, 64) == 48


def test_dgrad_table_reaches_full_and_partial_tiles():
    th, tw = S.DGRAD_TILE
    tiles = [(-(-H // th), -(-W // tw), H % th, W % tw) for _, H, W, _ in S.DGRAD]
    assert tiles == [(1, 1, 1, 1), (1, 1, 0, 0), (2, 2, 1, 1), (1, 1, 7, 63), (3, 3, 1, 2)]
    assert all(Co in (32, 64, 128) for *_, Co in S.DGRAD) and {s[3] for s in S.DGRAD} == {32, 64, 128}


def test_pool_bwd_table_reaches_partial_and_empty_waves_and_long_walks():
    got = []
    for B, H, W in S.POOL_BWD + (S.POOL_BWD_BIG,):
        assert H % 2 == 0 and W % 8 == 0
        NW = B * (H // 2) * (W // 2)
        wpw = S.c1pb_win_per_wave(NW)
        got.append((NW, wpw, -(-NW // (4 * wpw)), NW % 64))
    assert got[0] == (4, 16, 1, 4)                                      # wave 0: 4 of 16; waves 1 .. 3 empty
    assert got[1] == (36, 16, 1, 36)                                    # 16 + 16 + 4, wave 3 empty
    assert got[2] == (80, 16, 2, 16)                                    # the second block: one wave of 16
    assert got[3] == (132096, 20, 1652, 0) and 20 > 16 and (128 // 2) % 20 != 0 and (16 * 64) % 20 != 0
    assert all(n % 64 for n, *_ in got[:3])                             # window counts that are no multiple of 64


def test_head_and_pool_tables():
    assert S.HEAD_M[2] == 65541 and -(-S.HEAD_M[2] * (64 // 4) // 256) == 4097 > 1024 and -(-S.HEAD_M[2] * (32 // 4) // 256) > 1024
    assert S.HEAD_M[1] * (32 // 4) < 2 * 256 and S.HEAD_M[1] % 64 == 63
    for B, H, W, C in S.POOL_SHAPES:
        assert C % 4 == 0 and all(H % kh == 0 and W % kw == 0 for kh, kw in S.POOL_WINDOWS)
    B, H, W, C = S.POOL_SHAPES[2]
    assert B * (H // 2) * (W // 2) * (C // 4) > 256                      # more than one block
