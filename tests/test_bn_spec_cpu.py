"""tests/bn_spec.py held to torch in double precision, to exact rational arithmetic and to its own tables: the statements must be right
before tests/test_bn_kernels_gpu.py holds the kernels to them.  No GPU."""
import fractions

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_spec as S

EPS, MOM = 1e-5, 0.25                                    # a momentum other than the default 0.1
SMALL_RED = S.RED                                        # every real-data shape (RED_BIG and APPLY_BIG carry exact data only)


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def nchw(rows):
    """[M][C] -> [1][C][M][1] float64"""
    return t64(rows).t().reshape(1, rows.shape[1], rows.shape[0], 1)


def close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    assert bool((err <= tol).all()), (what, float((err / np.maximum(tol, 1e-300)).max()))


# ----------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("C,M", SMALL_RED, ids=str)
def test_train_stats_against_torch(C, M):
    """mean, invstd, scale, shift and the running statistics against F.batch_norm(training) in float64 to 1e-12; on the constant and the
    large-mean channel, where torch's two-pass variance and the one-pass statement differ, within the statement's own gates"""
    x = S.real_rows(M, C)
    gamma, beta, rm, rv, _ = S.vectors(C)
    st = S.train_stats(x, gamma, beta, EPS, MOM, rm, rv)
    if M == 1:                                           # torch refuses one value per channel: by hand
        assert np.array_equal(st.var, np.zeros(C)) and np.array_equal(st.unbiased, st.var)
        close(st.running_var, (1 - np.float32(MOM).astype(np.float64)) * rv.astype(np.float64), 1e-15, "running_var M == 1")
        close(st.mean, x[0].astype(np.float64), 0, "mean M == 1")
        return
    trm, trv = t64(rm), t64(rv)
    eps, mom = float(np.float32(EPS)), float(np.float32(MOM))
    out = F.batch_norm(nchw(x), trm, trv, t64(gamma), t64(beta), True, mom, eps).reshape(C, M).t().numpy()
    ref_mean = x.astype(np.float64).mean(0)
    ref_var = x.astype(np.float64).var(0)
    ref_is = 1 / np.sqrt(ref_var + eps)
    # 1e-12 relative + the statement's own fp64 gate: the one-pass variance against torch's two-pass one differs by the conditioning
    # term E[x^2] / var (3.6e5 on the mean-30, spread-0.05 channels, 1e10 on the large-mean channel, unbounded on the constant one)
    r64 = st.g_invstd / st.invstd
    for name, got, ref, gate in (("mean", st.mean, ref_mean, st.g_mean), ("invstd", st.invstd, ref_is, st.g_invstd),
                                 ("running_mean", st.running_mean, trm.numpy(), mom * st.g_mean),
                                 ("running_var", st.running_var, trv.numpy(), mom * st.g_var * M / (M - 1))):
        close(got, ref, 1e-12 * np.abs(ref) + gate, name)
    easy = st.g_var < 1e-12 * st.var                     # the well-conditioned channels: 1e-12 with nothing added
    assert int(easy.sum()) >= C // 2
    close(st.invstd[easy], ref_is[easy], 1e-12 * ref_is[easy], "invstd, well-conditioned channels")
    xs = np.abs(x.astype(np.float64) * st.scale)
    z = x.astype(np.float64) * st.scale + st.shift
    close(z, out, 1e-12 * (xs + np.abs(st.shift)) + (xs + np.abs(st.mean * st.scale)) * r64 + np.abs(st.scale) * st.g_mean, "x scale + shift")
    # the gates' precondition (bn_spec._stats_from_sums): the first-order factor 1.1 holds on every builder
    assert bool((st.g_var <= 0.1 * (st.var + eps)).all())


def test_one_pass_variance_loss_lies_inside_its_bound_and_the_bound_says_something():
    """the large-mean channel (mean 10^3, spread 10^-2): |two-pass - one-pass| <= g_var, and g_var is a small fraction of the variance"""
    for C, M in ((12, 130), (32, 8197)):
        x = S.real_rows(M, C)
        st = S.train_stats(x)
        two = S.two_pass_var(x)
        loss, bound, var = abs(two[S.BIG_CH] - st.var[S.BIG_CH]), st.g_var[S.BIG_CH], two[S.BIG_CH]
        print(f"one-pass variance, mean 1e3 spread 1e-2, M = {M}: var {var:.3e}, observed loss {loss:.2e}, bound {bound:.2e} "
              f"(loss / bound {loss / bound:.3f}, bound / var {bound / var:.2e})")
        assert loss <= bound
        assert bound < 1e-2 * var                        # not vacuous: the bound still pins the variance to 1 %
        assert 0.5e-4 < var < 2e-4
        assert st.var[S.CONST_CH] <= st.g_var[S.CONST_CH] and two[S.CONST_CH] == 0      # the constant channel: clamp or a tiny positive


@pytest.mark.parametrize("bias", (False, True), ids=("no_bias", "conv_bias"))
def test_eval_coeff_against_torch(bias):
    for C in (12, 96, 1024):
        gamma, beta, rm, rv, cb = S.vectors(C)
        x = S.real_rows(9, C)
        ec = S.eval_coeff(gamma, beta, rm, rv, EPS, cb if bias else None)
        xin = x.astype(np.float64) + (cb.astype(np.float64) if bias else 0.0)
        ref = F.batch_norm(nchw(xin), t64(rm), t64(rv), t64(gamma), t64(beta), False, 0.1, float(np.float32(EPS))).reshape(C, 9).t().numpy()
        got = x.astype(np.float64) * ec.scale + ec.shift
        close(got, ref, 1e-12 * (np.abs(x * ec.scale) + np.abs(ec.shift) + 1), "eval x scale + shift")
        assert np.array_equal(ec.mean, rm.astype(np.float64))
    ec = S.eval_coeff(None, None, rm, rv, EPS, None)
    close(ec.scale, ec.invstd, 0, "gamma None")
    close(ec.shift, -rm.astype(np.float64) * ec.invstd, 1e-15, "beta None")


# ----------------------------------------------------------------------------- fma, mask, NaN
def round_f32(fr):
    """a Fraction rounded once, half to even, to the fp32 grid (normal range)"""
    if fr == 0:
        return 0.0
    e = abs(fr.numerator).bit_length() - fr.denominator.bit_length()
    if fractions.Fraction(2) ** e > abs(fr):
        e -= 1
    return float(round(fr / fractions.Fraction(2) ** (e - 23)) * fractions.Fraction(2) ** (e - 23))


def test_fma_and_mask_sign_in_rational_arithmetic():
    """fma32 is the single rounding of the exact y * scale + shift and mask_f64 has the exact value's sign, element by element, on a
    sample of every table's data (exact and real; scale / shift as the device would hold them: float32)"""
    n = 0
    for C, M in S.RED:
        for kind in ("exact", "real"):
            y = (S.exact_rows if kind == "exact" else S.real_rows)(M, C)
            gamma, beta, *_ = S.vectors(C)
            st = S.train_stats(y, gamma, beta, EPS)
            sc, sh = S.f32(st.scale), S.f32(st.shift)
            z, mk = S.fma32(y, sc, sh), S.mask_f64(y, sc, sh)
            rows = np.unique(np.linspace(0, M - 1, 12).astype(int))
            for r in rows:
                for c in range(min(C, 24)):
                    ex = fractions.Fraction(float(y[r, c])) * fractions.Fraction(float(sc[c])) + fractions.Fraction(float(sh[c]))
                    assert float(z[r, c]) == round_f32(ex), (C, M, kind, r, c)
                    assert bool(mk[r, c]) == (ex > 0) == bool(z[r, c] > 0), (C, M, kind, r, c)
                    n += 1
    assert n > 1500
    # the case a cast of the fp64 sum gets wrong: (2^-12 + 2^-30)(2^-12 - 2^-30) + (1 + 2^-23) = 1 + 2^-23 + 2^-24 - 2^-60 exactly, just
    # BELOW the midpoint of 1 + 2^-23 and 1 + 2^-22; the fp64 sum is the midpoint itself and its cast ties to the even 1 + 2^-22
    y = np.array([[2.0 ** -12 + 2.0 ** -30]], dtype=np.float32)
    sc, sh = np.array([2.0 ** -12 - 2.0 ** -30], dtype=np.float32), np.array([1 + 2.0 ** -23], dtype=np.float32)
    ex = fractions.Fraction(float(y[0, 0])) * fractions.Fraction(float(sc[0])) + fractions.Fraction(float(sh[0]))
    assert ex == 1 + fractions.Fraction(2) ** -23 + fractions.Fraction(2) ** -24 - fractions.Fraction(2) ** -60
    naive = np.float32(np.float64(y[0, 0]) * np.float64(sc[0]) + np.float64(sh[0]))
    assert float(naive) == 1 + 2.0 ** -22 and round_f32(ex) == 1 + 2.0 ** -23 == float(S.fma32(y, sc, sh)[0, 0])
    assert bool(S.mask_f64(y, sc, sh)[0, 0])


def test_nan_rules_ties_and_all_zero_windows():
    nan = np.float32("nan")
    y = np.array([[1, -1, nan, 2], [3, -1, 0.5, 2], [-2, -1, 0.25, 2], [3, -1, nan, -5]], dtype=np.float32)          # one 2x2 window, C = 4
    one, zero = np.ones(4, dtype=np.float32), np.zeros(4, dtype=np.float32)
    a1 = S.bn_apply(y, one, zero, True)
    a0 = S.bn_apply(y, one, zero, False)
    assert not np.isnan(a1).any() and a1[0, 2] == 0 and a1[3, 2] == 0          # fmaxf: NaN -> 0 under the ReLU
    assert np.isnan(a0[0, 2]) and np.isnan(a0[3, 2]) and int(np.isnan(a0).sum()) == 2
    _, p1, arg1 = S.bn_apply_pool(y, one, zero, True, 1, 2, 2, 2, 2)
    _, p0, arg0 = S.bn_apply_pool(y, one, zero, False, 1, 2, 2, 2, 2)
    assert list(p1[0]) == [3, 0, 0.5, 2] and list(arg1.ravel()) == [1, 0, 1, 0]   # first maximum wins (3 at 1 and 3; all-zero window: 0)
    assert np.isnan(p0[0, 2]) and int(arg0.ravel()[2]) == 3                   # without the ReLU the NaN wins the pool (the last one)
    assert list(p0[0, [0, 1, 3]]) == [3, -1, 2] and list(arg0.ravel()[[0, 1, 3]]) == [1, 0, 0]
    dz = S.masked_dz(None, y, ("remask", one, zero), (np.full((1, 4), 7, dtype=np.float32), 1, 2, 2, 2))
    assert dz[1, 0] == 7 and dz[3, 0] == 0 and not dz[:, 1].any() and dz[1, 2] == 7 and dz[0, 3] == 7


# ----------------------------------------------------------------------------- backward
def autograd_bn(y, gamma, beta, da, training, relu, rm=None, rv=None):
    C, M = y.shape[1], y.shape[0]
    yt, gt, bt = nchw(y).requires_grad_(), t64(gamma).requires_grad_(), t64(beta).requires_grad_()
    out = F.batch_norm(yt, None if training else t64(rm), None if training else t64(rv), gt, bt, training, 0.1, float(np.float32(EPS)))
    out = F.relu(out) if relu else out
    out.backward(nchw(da))
    return out.detach().reshape(C, M).t().numpy(), yt.grad.reshape(C, M).t().numpy(), gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("training", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("C,M", [s for s in SMALL_RED if s[1] > 1], ids=str)
def test_backward_against_autograd(C, M, training):
    """relu(batch_norm) and batch_norm alone, training and eval: dy, dgamma, dbeta to 1e-12 x (1 + |mean| invstd), the condition number
    of xhat = (y - mean) invstd, which the statement evaluates as the kernel does.  The three ways to the mask agree."""
    y, da = S.real_rows(M, C), S.exact_rows(M, C, 5)
    gamma, beta, rm, rv, _ = S.vectors(C)
    yd = y.astype(np.float64)
    if training:
        mu, var = yd.mean(0), yd.var(0)
    else:
        mu, var = rm.astype(np.float64), rv.astype(np.float64)
    inv = 1 / np.sqrt(var + float(np.float32(EPS)))
    sc, sh = S.f32(gamma * inv), S.f32(beta - mu * gamma * inv)
    condn = 1 + np.abs(mu) * inv
    for relu in (True, False):
        a_ref, dy_ref, dg_ref, db_ref = autograd_bn(y, gamma, beta, da, training, relu, rm, rv)
        if relu:
            a = S.bn_apply(y, sc, sh, True)
            dz = S.masked_dz(da, y, ("remask", sc, sh))
            assert np.array_equal(dz, S.masked_dz(da, y, ("a", a)))
            decided = np.abs(a_ref) > 1e-5 * (np.abs(yd * sc) + np.abs(sh))              # fp32 scale / shift against torch's fp64 ones
            assert np.array_equal((a > 0)[decided], (a_ref > 0)[decided])
            if not np.array_equal(a > 0, a_ref > 0):
                dz = np.where(a_ref > 0, da, np.float32(0))                              # compare the formula on torch's own mask
        else:
            dz = S.masked_dz(da, y, None)
        b = S.bn_bwd(dz, y, gamma, mu, inv, training)
        top = np.abs(dy_ref).max(0) + 1e-30
        close(b.dy, dy_ref, 1e-12 * condn * top * 8, "dy")
        close(b.dgamma, dg_ref, 1e-12 * condn * (np.abs(dg_ref) + np.abs(f64sum(dz)) + 1), "dgamma")
        close(b.dbeta, db_ref, 1e-12 * (np.abs(db_ref) + 1), "dbeta")
        # the gate is one fp32 rounding of dy and an fp64-sized part: (depth + 8) u64 < 1e-13 times the terms, which are <= condn x top
        assert bool((b.g_dy >= S.EPS32 * np.abs(b.dy)).all())
        assert bool((b.g_dy <= 1.01 * S.EPS32 * np.abs(b.dy) + 1e-11 * condn * top).all())


def f64sum(a):
    return np.abs(np.asarray(a, dtype=np.float64)).sum(0)


@pytest.mark.parametrize("case", S.POOL + (S.POOL_BWD_RAGGED,), ids=str)
def test_pool_fused_backward_is_pool_backward_plus_skip_then_batchnorm_backward(case):
    """masked_dz(pool) = autograd of max_pool2d at the stored activation + the skip gradient, masked by a > 0; with and without da"""
    B, H, W, C, kh, kw = case
    M = B * H * W
    y = S.pool_rows(B, H, W, C, kw, "real")
    gamma, beta = S.exact_vectors(C)
    m32, i32, st = S.forced_stats(C)
    sc, sh = S.f32(gamma * i32), S.f32(beta - m32 * gamma * i32)
    a = S.bn_apply(y, sc, sh, True)
    dpool, dskip = S.exact_rows(M // (2 * kw), C, 1), S.exact_rows(M, C, 2)
    at = t64(a).reshape(B, H, W, C).permute(0, 3, 1, 2).requires_grad_()
    F.max_pool2d(at, (2, kw)).backward(t64(dpool).reshape(B, H // 2, W // kw, C).permute(0, 3, 1, 2))
    routed = at.grad.permute(0, 2, 3, 1).reshape(M, C).numpy()
    for da in (dskip, None):
        ref = np.where(a > 0, routed + (0 if da is None else da.astype(np.float64)), 0)
        got = S.masked_dz(da, y, ("remask", sc, sh), (dpool, B, H, W, kw))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref)
        plain = S.bn_bwd(np.where(a > 0, S.f32(ref), np.float32(0)), y, gamma, st[0], st[1], True)
        fused = S.bn_bwd(got, y, gamma, st[0], st[1], True)
        assert np.array_equal(plain.dy, fused.dy) and np.array_equal(plain.dgamma, fused.dgamma)


@pytest.mark.parametrize("blocks", S.PART_BLOCKS)
def test_from_partials_form_is_the_plain_form(blocks):
    for C in S.PART_C:
        M = S.PART_M
        y, da = S.exact_rows(M, C), S.exact_rows(M, C, 5)
        gamma, beta = S.exact_vectors(C)
        m32, i32, st = S.forced_stats(C)
        dz = S.masked_dz(da, y, ("remask", S.f32(gamma * i32), S.f32(beta - m32 * gamma * i32)))
        P = S.partial_rows(dz, y, st[0], st[1], blocks)
        plain, part = S.bn_bwd(dz, y, gamma, st[0], st[1], True), S.bn_bwd(dz, y, gamma, st[0], st[1], True, partials=P)
        for f in ("s", "q", "dy", "dgamma_f32", "dbeta_f32"):
            assert np.array_equal(getattr(plain, f), getattr(part, f)), f          # exact data: bit for bit
        yr = S.real_rows(M, C)
        dzr = S.masked_dz(da, yr, None)
        stt = S.train_stats(yr)
        Pr = S.partial_rows(dzr, yr, stt.mean, stt.invstd, blocks)
        plain, part = S.bn_bwd(dzr, yr, gamma, stt.mean, stt.invstd, True), S.bn_bwd(dzr, yr, gamma, stt.mean, stt.invstd, True, partials=Pr)
        close(part.s, plain.s, plain.g_dbeta, "s")
        close(part.q, plain.q, plain.g_dgamma, "q")
        close(part.dy, plain.dy, plain.g_dy, "dy")


def test_column_and_layout_statements():
    x = S.real_rows(130, 12)
    v, v32, gate = S.colsum(x)
    close(v, x.astype(np.float64).sum(0), 1e-12 * np.abs(x).sum(0), "colsum")
    old = S.vectors(12)[1]
    va, va32, gate_a = S.colsum(x, old)
    close(va, v + old, 1e-15 * (np.abs(v) + 1), "colsum accumulate")
    assert bool((gate_a > gate).all()) and va32.dtype == np.float32
    t = np.array([[0, -3, np.inf, np.nan], [1, 2, -np.inf, 2.5]], dtype=np.float32)
    assert S.absmax(t) == 3 and S.absmax(t[:, 2:3]) == 0 and S.absmax(np.zeros((2, 4))) == 0
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert S.transpose2d(a).tolist() == [[0, 3], [1, 4], [2, 5]]
    for Co, Ci, KH, KW in S.FLIP:
        w = np.arange(Co * KH * KW * Ci, dtype=np.float32).reshape(Co, KH, KW, Ci)
        wt = S.filter_flip_transpose(w)
        ref = torch.from_numpy(w).flip(1, 2).permute(3, 1, 2, 0).contiguous().numpy()
        assert wt.shape == (Ci, KH, KW, Co) and np.array_equal(wt, ref)
        assert Co % 4 and Ci % 4 or Co % 32 and Ci % 32


# ----------------------------------------------------------------------------- launch arithmetic: every table entry reaches its branch
def test_reduction_table_reaches_its_branches():
    g = {s: S.col_geom(s[1], s[0]) for s in S.RED + (S.RED_BIG,)}
    a = g[(12, 130)]
    assert (a.cols, a.rt, a.grid) == (3, 85, 1) and a.cols * a.rt == 255                 # thread 255 is idle
    assert g[(64, 5)].rt == 16 and 5 < 16 and g[(64, 5)].grid == 1
    assert g[(1024, 7)].rt == 1 and g[(1024, 7)].grid == 1
    assert (g[(1024, 33)].grid, g[(1024, 33)].rows_per_block) == (3, 11)
    b = g[(32, 8197)]
    assert (b.rt, b.grid, b.rows_per_block) == (32, 17, 483) and 8197 - 16 * 483 == 469  # ragged last block
    ag = S.apply_geom(8197, b.rt, 8)
    assert (ag.grid, ag.per_block) == (33, 249) and 8197 - 32 * 249 == 229
    for rows in (249, 229):                                                               # odd and even row counts per thread
        n = S.rows_per_thread(249, 32, rows)
        assert {k % 2 for k in n} == {0, 1}
    assert g[(96, 1)].grid == 1
    c = g[S.RED_BIG]
    assert c.want == 1025 and c.want > 1024 and c.rows_per_block == 17 and c.grid == 965  # the cap holds: 17 rows per thread, not 16
    assert S.apply_geom(S.RED_BIG[1], 1, 8).want == 2050 < 4096                           # apply_geom's cap is NOT reached (stated)
    assert S.colreduce_ws_bytes(S.RED_BIG[1], S.RED_BIG[0]) == (965 * 2 + 3) * 1024 * 8
    for C, M in S.RED + (S.RED_BIG, S.APPLY_BIG):
        assert S.exact_units(M) < 2 ** 53 and C % 4 == 0 and C <= 1024


def test_elementwise_tables_reach_their_branches():
    for C, M in S.RED + (S.RED_BIG,):
        assert S.grid_for(M * (C // 4))[1] == (1 if (C, M) != S.RED_BIG else 5)
    C, M = S.APPLY_BIG
    assert M * C // 4 > 4096 * 256 and S.grid_for(M * (C // 4)) == (4096, 2)
    B, H, W, C, kh, kw = S.POOL_APPLY_BIG
    n = B * (H // kh) * (W // kw) * (C // 4)
    assert n > 4096 * 256 and S.grid_for(n) == (4096, 2)
    for B, H, W, C, kh, kw in S.POOL:
        assert S.grid_for(B * (H // kh) * (W // kw) * (C // 4))[1] == 1
        gm, grid, wpb, ag = S.bwd_pool_geom(B, H, W, C, kw)
        assert 1 <= grid <= gm.grid
    assert {(H, W, C, kw) for _, H, W, C, _, kw in S.POOL} == {(H, W, C, kw) for H in (2, 8) for W in (4, 16) for C in (12, 64, 1024) for kw in (1, 2)}
    B, H, W, C, kh, kw = S.POOL_BWD_RAGGED
    gm, grid, wpb, ag = S.bwd_pool_geom(B, H, W, C, kw)
    nwin = B * H * W // (2 * kw)
    assert (grid, wpb) == (9, 115) and nwin - 8 * 115 == 112 and grid <= gm.grid          # several blocks, ragged last
    assert ag.grid == 9 and nwin - 8 * ag.per_block == 112


def test_partials_and_absmax_tables_reach_their_branches():
    assert [S.fold(b)[0] for b in S.PART_BLOCKS] == [False, False, False, True, True]
    assert 512 == 2 * S.SCRATCH_ROWS and S.fold(513) == (True, 171, 3) and S.fold(700) == (True, 234, 3)
    assert 700 - 233 * 3 == 1                                                             # a ragged last range
    assert 384 - 256 == 128 and 12 < 256 and 1024 % 256 == 0                              # partials_reduce_kernel's column passes
    for M, C, ld in S.ABSMAX:
        assert S.absmax_grid(M, C) == (1, 0) and ld >= C and ld % 4 == 0
    M, C, ld = S.ABSMAX_BIG
    grid, want = S.absmax_grid(M, C)
    assert grid == 2048 and want == 2050 and M * C * 4 < 70e6
    assert (7, 2048) in S.TRANSPOSE and (33, 31) in S.TRANSPOSE


# ----------------------------------------------------------------------------- abs-max builders
@pytest.mark.parametrize("C,M", S.RED, ids=str)
def test_absmax_positions_hold_the_unique_maximum(C, M):
    """each planted input puts the statement's single largest finite magnitude where it is meant to be, for the apply and for the
    backward form (eval mode: dy = k0 dz, so the plant is the maximum whatever the sums are)"""
    g = S.col_geom(M, C)
    ag = S.apply_geom(M, g.rt, 8)
    pos = S.amax_rows(C, M, ag.per_block, g.rt)
    assert pos["first"] == (0, 0) and pos["last"] == (M - 1, C - 1)
    if (C, M) == (32, 8197):
        r, c = pos["odd_tail"]
        rt, k = (r % ag.per_block) % g.rt, (r % ag.per_block) // g.rt
        assert S.rows_per_thread(ag.per_block, g.rt)[rt] % 2 == 1 and k == S.rows_per_thread(ag.per_block, g.rt)[rt] - 1
        assert pos["last_row_first_col"][0] == M - 1 and (M - 1) // ag.per_block == ag.grid - 1
    gamma, beta = S.exact_vectors(C)
    m32, i32, st = S.forced_stats(C)
    sc, sh = S.f32(gamma * i32), S.f32(beta - m32 * gamma * i32)
    y, da = S.exact_rows(M, C), S.exact_rows(M, C, 5)
    for name, where in pos.items():
        for sign in (1.0, -1.0):
            out = S.bn_apply(S.plant(y, where, (sign * 4096 - sh[where[1]]) / sc[where[1]]), sc, sh, False)
            assert S.unique_finite_max_at(out) == where and np.sign(out[where]) == sign, (name, sign)
            b = S.bn_bwd(S.plant(da, where, sign * 4096), y, gamma, st[0], st[1], False)
            assert S.unique_finite_max_at(b.dy) == where, (name, sign)
        out = S.bn_apply(S.plant(S.plant(y, where, 4096.0), (0, C - 1) if where != (0, C - 1) else (0, 0), np.inf), sc, sh, False)
        assert np.isinf(out).sum() == 1 and S.amax(out) < np.inf


@pytest.mark.parametrize("case", S.AMAX_POOL, ids=str)
def test_absmax_positions_of_the_pool_cases_hold_the_unique_maximum(case):
    """the planted activation is the statement's unique largest activation and pooled value, and the gradient planted on its window
    comes back as the unique largest dy at the same element (eval mode), with either sign"""
    B, H, W, C, kh, kw = case
    M = B * H * W
    gamma, beta = S.exact_vectors(C)
    m32, i32, st = S.forced_stats(C)
    sc, sh = S.f32(gamma * i32), S.f32(beta - m32 * gamma * i32)
    y, dpool = S.pool_rows(B, H, W, C, kw, "exact"), S.exact_rows(M // (2 * kw), C, 31)
    pos = S.amax_pool_rows(B, H, W, C, kw)
    assert pos["last"] == (M - 1, C - 1) and pos["last_window_first"][0] == (B * H - 2) * W + W - kw
    for name, where in pos.items():
        c = where[1]
        yy = S.plant(y, where, (4096 - sh[c]) / sc[c])
        a, p, arg = S.bn_apply_pool(yy, sc, sh, True, B, H, W, kh, kw)
        win = S.unique_finite_max_at(p)
        assert S.unique_finite_max_at(a) == where and win is not None and win[1] == c, name
        assert (win[0] == len(p) - 1) == (name != "first")
        for sign in (1.0, -1.0):
            dz = S.masked_dz(None, yy, ("remask", sc, sh), (S.plant(dpool, win, sign * 4096), B, H, W, kw))
            assert S.unique_finite_max_at(S.bn_bwd(dz, yy, gamma, st[0], st[1], False).dy) == where, (name, sign)
