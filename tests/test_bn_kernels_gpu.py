"""The BatchNorm, pool-fused and column kernels of csrc/norm_pool.hip, qea_absmax and qea_filter_flip_transpose against the fp64
statements of tests/bn_spec.py, at the shapes where their launch arithmetic changes (the tables of bn_spec, proved in
tests/test_bn_spec_cpu.py).  Two kinds of data per shape: `exact` (multiples of 2^-6, forced mean 0.5 / invstd 2 in the backward), on
which every fp32 cast of an exact sum must match the statement bit for bit, and `real`, gated per element by the bound derived next
to each statement ("BatchNorm, pool-fused and column kernels").  bn_apply / bn_apply_pool are held to the bit on both.

Every output lies in a sentinel-filled allocation wider and longer than the tensor; after each launch everything outside the
statement's columns must still hold the sentinel: pad columns, rows beyond M, the abs-max slot's neighbours, the workspace beyond
qea_colreduce_workspace_bytes.  Strided inputs carry NaN in their pad columns.  An abs-max slot must equal, to the bit, the largest
finite |v| of what the launch stored, read back from its output, and those stored values must pass the statement's gate.

QEA_BN_RATIOS=1 (with -s) prints the worst observed / gate ratio per kernel, the figures of DESIGN.md's table."""
import itertools
import os

import numpy as np
import pytest
import torch

import bn_spec as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.0
NAN = float("nan")
EPS, MOM = 1e-5, 0.25
WORST = {}
KINDS = ("exact", "real")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def sid(s):
    return "x".join(str(v) for v in s)


class Out:
    """a [rows][C] output as columns off .. off + C of a sentinel-filled [rows + 3][ld] allocation"""

    def __init__(self, rows, C, ld, off, dtype=torch.float32):
        self.buf = torch.full((rows + 3, ld), SENTINEL, device=DEV, dtype=dtype)
        self.rows, self.C, self.ld, self.off = rows, C, ld, off
        self.view = self.buf[:rows, off:off + C]

    def untouched(self):
        b = self.buf
        rest = torch.cat([b[:self.rows, :self.off].reshape(-1), b[:self.rows, self.off + self.C:].reshape(-1), b[self.rows:].reshape(-1)])
        return bool((rest == SENTINEL).all())

    def get(self):
        return host(self.view)


class Vec(Out):
    """a per-channel output vector between sentinels (8 elements before: the float4 loads of scale / shift stay 16-byte aligned)"""

    def __init__(self, C, init=None, dtype=torch.float32):
        self.buf = torch.full((C + 16,), SENTINEL, device=DEV, dtype=dtype)
        self.C = C
        self.view = self.buf[8:8 + C]
        if init is not None:
            self.view.copy_(dev(np.asarray(init)).to(dtype))

    def untouched(self):
        return bool((torch.cat([self.buf[:8], self.buf[8 + self.C:]]) == SENTINEL).all())


class Slot:
    """an abs-max slot with sentinel neighbours"""

    def __init__(self, init=0.0):
        self.buf = torch.full((8,), SENTINEL, device=DEV)
        self.buf[3] = init
        self.view = self.buf[3:4]

    def value(self):
        b = host(self.buf)
        assert np.array_equal(np.delete(b, 3), np.full(7, SENTINEL, dtype=np.float32)), "the abs-max slot's neighbours were written"
        return b[3]


def inp(a, ld, off):
    """a [rows][C] input as columns off .. off + C of a NaN-filled [rows][ld] buffer: a read of a pad column would show"""
    a = np.asarray(a, dtype=np.float32)
    buf = torch.full((a.shape[0], ld), NAN, device=DEV)
    buf[:, off:off + a.shape[1]] = dev(a)
    return buf[:, off:off + a.shape[1]]


class Workspace:
    """the column kernels' workspace as qea.ops hands it out, with a pattern behind the bytes the entry point may write"""

    def __init__(self, M, C):
        from qea import _lib, ops
        self.need = _lib.lib().qea_colreduce_workspace_bytes(M, C)
        assert self.need == S.colreduce_ws_bytes(M, C)
        self.ws = ops.workspace(self.need + 4096, torch.device("cuda", torch.cuda.current_device()))
        self.ws[self.need:].fill_(0xA5)

    def untouched(self):
        return bool((self.ws[self.need:] == 0xA5).all())


def same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.asarray(got).dtype)
    return np.array_equal(got, ref, equal_nan=True)


def within(kernel, tag, got, ref, gate):
    """every element within its gate, NaN patterns equal; keeps the worst observed / gate ratio per kernel"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64).reshape(got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{kernel} {tag}: NaN pattern"
    r = S.gate_ratio(got, ref, np.broadcast_to(np.asarray(gate, dtype=np.float64), got.shape))
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    if os.environ.get("QEA_BN_RATIOS"):
        print(f"[bn-ratio] {kernel} {tag}: {r:.4f} (worst so far {WORST[kernel]:.4f})")
    assert r <= 1, f"{kernel} {tag}: worst observed / gate = {r:.3f}"
    return r


def slot_holds_amax_of(slot, stored, tag):
    got, want = slot.value(), np.float32(S.amax(stored))
    assert got == want, f"{tag}: abs-max slot {got!r}, the launch stored {want!r}"


def rows_of(kind, M, C, *key):
    return (S.exact_rows if kind == "exact" else S.real_rows)(M, C, *key)


# ----------------------------------------------------------------------------- statistics
def run_train_stats(y, C, M, ld, off, full, kind):
    from qea import ops
    gamma, beta, rm, rv, _ = S.vectors(C)
    yd = inp(y, ld, off)
    outs = {k: Vec(C) for k in ("mean", "invstd", "scale", "shift")}
    st64 = Vec(2 * C, dtype=torch.float64) if full else None
    rmo, rvo = (Vec(C, rm), Vec(C, rv)) if full else (None, None)
    mom = MOM if full else 0.1
    w = Workspace(M, C)
    ops.bn_train_stats(yd, ld, M, C, dev(gamma) if full else None, dev(beta) if full else None, EPS, mom, rmo.view if full else None,
                       rvo.view if full else None, outs["mean"].view, outs["invstd"].view, outs["scale"].view, outs["shift"].view,
                       st64.view if full else None)
    torch.cuda.synchronize()
    assert w.untouched() and all(v.untouched() for v in outs.values())
    st = S.train_stats(y, gamma if full else None, beta if full else None, EPS, mom, rm if full else None, rv if full else None)
    tag = f"C={C} M={M} ld={ld} {kind} {'full' if full else 'bare'}"
    for k, field in (("mean", "mean_out"), ("invstd", "invstd_out"), ("scale", "scale"), ("shift", "shift")):
        within("bn_train_stats", f"{tag} {k}", outs[k].get(), getattr(st, field), getattr(st, "g_" + field))
    if kind == "exact":                                    # s is exact, s / M rounds once in fp64, the cast once more: the bits
        assert same_bits(outs["mean"].get(), st.mean.astype(np.float32)), tag
    if full:
        assert st64.untouched() and rmo.untouched() and rvo.untouched()
        s64 = st64.get()
        within("bn_train_stats", f"{tag} stat64 mean", s64[:C], st.mean, st.g_mean)
        within("bn_train_stats", f"{tag} stat64 invstd", s64[C:], st.invstd, st.g_invstd)
        within("bn_train_stats", f"{tag} running_mean", rmo.get(), st.running_mean, st.g_running_mean)
        within("bn_train_stats", f"{tag} running_var", rvo.get(), st.running_var, st.g_running_var)
        if kind == "exact":
            assert same_bits(s64[:C], st.mean), tag
    return outs, st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,M", S.RED, ids=str)
def test_bn_train_stats(C, M, kind):
    """every stride, with everything optional given (momentum 0.25, stat64) and with gamma, beta, running statistics and stat64 NULL;
    real data carries the constant channel (the var < 0 clamp) and the mean-10^3 channel (the one-pass variance's conditioning)"""
    y = rows_of(kind, M, C)
    for (ld, off), full in itertools.product(S.strides(C), (True, False)):
        run_train_stats(y, C, M, ld, off, full, kind)


def test_bn_train_stats_M_eq_1_keeps_the_biased_variance():
    """M == 1: var = 0, invstd = eps^-1/2 and running_var moves towards var itself, not var M / (M - 1) = 0 / 0"""
    C, M = 96, 1
    outs, st = run_train_stats(S.real_rows(M, C), C, M, C, 0, True, "real")
    assert np.array_equal(st.var, np.zeros(C)) and not np.isnan(outs["invstd"].get()).any()


def test_bn_train_stats_and_colsum_at_the_1024_block_cap():
    """(1024, 16400): col_geom wants 1025 blocks and gets 965 of 17 rows.  Exact data: mean and the column sums to the bit."""
    from qea import ops
    C, M = S.RED_BIG
    y = S.exact_rows(M, C)
    yd = dev(y)
    outs = {k: Vec(C) for k in ("mean", "invstd", "scale", "shift")}
    w = Workspace(M, C)
    ops.bn_train_stats(yd, C, M, C, None, None, EPS, 0.1, None, None, outs["mean"].view, outs["invstd"].view, outs["scale"].view,
                       outs["shift"].view, None)
    cs = Vec(C, np.ones(C, dtype=np.float32))
    ops.colsum(yd, C, M, C, cs.view, accumulate=True)
    torch.cuda.synchronize()
    assert w.untouched() and cs.untouched() and all(v.untouched() for v in outs.values())
    yy = y.astype(np.float64)
    s, q = yy.sum(0), (yy * yy).sum(0)
    st = S._stats_from_sums(s, q, np.abs(yy).sum(0), M, None, None, EPS, 0.1, None, None, S.sum_depth(M))
    assert same_bits(outs["mean"].get(), st.mean.astype(np.float32))
    assert same_bits(cs.get(), np.float32(1) + s.astype(np.float32))
    for k in ("invstd", "scale", "shift"):
        within("bn_train_stats", f"cap {k}", outs[k].get(), getattr(st, k), getattr(st, "g_" + k if k != "invstd" else "g_invstd_out"))


@pytest.mark.parametrize("bias", (False, True), ids=("no_bias", "conv_bias"))
def test_bn_eval_coeff_conv_bias(bias):
    from qea import ops
    for C, bare in ((12, False), (96, True), (1024, False)):
        gamma, beta, rm, rv, cb = S.vectors(C)
        outs = {k: Vec(C) for k in ("mean", "invstd", "scale", "shift")}
        ops.bn_eval_coeff(C, None if bare else dev(gamma), None if bare else dev(beta), dev(rm), dev(rv), EPS, dev(cb) if bias else None,
                          outs["mean"].view, outs["invstd"].view, outs["scale"].view, outs["shift"].view)
        torch.cuda.synchronize()
        assert all(v.untouched() for v in outs.values())
        ec = S.eval_coeff(None if bare else gamma, None if bare else beta, rm, rv, EPS, cb if bias else None)
        assert same_bits(outs["mean"].get(), rm)
        for k in ("invstd", "scale", "shift"):
            within("bn_eval_coeff", f"C={C} bias={bias} {k}", outs[k].get(), getattr(ec, k), getattr(ec, "g_" + k))
        if bias:                                             # the bias moves the shift by far more than the gate: ignoring it cannot pass
            no = S.eval_coeff(None if bare else gamma, None if bare else beta, rm, rv, EPS, None)
            assert float(np.abs(no.shift - ec.shift).max()) > 1e3 * float(ec.g_shift.max())


# ----------------------------------------------------------------------------- apply (+ pool)
def coeffs(kind, y, C):
    """float32 scale / shift (+ the mean / invstd behind them, fp64) for a case: forced statistics on exact data, the statement's on real"""
    if kind == "exact":
        gamma, beta = S.exact_vectors(C)
        m32, i32, st = S.forced_stats(C)
        return gamma, S.f32(gamma * i32), S.f32(beta - m32 * gamma * i32), st[0], st[1]
    gamma, beta, *_ = S.vectors(C)
    st = S.train_stats(y, gamma, beta, EPS)
    return gamma, S.f32(st.scale), S.f32(st.shift), st.mean, st.invstd


def run_apply(y, sc, sh, relu, ld_in, ld_out, slot_init=0.0, rows=None):
    """-> (stored a, slot); rows = (r0, r1): the launch covers that row range only (one slot shared by two launches)"""
    from qea import ops
    M, C = y.shape
    yd = inp(y, *ld_in)
    out = Out(M, C, *ld_out)
    slot = slot_init if isinstance(slot_init, Slot) else Slot(slot_init)
    r0, r1 = rows or (0, M)
    ops.bn_apply(yd[r0:r1], ld_in[0], out.view[r0:r1], ld_out[0], r1 - r0, C, dev(sc), dev(sh), relu=relu, amax=slot.view)
    torch.cuda.synchronize()
    if rows is None:
        assert out.untouched(), "bn_apply wrote outside its columns"
    return out, slot


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,M", S.RED, ids=str)
def test_bn_apply_relu_true_and_relu_false_with_a_nan(C, M, kind):
    """relu=True: fmaxf, a NaN becomes 0; relu=False: the NaN survives (one in channel 3, an inf in channel 3 too) and neither counts
    for the abs-max.  To the bit on both kinds of data: the statement is the single rounding of the exact y scale + shift."""
    y = rows_of(kind, M, C)
    y[0, 3] = np.inf
    y[M // 2, 3] = NAN                                     # (M == 1: the NaN alone)
    _, sc, sh, _, _ = coeffs(kind, rows_of(kind, M, C), C)
    lds = S.strides(C)
    for relu, (li, lo) in itertools.product((True, False), zip(lds, lds[1:] + lds[:1])):
        out, slot = run_apply(y, sc, sh, relu, li, lo)
        ref = S.bn_apply(y, sc, sh, relu)
        assert int(np.isnan(ref).sum()) == (0 if relu else 1) and (relu or int(np.isinf(ref).sum()) == (M > 1))
        assert same_bits(out.get(), ref), (C, M, kind, relu, li, lo)
        slot_holds_amax_of(slot, out.get(), f"bn_apply {C} {M} relu={relu}")


def test_bn_apply_second_grid_stride_trip():
    """(32, 131080): 64 float4 more than 4096 blocks x 256 threads cover in one trip"""
    C, M = S.APPLY_BIG
    y = S.real_rows(M, C)
    _, sc, sh, _, _ = coeffs("real", y[:4096], C)
    y[M - 1, C - 1] = -3e4                                   # the largest magnitude in the second trip's last element
    out, slot = run_apply(y, sc, sh, False, (C, 0), (C, 0))
    assert same_bits(out.get(), S.bn_apply(y, sc, sh, False))
    slot_holds_amax_of(slot, out.get(), "bn_apply second trip")
    assert S.unique_finite_max_at(out.get()) == (M - 1, C - 1)


def run_apply_pool(y, sc, sh, relu, case, ld_in, ld_a, ld_p):
    from qea import ops
    B, H, W, C, kh, kw = case
    M, MP = B * H * W, B * (H // kh) * (W // kw)
    yd = inp(y, *ld_in)
    a, p, sa, sp = Out(M, C, *ld_a), Out(MP, C, *ld_p), Slot(), Slot()
    ops.bn_apply_pool(yd, ld_in[0], a.view, ld_a[0], p.view, ld_p[0], B, H, W, C, dev(sc), dev(sh), kh, kw, relu=relu, amax=sa.view,
                      pooled_amax=sp.view)
    torch.cuda.synchronize()
    assert a.untouched() and p.untouched(), "bn_apply_pool wrote outside its columns"
    return a, p, sa, sp


def check_apply_pool(y, sc, sh, relu, case, lds, unfused=True):
    from qea import ops
    B, H, W, C, kh, kw = case
    a, p, sa, sp = run_apply_pool(y, sc, sh, relu, case, *lds)
    ra, rp, _ = S.bn_apply_pool(y, sc, sh, relu, B, H, W, kh, kw)
    tag = f"bn_apply_pool {case} relu={relu} {lds}"
    assert same_bits(a.get(), ra) and same_bits(p.get(), rp), tag
    slot_holds_amax_of(sa, a.get(), tag + " activation")
    slot_holds_amax_of(sp, p.get(), tag + " pooled")
    if unfused:                                              # norm_pool.hip: "both outputs are bit-identical to the two separate passes"
        a2, s2 = run_apply(y, sc, sh, relu, lds[0], lds[1])
        p2, sp2 = Out(p.rows, C, *lds[2]), Slot()
        ops.maxpool_fwd(a2.view, lds[1][0], p2.view, lds[2][0], B, H, W, C, kh, kw, amax=sp2.view)
        torch.cuda.synchronize()
        assert same_bits(a.get(), a2.get()) and same_bits(p.get(), p2.get()) and p2.untouched(), tag
        assert sa.value() == s2.value() and sp.value() == sp2.value(), tag
    return a, p


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", S.POOL, ids=sid)
def test_bn_apply_pool_relu_and_no_relu_where_a_nan_wins_the_pool(case, kind):
    B, H, W, C, kh, kw = case
    y = S.pool_rows(B, H, W, C, kw, kind)
    _, sc, sh, _, _ = coeffs(kind, S.pool_rows(B, H, W, C, kw, kind), C)
    y.reshape(B, H, W, C)[2, H - 2, 3, 3] = NAN              # the second element of its window: it must win without the ReLU
    y[0, 3] = np.inf
    lds = S.strides(C)
    for relu, k in itertools.product((True, False), range(3)):
        _, p = check_apply_pool(y, sc, sh, relu, case, (lds[k], lds[(k + 1) % 3], lds[(k + 2) % 3]))
        nans = int(np.isnan(p.get()).sum())
        assert nans == (0 if relu else 1) and (relu or int(np.isnan(p.get()[:, 3]).sum()) == 1)


def test_bn_apply_pool_second_grid_stride_trip():
    """131080 windows x 8 float4 columns: 64 more than one trip of 4096 x 256 threads; the largest magnitude in the last window"""
    case = S.POOL_APPLY_BIG
    B, H, W, C, kh, kw = case
    y = S.real_rows(B * H * W, C, 9)
    _, sc, sh, _, _ = coeffs("real", y[:4096], C)
    y[B * H * W - 1, C - 1] = 3e4 / sc[C - 1]
    a, p = check_apply_pool(y, sc, sh, True, case, ((C, 0), (C, 0), (C, 0)), unfused=False)
    assert S.unique_finite_max_at(p.get()) == (p.rows - 1, C - 1) and S.unique_finite_max_at(a.get()) == (B * H * W - 1, C - 1)


# ----------------------------------------------------------------------------- backward
# (mask form, training, stat64 kept, accumulate, gamma given, parameter gradients wanted)
BWD_FORMS = {"a_train_stat64": ("a", True, True, False, True, True),
             "remask_train_stat64_accumulate": ("remask", True, True, True, True, True),
             "no_relu_train_fp32_stats": (None, True, False, False, True, True),
             "eval_remask_fp32_stats": ("remask", False, False, False, True, True),
             "eval_a_stat64_accumulate_gamma_none": ("a", False, True, True, False, True),
             "remask_train_no_param_grads": ("remask", True, True, False, True, False)}
ALL_FORMS = dict(BWD_FORMS, eval_remask_stat64=("remask", False, True, False, True, True))     # (+ the abs-max cases' from-partials form)
BWD_LAYOUTS = {"packed": lambda C: ((C, 0),) * 4,
               "four_strides": lambda C: ((2 * C, C), (C + 8, 0), (C, 0), (2 * C + 4, C))}     # da, a, y, dy


def run_bwd(kernel, form, dz_in, y, C, M, kind, layout, pool=None, partials=None, slot=None, check=True):
    """one backward launch against the statement.  dz_in: da (pool: the skip gradient or None).  pool = (dpool, B, H, W, kw).
    partials = [blocks + 256][C][2] device tensor, blocks.  -> (dy Out, dgamma, dbeta, Slot, statement)"""
    from qea import ops
    mask, training, keep64, accumulate, with_gamma, want = ALL_FORMS[form]
    gamma, sc, sh, mu, inv = coeffs(kind, y, C)
    m32, i32 = S.f32(mu), S.f32(inv)
    l_da, l_a, l_y, l_dy = layout
    a = S.bn_apply(y, sc, sh, True)
    spec_mask = None if mask is None else (("a", a) if mask == "a" else ("remask", sc, sh))
    dz = S.masked_dz(dz_in, y, spec_mask, pool)
    old = (S.exact_rows(1, C, 21)[0], S.exact_rows(1, C, 22)[0])
    mu_k, inv_k = (mu, inv) if keep64 else (m32.astype(np.float64), i32.astype(np.float64))
    ref = S.bn_bwd(dz, y, gamma if with_gamma else None, mu_k, inv_k, training, old if accumulate else None,
                   None if partials is None else host(partials[0][:partials[1]]))
    yd = inp(y, *l_y)
    dad = None if dz_in is None else inp(dz_in, *l_da)
    dy = Out(M, C, *l_dy)
    dg, db = (Vec(C, old[0]), Vec(C, old[1])) if want else (None, None)
    slot = slot or Slot()
    st64 = dev(np.stack([mu, inv])) if keep64 else None
    args = dict(accumulate=accumulate, stat64=st64, amax=slot.view)
    if mask == "remask":
        args.update(relu_scale=dev(sc), relu_shift=dev(sh))
    gd, md, isd = dev(gamma) if with_gamma else None, dev(m32), dev(i32)
    w = Workspace(M, C)
    if pool is not None:
        dpool, B, H, W, kw = pool
        dpd = inp(dpool, *l_a)
        ops.bn_bwd_pool(dad, l_da[0], dpd, l_a[0], kw, yd, l_y[0], B, H, W, C, gd, md, isd, training, dg.view if want else None,
                        db.view if want else None, dy.view, l_dy[0], **args)
    else:
        ad = inp(a, *l_a) if mask == "a" else None
        ops.bn_bwd(dad, l_da[0], ad, l_a[0] if mask == "a" else 0, yd, l_y[0], M, C, gd, md, isd, training, dg.view if want else None,
                   db.view if want else None, dy.view, l_dy[0], partials=partials, **args)
    torch.cuda.synchronize()
    tag = f"{form} C={C} M={M} {kind}"
    assert dy.untouched() and w.untouched(), f"{kernel} {tag}: wrote outside its columns / its workspace"
    if not check:
        return dy, dg, db, slot, ref
    within(kernel, tag + " dy", dy.get(), ref.dy, ref.g_dy)
    slot_holds_amax_of(slot, dy.get(), f"{kernel} {tag}")
    if want:
        assert dg.untouched() and db.untouched()
        if kind == "exact":
            assert same_bits(dg.get(), ref.dgamma_f32) and same_bits(db.get(), ref.dbeta_f32), f"{kernel} {tag}: dgamma / dbeta bits"
        within(kernel, tag + " dgamma", dg.get(), ref.dgamma, ref.g_dgamma)
        within(kernel, tag + " dbeta", db.get(), ref.dbeta, ref.g_dbeta)
    return dy, dg, db, slot, ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", BWD_FORMS)
@pytest.mark.parametrize("C,M", S.RED, ids=str)
def test_bn_bwd_forms_incl_no_relu_and_training_false_remask(C, M, form, kind):
    """qea_bn_bwd in every form the ABI accepts (mask from a, recomputed, none; training=False with remask; stat64 NULL; gamma NULL;
    dgamma / dbeta NULL or accumulated), packed and with four different strides for da, a, y, dy"""
    y, da = rows_of(kind, M, C), S.exact_rows(M, C, 5) if kind == "exact" else S.real_rows(M, C, 5)
    for name, lay in BWD_LAYOUTS.items():
        run_bwd("bn_bwd", form, da, y, C, M, kind, lay(C))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("da_given", (True, False), ids=("da", "da_none"))
@pytest.mark.parametrize("case", S.POOL + (S.POOL_BWD_RAGGED,), ids=sid)
def test_bn_bwd_pool_da_and_da_none_against_statement_and_unfused(case, da_given, kind):
    """qea_bn_bwd_pool with and without the skip gradient (da=None: the CRNN's pool-only stage), training and eval (training=False,
    mask recomputed, stat64 NULL), against the statement and against qea_maxpool_bwd(accumulate) + qea_bn_bwd on a zero or given da:
    dgamma / dbeta / dy bit for bit on exact data (norm_pool.hip: "Values: identical"; the fp64 sums are exact there in any order)"""
    from qea import ops
    B, H, W, C, kh, kw = case
    M = B * H * W
    y = S.pool_rows(B, H, W, C, kw, kind)
    dpool = rows_of(kind, M // (2 * kw), C, 31)
    dskip = rows_of(kind, M, C, 32) if da_given else None
    for form, lay in (("remask_train_stat64_accumulate", "four_strides"), ("eval_remask_fp32_stats", "packed"),
                      ("remask_train_no_param_grads", "packed")):
        dy, dg, db, slot, ref = run_bwd("bn_bwd_pool", form, dskip, y, C, M, kind, BWD_LAYOUTS[lay](C), pool=(dpool, B, H, W, kw))
        # unfused: the stored activation, the pool's backward accumulated into the skip gradient (or zero), the plain backward
        _, sc, sh, _, _ = coeffs(kind, y, C)
        a, _ = run_apply(y, sc, sh, True, (C, 0), (C, 0))
        dad = dev(dskip) if da_given else torch.zeros(M, C, device=DEV)
        ops.maxpool_bwd(a.view, C, dev(dpool), C, dad, C, B, H, W, C, 2, kw, relu_mask=False, accumulate=True)
        torch.cuda.synchronize()
        assert same_bits(host(dad) * (a.get() > 0), ref.dz), (case, form)
        dy2, dg2, db2, slot2, _ = run_bwd("bn_bwd", form, host(dad), y, C, M, kind, BWD_LAYOUTS[lay](C), check=False)
        if kind == "exact":
            assert same_bits(dy.get(), dy2.get()) and slot.value() == slot2.value(), (case, form)
            if dg is not None:
                assert same_bits(dg.get(), dg2.get()) and same_bits(db.get(), db2.get()), (case, form)
        else:
            within("bn_bwd_pool", f"{case} {form} fused - unfused", dy.get(), dy2.get(), 2 * ref.g_dy)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", S.PART_C)
@pytest.mark.parametrize("blocks", S.PART_BLOCKS)
def test_bn_bwd_from_partials(blocks, C, kind):
    """the sums come from [blocks][C][2] partial rows (up to 512: read directly; 513, 700: folded through the 256 scratch rows behind
    them, pre-filled with 1e300 and never read unwritten); the rows and the unused scratch rows stay as they were"""
    M = S.PART_M
    y, da = rows_of(kind, M, C), rows_of(kind, M, C, 5)
    _, sc, sh, mu, inv = coeffs(kind, y, C)
    dz = S.masked_dz(da, y, ("remask", sc, sh))
    P = np.full((blocks + S.SCRATCH_ROWS, C, 2), 1e300)
    P[:blocks] = S.partial_rows(dz, y, mu, inv, blocks)
    Pd = dev(P)
    for form in ("remask_train_stat64_accumulate", "remask_train_no_param_grads"):
        dy, dg, db, slot, ref = run_bwd("bn_bwd_from_partials", form, da, y, C, M, kind, BWD_LAYOUTS["four_strides"](C), partials=(Pd, blocks))
        after = host(Pd)
        folded, rows, per = S.fold(blocks)
        assert np.array_equal(after[:blocks], P[:blocks]), "the partial rows were written"
        assert np.array_equal(after[blocks + (rows if folded else 0):], P[blocks + (rows if folded else 0):]), "scratch rows beyond the fold were written"
        if folded:
            assert bool((np.abs(after[blocks:blocks + rows]) < 1e200).all())
        if kind == "exact":                                  # the same sums as the plain form: the same constants, the same dy
            dy2, *_ = run_bwd("bn_bwd", form, da, y, C, M, kind, BWD_LAYOUTS["four_strides"](C), check=False)
            assert same_bits(dy.get(), dy2.get()), (blocks, C, form)


def test_bn_backward_reads_the_unrounded_stat64_of_the_forward():
    """qea_bn_train_stats -> qea_bn_bwd on the DEVICE's own stat64, scale and shift, real data.  The statement runs on its own fp64
    mean / invstd; the gate adds what the forward's gates g_mean and g_invstd (r = g_invstd / invstd) can move dy by:
        xhat = (y - mu) is:  |d xhat| <= is g_mean + |xhat| r =: ex;   m1 = mean(dz xhat):  |d m1| <= mean(|dz| ex) =: em1
        dy = g is (dz - m0 - xhat m1):  |d dy| <= |g| is (|xhat| em1 + ex |m1|) + r |g is| (|dz| + |m0| + |xhat m1|)
    A mean and invstd rounded to fp32 move the statement's dy by thousands of these gates on the channels of mean 30 and spread 0.05
    and, on the mean-10^3 channel, whose gate carries the one-pass variance's conditioning term, still by more than one (both asserted
    on the statement): the backward passes only if it reads the unrounded halves of stat64."""
    from qea import ops
    C, M = 32, 8197
    y, da = S.real_rows(M, C), S.real_rows(M, C, 5)
    gamma, beta, *_ = S.vectors(C)
    v = {k: Vec(C) for k in ("mean", "invstd", "scale", "shift")}
    st64 = Vec(2 * C, dtype=torch.float64)
    yd = dev(y)
    ops.bn_train_stats(yd, C, M, C, dev(gamma), dev(beta), EPS, 0.1, None, None, v["mean"].view, v["invstd"].view, v["scale"].view,
                       v["shift"].view, st64.view)
    dy, dg, db = Out(M, C, C, 0), Vec(C), Vec(C)
    ops.bn_bwd(dev(da), C, None, 0, yd, C, M, C, dev(gamma), v["mean"].view, v["invstd"].view, True, dg.view, db.view, dy.view, C,
               stat64=st64.view, relu_scale=v["scale"].view, relu_shift=v["shift"].view)
    torch.cuda.synchronize()
    st = S.train_stats(y, gamma, beta, EPS)
    dz = S.masked_dz(da, y, ("remask", v["scale"].get(), v["shift"].get()))        # the mask of the device's own fp32 coefficients
    ref = S.bn_bwd(dz, y, gamma, st.mean, st.invstd, True)
    g, r = gamma.astype(np.float64), st.g_invstd / st.invstd
    xhat = (y.astype(np.float64) - st.mean) * st.invstd
    adz = np.abs(dz.astype(np.float64))
    ex = st.invstd * st.g_mean + np.abs(xhat) * r
    m0, m1, em1 = ref.s / M, ref.q / M, (adz * ex).sum(0) / M
    extra = np.abs(g) * st.invstd * (np.abs(xhat) * em1 + ex * np.abs(m1)) + r * np.abs(g * st.invstd) * (adz + np.abs(m0) + np.abs(xhat * m1))
    within("bn_train_stats+bn_bwd", "dy on the device's stat64", dy.get(), ref.dy, ref.g_dy + extra)
    rounded = S.bn_bwd(dz, y, gamma, S.f32(st.mean).astype(np.float64), S.f32(st.invstd).astype(np.float64), True)
    moved = (np.abs(rounded.dy - ref.dy) / (ref.g_dy + extra)).max(0)
    assert float(moved.max()) > 100 and float(moved[S.BIG_CH]) > 1, "the case no longer tells fp32 statistics from stat64"


# ----------------------------------------------------------------------------- column and layout kernels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,M", S.RED, ids=str)
def test_colsum_overwrite_and_accumulate(C, M, kind):
    from qea import ops
    x = rows_of(kind, M, C, 41)
    old = S.exact_rows(1, C, 42)[0]
    for (ld, off), acc in itertools.product(S.strides(C), (False, True)):
        out = Vec(C, old)
        w = Workspace(M, C)
        ops.colsum(inp(x, ld, off), ld, M, C, out.view, accumulate=acc)
        torch.cuda.synchronize()
        assert out.untouched() and w.untouched()
        v, v32, gate = S.colsum(x, old if acc else None)
        if kind == "exact":
            assert same_bits(out.get(), v32), (C, M, ld, acc)
        within("colsum", f"C={C} M={M} ld={ld} acc={acc} {kind}", out.get(), v, gate)


def run_absmax(x, M, C, ld):
    """x as the first C columns of a [M][ld] buffer whose pad columns hold 1e30: a pad column read would be the maximum"""
    from qea import _lib
    xd = torch.full((M, ld), 1e30, device=DEV)
    xd[:, :C] = dev(np.asarray(x, dtype=np.float32))
    slot = Slot(SENTINEL)                                    # qea_absmax zero-fills its output itself
    _lib.check(_lib.lib().qea_absmax(xd.data_ptr(), ld, M, C, slot.view.data_ptr(), torch.cuda.current_stream().cuda_stream), "qea_absmax")
    torch.cuda.synchronize()
    return slot.value()


def test_absmax_tiny_shapes_nan_inf_and_zero():
    from qea import ops
    for M, C, ld in S.ABSMAX:
        x = S.exact_rows(M, C, 51)
        for where, value in (((0, 0), 9.0), ((M - 1, C - 1), -9.0)):
            xx = S.plant(x, where, value)
            xx[0, 1], xx[M - 1, 2] = np.inf, NAN             # (columns 1 and 2: never the planted element)
            if C > 4:
                xx[0, 4] = -np.inf
            assert run_absmax(xx, M, C, ld) == S.absmax(xx) == 9.0
        assert run_absmax(np.zeros((M, C)), M, C, ld) == 0
        assert run_absmax(np.full((M, C), np.inf) * np.where(np.arange(C) % 2, 1, -1), M, C, ld) == 0
        assert run_absmax(np.full((M, C), NAN), M, C, ld) == 0
        assert float(ops.absmax(dev(S.plant(x, (0, 0), 9.0)), C, M, C).item()) == 9.0


def test_absmax_above_the_2048_block_cap():
    """(16400, 1024): 4,198,400 float4 ask for 2050 blocks, the grid is 2048 and strides; the maximum in the last element, then the first"""
    M, C, ld = S.ABSMAX_BIG
    from qea import _lib as L
    x = torch.from_numpy(S.exact_rows(M, C, 52)).to(DEV)
    for r, c, v in ((M - 1, C - 1, -77.0), (0, 0, 99.0)):
        x[r, c] = v
        x[M // 2, 5] = float("inf")
        slot = Slot(SENTINEL)
        L.check(L.lib().qea_absmax(x.data_ptr(), ld, M, C, slot.view.data_ptr(), torch.cuda.current_stream().cuda_stream), "qea_absmax")
        torch.cuda.synchronize()
        assert slot.value() == abs(v)


def test_transpose2d_and_filter_flip_transpose():
    from qea import ops
    for R, Cc in S.TRANSPOSE:
        a = np.arange(R * Cc, dtype=np.float32).reshape(R, Cc) + 1
        out = Out(Cc, R, R, 0)
        flat = out.buf.view(-1)[:R * Cc]
        ops.transpose2d(dev(a), flat, R, Cc)
        torch.cuda.synchronize()
        assert same_bits(host(flat).reshape(Cc, R), S.transpose2d(a)), (R, Cc)
        assert bool((out.buf.view(-1)[R * Cc:] == SENTINEL).all())
    for Co, Ci, KH, KW in S.FLIP:
        w = S.exact_rows(Co * KH * KW, Ci, 61).reshape(Co, KH, KW, Ci)
        n = Co * KH * KW * Ci
        buf = torch.full((n + 64,), SENTINEL, device=DEV)
        ops.filter_flip_transpose(dev(w), buf[:n], Co, Ci, KH, KW)
        torch.cuda.synchronize()
        assert same_bits(host(buf[:n]).reshape(Ci, KH, KW, Co), S.filter_flip_transpose(w)), (Co, Ci, KH, KW)
        assert bool((buf[n:] == SENTINEL).all())


# ----------------------------------------------------------------------------- abs-max positions and slot states
@pytest.mark.parametrize("C,M", [(12, 130), (32, 8197), (1024, 33)], ids=str)
def test_absmax_slot_finds_the_maximum_at_every_position(C, M):
    """the single largest stored magnitude at the first and last element, the last row of the ragged last block, the column next to the
    idle lane, a row of bn_bwd_apply_kernel's odd tail; positive and negative; for bn_apply, bn_bwd and bn_bwd_from_partials"""
    g = S.col_geom(M, C)
    ag = S.apply_geom(M, g.rt, 8)
    gamma, sc, sh, mu, inv = coeffs("exact", None, C)
    y, da = S.exact_rows(M, C), S.exact_rows(M, C, 5)
    P = np.zeros((3 + S.SCRATCH_ROWS, C, 2))
    for (name, where), sign in itertools.product(S.amax_rows(C, M, ag.per_block, g.rt).items(), (1.0, -1.0)):
        yy = S.plant(y, where, (sign * 4096 - sh[where[1]]) / sc[where[1]])
        out, slot = run_apply(yy, sc, sh, False, (C, 0), (C, 0))
        assert S.unique_finite_max_at(out.get()) == where, name
        slot_holds_amax_of(slot, out.get(), f"bn_apply {name} {sign}")
        dd = S.plant(da, where, sign * 4096)
        for kernel, part in (("bn_bwd", None), ("bn_bwd_from_partials", (dev(P), 3))):
            dy, _, _, slot, _ = run_bwd(kernel, "eval_remask_stat64" if part else "eval_remask_fp32_stats", dd, S.plant(y, where, (1 - sh[where[1]]) / sc[where[1]]),
                                        C, M, "exact", BWD_LAYOUTS["packed"](C), partials=part)
            assert S.unique_finite_max_at(dy.get()) == where, (kernel, name)


@pytest.mark.parametrize("case", S.AMAX_POOL, ids=sid)
def test_absmax_slots_of_the_pool_kernels_find_the_last_window(case):
    """the largest activation, pooled value and dy in the last window's last element, in its first, and in the very first element"""
    B, H, W, C, kh, kw = case
    M = B * H * W
    gamma, sc, sh, mu, inv = coeffs("exact", None, C)
    y, dpool = S.pool_rows(B, H, W, C, kw, "exact"), S.exact_rows(M // (2 * kw), C, 31)
    for where in S.amax_pool_rows(B, H, W, C, kw).values():
        c = where[1]
        yy = S.plant(y, where, (4096 - sh[c]) / sc[c])
        a, p = check_apply_pool(yy, sc, sh, True, case, ((C, 0),) * 3, unfused=False)
        assert S.unique_finite_max_at(a.get()) == where and S.unique_finite_max_at(p.get())[1] == c
        win = S.unique_finite_max_at(p.get())[0]
        for sign in (1.0, -1.0):
            dy, _, _, slot, _ = run_bwd("bn_bwd_pool", "eval_remask_fp32_stats", None, yy, C, M, "exact", BWD_LAYOUTS["packed"](C),
                                        pool=(S.plant(dpool, (win, c), sign * 4096), B, H, W, kw))
            assert S.unique_finite_max_at(dy.get()) == where


def test_absmax_slot_states_inf_zero_larger_smaller_and_shared():
    C, M = 12, 130
    gamma, sc, sh, mu, inv = coeffs("exact", None, C)
    y = S.exact_rows(M, C)
    top = S.amax(S.bn_apply(y, sc, sh, False))
    # a stored +inf larger than everything is ignored
    out, slot = run_apply(S.plant(y, (M - 1, C - 1), np.inf), sc, sh, False, (C, 0), (C, 0))
    assert np.isinf(out.get()[M - 1, C - 1]) and slot.value() == np.float32(S.amax(out.get())) and slot.value() < 1e3
    # an all-zero output leaves the zero
    out, slot = run_apply(y, np.zeros(C, dtype=np.float32), np.zeros(C, dtype=np.float32), True, (C, 0), (C, 0))
    assert not out.get().any() and slot.value() == 0
    # a larger value stays, a smaller one is raised
    assert run_apply(y, sc, sh, False, (C, 0), (C, 0), slot_init=1e6)[1].value() == np.float32(1e6)
    assert run_apply(y, sc, sh, False, (C, 0), (C, 0), slot_init=2.0 ** -20)[1].value() == np.float32(top)
    # one slot shared by two launches over two row ranges (a BatchNorm applied per statistics group): the maximum in either range
    for where in ((3, 5), (M - 2, 7)):
        yy = S.plant(y, where, (-4096 - sh[where[1]]) / sc[where[1]])
        slot = Slot()
        out1, _ = run_apply(yy, sc, sh, False, (C, 0), (C, 0), slot_init=slot, rows=(0, 70))
        out2, _ = run_apply(yy, sc, sh, False, (C, 0), (C, 0), slot_init=slot, rows=(70, M))
        stored = np.concatenate([out1.get()[:70], out2.get()[70:]])
        assert same_bits(stored, S.bn_apply(yy, sc, sh, False)) and slot.value() == np.float32(S.amax(stored)) == 4096
        assert bool((out1.get()[70:] == SENTINEL).all()) and bool((out2.get()[:70] == SENTINEL).all())


# ----------------------------------------------------------------------------- refusals: argument checks, nothing launches
def test_refusals_leave_every_output_untouched():
    from qea import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    Cb, M, B, H, W = 1028, 8, 1, 2, 4                       # every buffer is large enough for the widest refused C: nothing could run out of bounds
    f = lambda: torch.full((M + 3, 2 * Cb + 8), SENTINEL, device=DEV)       # noqa: E731
    x, a, y, out, out2, v1, v2, v3, v4 = (f() for _ in range(9))
    d64 = torch.full((4 * Cb,), SENTINEL, device=DEV, dtype=torch.float64)
    parts = torch.zeros((3 + S.SCRATCH_ROWS) * Cb * 2, device=DEV, dtype=torch.float64)
    ws = torch.full((1 << 20,), 0xA5, device=DEV, dtype=torch.uint8)
    slot = Slot(SENTINEL)
    p = lambda t: t.data_ptr()                               # noqa: E731
    need = lambda C: L.qea_colreduce_workspace_bytes(M, C)   # noqa: E731

    def stats(C, ld, wb=None):
        return L.qea_bn_train_stats(p(y), ld, M, C, p(v1), p(v2), EPS, 0.1, p(v3), p(v4), p(out), p(out2), p(x), p(a), p(d64), p(ws), need(16) if wb is None else wb, st)

    def bwd(C, ld=(16, 16, 16, 16), a_=None, rs=None, rh=None, wb=None):
        return L.qea_bn_bwd(p(x), ld[0], a_, ld[1], rs, rh, p(y), ld[2], M, C, p(v1), p(v2), p(v3), p(d64), 1, p(out2), p(v4), 0, p(out), ld[3], p(ws),
                            (1 << 20) if wb is None else wb, p(slot.view), st)

    def bwd_pool(C, kw=2, Hh=H, rs=p(v1), rh=p(v2), ld=16, wb=None):
        return L.qea_bn_bwd_pool(p(x), ld, p(a), 16, kw, rs, rh, p(y), 16, B, Hh, W, C, p(v1), p(v2), p(v3), p(d64), 1, p(out2), p(v4), 0, p(out), 16, p(ws),
                                 (1 << 20) if wb is None else wb, p(slot.view), st)

    def from_partials(C, s64=p(d64), ld=16, wb=None):
        return L.qea_bn_bwd_from_partials(p(parts), 3, p(x), ld, p(v1), p(v2), p(y), 16, M, C, p(v1), p(v2), p(v3), s64, 1, p(out2), p(v4), 0, p(out), 16, p(ws),
                                          (1 << 20) if wb is None else wb, p(slot.view), st)

    def colsum(C, ld, wb=None):
        return L.qea_colsum(p(x), ld, M, C, p(out), 0, p(ws), (1 << 20) if wb is None else wb, st)

    def apply(C, ldy=16, lda=16):
        return L.qea_bn_apply(p(y), ldy, p(out), lda, M, C, p(v1), p(v2), 1, p(slot.view), st)

    def apply_pool(C, ldy=16, lda=16, ldp=16):
        return L.qea_bn_apply_pool(p(y), ldy, p(out), lda, p(out2), ldp, B, H, W, C, p(v1), p(v2), 1, 2, 2, p(slot.view), p(slot.view), st)

    def absmax(C, ld):
        return L.qea_absmax(p(x), ld, M, C, p(slot.view), st)

    cases = []
    for name, fn in (("qea_bn_train_stats", lambda C: stats(C, 2 * Cb)), ("qea_bn_bwd", lambda C: bwd(C, (2 * Cb,) * 4)),
                     ("qea_bn_bwd_pool", lambda C: bwd_pool(C)), ("qea_bn_bwd_from_partials", lambda C: from_partials(C)),
                     ("qea_colsum", lambda C: colsum(C, 2 * Cb))):
        cases += [(f"{name}: need C % 4 == 0 and C <= 1024", lambda fn=fn, C=C: fn(C)) for C in (10, Cb)]
    cases += [("qea_bn_apply: bad arguments", lambda: apply(10)), ("qea_bn_apply_pool: bad arguments", lambda: apply_pool(10)),
              ("qea_absmax: bad arguments", lambda: absmax(10, 16))]
    # a stride that is not a multiple of 4, in each position
    cases += [("qea_bn_train_stats: strides must be multiples of 4", lambda: stats(16, 18)),
              ("qea_colsum: strides must be multiples of 4", lambda: colsum(16, 18)),
              ("qea_bn_bwd_pool: strides must be multiples of 4", lambda: bwd_pool(16, ld=18)),
              ("qea_bn_bwd_from_partials: strides must be multiples of 4", lambda: from_partials(16, ld=18)),
              ("qea_bn_apply: bad arguments", lambda: apply(16, ldy=18)), ("qea_bn_apply: bad arguments", lambda: apply(16, lda=18)),
              ("qea_bn_apply_pool: bad arguments", lambda: apply_pool(16, ldy=18)), ("qea_bn_apply_pool: bad arguments", lambda: apply_pool(16, lda=18)),
              ("qea_bn_apply_pool: bad arguments", lambda: apply_pool(16, ldp=18)), ("qea_absmax: bad arguments", lambda: absmax(16, 18))]
    for k in range(4):
        ld = tuple(18 if i == k else 16 for i in range(4))
        cases.append(("qea_bn_bwd: strides must be multiples of 4", lambda ld=ld: bwd(16, ld, a_=p(a))))
    # a workspace one byte short of qea_colreduce_workspace_bytes
    cases += [("qea_bn_train_stats: workspace too small", lambda: stats(16, 16, wb=need(16) - 1)),
              ("qea_bn_bwd: workspace too small", lambda: bwd(16, wb=need(16) - 1)),
              ("qea_bn_bwd_pool: workspace too small", lambda: bwd_pool(16, wb=need(16) - 1)),
              ("qea_colsum: workspace too small", lambda: colsum(16, 16, wb=need(16) - 1)),
              ("qea_bn_bwd_from_partials: workspace too small", lambda: from_partials(16, wb=3 * 16 * 8 - 1))]
    cases += [("qea_bn_bwd: give the ReLU mask either as a or as relu_scale", lambda: bwd(16, a_=p(a), rs=p(v1), rh=p(v2))),
              ("qea_bn_bwd: relu_scale and relu_shift go together", lambda: bwd(16, rs=p(v1))),
              ("qea_bn_bwd_pool: 2 x kw windows", lambda: bwd_pool(16, kw=3)), ("qea_bn_bwd_pool: 2 x kw windows", lambda: bwd_pool(16, Hh=3)),
              ("qea_bn_bwd_pool: null pointer", lambda: bwd_pool(16, rs=None, rh=None)),
              ("qea_bn_bwd_from_partials: null pointer", lambda: from_partials(16, s64=None)),
              ("qea_absmax: bad arguments", lambda: absmax(16, 12))]
    assert need(16) > 1 and need(16) == S.colreduce_ws_bytes(M, 16)
    accepted = []
    for i, (match, call) in enumerate(cases):
        if call() == 0:
            accepted.append((i, match))
        else:
            msg = L.qea_last_error().decode()
            assert msg.startswith(match), (i, match, msg)
    torch.cuda.synchronize()
    assert not accepted, f"accepted instead of refused: {accepted}"
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all()) and slot.value() == np.float32(SENTINEL)
