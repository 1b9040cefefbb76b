"""The single-channel kernels of csrc/conv_c1.hip (C_in = 1 convolution: forward, forward + pool, weight / bias gradient, input
gradient, the backward from the pooled gradient; the UNet head) and the two max-pool kernels of csrc/norm_pool.hip against the fp64
statements of tests/c1_spec.py.  Two kinds of data per shape: `int`, on which every partial sum is an integer below 2^24 and the kernel
must equal the statement exactly, and `real`, gated per element by a count of fp32 roundings times the sum of the magnitudes of the
terms ("Single-channel kernels"): no gate is taken from what a kernel gives.  Outputs go into sentinel-filled buffers
wider than the tensor (ld = C at offset 0 and ld = 2C at offset C), strided inputs carry NaN in their pad columns, x lies between NaN
guards.  Every test prints its worst error / gate ratio (run with -s)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import c1_spec as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = S.EPS32
SENTINEL = -777.0
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layouts(C):
    """(ld, column offset): the tensor alone, and as the second half of a 2C-wide concat buffer"""
    return ((C, 0), (2 * C, C))


def strided(a2d, ld, off, fill):
    """a [rows][C] as columns off .. off + C of a [rows][ld] buffer filled with `fill` -> (buffer, view)"""
    a2d = a2d if torch.is_tensor(a2d) else dev(np.asarray(a2d, dtype=np.float32))
    rows, C = a2d.shape
    buf = torch.full((rows, ld), fill, device=DEV)
    buf[:, off:off + C] = a2d
    return buf, buf[:, off:off + C]


def out_buf(rows, C, ld, off):
    buf = torch.full((rows, ld), SENTINEL, device=DEV)
    return buf, buf[:, off:off + C]


def pads_hold(buf, C, off, fill=SENTINEL):
    """the columns of `buf` outside off .. off + C still hold the fill"""
    pad = torch.cat([buf[:, :off], buf[:, off + C:]], dim=1)
    return bool(pad.isnan().all()) if fill != fill else bool((pad == fill).all())


def guarded(a, fill=SENTINEL, guard=64):
    """a flat copy of `a` between two guards of `guard` elements -> (buffer, view of a's shape)"""
    a = np.asarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * guard,), fill, device=DEV)
    buf[guard:guard + a.size] = dev(a.ravel())
    return buf, buf[guard:guard + a.size].view(*a.shape)


def guards_hold(buf, fill=SENTINEL, guard=64):
    g = torch.cat([buf[:guard], buf[-guard:]])
    return bool(g.isnan().all()) if fill != fill else bool((g == fill).all())


def image(x):
    """x [B][H][W] on the device between NaN guards: a read outside the tensor would show"""
    return guarded(x, NAN)[1]


def host(t):
    return t.detach().cpu().numpy()


def data(kind, B, H, W, Co, scale=1.0):
    return S.int_data(B, H, W, Co) if kind == "int" else S.real_data(B, H, W, Co, scale)


KINDS = (("int", 1.0),) + tuple(("real", s) for s in S.REAL_SCALES)
KIND_IDS = ["int", "real", "real_2^-12"]


def check(tag, kind, got, ref, gate):
    """int: equal; real: within the gate, NaN and inf patterns equal -> the worst error / gate"""
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref, dtype=np.float64).reshape(got.shape)
    if kind == "int":
        assert np.array_equal(got, ref), f"{tag}: {int((got != ref).sum())} of {got.size} elements differ on exact data"
        return 0.0
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN pattern"
    r = S.gate_ratio(got, ref, np.asarray(gate, dtype=np.float64).reshape(got.shape))
    assert r <= 1, (tag, r)
    return r


# ----------------------------------------------------------------------------- forward
def run_fwd(xd, d, shape, bias, relu, ld, off):
    from qea import ops
    B, H, W, Co = shape
    buf, y = out_buf(B * H * W, Co, ld, off)
    ops.conv_c1_fwd(xd, dev(d.w), dev(d.bias) if bias else None, y, ld, B, H, W, Co, relu=relu)
    torch.cuda.synchronize()
    assert pads_hold(buf, Co, off), "conv_c1_fwd wrote outside its columns"
    return y


@pytest.mark.parametrize("kind,scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", S.FWD4 + S.FWD1, ids=str)
def test_conv_c1_fwd(shape, kind, scale):
    """both forward kernels (S.FWD4: four pixels per thread; S.FWD1: one), with and without bias and ReLU, both layouts; gate
    10 x 2^-24 x (|bias| + sum |w x|)"""
    B, H, W, Co = shape
    d = data(kind, B, H, W, Co, scale)
    xd = image(d.x)
    worst = 0.0
    for bias, relu, (ld, off) in itertools.product((True, False), (True, False), layouts(Co)):
        ref, cond = S.conv_fwd(d.x, d.w, d.bias if bias else None, relu)
        got = run_fwd(xd, d, shape, bias, relu, ld, off)
        worst = max(worst, check(f"fwd {shape} bias={bias} relu={relu} ld={ld}", kind, got, ref.reshape(-1, Co),
                                 S.FWD_ROUNDINGS * EPS32 * cond))
    print(f"conv_c1_fwd {shape} {kind} x{scale:g}: worst error / gate {worst:.3f}")


@pytest.mark.parametrize("shape", (S.FWD4_BIG, S.FWD1_BIG), ids=str)
def test_conv_c1_fwd_second_grid_stride_trip(shape):
    """more pixels than one trip of the grid covers (524,288 for the four-pixel kernel, 65,536 for the one-pixel kernel, at Co = 128):
    exact data, the four bias / ReLU forms launched once each and compared image chunk by image chunk"""
    B, H, W, Co = shape
    d = S.int_data(B, H, W, Co)
    xd = image(d.x)
    forms = list(itertools.product((True, False), (True, False)))
    got = [run_fwd(xd, d, shape, bias, relu, 2 * Co, Co).view(B, H, W, Co) for bias, relu in forms]
    step = 4
    for b0 in range(0, B, step):
        pre = S.conv_fwd(d.x[b0:b0 + step], d.w, None, False)[0]
        for (bias, relu), g in zip(forms, got):
            ref = pre + d.bias.astype(np.float64) if bias else pre
            ref = S.relu(ref) if relu else ref
            assert np.array_equal(host(g[b0:b0 + step]), ref), (shape, bias, relu, b0)


@pytest.mark.parametrize("kind,scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", S.FWD_POOL, ids=str)
def test_conv_c1_fwd_pool(shape, kind, scale):
    """conv + ReLU + pool(2, 2) in one kernel against the STATEMENT (not the separate kernels): y where given (and y = None), the
    pooled tensor within the largest of its window's four gates (max is 1-Lipschitz in the sup norm, so an fp32 winner that is not
    the statement's still lands there), the abs-max slot; then the same with a NaN and a +inf in x: NaN pattern exact (the ReLU is
    fmaxf: it turns a NaN into 0; without it the NaN wins the pool), the slot still the largest FINITE pooled magnitude"""
    from qea import ops
    B, H, W, Co = shape
    d = data(kind, B, H, W, Co, scale)
    x2 = d.x.copy()
    x2[0, 0, 0] = np.nan
    x2[-1, -1, -1] = np.inf
    worst = 0.0
    for x, relu, with_y, (ld, off) in itertools.product((d.x, x2), (True, False), (True, False), layouts(Co)):
        ref, cond = S.conv_fwd(x, d.w, d.bias, relu)
        gate = S.FWD_ROUNDINGS * EPS32 * cond
        pref, _ = S.pool(ref, 2, 2)
        # (an element with a NaN or inf in its patch is NaN, +-inf or, after the ReLU, 0 on both sides: no error of its own)
        pgate = S._windows(np.where(np.isfinite(gate), gate, 0.0), 2, 2).max(axis=3)
        ybuf, y = out_buf(B * H * W, Co, ld, off)
        pbuf, p = out_buf(B * H * W // 4, Co, ld, off)
        slot = torch.zeros(1, device=DEV)
        took = ops.conv_c1_fwd_pool(image(x), dev(d.w), dev(d.bias), y if with_y else None, ld, p, ld, B, H, W, Co, relu=relu, pooled_amax=slot)
        torch.cuda.synchronize()
        assert took is True and pads_hold(pbuf, Co, off)
        assert pads_hold(ybuf, Co, off) if with_y else bool((ybuf == SENTINEL).all())
        tag = f"fwd_pool {shape} relu={relu} y={with_y} ld={ld} nan={x is x2}"
        if with_y:
            worst = max(worst, check(tag + " y", kind if x is d.x else "real", y, ref.reshape(-1, Co), gate))
        worst = max(worst, check(tag + " pooled", kind if x is d.x else "real", p, pref.reshape(-1, Co), pgate))
        assert float(slot.item()) == S.amax(host(p)), tag                # of the kernel's own pooled values: exact
        if kind == "int" and x is d.x:
            assert float(slot.item()) == S.amax(pref)
        if x is x2:
            assert np.isnan(pref).any() == (not relu) and np.isinf(pref).any()
    print(f"conv_c1_fwd_pool {shape} {kind} x{scale:g}: worst error / gate {worst:.3f}")


@pytest.mark.parametrize("shape", S.FWD_POOL, ids=str)
def test_conv_c1_fwd_pool_keeps_the_first_of_tied_zeros(shape):
    """The fused kernel shows its winner only through the value, so first against last maximum shows only in the sign of a zero.
    Channel 3 gets a filter and a bias of -0.0: every product with x >= 0 (and with the padding) is -0.0 and the pre-activation is
    -0.0, except where the patch holds the one negative pixel x[0][0][2], whose product is +0.0 and makes the sum +0.0.  Window
    (0, 0) of image 0 then scans -0, +0, -0, +0 and must keep the first, -0.0; window (0, 1), whose first element sees the negative
    pixel, is +0.0; every other window is -0.0."""
    from qea import ops
    B, H, W, Co = shape
    d = S.int_data(B, H, W, Co)
    x, w, bias = d.x.copy(), d.w.copy(), d.bias.copy()
    x[0, 0, 2] = -1
    w[3], bias[3] = np.float32(-0.0), np.float32(-0.0)
    want = np.full((B, H // 2, W // 2), -0.0, dtype=np.float32)
    want[0, 0, 1] = 0.0
    for ld, off in layouts(Co):
        pbuf, p = out_buf(B * H * W // 4, Co, ld, off)
        assert ops.conv_c1_fwd_pool(image(x), dev(w), dev(bias), None, ld, p, ld, B, H, W, Co, relu=False)
        torch.cuda.synchronize()
        got = host(p).reshape(B, H // 2, W // 2, Co)
        assert np.array_equal(bits(got[..., 3]), bits(want)), (shape, ld)
        assert np.array_equal(np.delete(got, 3, axis=3), np.delete(S.pool(S.conv_fwd(x, w, bias, False)[0], 2, 2)[0], 3, axis=3))


def test_conv_c1_fwd_pool_declines_an_odd_height():
    from qea import ops
    buf, p = out_buf(3, 32, 32, 0)
    assert ops.conv_c1_fwd_pool(image(np.zeros((1, 3, 4))), torch.zeros(32, 9, device=DEV), None, None, 32, p, 32, 1, 3, 4, 32) is False
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ----------------------------------------------------------------------------- weight gradient
def wgrad_cases(kind, d, dy, shape, prev_w, prev_b):
    """plain, accumulate onto non-zero dw / db, and the UNet's call: db = None with accumulate -> worst ratio"""
    from qea import ops
    B, H, W, Co = shape
    M = B * H * W
    xd = image(d.x)
    worst = 0.0
    if kind == "int" and M > 10 ** 6:                                    # nine shifted matrix-vector products per image chunk, exact
        dw, db = np.zeros((Co, 9)), np.zeros(Co)
        for b0 in range(B):
            a = S.conv_wgrad(d.x[b0:b0 + 1], dy[b0:b0 + 1])
            dw, db = dw + a[0], db + a[1]
        cw = cb = None
    else:
        dw, db, cw, cb = S.conv_wgrad(d.x, dy)
    n = S.wgrad_chain(M, Co) + 1
    lays = layouts(Co)[1:] if M > 10 ** 6 else layouts(Co)
    for ld, off in lays:
        dyd = strided(dev(dy.reshape(M, Co)).float(), ld, off, NAN)[1]
        for acc, with_db in ((False, True), (True, True), (True, False)):
            wbuf, dwd = guarded(prev_w)
            bbuf, dbd = guarded(prev_b)
            ops.conv_c1_wgrad(xd, dyd, ld, dwd, dbd if with_db else None, B, H, W, Co, accumulate=acc)
            torch.cuda.synchronize()
            assert guards_hold(wbuf) and guards_hold(bbuf)
            rw = dw + prev_w if acc else dw
            rb = db + prev_b if acc else db
            tag = f"wgrad {shape} {kind} ld={ld} accumulate={acc} db={with_db}"
            gw = gb = None
            if kind != "int":
                gw, gb = n * EPS32 * cw + acc * EPS32 * np.abs(rw), n * EPS32 * cb + acc * EPS32 * np.abs(rb)
            worst = max(worst, check(tag + " dw", kind, dwd, rw, gw))
            if with_db:
                worst = max(worst, check(tag + " db", kind, dbd, rb, gb))
            else:
                assert np.array_equal(host(dbd), prev_b), "db = None: nothing may be written"
    return worst


@pytest.mark.parametrize("kind,scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", S.WGRAD, ids=str)
def test_conv_c1_wgrad(shape, kind, scale):
    """gate (n + 1) x 2^-24 x sum |dy x| with n = rows_per_thread + rt_n, the longest fp32 chain (c1_spec.c1_wgrad_geom), plus
    2^-24 |previous + result| when accumulating"""
    B, H, W, Co = shape
    d = data(kind, B, H, W, Co, scale)
    r = np.random.RandomState(7)
    if kind == "int":
        pw, pb = r.randint(-3, 4, (Co, 9)).astype(np.float32), r.randint(-3, 4, Co).astype(np.float32)
    else:
        pw, pb = (r.randn(Co, 9) * scale * scale).astype(np.float32), (r.randn(Co) * scale).astype(np.float32)
    worst = wgrad_cases(kind, d, d.dy.astype(np.float32), shape, pw, pb)
    print(f"conv_c1_wgrad {shape} {kind} x{scale:g}: worst error / gate {worst:.3f}")


def test_conv_c1_wgrad_more_than_32_rows_per_thread():
    """1,179,648 pixels at Co = 128: rows_per_thread = 36 on 4096 blocks; exact data, sums up to 3 M < 2^24"""
    B, H, W, Co = S.WGRAD_BIG
    d = S.int_data(B, H, W, Co)
    r = np.random.RandomState(8)
    wgrad_cases("int", d, d.dy, S.WGRAD_BIG, r.randint(-3, 4, (Co, 9)).astype(np.float32), r.randint(-3, 4, Co).astype(np.float32))


# ----------------------------------------------------------------------------- input gradient
@pytest.mark.parametrize("kind,scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", S.DGRAD, ids=str)
def test_conv_c1_dgrad(shape, kind, scale):
    """the 8 x 64 tiled kernel at full and partial tiles, plain and accumulating; gate 9 Co x 2^-24 x sum |dy w| (+ 2^-24 |previous +
    result| when accumulating)"""
    from qea import ops
    B, H, W, Co = shape
    M = B * H * W
    d = data(kind, B, H, W, Co, scale)
    dy = d.dy.astype(np.float32)
    dx, cond = S.conv_dgrad(dy, d.w)
    r = np.random.RandomState(9)
    prev = r.randint(-3, 4, (B, H, W)).astype(np.float32) if kind == "int" else (r.randn(B, H, W) * scale).astype(np.float32)
    worst = 0.0
    for (ld, off), acc in itertools.product(layouts(Co), (False, True)):
        dyd = strided(dy.reshape(M, Co), ld, off, NAN)[1]
        buf, dxd = guarded(prev)
        ops.conv_c1_dgrad(dyd, ld, dev(d.w), dxd, B, H, W, Co, accumulate=acc)
        torch.cuda.synchronize()
        assert guards_hold(buf)
        ref = dx + prev if acc else dx
        worst = max(worst, check(f"dgrad {shape} ld={ld} accumulate={acc}", kind, dxd, ref, 9 * Co * EPS32 * cond + acc * EPS32 * np.abs(ref)))
    print(f"conv_c1_dgrad {shape} {kind} x{scale:g}: worst error / gate {worst:.3f}")


# ----------------------------------------------------------------------------- conv -> ReLU -> pool backward from the pooled gradient
def pool_bwd_reference(d, dpool, bias):
    """the statement, image by image where the shape is large (the images are independent; dw and db add)"""
    B = d.x.shape[0]
    if d.x.size < 10 ** 5:
        return S.conv_pool_bwd(d.x, d.w, bias, dpool)
    parts = [S.conv_pool_bwd(d.x[b:b + 8], d.w, bias, dpool[b:b + 8])[:4] for b in range(0, B, 8)]
    return S.PoolBwd(np.concatenate([p[0] for p in parts]), sum(p[1] for p in parts), sum(p[2] for p in parts),
                     np.concatenate([p[3] for p in parts]), None, None, None, None, None)


def run_pool_bwd(kind, shape, scale=1.0):
    from qea import ops
    B, H, W = shape
    Co, NW, M = 64, B * (H // 2) * (W // 2), B * H * W
    d = data(kind, B, H, W, Co, scale)
    dpool = S.pool_dpool(B, H, W, Co, kind, scale)
    xd, wd, bd = image(d.x), dev(d.w), dev(d.bias)
    rs = np.random.RandomState(10)
    if kind == "int":
        pw, pb = rs.randint(-3, 4, (Co, 9)).astype(np.float32), rs.randint(-3, 4, Co).astype(np.float32)
    else:
        pw, pb = (rs.randn(Co, 9) * scale * scale).astype(np.float32), (rs.randn(Co) * scale).astype(np.float32)
    n = 4 * S.c1pb_win_per_wave(NW) + 1
    worst, n_und = 0.0, 0
    big = M > 10 ** 5
    for with_bias in (True, False):
        r = pool_bwd_reference(d, dpool, d.bias if with_bias else None)
        und = np.zeros(dpool.shape, dtype=bool) if kind == "int" else S.undecided(r.pre, r.cond_pre)
        sw, sb, sx = S.undecided_slack(d.x, d.w, dpool, und)
        n_und = max(n_und, int(und.sum()))
        # (dx, dw, accumulate): everything; no dx; dx alone; accumulate (dw and db only: dx is overwritten)
        forms = ((True, True, False), (False, True, False), (True, False, False), (True, True, True)) if with_bias else ((True, True, False),)
        for (with_dx, with_dw, acc), (ld, off) in itertools.product(forms, layouts(Co)[1:] if big else layouts(Co)):
            gbuf, g = strided(dpool.reshape(NW, Co), ld, off, NAN)
            wbuf, dwd = guarded(pw)
            bbuf, dbd = guarded(pb)
            xbuf, dxd = guarded(np.full((B, H, W), SENTINEL))
            ops.conv_c1_pool_bwd(xd, wd, bd if with_bias else None, g, ld, dwd if with_dw else None, dbd if with_dw else None,
                                 dxd if with_dx else None, B, H, W, Co, accumulate=acc)
            torch.cuda.synchronize()
            tag = f"pool_bwd {shape} {kind} bias={with_bias} dx={with_dx} dw={with_dw} accumulate={acc} ld={ld}"
            assert pads_hold(gbuf, Co, off, NAN) and guards_hold(wbuf) and guards_hold(bbuf) and guards_hold(xbuf), tag
            # the masked gradient: bit for bit in both kinds; an undecided window may hold its gradient or zero
            got, ref, raw = host(g), r.masked.reshape(NW, Co), dpool.reshape(NW, Co)
            u = und.reshape(NW, Co)
            assert np.array_equal(got[~u], ref[~u].astype(np.float32)) and ((got[u] == raw[u]) | (got[u] == 0)).all(), tag
            if with_dw:
                rw, rb = (r.dw + pw, r.db + pb) if acc else (r.dw, r.db)
                gw = gb = None
                if kind != "int":
                    gw, gb = n * EPS32 * r.cond_w + acc * EPS32 * np.abs(rw) + sw, n * EPS32 * r.cond_b + acc * EPS32 * np.abs(rb) + sb
                worst = max(worst, check(tag + " dw", kind, dwd, rw, gw), check(tag + " db", kind, dbd, rb, gb))
            else:
                assert np.array_equal(host(dwd), pw) and np.array_equal(host(dbd), pb), tag
            if with_dx:
                worst = max(worst, check(tag + " dx", kind, dxd, r.dx, None if kind == "int" else 9 * Co * EPS32 * r.cond_x + sx))
            else:
                assert bool((dxd == SENTINEL).all()), tag
    print(f"conv_c1_pool_bwd {shape} {kind} x{scale:g}: worst error / gate {worst:.3f}, {n_und} of {dpool.size} windows undecided")


@pytest.mark.parametrize("kind,scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", S.POOL_BWD, ids=str)
def test_conv_c1_pool_bwd(shape, kind, scale):
    """window counts that are no multiple of 64 (a partly filled wave, empty waves, a partly filled second block); with and without
    dx, dw, bias; accumulate.  Gates: dw, db (n + 1) x 2^-24 x cond with n = 4 x win_per_wave; dx 9 Co x 2^-24 x cond."""
    run_pool_bwd(kind, shape, scale)


def test_conv_c1_pool_bwd_waves_that_start_mid_row_and_cross_images():
    """132,096 windows: win_per_wave = 20 against rows of 64 windows and images of 1024; exact data"""
    run_pool_bwd("int", S.POOL_BWD_BIG)


# ----------------------------------------------------------------------------- head
@pytest.mark.parametrize("C", S.HEAD_C)
@pytest.mark.parametrize("M", S.HEAD_M)
def test_head_fwd_bwd(M, C):
    """sigmoid(x w + b) and its backward at ldx, lddx in {C, 2C}, accumulate both ways.  Forward gate: c1_spec.head_fwd.  Backward (from
    the device's own fp32 y): dx 4 x 2^-24 |ref|, dw 5 x 2^-24 sum |dz x|, db 4 x 2^-24 sum |dz| (+ 2^-24 |previous + result| when
    accumulating); on the int kind dz is -1, 0 or 1 and the backward is exact."""
    from qea import ops
    worst = dict(y=0.0, dx=0.0, dw=0.0, db=0.0)
    for kind, scale in KINDS:
        x, w, b, dyy, y32 = S.head_data(M, C, kind, scale)
        wd, bd = dev(w), dev(np.asarray([b], dtype=np.float32))
        yref, ygate = S.head_fwd(x, w, b)
        rs = np.random.RandomState(11)
        pw = rs.randint(-3, 4, C).astype(np.float32) if kind == "int" else (rs.randn(C) * scale * scale).astype(np.float32)
        pb = np.asarray([2.0 if kind == "int" else 0.3 * scale], dtype=np.float32)
        for (ldx, offx), (lddx, offdx), acc in itertools.product(layouts(C), layouts(C), (False, True)):
            xd = strided(x, ldx, offx, NAN)[1]
            ybuf, yd = guarded(np.full(M, SENTINEL))
            ops.head_fwd(xd, ldx, wd, bd, yd, M, C)
            torch.cuda.synchronize()
            assert guards_hold(ybuf)
            worst["y"] = max(worst["y"], check(f"head_fwd M={M} C={C} {kind} ldx={ldx}", "real", yd, yref, ygate))
            y_in = yd if y32 is None else dev(y32)
            r = S.head_bwd(x, host(y_in), dyy, w)
            dbuf, dxd = out_buf(M, C, lddx, offdx)
            wbuf, dwd = guarded(pw)
            bbuf, dbd = guarded(pb)
            ops.head_bwd(xd, ldx, y_in, dev(dyy), wd, dxd, lddx, dwd, dbd, M, C, accumulate=acc)
            torch.cuda.synchronize()
            tag = f"head_bwd M={M} C={C} {kind} ldx={ldx} lddx={lddx} accumulate={acc}"
            assert pads_hold(dbuf, C, offdx) and guards_hold(wbuf) and guards_hold(bbuf), tag
            rw, rb = (r.dw + pw, r.db + pb) if acc else (r.dw, np.asarray([r.db]))
            worst["dx"] = max(worst["dx"], check(tag + " dx", kind, dxd, r.dx, 4 * EPS32 * np.abs(r.dx)))
            worst["dw"] = max(worst["dw"], check(tag + " dw", kind, dwd, rw, 5 * EPS32 * r.cond_w + acc * EPS32 * np.abs(rw)))
            worst["db"] = max(worst["db"], check(tag + " db", kind, dbd, rb, 4 * EPS32 * r.cond_b + acc * EPS32 * np.abs(rb)))
    print(f"head M={M} C={C}: worst error / gate " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- max-pool
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("window", S.POOL_WINDOWS, ids=str)
@pytest.mark.parametrize("shape", S.POOL_SHAPES, ids=str)
def test_maxpool_fwd_bwd(shape, window):
    """bit for bit against the statement on data with NaN, +-inf, +-0 ties and positive ties; contiguous and as the second half of a
    2C-wide buffer (x, the pooled tensor and dx alike); relu_mask and accumulate both ways; the abs-max slot from zero, from above the
    result (left alone) and from below it (raised)"""
    from qea import ops
    (kh, kw), (B, H, W, C) = window, shape
    x, dy = S.pool_data(B, H, W, C, kh, kw)
    M, OM = B * H * W, B * (H // kh) * (W // kw)
    pooled, _ = S.pool(x, kh, kw)
    prev = (np.random.RandomState(12).randn(B, H, W, C) * 0.5).astype(np.float32)

    def slots(run, want):
        for start, end in ((0.0, want), (2 * want + 1, 2 * want + 1), (0.5 * want, want)):
            slot = torch.full((1,), start, device=DEV)
            run(slot)
            torch.cuda.synchronize()
            assert float(slot.item()) == float(np.float32(end)), (shape, window, start, want, float(slot.item()))

    for ld, off in layouts(C):
        xd = strided(x.reshape(M, C), ld, off, NAN)[1]
        ybuf, yd = out_buf(OM, C, ld, off)
        ops.maxpool_fwd(xd, ld, yd, ld, B, H, W, C, kh, kw)
        torch.cuda.synchronize()
        assert pads_hold(ybuf, C, off) and np.array_equal(bits(host(yd)), bits(pooled.reshape(OM, C))), (shape, window, ld)
        slots(lambda s: ops.maxpool_fwd(xd, ld, yd, ld, B, H, W, C, kh, kw, amax=s), S.amax(pooled))
        dyd = strided(dy.reshape(OM, C), ld, off, NAN)[1]
        for relu_mask, acc in itertools.product((False, True), (False, True)):
            routed = S.pool_bwd(x, dy, kh, kw, relu_mask)
            ref = (prev + routed) if acc else routed                    # one fp32 add: IEEE decides its bits
            assert ref.dtype == np.float32

            def run(slot, keep=None):
                dbuf, dxd = strided(prev.reshape(M, C), ld, off, SENTINEL) if acc else out_buf(M, C, ld, off)
                ops.maxpool_bwd(xd, ld, dyd, ld, dxd, ld, B, H, W, C, kh, kw, relu_mask=relu_mask, accumulate=acc, amax=slot)
                if keep is not None:
                    keep.extend((dbuf, dxd))

            kept = []
            run(None, kept)
            torch.cuda.synchronize()
            tag = (shape, window, ld, relu_mask, acc)
            assert pads_hold(kept[0], C, off), tag
            assert np.array_equal(bits(host(kept[1])), bits(ref.reshape(M, C))), tag
            slots(run, S.amax(ref))
    assert np.isnan(pooled).any() and np.isinf(pooled).any() and (pooled > 0).any()
    assert C < 64 or (np.signbit(pooled[pooled == 0]).any() and not np.signbit(pooled[pooled == 0]).all())      # windows of zeros kept -0.0 and +0.0


# ----------------------------------------------------------------------------- refusals: before any launch
def test_refusals_name_the_reason_and_write_nothing():
    from qea import _lib, ops
    z = functools.partial(torch.zeros, device=DEV)
    full = functools.partial(torch.full, fill_value=SENTINEL, device=DEV)
    for H, W, Co in ((4, 12, 64), (4, 8, 32)):                           # W % 8 != 0; Co = 32
        g, dw, db, dx = full((H * W // 4, Co)), full((Co, 9)), full((Co,)), full((1, H, W))
        with pytest.raises(_lib.QeaError, match="needs Co == 64, even H, W % 8 == 0"):
            ops.conv_c1_pool_bwd(z(1, H, W), z(Co, 9), z(Co), g, Co, dw, db, dx, 1, H, W, Co)
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (g, dw, db, dx))
    dx = full((1, 4, 8))
    with pytest.raises(_lib.QeaError, match=r"Co=48 not in \{32,64,128\}"):
        ops.conv_c1_dgrad(z(32, 48), 48, z(48, 9), dx, 1, 4, 8, 48)
    y, dxh, dw, db = full((8,)), full((8, 48)), full((48,)), full((1,))
    with pytest.raises(_lib.QeaError, match=r"qea_head_fwd: C=48 not in \{32,64\}"):
        ops.head_fwd(z(8, 48), 48, z(48), z(1), y, 8, 48)
    with pytest.raises(_lib.QeaError, match=r"qea_head_bwd: C=48 not in \{32,64\}"):
        ops.head_bwd(z(8, 48), 48, z(8), z(8), z(48), dxh, 48, dw, db, 8, 48)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (dx, y, dxh, dw, db))
