"""Every descriptor field of qea_conv_igemm / qea_conv_wgrad on every tile, against the fp64 statement of tests/conv_spec.py.

Each device operand is a view into a larger allocation filled with NaN (conv_spec.Operand: guard bands of 256 rows in front and
behind, NaN and inf between the channel slices); outputs start as NaN, or as y_prev / dw_prev under accumulate.  After a launch the
written slice is compared with the spec and EVERY other byte of the allocation must be bit-unchanged, so a read outside a slice shows
up as NaN in the result (a neighbour channel times a zero weight included) and a store outside it is seen, while no access a wrong
kernel could make leaves the allocation.  The inputs are checked bit-unchanged once all launches of a test are through.

Gates: the project's own (CONV_GATE 2e-6, WGRAD_GATE 3e-5 of tests/test_operand_scale_gpu.py) times the case's max |spec| (of the total
under accumulate), no absolute floor, no element excluded; where the mask is not > 0 and accumulate is off the stored value is exactly
0.  The worst error / gate per (family, case) is printed (pytest -s) for the table in DESIGN.md section 4.  Every test runs in the
session's mode (split_f16, QEA_SPLIT=bf16, QEA_MFMA=f32); the operand forms of the split tiles are selected as
test_presplit_planes_bit_identical does (ops.PRESPLIT, ops.set_mfma_mode)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import conv_spec as cs

pytestmark = pytest.mark.gpu

CONV_F32_TILES = (1, 2, 3, 5, 6, 7, 8, 9)
CONV_SPLIT_TILES = (20, 21, 22, 23, 25)
WGRAD_F32_TILES = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11)
WGRAD_SPLIT_TILES = (20, 21, 22)
# operand forms of the split conv tiles: name -> (mfma mode, PRESPLIT["on"], PRESPLIT["x"]); None = as the session runs them
CONV_FORMS = {"session": None, "on the fly": ("split_bf16", False, False), "hybrid bf16": ("split_bf16", True, False),
              "hybrid fp16": ("split_f16", True, False), "both pre-split": ("split_bf16", True, True)}

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    from qea import ops
    print(f"\nconv-descriptor summary, mode {ops.mfma_mode()}: worst error / gate")
    for fam, case in sorted(WORST):
        print(f"  {fam:34s} {case:22s} {WORST[fam, case]:.3g}")


@contextlib.contextmanager
def _form(form):
    from qea import ops
    if form is None:
        yield
        return
    mode, on, x = form
    prev = ops.set_mfma_mode(mode)
    ops.PRESPLIT["on"], ops.PRESPLIT["x"] = on, x
    try:
        yield
    finally:
        ops.PRESPLIT["on"], ops.PRESPLIT["x"] = True, False
        ops.set_mfma_mode(prev)


def _up(op):
    return torch.from_numpy(op.buf).cuda()


def _at(t, op):
    """the device view whose data pointer is the first float of the slice"""
    return t[op.base:]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _unchanged(t, op):
    return np.array_equal(_bits(t.cpu().numpy()), _bits(op.buf))


def _slot(value):
    """a one-float abs-max slot as an Operand (NaN around it)"""
    return cs.Operand(1, 4).set([value, 0, 0, 0])


def _sl(op, flat):
    return np.asarray(flat)[op.guard:op.guard + op.rows * op.ld].reshape(op.rows, op.ld)[:, op.off:op.off + op.width]


def _judge(family, case, what, got, before, spec, written, gate, fails, zero_at=None):
    """got / before: the allocation after / before the launch (fp32, flat); spec: its fp64 statement; written: the stores.
    Appends one line per broken property to `fails`; keeps the worst error / gate of (family, case)."""
    if not np.array_equal(_bits(got)[~written], _bits(before)[~written]):
        n = int((_bits(got)[~written] != _bits(before)[~written]).sum())
        fails.append(f"{family} / {case} / {what}: {n} floats outside the written slice changed")
    g, s = got[written].astype(np.float64), spec[written]
    top = np.abs(s).max()
    with np.errstate(invalid="ignore"):
        err = np.abs(g - s)
    if not np.isfinite(err).all():
        fails.append(f"{family} / {case} / {what}: {int((~np.isfinite(err)).sum())} of {err.size} written values are not finite")
        ratio = float("inf")
    else:
        ratio = float(err.max() / (gate * top))
        if ratio > 1.0:
            fails.append(f"{family} / {case} / {what}: max error {err.max():.3e} = {ratio:.3g} x gate ({gate:g} * {top:.3g})")
    if zero_at is not None and not (got[zero_at] == 0).all():
        fails.append(f"{family} / {case} / {what}: a masked-off value is not exactly 0")
    WORST[family, case] = max(WORST.get((family, case), 0.0), ratio)
    return ratio


# ----------------------------------------------------------------------------- conv
class _ConvDev:
    def __init__(self, name):
        self.c = c = cs.conv_case(name)
        self.x, self.w = _up(c.x), _up(c.w)
        self.scale, self.bias, self.mask = (_up(o) if o else None for o in (c.scale, c.bias, c.mask))
        self.xmax_op = _slot(np.abs(c.x.view()).max())
        self.xmax = _up(self.xmax_op)
        self.ymax_op = _slot(0.0)                                            # y_absmax: a zero-filled slot the launch raises
        self.spec, self.written = cs.conv_case_spec(name)
        self.zero_at = None
        if c.mask and not c.d.accumulate:
            z = np.zeros(c.y.buf.shape, dtype=bool)
            _sl(c.y, z)[...] = ~(c.mask.view() > 0)
            self.zero_at = z

    def launch(self, tile, x_amax=False):
        """-> the y allocation and the y_absmax slot's allocation after the launch (numpy)"""
        from qea import ops
        c, d = self.c, self.c.d
        y, ymax = _up(c.y), _up(self.ymax_op)
        ops.conv_igemm(_at(self.x, c.x), _at(self.w, c.w), _at(y, c.y), B=d.B, H=d.H, W=d.W, Cin=d.Cin, OH=d.OH, OW=d.OW, N=d.N, KH=d.KH, KW=d.KW,
                       pad=(d.pad_h, d.pad_w), stride=(d.stride_h, d.stride_w), ldx=d.ldx, ldy=d.ldy,
                       scale=_at(self.scale, c.scale) if c.scale else None, bias=_at(self.bias, c.bias) if c.bias else None,
                       mask=_at(self.mask, c.mask) if c.mask else None, ldmask=d.ldmask, relu=bool(d.relu), accumulate=bool(d.accumulate),
                       out_mode=d.out_mode, tile=tile, x_amax=_at(self.xmax, self.xmax_op)[:1] if x_amax else None,
                       y_amax=_at(ymax, self.ymax_op)[:1])
        return y.cpu().numpy(), ymax.cpu().numpy()

    def judge(self, family, what, got, fails):
        """the y allocation against the spec; the y_absmax slot = the largest finite |stored value|, to the bit, nothing around it touched"""
        got, ymax = got
        stored = np.abs(got[self.written])
        want = self.ymax_op.buf.copy()
        want[self.ymax_op.base] = stored[np.isfinite(stored)].max(initial=0.0)
        if not np.array_equal(_bits(ymax), _bits(want)):
            fails.append(f"{family} / {self.c.name} / {what}: y_absmax is {ymax[self.ymax_op.base]!r}, the stored values' is {want[self.ymax_op.base]!r}"
                         " (or its neighbours changed)")
        return _judge(family, self.c.name, what, got, self.c.y.buf, self.spec, self.written, cs.CONV_GATE, fails, self.zero_at)

    def inputs_unchanged(self, fails):
        c = self.c
        for nm, t, op in (("x", self.x, c.x), ("w", self.w, c.w), ("scale", self.scale, c.scale), ("bias", self.bias, c.bias),
                          ("mask", self.mask, c.mask), ("x_absmax", self.xmax, self.xmax_op)):
            if op is not None and not _unchanged(t, op):
                fails.append(f"{c.name}: the {nm} allocation changed")


@pytest.mark.parametrize("name", list(cs.CONV_CASES))
def test_conv_fields_on_the_fp32_tiles(name):
    dev, fails = _ConvDev(name), []
    for tile in CONV_F32_TILES:
        r = dev.judge("conv fp32 tiles 1-9", f"tile {tile}", dev.launch(tile), fails)
        print(f"conv {name} tile {tile}: worst error / gate = {r:.3g}")
    dev.inputs_unchanged(fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(cs.CONV_CASES))
def test_conv_fields_on_the_split_tiles_in_every_operand_form(name):
    dev, fails = _ConvDev(name), []
    for fname, form in CONV_FORMS.items():
        for tile in CONV_SPLIT_TILES:
            with _form(form):
                got = dev.launch(tile, x_amax=fname == "hybrid fp16")        # (the caller's slot, from a NaN-guarded allocation)
            r = dev.judge(f"conv split tiles, {fname}", f"tile {tile}", got, fails)
            print(f"conv {name} tile {tile} {fname}: worst error / gate = {r:.3g}")
    dev.inputs_unchanged(fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(cs.CONV_CASES))
def test_conv_fields_on_the_automatic_tile(name):
    from qea import ops
    dev, fails = _ConvDev(name), []
    ops.prof_enable(ops.PROF_CONV_IGEMM, True)
    try:
        ops.prof_reset()
        got = dev.launch(0)
        torch.cuda.synchronize()
        ran = [t for t in CONV_F32_TILES + CONV_SPLIT_TILES + (4, 26) if ops.prof_read_tagged(ops.PROF_CONV_IGEMM, t)["launches"] == 1]
    finally:
        ops.prof_enable(ops.PROF_CONV_IGEMM, False)
    assert len(ran) == 1, f"{name}: tile 0 ran on none or several of the tiles this case can take: {ran}"
    r = dev.judge("conv tile 0", f"tile 0 -> {ran[0]}", got, fails)
    print(f"conv {name} tile 0 ran on tile {ran[0]} ({ops.mfma_mode()}): worst error / gate = {r:.3g}")
    dev.inputs_unchanged(fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tile,switch,message", [(4, "accumulate", r"tile 4 \(LDS-halo 3x3\) needs"), (4, "mask", r"tile 4 \(LDS-halo 3x3\) needs"),
                                                 (24, "accumulate", "tile 24 needs"), (26, "accumulate", "tile 26 needs"),
                                                 (26, "scale", "tile 26 needs"), (26, "mask", "tile 26 needs")])
def test_conv_tiles_refuse_what_they_cannot_take(tile, switch, message):
    """the LDS-halo kernels have no accumulate (tile 4: no mask either), the 1x1 LDS tile no scale / mask / accumulate: a forced launch
    is refused with the tile's message before anything runs, the output allocation stays bit-unchanged"""
    from qea import _lib, ops
    rng = np.random.default_rng(tile)
    if tile == 26:
        B, H, W, Cin, N, k, pad = 1, 1, 40, 64, 128, 1, 0
    else:
        B, H, W, Cin, N, k, pad = 1, 8, 32, 32, 32, 3, 1
    M = B * H * W
    x = cs.Operand(M, Cin, Cin + 32, 32).set(rng.standard_normal((M, Cin)))
    w = cs.Operand(N, k * k * Cin).set(rng.standard_normal((N, k * k * Cin)))
    y = cs.Operand(M, N, N + 8, 4).set(rng.standard_normal((M, N)))
    extra = cs.Operand(M, N, N + 8, 4).set(rng.standard_normal((M, N))) if switch == "mask" else cs.Operand(1, N).set(rng.random(N) + 0.5)
    xd, wd, yd, ed = _up(x), _up(w), _up(y), _up(extra)
    kw = {"accumulate": dict(accumulate=True), "scale": dict(scale=_at(ed, extra)), "mask": dict(mask=_at(ed, extra), ldmask=extra.ld)}[switch]
    prev = ops.set_mfma_mode("split_f16")
    try:
        with pytest.raises(_lib.QeaError, match=message):
            ops.conv_igemm(_at(xd, x), _at(wd, w), _at(yd, y), B=B, H=H, W=W, Cin=Cin, OH=H, OW=W, N=N, KH=k, KW=k, pad=(pad, pad), ldx=x.ld, ldy=y.ld,
                           tile=tile, **kw)
    finally:
        ops.set_mfma_mode(prev)
    torch.cuda.synchronize()
    assert _unchanged(yd, y), "a refused launch wrote the output allocation"
    assert _unchanged(xd, x) and _unchanged(wd, w) and _unchanged(ed, extra)


# ----------------------------------------------------------------------------- wgrad
class _WgradDev:
    def __init__(self, name):
        self.c = c = cs.wgrad_case(name)
        d = c.d
        self.p, self.q = _up(c.p), _up(c.q)
        self.pmax_op, self.qmax_op = _slot(np.abs(c.p.view()).max()), _slot(np.abs(c.q.view()).max())
        self.pmax, self.qmax = _up(self.pmax_op), _up(self.qmax_op)
        self.dw_op = {acc: cs.Operand(d.R, d.KH * d.KW * d.C) for acc in (False, True)}     # NaN / dw_prev
        self.db_op = {acc: cs.Operand(1, d.R) for acc in (False, True)}
        self.dw_op[True].set(c.dw_prev)
        self.db_op[True].set(c.db_prev)

    def args(self, dw, db, acc, splits, tile, amax):
        c, d = self.c, self.c.d
        return (_at(self.p, c.p), _at(self.q, c.q), _at(dw, self.dw_op[acc])), dict(
            B=d.B, PH=d.PH, PW=d.PW, QH=d.QH, QW=d.QW, R=d.R, Cc=d.C, KH=d.KH, KW=d.KW, pad=(d.pad_h, d.pad_w), stride=(d.stride_h, d.stride_w),
            ldp=d.ldp, ldq=d.ldq, accumulate=acc, splits=splits, tile=tile, dbias=_at(db, self.db_op[acc]),
            p_amax=_at(self.pmax, self.pmax_op)[:1] if amax else None, q_amax=_at(self.qmax, self.qmax_op)[:1] if amax else None)

    def run(self, family, tile, splits, acc, amax, fails):
        from qea import ops
        c, d = self.c, self.c.d
        dw, db = _up(self.dw_op[acc]), _up(self.db_op[acc])
        a, kw = self.args(dw, db, acc, splits, tile, amax)
        ops.conv_wgrad(*a, **kw)
        what = f"tile {tile} splits {splits} accumulate {int(acc)} abs-max {int(amax)}"
        sdw, sdb = cs.wgrad_case_spec(c.name, None, splits)
        for nm, t, op, s, prev in (("dw", dw, self.dw_op[acc], sdw, c.dw_prev), ("dbias", db, self.db_op[acc], sdb, c.db_prev)):
            spec = op.buf.astype(np.float64)
            _sl(op, spec)[...] = (s + prev.astype(np.float64) if acc else s).reshape(op.rows, op.width)
            r = _judge(family if nm == "dw" else "wgrad dbias (colsum or fused)", c.name, f"{what} {nm}", t.cpu().numpy(), op.buf, spec, op.inside(),
                       cs.WGRAD_GATE, fails)
            if nm == "dw":
                print(f"wgrad {c.name} {what}: worst error / gate = {r:.3g}")

    def inputs_unchanged(self, fails):
        c = self.c
        for nm, t, op in (("p", self.p, c.p), ("q", self.q, c.q), ("p_absmax", self.pmax, self.pmax_op), ("q_absmax", self.qmax, self.qmax_op)):
            if not _unchanged(t, op):
                fails.append(f"{c.name}: the {nm} allocation changed")


@pytest.mark.parametrize("name", cs.GENERIC_WGRAD_CASES)
def test_wgrad_fields_on_the_generic_tiles(name):
    dev, fails = _WgradDev(name), []
    for splits in (1, 3):
        for acc in (False, True):
            for tile in WGRAD_F32_TILES:
                dev.run("wgrad fp32 tiles 1-11", tile, splits, acc, False, fails)
            for tile in WGRAD_SPLIT_TILES:
                with _form(("split_f16", True, False)):
                    dev.run("wgrad split tiles 20-22, fp16", tile, splits, acc, True, fails)
                with _form(("split_bf16", True, False)):                      # no abs-max pointers: the three-way bf16 form
                    dev.run("wgrad split tiles 20-22, bf16", tile, splits, acc, False, fails)
    dev.inputs_unchanged(fails)
    assert not fails, "\n".join(fails)


def _takes(name, tile):
    return not (tile == 6 and cs.WGRAD_CASES[name]["PW"] % 32)              # the fp32 LDS-halo kernel needs PW % 32 == 0


_REFUSAL = {6: r"tile 6 \(LDS-halo\) needs", 23: r"tile 23 \(nine-tap split-bf16\) needs", 29: r"tile 23 \(nine-tap split-bf16\) needs"}


@pytest.mark.parametrize("name", cs.PIXEL_TILE_WGRAD_CASES)
def test_wgrad_slices_on_the_pixel_tile_kernels(name):
    """the fp32 LDS-halo kernel (6) and the nine-tap kernel in its producer / consumer or ring form (23, R = C = 64, abs-max given), its
    every-wave-stages form (29) and its three-way bf16 form (no abs-max), reading channel slices; dbias inside the launch where
    qea_conv_wgrad_fuses_bias says so (ops.conv_wgrad asks), by the column-sum pass otherwise"""
    dev, fails = _WgradDev(name), []
    for splits in (1, 3):
        for acc in (False, True):
            if _takes(name, 6):
                dev.run("wgrad fp32 halo (6)", 6, splits, acc, False, fails)
            for tile in (23, 29):
                with _form(("split_f16", True, False)):
                    dev.run(f"wgrad nine-tap ({tile}), fp16", tile, splits, acc, True, fails)
                with _form(("split_bf16", True, False)):
                    dev.run(f"wgrad nine-tap ({tile}), bf16", tile, splits, acc, False, fails)
    dev.inputs_unchanged(fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,tile", [(n, t) for n in ("asym", "convt", "linear") for t in (6, 23, 29)] + [("slices-32-w16", 6), ("slices-64-w16", 6)])
def test_wgrad_pixel_tile_kernels_refuse_other_geometries(name, tile):
    from qea import _lib, ops
    dev = _WgradDev(name)
    for acc in (False, True):
        dw, db = _up(dev.dw_op[acc]), _up(dev.db_op[acc])
        a, kw = dev.args(dw, db, acc, 1, tile, False)
        with pytest.raises(_lib.QeaError, match=_REFUSAL[tile]):
            ops.conv_wgrad(*a, **kw)
        torch.cuda.synchronize()
        assert _unchanged(dw, dev.dw_op[acc]) and _unchanged(db, dev.db_op[acc]), "a refused launch wrote an output allocation"
    fails = []
    dev.inputs_unchanged(fails)
    assert not fails, fails


def test_the_bias_query_is_what_the_pixel_tile_launch_does():
    """qea_conv_wgrad_fuses_bias: 1 exactly for the producer / consumer nine-tap form (64-channel blocks, both abs-max pointers, not tile 29)"""
    from qea import _lib
    L = _lib.lib()
    slot = torch.ones(2, device="cuda")
    for name in cs.PIXEL_TILE_WGRAD_CASES:
        d = cs.wgrad_case(name).d
        for tile in (6, 23, 29):
            for amax in (False, True):
                wd = _lib.WgradDesc(B=d.B, PH=d.PH, PW=d.PW, QH=d.QH, QW=d.QW, R=d.R, C=d.C, KH=d.KH, KW=d.KW, pad_h=d.pad_h, pad_w=d.pad_w,
                                    stride_h=d.stride_h, stride_w=d.stride_w, ldp=d.ldp, ldq=d.ldq, tile=tile)
                if amax:
                    wd.p_absmax, wd.q_absmax = slot.data_ptr(), slot.data_ptr() + 4
                assert L.qea_conv_wgrad_fuses_bias(C.byref(wd)) == int(tile == 23 and amax and d.R == 64), (name, tile, amax)
