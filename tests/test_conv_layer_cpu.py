"""qea/conv.py held to torch: every descriptor a Conv record hands to ops.conv_igemm / ops.conv_wgrad — forward, input gradient (or the
adjoint scatter) and weight gradient of one geometry — is evaluated with the fp64 statement of those entry points (tests/conv_spec.py)
and must give torch's conv2d / conv_transpose2d and their autograd gradients in float64.  The four ops functions are replaced by
recorders (the derived filters are made on the host by the formulas of their docstrings), the operands live in conv_spec.Operand
allocations so that a wrong pixel stride or plane reads NaN.  The operands are handed over as qea/act.py records: what a record states
(pixel stride, abs-max slot, pooled output, mask) must be what the launch is given, its views must share its slot, and a record that
is not the layer's is refused before any launch.  qea/batchnorm.py's forward / backward are held to the same with recorders for the
ops.bn_* functions.  No GPU, nothing of the library."""
import inspect
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_spec as cs
from qea import batchnorm, conv, ops
from qea.act import Act

RETURNED = ("partials", 3)          # what the conv_igemm stand-in returns: the methods hand it back
REL = 1e-12          # times max |reference|: the gate tests/test_conv_spec_cpu.py holds the same statement to


@pytest.fixture
def calls(monkeypatch):
    """the ops functions qea/conv.py may call, replaced: -> the list of (name, positional tensors, keywords) they were called with"""
    log = []

    def flip_transposed(w, Co, Ci, KH, KW):
        log.append(("flip_transposed", (w,), dict(Co=Co, Ci=Ci, KH=KH, KW=KW)))
        return w.reshape(Co, KH, KW, Ci).flip(1, 2).permute(3, 1, 2, 0).contiguous()      # wt[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci]

    def transposed(w, R, Cc):
        log.append(("transposed", (w,), dict(R=R, Cc=Cc)))
        return w.reshape(R, Cc).t().contiguous()                                          # out[c][r] = w[r][c]

    monkeypatch.setattr(ops, "flip_transposed", flip_transposed)
    monkeypatch.setattr(ops, "transposed", transposed)
    monkeypatch.setattr(ops, "conv_igemm", lambda x, w, y, **kw: log.append(("conv_igemm", (x, w, y), kw)) or RETURNED)
    monkeypatch.setattr(ops, "conv_wgrad", lambda p, q, dw, **kw: log.append(("conv_wgrad", (p, q, dw), kw)))
    monkeypatch.setattr(ops, "conv_can_pool", lambda **kw: log.append(("conv_can_pool", (), kw)) or True)
    return log


def _operand(rng, rows, width, ld=None, off=0, fill=True):
    """-> (the Operand, its slice as the record a caller would pass: the strided host tensor, with an abs-max slot of its own)"""
    op = cs.Operand(rows, width, ld, off)
    if fill:
        op.set(rng.standard_normal((rows, width)))
    return op, Act(torch.from_numpy(op.buf)[op.base:].as_strided((rows, width), (op.ld, 1)), amax=torch.zeros(1))


def _carries(call, **fields):
    """the recorded keywords are the records' fields (tensors and None: the same objects)"""
    for k, v in fields.items():
        got = call[2][k]
        assert (got is v) if (v is None or torch.is_tensor(v)) else (got == v), (call[0], k, got, v)


def _place(t, op):
    """descriptor fields of a strided operand: the recorded tensor must be the slice of `op`'s allocation, found by its storage offset"""
    assert t.untyped_storage().data_ptr() == torch.from_numpy(op.buf).untyped_storage().data_ptr()
    return t.storage_offset(), 0


def _run_igemm(call, x_op, y_op, bias=None):
    """the recorded conv_igemm call under the fp64 statement -> the output slice [rows][width] of y_op"""
    name, (x, w, y), kw = call
    assert name == "conv_igemm"
    d = types.SimpleNamespace(**{k: kw[k] for k in ("B", "H", "W", "Cin", "OH", "OW", "N", "KH", "KW", "ldx", "ldy")},
                              pad_h=kw.get("pad", (0, 0))[0], pad_w=kw.get("pad", (0, 0))[1], stride_h=kw.get("stride", (1, 1))[0],
                              stride_w=kw.get("stride", (1, 1))[1], ldmask=0, relu=0, accumulate=0, out_mode=kw.get("out_mode", cs.OUT_NHWC))
    (d.x_guard, d.x_off), (d.y_guard, d.y_off) = _place(x, x_op), _place(y, y_op)
    out, written = cs.conv_igemm_spec(d, x_op.buf, w.numpy().reshape(d.N, d.KH, d.KW, d.Cin), None, bias, None, y_op.buf)
    assert np.array_equal(written, y_op.inside()), "the launch stores exactly the output slice"
    got = out[y_op.guard:y_op.guard + y_op.rows * y_op.ld].reshape(y_op.rows, y_op.ld)[:, y_op.off:y_op.off + y_op.width]
    assert np.isfinite(got).all()
    return got


def _run_wgrad(call, p_op, q_op):
    name, (p, q, dw), kw = call
    assert name == "conv_wgrad"
    d = types.SimpleNamespace(**{k: kw[k] for k in ("B", "PH", "PW", "QH", "QW", "R", "KH", "KW", "ldp", "ldq")}, C=kw["Cc"],
                              pad_h=kw.get("pad", (0, 0))[0], pad_w=kw.get("pad", (0, 0))[1], stride_h=kw.get("stride", (1, 1))[0],
                              stride_w=kw.get("stride", (1, 1))[1], accumulate=0, splits=1)
    (d.p_guard, d.p_off), (d.q_guard, d.q_off) = _place(p, p_op), _place(q, q_op)
    got, _ = cs.conv_wgrad_spec(d, p_op.buf, q_op.buf, None)
    assert tuple(dw.shape) == got.shape and np.isfinite(got).all()
    return got


def _close(got, ref, what):
    ref = ref.detach().numpy()
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max()
    assert err <= REL * np.abs(ref).max(), (what, err)


def _f64(op, *shape):
    return torch.from_numpy(op.view().astype(np.float64)).view(*shape)


# name -> (record, (ldx, off) of the input rows, (ldy, off) of the output rows, out_mode)
LAYERS = {
    "3x3-slices": (lambda: conv.Conv(2, 3, 5, 4, 8, 3, 3, pad=(1, 1)), (12, 8), (20, 4), cs.OUT_NHWC),
    "conv7-tbc": (lambda: conv.Conv(3, 2, 5, 4, 8, 2, 2), (4, 0), (8, 0), cs.OUT_TBC),
    "gemm": (lambda: conv.gemm(7, 8, 4), (8, 0), (4, 0), cs.OUT_NHWC),
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_fwd_dgrad_wgrad_are_torch_in_float64(name, calls):
    make, (ldx, xoff), (ldy, yoff), mode = LAYERS[name]
    cv = make()
    rng = np.random.default_rng(list(LAYERS).index(name) + 1)
    x_op, x = _operand(rng, cv.B * cv.H * cv.W, cv.Cin, ldx, xoff)
    w_op, w = _operand(rng, cv.N, cv.KH * cv.KW * cv.Cin)
    y_op, y = _operand(rng, cv.B * cv.OH * cv.OW, cv.N, ldy, yoff, fill=False)
    dy_op, dy = _operand(rng, cv.B * cv.OH * cv.OW, cv.N, ldy, yoff)            # (the gradient of y, in y's own row order and slice)
    dx_op, dx = _operand(rng, cv.B * cv.H * cv.W, cv.Cin, ldx, xoff, fill=False)
    bias = rng.standard_normal(cv.N)
    dw = torch.empty(cv.N, cv.KH, cv.KW, cv.Cin)
    extra = {"out_mode": mode} if mode != cs.OUT_NHWC else {}
    w = w.t
    assert (x.ld, y.ld, x.C, y.C) == (ldx, ldy, cv.Cin, cv.N)
    assert cv.fwd(x, w, y, bias=torch.from_numpy(bias), **extra) is RETURNED
    assert cv.dgrad(dy, w, dx) is RETURNED
    cv.wgrad(dy, x, dw, accumulate=True)
    assert [c[0] for c in calls] == ["conv_igemm", "flip_transposed", "conv_igemm", "conv_wgrad"]
    fwd, flip, dgrad, wgrad = calls
    assert fwd[1][1] is w and fwd[2]["w_src"][0] == "fwd" and fwd[2]["w_src"][1] is w and fwd[2]["bias"] is not None
    assert flip[1][0] is w and dgrad[2]["w_src"][0] == "flipT" and dgrad[2]["w_src"][1] is w
    assert wgrad[2]["accumulate"] is True and "bias" not in dgrad[2]
    assert fwd[1][0] is x.t and fwd[1][2] is y.t and dgrad[1][0] is dy.t and dgrad[1][2] is dx.t and wgrad[1][:2] == (dy.t, x.t)
    _carries(fwd, ldx=x.ld, ldy=y.ld, x_amax=x.amax, y_amax=y.amax, pool=None)
    _carries(dgrad, ldx=dy.ld, ldy=dx.ld, x_amax=dy.amax, y_amax=dx.amax, mask=None, ldmask=0)
    assert "mask" not in fwd[2] and "pool" not in dgrad[2]                     # (a pool rides behind a forward, a mask in a dgrad only)
    _carries(wgrad, ldp=dy.ld, ldq=x.ld, p_amax=dy.amax, q_amax=x.amax)

    xt = _f64(x_op, cv.B, cv.H, cv.W, cv.Cin).permute(0, 3, 1, 2).requires_grad_()
    wt = _f64(w_op, cv.N, cv.KH, cv.KW, cv.Cin).permute(0, 3, 1, 2).requires_grad_()
    ref = F.conv2d(xt, wt, torch.from_numpy(bias), stride=cv.stride, padding=cv.pad)
    assert tuple(ref.shape) == (cv.B, cv.N, cv.OH, cv.OW)
    rows = (lambda t: t[:, 0].permute(1, 0, 2)) if mode == cs.OUT_TBC else (lambda t: t)      # [B][OH][OW][N] -> the launch's row order
    _close(_run_igemm(fwd, x_op, y_op, bias), rows(ref.permute(0, 2, 3, 1)).reshape(-1, cv.N), name + " fwd")
    # the gradient arrives in NHWC row order whatever order the forward wrote (conv7's comes from the OUT_TBC GEMM of the BiLSTM's)
    ref.backward(_f64(dy_op, cv.B, cv.OH, cv.OW, cv.N).permute(0, 3, 1, 2))
    _close(_run_igemm(dgrad, dy_op, dx_op), xt.grad.permute(0, 2, 3, 1).reshape(-1, cv.Cin), name + " dgrad")
    _close(_run_wgrad(wgrad, dy_op, x_op), wt.grad.permute(0, 2, 3, 1), name + " wgrad")


def test_up_convolution_is_conv_transpose2d_in_float64(calls):
    """the UNet's up-convolution h=2, w=3, dcin=8 -> c=4 into the low half of a 2c-wide row: forward = scatter_adjoint, input gradient =
    the record's fwd, weight gradient = its wgrad(dy = the up-conv's input, x = the gradient of its output)"""
    B, h, w_, dcin, c = 2, 2, 3, 8, 4
    up = conv.Conv(B, 2 * h, 2 * w_, c, dcin, 2, 2, stride=(2, 2))
    assert (up.OH, up.OW) == (h, w_)
    rng = np.random.default_rng(7)
    d_op, d = _operand(rng, B * h * w_, dcin)                                   # the up-conv's input
    w_op, w = _operand(rng, dcin, 4 * c)                                        # [dcin][2][2][c]
    cat_op, cat = _operand(rng, B * 4 * h * w_, c, 2 * c, 0, fill=False)
    dcat_op, dcat = _operand(rng, B * 4 * h * w_, c, 2 * c, 0)
    dd_op, dd = _operand(rng, B * h * w_, dcin, fill=False)
    bias = rng.standard_normal(c)
    dw = torch.empty(dcin, 2, 2, c)
    w = w.t
    assert up.scatter_adjoint(d, w, cat, bias=torch.from_numpy(bias)) is RETURNED
    up.fwd(dcat, w, dd)
    up.wgrad(d, dcat, dw)
    assert [k[0] for k in calls] == ["transposed", "conv_igemm", "conv_igemm", "conv_wgrad"]
    tr, fwd, bwd, wgrad = calls
    assert tr[1][0] is w and fwd[2]["w_src"][0] == "T" and fwd[2]["w_src"][1] is w and fwd[2]["out_mode"] == cs.OUT_CONVT
    assert bwd[1][1] is w and bwd[2]["w_src"][0] == "fwd" and bwd[2]["w_src"][1] is w
    _carries(fwd, ldx=dcin, ldy=2 * c, x_amax=d.amax, y_amax=cat.amax)
    _carries(bwd, ldx=2 * c, ldy=dcin, x_amax=dcat.amax, y_amax=dd.amax, pool=None)
    _carries(wgrad, ldp=dcin, ldq=2 * c, p_amax=d.amax, q_amax=dcat.amax)

    dt = _f64(d_op, B, h, w_, dcin).permute(0, 3, 1, 2).requires_grad_()
    wt = _f64(w_op, dcin, 2, 2, c).permute(0, 3, 1, 2).requires_grad_()          # ConvTranspose2d's [in][out][kh][kw]
    ref = F.conv_transpose2d(dt, wt, torch.from_numpy(bias), stride=2)
    _close(_run_igemm(fwd, d_op, cat_op, bias), ref.permute(0, 2, 3, 1).reshape(-1, c), "up-conv forward")
    ref.backward(_f64(dcat_op, B, 2 * h, 2 * w_, c).permute(0, 3, 1, 2))
    _close(_run_igemm(bwd, dcat_op, dd_op), dt.grad.permute(0, 2, 3, 1).reshape(-1, dcin), "up-conv input gradient")
    _close(_run_wgrad(wgrad, d_op, dcat_op), wt.grad.permute(0, 2, 3, 1), "up-conv weight gradient")


def test_caller_derived_filter_keeps_its_tag(calls):
    """the one path where the caller spells w_src: a filter it derived itself"""
    w, src = torch.zeros(4, 8), torch.zeros(8, 4)
    conv.gemm(7, 8, 4).fwd(Act(torch.zeros(7, 8)), w, Act(torch.zeros(7, 4)), w_src=("catT", src, (src,)))
    assert calls[0][1][1] is w and calls[0][2]["w_src"] == ("catT", src, (src,))


def test_with_batch_rebinds_the_batch_only():
    cv = conv.Conv(6, 3, 5, 4, 8, 3, 3, pad=(1, 1)).with_batch(2)
    assert (cv.B, cv.H, cv.W, cv.Cin, cv.N, cv.KH, cv.KW, cv.pad, cv.stride, cv.OH, cv.OW) == (2, 3, 5, 4, 8, 3, 3, (1, 1), (1, 1), 3, 5)


def test_refusals_come_before_any_launch(calls):
    z, a = torch.zeros(1), Act(torch.zeros(1, 1))
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2, stride=(2, 2)).dgrad(a, z, a)
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2).scatter_adjoint(a, z, a)                                 # stride != kernel
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2, pad=(1, 1), stride=(2, 2)).scatter_adjoint(a, z, a)      # pad != 0
    with pytest.raises(ValueError):
        conv.Conv(2, 5, 6, 4, 8, 2, 2, stride=(2, 2))                                           # (5 - 2) / 2 + 1 is no whole number
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 8, 4, 8, 3, 3, pad=(1, 1), stride=(1, 3))                               # (8 + 2 - 3) / 3 neither
    assert calls == []


# ---------------------------------------------------------------------------------------------------------------- operand records
def _same_slot(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.storage_offset() == b.storage_offset() and a.shape == b.shape


def test_record_views_share_the_slot_and_keep_the_stride():
    slot = ops.AmaxPool("cpu", n=4)
    cat = Act.empty(6, 10, "cpu", slot)
    nxt = Act.empty((3, 2), 10, "cpu", slot)                                      # [T][B][C]: every leading dimension is rows
    assert (cat.C, cat.ld, cat.nrows, tuple(cat.t.shape)) == (10, 10, 6, (6, 10)) and (nxt.C, nxt.ld, nxt.nrows) == (10, 10, 6)
    assert (cat.amax.storage_offset(), nxt.amax.storage_offset()) == (0, 1) and cat.amax.shape == (1,)      # slots in the order taken
    half = cat.cols(4, 3)
    assert (half.C, half.ld, half.nrows) == (3, 10, 6) and half.t.storage_offset() == 4 and tuple(half.t.shape) == (6, 3)
    part = half.rows(2, 3)
    assert (part.C, part.ld, part.nrows) == (3, 10, 3) and part.t.storage_offset() == 24 and tuple(part.t.stride()) == (10, 1)
    up = Act(cat.t, 5, cat.ld, cat.amax)                                          # the up half of a concat buffer: the whole tensor
    assert up.t is cat.t and (up.C, up.ld, up.nrows) == (5, 10, 6)
    step = nxt.rows(1, 2).cols(5, 5)
    assert (step.C, step.ld, step.nrows) == (5, 10, 4) and step.t.storage_offset() == 25 and tuple(step.t.shape) == (2, 2, 5)
    for view, parent in ((half, cat), (part, cat), (up, cat), (step, nxt)):
        assert _same_slot(view.amax, parent.amax)
    wrapped = Act(cat.t[:, 5:])                                                   # defaults are read from the view
    assert (wrapped.C, wrapped.ld, wrapped.amax) == (5, 10, None)
    off = ops.AmaxPool("cpu", on=False)
    assert Act.empty(4, 3, "cpu", off).amax is None and Act.empty(4, 3, "cpu").amax is None
    # a reader of a saved context takes the record for its tensor
    assert half.shape == (6, 3) and half.detach().data_ptr() == half.t.data_ptr() and torch.equal(half[1:3] > 0, half.t[1:3] > 0)
    with pytest.raises(AttributeError):
        half.lda


def test_record_refuses_what_no_kernel_can_read():
    t = torch.zeros(4, 6)
    with pytest.raises(ValueError):
        Act(t.t())                                                                # channel stride 4
    with pytest.raises(ValueError):
        Act(t, C=4, ld=3)                                                         # rows would overlap
    with pytest.raises(ValueError):
        Act(t, C=8, ld=8)                                                         # wider than the row


def test_pool_and_mask_records_are_unpacked_at_the_launch(calls):
    cv = conv.Conv(2, 4, 6, 4, 8, 3, 3, pad=(1, 1))
    rng = np.random.default_rng(11)
    _, x = _operand(rng, 48, 4, 12, 8)
    _, y = _operand(rng, 48, 8, 20, 4)
    _, pooled = _operand(rng, 2 * 2 * 3, 8, 16, 8)
    _, mask = _operand(rng, 48, 4, 8, 4)
    w = torch.zeros(8, 36)
    assert cv.can_pool(2, x, y) is True
    cv.fwd(x, w, y, pool=(pooled, 2))
    cv.dgrad(y, w, x, mask=mask)
    can, fwd, _, dgrad = calls
    assert can[0] == "conv_can_pool" and can[2] == dict(B=2, H=4, W=6, Cin=4, N=8, kw=2, ldx=12, ldy=20)
    _carries(fwd, ldx=12, ldy=20, x_amax=x.amax, y_amax=y.amax)
    assert len(fwd[2]["pool"]) == 4 and fwd[2]["pool"][0] is pooled.t and fwd[2]["pool"][1:3] == (16, 2) and fwd[2]["pool"][3] is pooled.amax
    _carries(dgrad, ldx=20, ldy=12, x_amax=y.amax, y_amax=x.amax, mask=mask.t, ldmask=8)


def _z(rows, C, ld=None):
    return Act(torch.zeros(rows, ld or C)[:, :C])


# method -> the calls that must be refused: a record whose channels or rows are not the layer's (the layer: 2 x 4 x 6, 4 -> 8 channels)
MISMATCHES = {
    "fwd": lambda cv, w: [lambda: cv.fwd(_z(48, 5, 8), w, _z(48, 8)),             # x.C != Cin
                          lambda: cv.fwd(_z(47, 4), w, _z(48, 8)),                # x.rows != B*H*W
                          lambda: cv.fwd(_z(48, 4), w, _z(48, 4, 8)),             # y.C != N
                          lambda: cv.fwd(_z(48, 4), w, _z(24, 8)),                # y.rows != B*OH*OW
                          lambda: cv.fwd(_z(48, 4), w, _z(48, 8), pool=(_z(48, 8), 2))],      # the pooled rows are B*(OH/2)*(OW/kw)
    "dgrad": lambda cv, w: [lambda: cv.dgrad(_z(48, 4, 8), w, _z(48, 4)),         # dy.C != N
                            lambda: cv.dgrad(_z(48, 8), w, _z(48, 8)),            # dx.C != Cin
                            lambda: cv.dgrad(_z(48, 8), w, _z(96, 4)),            # dx.rows
                            lambda: cv.dgrad(_z(48, 8), w, _z(48, 4), mask=_z(48, 8))],       # the mask lies on dx's plane
    "wgrad": lambda cv, w: [lambda: cv.wgrad(_z(48, 4), _z(48, 4), w),            # dy.C != N
                            lambda: cv.wgrad(_z(48, 8), _z(48, 8), w),            # x.C != Cin
                            lambda: cv.wgrad(_z(12, 8), _z(48, 4), w),            # dy.rows
                            lambda: cv.wgrad(_z(48, 8), _z(12, 4), w)],           # x.rows
}


@pytest.mark.parametrize("method", list(MISMATCHES))
def test_a_record_that_is_not_the_layers_is_refused_before_any_launch(method, calls):
    cv = conv.Conv(2, 4, 6, 4, 8, 3, 3, pad=(1, 1))
    for call in MISMATCHES[method](cv, torch.zeros(8, 3, 3, 4)):
        with pytest.raises(ValueError):
            call()
    assert calls == []


def test_the_adjoint_scatter_refuses_records_of_the_wrong_side(calls):
    up = conv.Conv(2, 4, 6, 4, 8, 2, 2, stride=(2, 2))                            # its adjoint: [2*2*3][8] -> [2*4*6][4]
    w = torch.zeros(8, 16)
    for x, y in ((_z(12, 4, 8), _z(48, 4, 8)),                                    # x.C != N
                 (_z(12, 8), _z(48, 8)),                                          # y.C != Cin (the whole concat row taken for the up half)
                 (_z(48, 8), _z(48, 4, 8)),                                       # x.rows != B*OH*OW
                 (_z(12, 8), _z(12, 4, 8))):                                      # y.rows != B*H*W
        with pytest.raises(ValueError):
            up.scatter_adjoint(x, w, y)
    assert calls == []
    up.scatter_adjoint(_z(12, 8), w, Act(torch.zeros(48, 8), C=4))
    assert [k[0] for k in calls] == ["transposed", "conv_igemm"]


# ------------------------------------------------------------------------------------------------------------------- batchnorm
@pytest.fixture
def bn_calls(monkeypatch):
    """the ops.bn_* functions replaced: -> the list of (name, {parameter: argument}) they were called with"""
    log = []
    for name in ("bn_train_stats", "bn_train_stats_from_partials", "bn_eval_coeff", "bn_apply", "bn_apply_pool", "bn_bwd", "bn_bwd_pool"):
        sig = inspect.signature(getattr(ops, name))
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _s=sig, **kw: log.append((_n, _s.bind(*a, **kw).arguments)))
    return log


def _is_rows(t, parent, r0, n, c0, C):
    """t is rows r0 .. r0 + n, channels c0 .. c0 + C of the dense 2-D tensor `parent`, as a view of it"""
    ld = parent.shape[1]
    return (t.untyped_storage().data_ptr() == parent.untyped_storage().data_ptr() and t.storage_offset() == r0 * ld + c0
            and tuple(t.shape) == (n, C) and (n == 1 or t.stride(0) == ld) and t.stride(1) == 1)


def test_batchnorm_stage_hands_each_group_its_rows_strides_and_the_one_slot(bn_calls):
    """two statistics groups, the output in the right half of a [M][2C] concat buffer, a 2x2-pooled output: what unet/train_bn_groups2 of
    the pinned launch list holds on the device"""
    B, h, w, C = 4, 4, 6, 8
    per, pper = h * w, (h // 2) * (w // 2)
    slot = ops.AmaxPool("cpu")
    cat = Act.empty(B * per, 2 * C, "cpu", slot)
    pooled, y = Act.empty(B * pper, C, "cpu", slot), Act.empty(B * per, C, "cpu")
    gamma, beta, rm, rv = (torch.zeros(C) for _ in range(4))
    parts = batchnorm.partition(2, B)
    st, pooled_here = batchnorm.forward(y, cat.cols(C, C), h, w, gamma, beta, rm, rv, True, parts, True, pool=(pooled, 2, 2))
    assert pooled_here and [n for n, _ in bn_calls] == ["bn_train_stats", "bn_apply_pool"] * 2
    assert (st.C, st.parts, st.y) == (C, parts, y) and tuple(st.coef.shape) == (2, 4, C) and tuple(st.stat64.shape) == (2, 2, C)
    for g, (b0, nb) in enumerate(parts):
        stats, apply = bn_calls[2 * g][1], bn_calls[2 * g + 1][1]
        assert _is_rows(stats["y"], y.t, b0 * per, nb * per, 0, C) and (stats["ldy"], stats["M"], stats["C_"]) == (C, nb * per, C)
        assert stats["stat64"].data_ptr() == st.stat64[g].data_ptr() and stats["scale"].data_ptr() == st.coef[g, 2].data_ptr()
        assert _is_rows(apply["y"], y.t, b0 * per, nb * per, 0, C) and _is_rows(apply["a"], cat.t, b0 * per, nb * per, C, C)
        assert _is_rows(apply["pooled"], pooled.t, b0 * pper, nb * pper, 0, C)
        assert (apply["ldy"], apply["lda"], apply["ldp"], apply["B"], apply["H"], apply["W"], apply["C_"], apply["kh"], apply["kw"]) == \
            (C, 2 * C, C, nb, h, w, C, 2, 2)
        assert apply["amax"] is cat.amax and apply["pooled_amax"] is pooled.amax and apply["relu"] is True
        assert apply["scale"].data_ptr() == st.coef[g, 2].data_ptr() and apply["shift"].data_ptr() == st.coef[g, 3].data_ptr()
    # the same stage without a pool behind it; eval mode is one group whatever `parts` says
    del bn_calls[:]
    _, pooled_here = batchnorm.forward(y, cat.cols(C, C), h, w, gamma, beta, rm, rv, True, parts, False)
    assert not pooled_here and [n for n, _ in bn_calls] == ["bn_train_stats", "bn_apply"] * 2
    for g, (b0, nb) in enumerate(parts):
        apply = bn_calls[2 * g + 1][1]
        assert _is_rows(apply["a"], cat.t, b0 * per, nb * per, C, C) and (apply["ldy"], apply["lda"], apply["M"]) == (C, 2 * C, nb * per)
        assert apply["amax"] is cat.amax and bn_calls[2 * g][1]["stat64"] is None
    del bn_calls[:]
    ev, _ = batchnorm.forward(y, cat.cols(C, C), h, w, gamma, beta, rm, rv, False, parts, True)
    assert [n for n, _ in bn_calls] == ["bn_eval_coeff", "bn_apply"] and ev.parts == [(0, B)] and bn_calls[1][1]["M"] == B * per

    # backward of the two-group stage: da = the right half of the concat buffer's gradient, dy dense with its slot
    del bn_calls[:]
    dcat, dy = Act.empty(B * per, 2 * C, "cpu", slot), Act.empty(B * per, C, "cpu", slot)
    dgamma, dbeta = torch.zeros(C), torch.zeros(C)
    batchnorm.backward(st, dcat.cols(C, C), dy, gamma, dgamma, dbeta)
    assert [n for n, _ in bn_calls] == ["bn_bwd"] * 2
    for g, (b0, nb) in enumerate(parts):
        k = bn_calls[g][1]
        assert _is_rows(k["da"], dcat.t, b0 * per, nb * per, C, C) and _is_rows(k["dy"], dy.t, b0 * per, nb * per, 0, C)
        assert _is_rows(k["y"], y.t, b0 * per, nb * per, 0, C) and (k["ldda"], k["ldy"], k["lddy"], k["M"], k["C_"]) == (2 * C, C, C, nb * per, C)
        assert k["amax"] is dy.amax and k["a"] is None and k["training"] is True and k["stat64"].data_ptr() == st.stat64[g].data_ptr()
        assert k["dgamma"] is dgamma and k["dbeta"] is dbeta and k["accumulate"] is True
    # ... and with the pool's gradient still to route (kw = 2), once beside da and once alone (da None: pixel stride 0)
    dpool = Act.empty(B * pper, C, "cpu")
    for da in (dcat.cols(C, C), None):
        del bn_calls[:]
        batchnorm.backward(st, da, dy, gamma, dgamma, dbeta, pool=(dpool, 2))
        assert [n for n, _ in bn_calls] == ["bn_bwd_pool"] * 2
        for g, (b0, nb) in enumerate(parts):
            k = bn_calls[g][1]
            assert _is_rows(k["dpool"], dpool.t, b0 * pper, nb * pper, 0, C) and (k["lddp"], k["kw"], k["B"], k["H"], k["W"]) == (C, 2, nb, h, w)
            assert (k["da"] is None and k["ldda"] == 0) if da is None else (_is_rows(k["da"], dcat.t, b0 * per, nb * per, C, C) and k["ldda"] == 2 * C)
            assert _is_rows(k["dy"], dy.t, b0 * per, nb * per, 0, C) and k["amax"] is dy.amax
    # the replica-group slice of the stage is that group's rows and coefficients
    sub = st.restricted(2, 2)
    assert _is_rows(sub.y.t, y.t, 2 * per, 2 * per, 0, C) and sub.parts == [(0, 2)] and sub.coef.data_ptr() == st.coef[1].data_ptr()
