"""qea/conv.py held to torch: every descriptor a Conv record hands to ops.conv_igemm / ops.conv_wgrad — forward, input gradient (or the
adjoint scatter) and weight gradient of one geometry — is evaluated with the fp64 statement of those entry points (tests/conv_spec.py)
and must give torch's conv2d / conv_transpose2d and their autograd gradients in float64.  The four ops functions are replaced by
recorders (the derived filters are made on the host by the formulas of their docstrings), the operands live in conv_spec.Operand
allocations so that a wrong pixel stride or plane reads NaN.  No GPU, nothing of the library."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_spec as cs
from qea import conv, ops

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
    return log


def _operand(rng, rows, width, ld=None, off=0, fill=True):
    """-> (the Operand, its slice as the strided host tensor a caller would pass)"""
    op = cs.Operand(rows, width, ld, off)
    if fill:
        op.set(rng.standard_normal((rows, width)))
    return op, torch.from_numpy(op.buf)[op.base:].as_strided((rows, width), (op.ld, 1))


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
    assert cv.fwd(x, ldx, w, y, ldy, bias=torch.from_numpy(bias), **extra) is RETURNED
    assert cv.dgrad(dy, ldy, w, dx, ldx) is RETURNED
    cv.wgrad(dy, ldy, x, ldx, dw, accumulate=True)
    assert [c[0] for c in calls] == ["conv_igemm", "flip_transposed", "conv_igemm", "conv_wgrad"]
    fwd, flip, dgrad, wgrad = calls
    assert fwd[1][1] is w and fwd[2]["w_src"][0] == "fwd" and fwd[2]["w_src"][1] is w and fwd[2]["bias"] is not None
    assert flip[1][0] is w and dgrad[2]["w_src"][0] == "flipT" and dgrad[2]["w_src"][1] is w
    assert wgrad[2]["accumulate"] is True and "bias" not in dgrad[2]

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
    assert up.scatter_adjoint(d, dcin, w, cat, 2 * c, bias=torch.from_numpy(bias)) is RETURNED
    up.fwd(dcat, 2 * c, w, dd, dcin)
    up.wgrad(d, dcin, dcat, 2 * c, dw)
    assert [k[0] for k in calls] == ["transposed", "conv_igemm", "conv_igemm", "conv_wgrad"]
    tr, fwd, bwd, wgrad = calls
    assert tr[1][0] is w and fwd[2]["w_src"][0] == "T" and fwd[2]["w_src"][1] is w and fwd[2]["out_mode"] == cs.OUT_CONVT
    assert bwd[1][1] is w and bwd[2]["w_src"][0] == "fwd" and bwd[2]["w_src"][1] is w

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
    conv.gemm(7, 8, 4).fwd(torch.zeros(7, 8), 8, w, torch.zeros(7, 4), 4, w_src=("catT", src, (src,)))
    assert calls[0][1][1] is w and calls[0][2]["w_src"] == ("catT", src, (src,))


def test_with_batch_rebinds_the_batch_only():
    cv = conv.Conv(6, 3, 5, 4, 8, 3, 3, pad=(1, 1)).with_batch(2)
    assert (cv.B, cv.H, cv.W, cv.Cin, cv.N, cv.KH, cv.KW, cv.pad, cv.stride, cv.OH, cv.OW) == (2, 3, 5, 4, 8, 3, 3, (1, 1), (1, 1), 3, 5)


def test_refusals_come_before_any_launch(calls):
    z = torch.zeros(1)
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2, stride=(2, 2)).dgrad(z, 8, z, z, 4)
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2).scatter_adjoint(z, 8, z, z, 4)                           # stride != kernel
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 6, 4, 8, 2, 2, pad=(1, 1), stride=(2, 2)).scatter_adjoint(z, 8, z, z, 4)    # pad != 0
    with pytest.raises(ValueError):
        conv.Conv(2, 5, 6, 4, 8, 2, 2, stride=(2, 2))                                           # (5 - 2) / 2 + 1 is no whole number
    with pytest.raises(ValueError):
        conv.Conv(2, 4, 8, 4, 8, 3, 3, pad=(1, 1), stride=(1, 3))                               # (8 + 2 - 3) / 3 neither
    assert calls == []
