"""tests/conv_spec.py held to torch in float64 (conv2d, conv_transpose2d, autograd's w.grad) on every case geometry, and the case
tables shown to have teeth: every named way of misreading a descriptor field moves at least one case by more than 100 x the gate the
device is held to (tests/test_conv_descriptor_gpu.py).  No GPU, nothing of the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_spec as cs

REL = 1e-12


def _sl(op, buf):
    """the slice of an operand's allocation `buf` (a flat array of the allocation's size) as [rows][width]"""
    return np.asarray(buf)[op.guard:op.guard + op.rows * op.ld].reshape(op.rows, op.ld)[:, op.off:op.off + op.width]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@pytest.mark.parametrize("name", list(cs.CONV_CASES))
def test_conv_spec_is_torch_in_float64(name):
    c = cs.conv_case(name)
    d = c.d
    y, written = cs.conv_case_spec(name)
    assert np.array_equal(written, c.y.inside()), "the spec stores exactly the slice"
    before = c.y.buf.astype(np.float64)
    assert np.array_equal(y[~written], before[~written], equal_nan=True)
    x = _t(c.x.view()).view(d.B, d.H, d.W, d.Cin).permute(0, 3, 1, 2)
    w = _t(c.w.view()).view(d.N, d.KH, d.KW, d.Cin)
    bias = _t(c.bias.view()[0]) if c.bias else None
    if d.out_mode == cs.OUT_CONVT:
        co = d.N // 4
        wt = w.view(2, 2, co, d.Cin).permute(3, 2, 0, 1)                     # [Cin][co][a][bb]
        ref = F.conv_transpose2d(x, wt, bias, stride=2).permute(0, 2, 3, 1).reshape(-1, co)
        assert c.scale is None
    else:
        ref = F.conv2d(x, w.permute(0, 3, 1, 2), None, stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w))
        assert tuple(ref.shape[2:]) == (d.OH, d.OW)
        ref = ref.permute(0, 2, 3, 1)                                        # [B][OH][OW][N]
        if c.scale:
            ref = ref * _t(c.scale.view()[0])
        if bias is not None:
            ref = ref + bias
        if d.out_mode == cs.OUT_TBC:
            ref = ref[:, 0].permute(1, 0, 2)                                 # [OW][B][N]
        ref = ref.reshape(-1, d.N)
    if d.relu:
        ref = ref.relu()
    if c.mask:
        ref = torch.where(torch.from_numpy(c.mask.view() > 0), ref, torch.zeros_like(ref))
    if d.accumulate:
        ref = ref + _t(c.y.view())
    got = _sl(c.y, y)
    assert np.isfinite(got).all()
    err = np.abs(got - ref.numpy()).max()
    assert err <= REL * np.abs(ref.numpy()).max(), (name, err)
    if c.mask:
        assert (got[~(c.mask.view() > 0)] == (_sl(c.y, before)[~(c.mask.view() > 0)] if d.accumulate else 0.0)).all()


@pytest.mark.parametrize("name", list(cs.WGRAD_CASES))
def test_wgrad_spec_is_autograd_in_float64(name):
    c = cs.wgrad_case(name)
    d = c.d
    p = _t(c.p.view()).view(d.B, d.PH, d.PW, d.R).permute(0, 3, 1, 2)
    q = _t(c.q.view()).view(d.B, d.QH, d.QW, d.C).permute(0, 3, 1, 2)
    w = torch.zeros(d.R, d.C, d.KH, d.KW, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(q, w, stride=(d.stride_h, d.stride_w), padding=(d.pad_h, d.pad_w))
    assert tuple(out.shape[2:]) == (d.PH, d.PW)
    out.backward(p)
    ref = w.grad.permute(0, 2, 3, 1).numpy()
    for splits in (1, 3):
        dw, db = cs.wgrad_case_spec(name, None, splits)
        assert np.abs(dw - ref).max() <= REL * np.abs(ref).max(), name
        assert np.abs(db - c.p.view().astype(np.float64).sum(0)).max() <= REL * np.abs(db).max()
    if name == "convt":                                                      # the same numbers as nn.ConvTranspose2d's weight gradient
        wt = torch.zeros(d.R, d.C, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(p, wt, stride=2).backward(q)
        assert np.abs(dw - wt.grad.permute(0, 2, 3, 1).numpy()).max() <= REL * np.abs(ref).max()
    # accumulate: the prior value is added once
    dacc = cs.conv_wgrad_spec(type(d)(**{**vars(d), "accumulate": 1}), c.p.buf, c.q.buf, c.dw_prev)[0]
    assert np.abs(dacc - (ref + c.dw_prev)).max() <= REL * np.abs(ref + c.dw_prev).max()


@pytest.mark.parametrize("perturb", cs.PERTURBATIONS["conv"])
def test_every_conv_perturbation_moves_a_case(perturb):
    ratios = {}
    for name in cs.CONV_CASES:
        y, written = cs.conv_case_spec(name)
        y2, written2 = cs.conv_case_spec(name, perturb)
        top = np.abs(y[written]).max()
        ratios[name] = np.inf if not np.array_equal(written, written2) else cs.moved(y, y2) / (cs.CONV_GATE * top)
    print(perturb, {k: f"{v:.3g}" for k, v in ratios.items() if v > 0})
    assert max(ratios.values()) > 100, (perturb, "no case notices: a case is missing")


@pytest.mark.parametrize("perturb", cs.PERTURBATIONS["wgrad"])
def test_every_wgrad_perturbation_moves_a_case(perturb):
    ratios = {}
    for name in cs.WGRAD_CASES:
        for splits in (1, 3):
            dw, _ = cs.wgrad_case_spec(name, None, splits)
            dw2, _ = cs.wgrad_case_spec(name, perturb, splits)
            ratios[name, splits] = cs.moved(dw, dw2) / (cs.WGRAD_GATE * np.abs(dw).max())
    print(perturb, {k: f"{v:.3g}" for k, v in ratios.items() if v > 0})
    assert max(ratios.values()) > 100, (perturb, "no case notices: a case is missing")


def test_the_walked_pixel_is_the_pixel():
    """the gather's carry arithmetic, as conv_spec states it, reaches pixel m = (b, ph, pw) for every image size, smaller than a stage or not"""
    for PH, PW in ((1, 1), (2, 3), (1, 31), (5, 7), (4, 8), (1, 217), (3, 40), (33, 1)):
        for m in range(0, 400, 7):
            b, rem = divmod(m, PH * PW)
            assert cs._walked_pixel(m, PH, PW, False) == (b, *divmod(rem, PW)), (PH, PW, m)


def test_operand_layout():
    op = cs.Operand(5, 8, 24, 4).set(np.arange(40))
    assert op.buf.size == (2 * cs.GUARD_ROWS + 5) * 24 and op.base % 4 == 0
    assert np.isnan(op.buf[:op.guard]).all() and np.isnan(op.buf[op.guard + 5 * 24:]).all()
    assert op.buf[op.base + 3 * 24 + 2] == 26 and op.inside().sum() == 40
    gaps = op.buf[~op.inside()]
    assert not np.isfinite(gaps).any() and np.isinf(gaps).any() and np.isnan(gaps).any()
