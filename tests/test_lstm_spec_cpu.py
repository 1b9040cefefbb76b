"""tests/lstm_spec.py, the fp64 specification of the BiLSTM layer that tests/test_lstm_paths_gpu.py holds the three kernel paths to,
against torch.nn.LSTM and the oracle in fp64; and the conditions on the saturated operands that make them a test of the gate
non-linearities rather than of nothing (conditions on the INPUTS: if one fails, the builder changes, not the condition)."""
import pytest
import torch

import lstm_spec as S


@pytest.mark.parametrize("T,B", [(5, 3), (1, 2)])
def test_spec_equals_nn_lstm_and_the_oracle_in_fp64(T, B):
    """nn.LSTM(2048, 256, bidirectional=True) with zero biases and an identity input projection (direction d takes columns
    d*1024 .. of gx unchanged, every other input weight zero), and oracle.model_oracle.lstm_layer_dir with the same projection:
    y, and through autograd d loss / d gx = the gate gradients, to 1e-12."""
    from oracle import model_oracle as mo
    gx, wh, dy = S.case(T, B, seed=11 * T + B)
    ref = S.reference(gx, wh, dy)
    proj = [torch.zeros(1024, 2048, dtype=torch.double) for _ in range(2)]
    for d in range(2):
        proj[d][:, d * 1024:(d + 1) * 1024] = torch.eye(1024, dtype=torch.double)
    zero = torch.zeros(1024, dtype=torch.double)

    net = torch.nn.LSTM(2048, 256, bidirectional=True).double()
    with torch.no_grad():
        for d, suf in enumerate(("", "_reverse")):
            getattr(net, "weight_ih_l0" + suf).copy_(proj[d])
            getattr(net, "weight_hh_l0" + suf).copy_(wh[d].double())
            getattr(net, "bias_ih_l0" + suf).zero_()
            getattr(net, "bias_hh_l0" + suf).zero_()
    x = gx.double().requires_grad_()
    y, _ = net(x)
    y.backward(dy.double())
    assert (y.detach() - ref.y).abs().max().item() <= 1e-12
    assert (x.grad - ref.dgates).abs().max().item() <= 1e-12

    x = gx.double().requires_grad_()
    y = torch.cat([mo.lstm_layer_dir(x, proj[d], wh[d].double(), zero, zero, bool(d)) for d in range(2)], dim=2)
    y.backward(dy.double())
    assert (y.detach() - ref.y).abs().max().item() <= 1e-12
    assert (x.grad - ref.dgates).abs().max().item() <= 1e-12

    # what neither of the two returns is tied to what they do: y = o * tanh(c), c from the activations, dc0 = 0 where T steps of
    # forget gates in (0, 1) cannot have made it so
    o = torch.cat([ref.acts[:, :, d * 1024 + 768:(d + 1) * 1024] for d in range(2)], dim=2)
    assert (o * torch.tanh(ref.c) - ref.y).abs().max().item() <= 1e-15
    i, f, g = (torch.cat([ref.acts[:, :, d * 1024 + k * 256:d * 1024 + (k + 1) * 256] for d in range(2)], dim=2) for k in range(3))
    c_prev = torch.zeros_like(ref.c)                        # the predecessor in time: t - 1 in direction 0, t + 1 in direction 1
    c_prev[1:, :, :256] = ref.c[:-1, :, :256]
    c_prev[:-1, :, 256:] = ref.c[1:, :, 256:]
    assert (f * c_prev + i * g - ref.c).abs().max().item() <= 1e-15
    assert ref.dc0.shape == (B, 512) and torch.isfinite(ref.dc0).all() and (ref.dc0 != 0).all()


def test_unit_case_keeps_the_operands_of_the_operand_scale_tests():
    """`case(T, B)` draws gx, the two W_hh and dy in that order from the seed T * 1000 + B"""
    gx, wh, dy = S.case(3, 4)
    g = torch.Generator().manual_seed(3004)
    assert torch.equal(gx, torch.randn(3, 4, 2048, generator=g) * 0.5)
    assert all(torch.equal(w, torch.randn(1024, 256, generator=g) / 16) for w in wh)
    assert torch.equal(dy, torch.randn(3, 4, 512, generator=g))


@pytest.mark.parametrize("T,B", S.SATURATED_SHAPES)       # the shapes test_lstm_paths_gpu.py runs them at
def test_saturated_case_saturates_and_keeps_gradients_of_ordinary_size(T, B):
    gx, wh, dy = S.saturated_case(T, B)
    ux, uwh, udy = S.case(T, B)
    assert all(torch.equal(a, b) for a, b in zip(wh, uwh)) and torch.equal(dy, udy)
    changed = (gx != ux).view(T, B, 2, 4, 256)
    per = changed.sum(dim=(0, 2, 4))                        # [B][kind]
    assert (per == T * 512 // 8).all(), "one eighth of every sample's pre-activations of every gate kind"
    big = gx[gx != ux].abs()
    assert sorted(set(big.tolist())) == sorted(S.SATURATING)
    assert torch.equal(gx.double().float(), gx)
    ref, unit = S.reference(gx, wh, dy), S.reference(ux, uwh, udy)
    for name, t in ref._asdict().items():
        assert torch.isfinite(t).all(), name
    top, utop = ref.dgates.abs().amax(dim=(0, 2)), unit.dgates.abs().amax(dim=(0, 2))
    assert (top >= 1e-3 * utop).all(), (top / utop).min().item()
    a32 = ref.acts.float().view(T, B, 2, 4, 256)
    for k, kind in enumerate(S.GATE_KINDS):
        assert ((a32[:, :, :, k] == 0.0) | (a32[:, :, :, k] == 1.0)).any(), kind
