"""Every arithmetic path of the BiLSTM layer against ONE fp64 specification (tests/lstm_spec.py), element by element, at the batch
sizes where a path changes its workgroup shape and at the sequence lengths where the in-launch exchange changes its behaviour.

Paths: "seq" (one launch per pass, csrc/lstm_seq.hip), "bf3" (per-step split-bf16 kernels) and "f32" (per-step fp32-MFMA kernels,
both csrc/lstm.hip), each forced the way test_kernels_gpu.py::test_lstm_layer_fwd_bwd forces it.  Shapes: the ragged last row block
(B % 32 in {0, 1, 31}), the first B of every 128-row workgroup shape (seq forward above 512, seq backward above 1024, bf3 forward
from 1536), T = 1 (no exchange), T = 2 (one exchange, no buffer reuse; T = 4 is the first length that reads a reused buffer), and
operands whose gate pre-activations reach +-1e4 (tests/test_lstm_spec_cpu.py checks on the CPU that they saturate every gate kind
and keep every sample's gradients at ordinary size).

Everything a pass writes is compared: y, c and the saved activations of the forward, each within FWD_GATE = 2e-5 of the tensor's
max |ref| (the forward gate of test_lstm_layer_fwd_bwd; c and the activations are intermediates of the same arithmetic,
y = o * tanh(c)), no floor, output buffers pre-filled with NaN; the gate gradients and dc of the backward per SAMPLE within
LSTM_GATE = 1e-4 of that sample's own max |ref|.  The one-launch kernels' carried abs-max slots must equal the tensors' maxima
exactly, and their timeout word (ops.lstm_seq_timed_out) is read after every pass before any number is looked at.  B never exceeds
2048 and nothing here tries to make a hand-off time out.

The worst error / gate ratio per (path, tensor) is printed (pytest -s), with the same ratio of a plain fp32 host implementation
beside it (oracle.model_oracle.lstm_layer_dir in fp32 for y and the gate gradients, the specification's own loop in fp32 for c,
the activations and dc), for the table in DESIGN.md §4."""
import functools

import pytest
import torch

import lstm_spec as S

pytestmark = pytest.mark.gpu

FWD_GATE, LSTM_GATE = 2e-5, 1e-4          # test_lstm_layer_fwd_bwd's forward gate; the LSTM backward gate of test_operand_scale_gpu.py

PATHS = ["seq", "bf3", "f32"]
CASES = ([("unit", 4, B) for B in (1, 31, 32, 33)]                     # ragged last row block
         + [("unit", 4, B) for B in (512, 513)]                        # seq forward: 128-row workgroups above 512 rows
         + [("unit", 4, B) for B in (1024, 1025)]                      # seq backward: 128-row workgroups above 1024 rows
         + [("unit", 4, B) for B in (1535, 1536, 1537)]                # bf3 forward: 128-row workgroups from 1536 rows
         + [("unit", 1, B) for B in (33, 1025)]                        # no exchange
         + [("unit", 2, B) for B in (33, 1025)]                        # one exchange, no buffer reuse
         + [("saturated", T, B) for T, B in S.SATURATED_SHAPES])
RAGGED = [B for kind, T, B in CASES if kind == "unit" and T == 4 and B % 32]


def _id(case):
    return f"{case[0]}-T{case[1]}-B{case[2]}"


WORST, ORACLE = {}, {}       # (path, tensor) -> worst error / gate of the device; tensor -> the same of the fp32 host implementation
TOPS = {}                    # case -> (max |ref y|, per-sample max |ref dc0|): what the agreement test needs of the specification
RESULTS = {}                 # (path, case) -> (y, dc or None) on the host, for the agreement test


def _operands(case):
    kind, T, B = case
    return (S.case if kind == "unit" else S.saturated_case)(T, B)


def _ratio(got, ref, per_sample):
    """worst error / gate: FWD_GATE x the tensor's max |ref|, or LSTM_GATE x every sample's own max |ref| (no floor: 0 / 0 counts as 0)"""
    if per_sample:
        err, top = S.per_sample(got, ref)
        gate = LSTM_GATE * top
    else:
        err, gate = (got.cpu().double() - ref).abs().max().reshape(1), FWD_GATE * ref.abs().max().reshape(1)
    assert torch.isfinite(err).all()
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return r.max().item()


FORWARD, BACKWARD = ("y", "c", "activations"), ("gate gradients", "dc")


@functools.lru_cache(maxsize=1)
def _spec(case):
    """the fp64 reference of a case, built once for the three paths (the cases run shape by shape), and the fp32 host figures"""
    from oracle import model_oracle as mo
    gx, wh, dy = _operands(case)
    ref = S.reference(gx, wh, dy)
    TOPS[case] = (ref.y.abs().max().item(), ref.dc0.abs().amax(dim=1))
    x = gx.clone().requires_grad_()
    eye, zero = torch.eye(1024), torch.zeros(1024)
    y32 = torch.cat([mo.lstm_layer_dir(x[:, :, d * 1024:(d + 1) * 1024], eye, wh[d], zero, zero, bool(d)) for d in range(2)], dim=2)
    y32.backward(dy)
    r32 = S.reference(gx, wh, dy, dtype=torch.float32)
    host = {"y": _ratio(y32.detach(), ref.y, False), "c": _ratio(r32.c, ref.c, False), "activations": _ratio(r32.acts, ref.acts, False),
            "gate gradients": _ratio(x.grad, ref.dgates, True), "dc": _ratio(r32.dc0, ref.dc0, True)}
    for k, v in host.items():
        ORACLE[k] = max(ORACLE.get(k, 0.0), v)
    return gx, wh, dy, ref, host


def _packs(path, wh):
    """-> (fwd pack, bwd pack) of the path, as test_lstm_layer_fwd_bwd selects them"""
    from qea import _lib, ops
    whd = [w.cuda() for w in wh]
    if path == "seq":
        old = ops.LSTM_SEQ["on"]
        ops.LSTM_SEQ["on"] = True
        try:
            pf, pb, mode = ops.lstm_packs(whd[0], whd[1])
        finally:
            ops.LSTM_SEQ["on"] = old
        assert mode == "seq"
        return pf, pb
    if path == "bf3":
        nb = _lib.lib().qea_lstm_pack_whh_split_bytes()
        pf, pb = torch.empty(2, nb, dtype=torch.uint8, device="cuda"), torch.empty(2, nb, dtype=torch.uint8, device="cuda")
    else:
        pf, pb = torch.empty(2, 1024 * 256, device="cuda"), torch.empty(2, 1024 * 256, device="cuda")
    for d in range(2):
        (ops.lstm_pack_whh_split if path == "bf3" else ops.lstm_pack_whh)(whd[d], pf[d], pb[d])
    return pf, pb


def _skip_unless_available(path):
    from qea import ops
    if path == "seq" and ops.mfma_mode() != "split_f16":
        pytest.skip("the one-launch layer kernels are the fp16-split mode's")


def _no_timeout(which):
    from qea import ops
    assert not ops.lstm_seq_timed_out(which), f"in-launch hand-off timed out ({which})"


def _layer(path, gx, wh, dy):
    """one forward and (dy given) one backward of the path into NaN-filled buffers
    -> y, c, activations, gate gradients, dc (None where the path has none), y_amax, g_amax (None where the path carries none)"""
    from qea import ops
    T, B, _ = gx.shape
    nan = float("nan")
    pf, pb = _packs(path, wh)
    seq = path == "seq"
    gates = gx.cuda().clone()
    c, y = torch.full((T, B, 512), nan, device="cuda"), torch.full((T, B, 512), nan, device="cuda")
    ya, ga = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    carried = ops.lstm_layer_fwd_any(gates, c, y, pf, path, T, B, y_amax=ya)
    torch.cuda.synchronize()
    if seq:
        _no_timeout("fwd")
    assert bool(carried) == seq
    acts = gates.clone()
    if dy is None:
        return y, c, acts, None, None, (ya if seq else None), None
    dc = None if seq else torch.full((B, 512), nan, device="cuda")
    carried = ops.lstm_layer_bwd_any(gates, c, dy.cuda(), pb, path, dc, T, B, g_amax=ga)
    torch.cuda.synchronize()
    if seq:
        _no_timeout("bwd")
    assert bool(carried) == seq
    return y, c, acts, gates, dc, (ya if seq else None), (ga if seq else None)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    from qea import ops
    print(f"\nlstm paths summary, mode {ops.mfma_mode()}: worst error / gate per (path, tensor); fp32 host implementation beside it")
    for t in FORWARD + BACKWARD:
        row = "  ".join(f"{p} {WORST[(p, t)]:.3g}" if (p, t) in WORST else f"{p} -" for p in PATHS)
        print(f"  {t:15s} {row}   fp32 host {ORACLE.get(t, float('nan')):.3g}")
    RESULTS.clear()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_path_conforms_to_the_spec(case, path):
    _skip_unless_available(path)
    gx, wh, dy, ref, host = _spec(case)
    y, c, acts, dgates, dc, ya, ga = _layer(path, gx, wh, dy)
    got = {"y": (y, ref.y), "c": (c, ref.c), "activations": (acts, ref.acts), "gate gradients": (dgates, ref.dgates)}
    if dc is not None:
        got["dc"] = (dc, ref.dc0)
    for name, (t, _) in got.items():
        assert torch.isfinite(t).all(), (path, name)                      # the NaN fill is gone from every row, nothing non-finite made
    ratios = {name: _ratio(t, r, name in BACKWARD) for name, (t, r) in got.items()}
    for name, v in ratios.items():
        WORST[(path, name)] = max(WORST.get((path, name), 0.0), v)
        print(f"lstm paths {_id(case)} {path} {name}: worst error / gate = {v:.3g} (fp32 host {host[name]:.3g})")
    RESULTS[(path, case)] = (y.cpu(), None if dc is None else dc.cpu())
    assert all(v <= 1.0 for v in ratios.values()), (path, ratios)
    if path == "seq":
        assert ya.item() == y.abs().max().item() and ga.item() == dgates.abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_paths_agree_with_each_other(case):
    """All paths' y within 4e-5 x max |ref y| of each other (twice the forward gate: the triangle inequality, nothing new), the two
    step kernels' dc within the backward gate of each other, per sample."""
    from qea import ops
    paths = [p for p in PATHS if p != "seq" or ops.mfma_mode() == "split_f16"]
    if case not in TOPS:
        _spec(case)
    y_top, dc_top = TOPS[case]
    for p in paths:
        if (p, case) not in RESULTS:
            gx, wh, dy = _operands(case)
            y, _, _, _, dc, _, _ = _layer(p, gx, wh, dy)
            RESULTS[(p, case)] = (y.cpu(), None if dc is None else dc.cpu())
    for i, p in enumerate(paths):
        for q in paths[i + 1:]:
            err = (RESULTS[(p, case)][0].double() - RESULTS[(q, case)][0].double()).abs().max().item()
            assert err <= 2 * FWD_GATE * y_top, (p, q, err / y_top)
    err = (RESULTS[("bf3", case)][1].double() - RESULTS[("f32", case)][1].double()).abs().amax(dim=1)
    assert torch.isfinite(err).all() and (err <= LSTM_GATE * dc_top).all(), (err / dc_top).max().item()


@pytest.mark.parametrize("B", RAGGED)
def test_seq_carried_absmax_when_the_largest_value_sits_in_the_last_valid_row(B):
    """The last valid row's output-gate pre-activations times 8 (sigma(o) leaves the unit-scale range), and its input- and cell-gate
    ones as well: with the output gate alone the row reaches max |h| = 0.61 at T = 4, which is the largest of 33 rows but not of 513
    (0.61 again) or 1535 (0.62).  The largest |h| of the layer then sits in row B - 1 of a ragged last row block (checked on the
    specification), next to the rows the kernel computes and masks."""
    _skip_unless_available("seq")
    T = 4
    gx, wh, dy = S.case(T, B)
    gx = gx.clone()
    for k in (0, 2, 3):
        gx.view(T, B, 2, 4, 256)[:, B - 1, :, k] *= 8
    ref = S.reference(gx, wh, None)
    assert ref.y.abs().amax(dim=(0, 2)).argmax().item() == B - 1
    y, c, acts, dgates, _, ya, ga = _layer("seq", gx, wh, dy)
    assert all(torch.isfinite(t).all() for t in (y, c, acts, dgates))
    assert _ratio(y, ref.y, False) <= 1.0
    assert y.abs().amax(dim=(0, 2)).argmax().item() == B - 1
    assert ya.item() == y.abs().max().item() and ga.item() == dgates.abs().max().item()
