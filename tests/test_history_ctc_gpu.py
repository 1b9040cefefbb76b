"""The label-history weighted CTC loss in one device pass (csrc/ctc_history.hip through tracking_utils.weighted_ctc_loss): both
weight forms against the fp64 loop, the long / short shapes, an infeasible label, the fixed launch count, bit-reproducibility,
hipGraph replay, bit-equality with the plain CTC kernels at W = 1, and the routing back to the loop over the depths.

The fp64 reference is tracking_utils.weighted_ctc_loss itself on CPU fp64 log-probs with torch.nn.CTCLoss: CPU tensors and torch's
loss both send that call to the loop, so the reference never passes through the code under test."""
import math
import types

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

GATE = 1e-4                                    # the project's stated gate
C = len(H.CHAR_SET)                            # the CRNN's class count
CHARS = H.CHAR_SET[1:]


@pytest.fixture(autouse=True)
def _fused_path(monkeypatch):
    monkeypatch.delenv("QEA_HISTORY_CTC", raising=False)


def _word(rng, n):
    return "".join(rng.choice(CHARS, n))


def _batches(table, W):
    """table[strip][depth] = label or None -> target_batches as generate_ctc_target_batches returns them"""
    out = []
    for i in range(W):
        picked = [(j, row[i]) for j, row in enumerate(table) if i < len(row) and row[i] is not None]
        assert picked, f"depth {i} has no strip"
        labels = [l for _, l in picked]
        out.append([torch.tensor([H.C2I[c] for c in "".join(labels)], dtype=torch.int), torch.tensor([len(l) for l in labels], dtype=torch.int),
                    [j for j, _ in picked]])
    return out


def _table(W, seed):
    """9 strips with ragged depths; planted: no history at all, an empty label, one repeated character, 12 characters, and a strip
    present at depth 1 but not at depth 0 (no generator builds that: it is there for the packer and the kernel)"""
    rng = np.random.RandomState(seed)
    full = lambda: [_word(rng, rng.randint(1, 10)) for _ in range(W)]
    table = [full(), [None] * W, [""], ["aaaa", _word(rng, 3)], full(), [None, _word(rng, 5)], full(), full()[:2], full()]
    table[4][0] = _word(rng, 12)
    table[8][W - 1] = ""
    return [row + [None] * (W - len(row)) for row in table]


def _weights(form, N, W, seed):
    if form == "decaying":
        return torch.tensor([0.7 ** i for i in range(W)])
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, W + 1, generator=g)
    w[:, 0] = 1
    w[0, 1] = 0                                                     # a zero weight on a label that is present
    return w


def _self(form, W, device, torch_loss=False):
    from qea.loss import CTCLoss
    mk = torch.nn.CTCLoss if torch_loss else CTCLoss
    return types.SimpleNamespace(window_size=W, weightgen_method="decaying" if form == "decaying" else "levenshtein", device=device,
                                 primary_loss_fn=mk(), primary_loss_fn_sample_wise=mk(reduction="none"))


def _log_probs(T, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, N, C, generator=g).log_softmax(2)


def _reference(form, W, lp, pred, batches, w):
    """fp64 on the CPU through the loop -> (loss, gradient)"""
    import tracking_utils as tu
    x = lp.double().requires_grad_(True)
    loss = tu.weighted_ctc_loss(_self(form, W, torch.device("cpu"), torch_loss=True), x, pred, batches, w.double())
    loss.backward()
    return loss.item(), x.grad


def _device(form, W, lp, pred, batches, w, self=None):
    import tracking_utils as tu
    x = lp.cuda().requires_grad_(True)
    loss = tu.weighted_ctc_loss(self or _self(form, W, torch.device("cuda")), x, pred, batches, w.cuda() if not w.is_cuda else w)
    loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("form", ["sample_wise", "decaying"])
@pytest.mark.parametrize("W", [3, 8])
def test_parity_with_the_fp64_loop(form, W, monkeypatch):
    from qea import ops
    T, N = 31, 9
    table = _table(W, seed=W)
    batches = _batches(table, W)
    assert not set(batches[1][2]) <= set(batches[0][2])                        # the hand-built non-nested depth
    lp, pred, w = _log_probs(T, N, 10 + W), torch.full((N,), T, dtype=torch.int), _weights(form, N, W, 3)
    ref_loss, ref_grad = _reference(form, W, lp, pred, batches, w)
    assert math.isfinite(ref_loss)
    before = ops.HISTORY_CTC_LAUNCHES["ctc"]
    loss, grad = _device(form, W, lp, pred, batches, w)
    assert ops.HISTORY_CTC_LAUNCHES["ctc"] - before == 3                       # the fused call ran
    monkeypatch.setenv("QEA_HISTORY_CTC", "steps")
    loss_s, grad_s = _device(form, W, lp, pred, batches, w)
    assert ops.HISTORY_CTC_LAUNCHES["ctc"] - before == 3                       # and the switch kept the loop
    e = dict(fused=(_rel(loss.item(), ref_loss), H.full_rel_err(grad, ref_grad)), steps=(_rel(loss_s.item(), ref_loss), H.full_rel_err(grad_s, ref_grad)))
    print(f"\n[gate] history CTC T={T} N={N} W={W} {form}: worst error against the fp64 loop (loss, gradient): fused {e['fused'][0]:.2e} "
          f"{e['fused'][1]:.2e}, QEA_HISTORY_CTC=steps {e['steps'][0]:.2e} {e['steps'][1]:.2e} (gate {GATE:.0e})")
    assert max(e["fused"]) <= GATE and max(e["steps"]) <= GATE, e
    assert (grad[:, 1, :] == 0).all()                                           # the strip without history: exactly zero rows


def test_long_shape_255_states():
    rng = np.random.RandomState(4)
    T, N, W = 260, 2, 2
    table = [[_word(rng, 127), _word(rng, 9)], [_word(rng, 40), None]]
    batches = _batches(table, W)
    lp, pred, w = _log_probs(T, N, 6), torch.full((N,), T, dtype=torch.int), _weights("sample_wise", N, W, 5)
    w[0, 1] = 0.5
    ref_loss, ref_grad = _reference("sample_wise", W, lp, pred, batches, w)
    assert math.isfinite(ref_loss)
    loss, grad = _device("sample_wise", W, lp, pred, batches, w)
    e = (_rel(loss.item(), ref_loss), H.full_rel_err(grad, ref_grad))
    print(f"\n[gate] history CTC T=260 N=2 W=2, 127 characters: worst error (loss, gradient) {e[0]:.2e} {e[1]:.2e}")
    assert max(e) <= GATE, e


def test_short_shape_and_input_lengths_through_the_binding():
    from qea import history, ops
    T, N, W = 8, 3, 2
    table = [["abc", "de"], ["fg", "h"], ["i", ""]]                             # feasible at lengths 8, 5 and 1
    batches = _batches(table, W)
    pred = torch.tensor([8, 5, 1], dtype=torch.int)
    lp, w = _log_probs(T, N, 8), _weights("decaying", N, W, 0)
    ref_loss, ref_grad = _reference("decaying", W, lp, pred, batches, w)
    assert math.isfinite(ref_loss)
    pk = history.TargetBatchPacker()
    packed = pk.pack(batches, N, pred)
    dev = pk.to_device(packed[:2], torch.device("cuda"))
    depth_n, lens, offs, chars, in_len = pk.unpack(dev, N, W, packed[3])
    loss, grad, nll = ops.ctc_history_loss(lp.cuda(), in_len, lens, offs, chars, depth_n, w.cuda(), 0, 1, 1, 2 * packed[4] + 1)
    e = (_rel(loss.item(), ref_loss), H.full_rel_err(grad, ref_grad))
    print(f"\n[gate] history CTC T=8 N=3 W=2, input lengths 8/5/1: worst error (loss, gradient) {e[0]:.2e} {e[1]:.2e}")
    assert max(e) <= GATE, e
    grad = grad.cpu()
    for n, L in enumerate(pred.tolist()):
        assert (grad[L:, n, :] == 0).all() and (grad[:L, n, :] != 0).any(), n
    # nll [N][W]: the per-problem values of torch's own loss
    for i, (y, ys, idx) in enumerate(batches):
        want = torch.nn.functional.ctc_loss(lp.double()[:, idx, :], y, pred[idx], ys, reduction="none")
        assert torch.allclose(nll[idx, i].cpu().double(), want, rtol=1e-6, atol=0)
    # loss only: no gradient buffer, two launches
    before = ops.HISTORY_CTC_LAUNCHES["ctc"]
    loss2, none, _ = ops.ctc_history_loss(lp.cuda(), in_len, lens, offs, chars, depth_n, w.cuda(), 0, 1, 1, 2 * packed[4] + 1, need_grad=False)
    assert none is None and ops.HISTORY_CTC_LAUNCHES["ctc"] - before == 2 and torch.equal(loss2, loss)


@pytest.mark.parametrize("form", ["sample_wise", "decaying"])
def test_infeasible_label_poisons_its_own_strip_only(form, monkeypatch):
    """Strip 4 carries a 40-character label at depth 1 with T = 31.  The reference for the other strips is the same call with that
    label replaced by a feasible one: the label of one strip does not enter another strip's rows, and the depth keeps its count of
    strips (the mean's denominator), exactly as in the call under test."""
    T, N, W = 31, 9, 3
    rng = np.random.RandomState(2)
    table = _table(W, seed=7)
    feasible = [list(r) for r in table]
    table[4][1] = _word(rng, 40)
    batches, batches_ok = _batches(table, W), _batches(feasible, W)
    lp, pred, w = _log_probs(T, N, 12), torch.full((N,), T, dtype=torch.int), _weights(form, N, W, 3)
    ref_loss, ref_grad = _reference(form, W, lp, pred, batches_ok, w)
    assert math.isfinite(ref_loss)
    loss, grad = _device(form, W, lp, pred, batches, w)
    assert not math.isfinite(loss.item())
    assert torch.isnan(grad[:, 4, :]).all()
    others = [n for n in range(N) if n != 4]
    assert torch.isfinite(grad[:, others, :]).all()
    err = H.full_rel_err(grad[:, others, :], ref_grad[:, others, :])
    print(f"\n[gate] history CTC with an infeasible label, {form}: the other strips' gradient error {err:.2e}")
    assert err <= GATE
    monkeypatch.setenv("QEA_HISTORY_CTC", "steps")
    loss_s, grad_s = _device(form, W, lp, pred, batches, w)
    assert not math.isfinite(loss_s.item())
    assert torch.equal(torch.isfinite(grad_s), torch.isfinite(grad))


def _static_inputs(W, T=31, N=9, seed=1):
    """device tensors of one sample-wise call, as tracking_utils hands them to HistoryCTCFn"""
    from qea import history
    batches = _batches(_table(W, seed=seed), W)
    pk = history.TargetBatchPacker()
    packed = pk.pack(batches, N, torch.full((N,), T, dtype=torch.int))
    dev = pk.to_device(packed[:2], torch.device("cuda"))
    depth_n, lens, offs, chars, in_len = pk.unpack(dev, N, W, packed[3])
    w = _weights("sample_wise", N, W, 3).cuda()
    lp = _log_probs(T, N, seed + 20).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    return lp, (in_len, lens, offs, chars, depth_n, w, W + 1, 1, 0, 2 * packed[4] + 1, 0)


def _run(lp, rest):
    from qea.autograd import HistoryCTCFn
    lp.grad = None
    loss = HistoryCTCFn.apply(lp, *rest)
    loss.backward()
    return loss


def test_fixed_launch_count_reproducible_and_lean():
    from qea import ops
    counts = {}
    for W in (5, 2):
        lp, rest = _static_inputs(W)
        before = ops.HISTORY_CTC_LAUNCHES["ctc"]
        _run(lp, rest)
        counts[W] = ops.HISTORY_CTC_LAUNCHES["ctc"] - before
    assert counts == {5: 3, 2: 3}, counts
    lp, rest = _static_inputs(5)
    first = _run(lp, rest).detach().clone()                                     # warm-up: the workspace exists from here on
    g_first = lp.grad.clone()
    T, N, _ = lp.shape
    ws_bytes = ops.ctc_history_workspace_bytes(T, N, 5, rest[-2])
    assert ws_bytes == (2 * T * rest[-2] + 2) * N * 5 * 8
    lp.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    second = _run(lp, rest)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    assert torch.equal(second.detach(), first) and torch.equal(lp.grad, g_first)          # bit-identical from run to run
    bound = 2 * T * N * C * 4 + ws_bytes
    print(f"\n[gate] history CTC, memory allocated during one call plus backward: {delta} bytes (bound {bound})")
    assert delta < bound, (delta, bound)


def test_graph_replay_is_bit_equal_to_eager():
    lp, rest = _static_inputs(5, seed=2)
    eager = _run(lp, rest).detach().clone()
    g_eager = lp.grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(lp, rest)
    torch.cuda.current_stream().wait_stream(side)
    lp.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = _run(lp, rest)
    for _ in range(2):
        lp.grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager) and torch.equal(lp.grad, g_eager)


def test_window_one_is_bit_equal_to_the_plain_ctc_kernels():
    """csrc/ctc.hip and csrc/ctc_history.hip run the one recursion of csrc/ctc_core.h: at W = 1 with every coefficient 0.25 (a power
    of two, so the scaling is exact) the per-problem nll, the gradient and the loss agree bit for bit with the plain kernels."""
    from qea import ops
    T, N = 80, 4
    rng = np.random.RandomState(0)
    labels = [_word(rng, 65), "", "aab", _word(rng, 5)]          # S = 131: three waves in the scan, two rounds of the gradient's staging
    in_len = [80, 3, 7, 80]
    lp = _log_probs(T, N, 31)
    y = torch.tensor([H.C2I[c] for c in "".join(labels)], dtype=torch.int)
    ys = torch.tensor([len(l) for l in labels], dtype=torch.int)
    il = torch.tensor(in_len, dtype=torch.int)
    assert torch.isfinite(torch.nn.functional.ctc_loss(lp.double(), y, il, ys, reduction="none")).all()
    off = torch.zeros(N, dtype=torch.int64)
    off[1:] = torch.cumsum(ys.long(), 0)[:-1]
    S_max = 2 * 65 + 1
    dev = "cuda"
    lpd, yd, ysd, ild = lp.to(dev), y.to(dev), ys.to(dev), il.to(dev)
    nll_p, loss_p, grad_p = torch.empty(N, device=dev), torch.empty(1, device=dev), torch.empty(T, N, C, device=dev)
    ops.ctc_loss(lpd, N * C, C, yd, off.to(dev), ild, ysd, T, N, C, 0, S_max, 0, 1.0, nll_p, loss_p, grad_p, N * C, C)
    w = torch.ones(N, 2, device=dev)
    depth_n = torch.tensor([4], dtype=torch.int, device=dev)
    loss_h, grad_h, nll_h = ops.ctc_history_loss(lpd, ild, ysd.reshape(N, 1), off.int().to(dev).reshape(N, 1), yd, depth_n, w, 2, 1, 0, S_max)
    torch.cuda.synchronize()
    assert torch.equal(nll_h[:, 0], nll_p)
    assert torch.equal(grad_h, grad_p * 0.25)
    assert torch.equal(loss_h, loss_p * 0.25)
    for n, L in enumerate(in_len):
        assert (grad_h[L:, n, :] == 0).all() and (grad_p[L:, n, :] == 0).all(), n
        assert (grad_p[:L, n, :] != 0).any(), n
    tiny = torch.finfo(torch.float32).tiny                       # no subnormal on either side of the scaling by 0.25
    for v in (nll_p, loss_p, grad_p, nll_h, loss_h, grad_h):
        assert torch.isfinite(v).all() and (v[v != 0].abs() >= tiny).all()


@pytest.mark.parametrize("why", ["weights_require_grad", "torch_ctc_loss", "label_of_130", "env_switch"])
def test_routing_back_to_the_loop(why, monkeypatch):
    from qea import ops
    from qea.loss import CTCLoss
    T, N, W = 31, 9, 3
    form = "decaying"
    table = _table(W, seed=9)
    lp, pred, w = _log_probs(T, N, 14), torch.full((N,), T, dtype=torch.int), _weights(form, N, W, 3)
    self = _self(form, W, torch.device("cuda"))
    wd = w.cuda()
    if why == "weights_require_grad":
        wd.requires_grad_(True)
    elif why == "torch_ctc_loss":
        self.primary_loss_fn = torch.nn.CTCLoss()
    elif why == "label_of_130":
        T = 280
        lp, pred = _log_probs(T, N, 14), torch.full((N,), T, dtype=torch.int)
        table[6][0] = _word(np.random.RandomState(1), 130)
        self.primary_loss_fn = torch.nn.CTCLoss()                               # the project's own CTC refuses 130 characters by itself
    else:
        monkeypatch.setenv("QEA_HISTORY_CTC", "steps")
    batches = _batches(table, W)
    if why == "label_of_130":
        from qea import history
        assert history.ctc_route(lp.cuda(), wd, W, 130, CTCLoss()) == "steps" and history.ctc_route(lp.cuda(), wd, W, 127, CTCLoss()) == "fused"
    ref_loss, ref_grad = _reference(form, W, lp, pred, batches, w)
    assert math.isfinite(ref_loss)
    before = ops.HISTORY_CTC_LAUNCHES["ctc"]
    loss, grad = _device(form, W, lp, pred, batches, wd, self=self)
    assert ops.HISTORY_CTC_LAUNCHES["ctc"] == before                            # the counter did not move
    e = (_rel(loss.item(), ref_loss), H.full_rel_err(grad, ref_grad))
    gate_grad = GATE
    if isinstance(self.primary_loss_fn, torch.nn.CTCLoss):
        # these two cases run ATen's own CTC kernels, whose recursion is fp32: alpha, beta and nll are sums of T terms of magnitude
        # up to |nll|, each step rounded to 2^-24 relative, and the gradient takes exp(alpha + beta + nll - lp), so its relative
        # error is the absolute error of that exponent: about 2^-24 * |nll| * sqrt(3 T) for three independent sums of T roundings.
        # That is 7e-5 at T = 31 (the project's gate holds) and 2e-3 at T = 280 with the 130-character label.
        nll_max = max(torch.nn.functional.ctc_loss(lp.double()[:, idx, :], y, pred[idx], ys, reduction="none").max().item() for y, ys, idx in batches)
        gate_grad = max(GATE, 2.0 ** -24 * nll_max * math.sqrt(3 * T))
    print(f"\n[gate] history CTC routed to the loop ({why}): loss error {e[0]:.2e} (gate {GATE:.0e}), gradient error {e[1]:.2e} (gate {gate_grad:.1e})")
    assert e[0] <= GATE and e[1] <= gate_grad, (why, e, gate_grad)
    if why == "weights_require_grad":
        assert wd.grad is not None and wd.grad.abs().sum() > 0                  # the loop carries the weights' graph
    if why == "label_of_130":
        # with the project's own loss the loop is taken as well: its per-depth call is the one that refuses the label
        import tracking_utils as tu
        from qea._lib import QeaError
        with pytest.raises(QeaError, match="127"):
            tu.weighted_ctc_loss(_self(form, W, torch.device("cuda")), lp.cuda(), pred, batches, wd)
        assert ops.HISTORY_CTC_LAUNCHES["ctc"] == before
