"""The UNet and CRNN engines under tests/slot_audit.py: in a real forward and backward, does the abs-max slot a split-fp16 launch is
handed bound the data it reads?  (The kernel tests show that a producer leaves the exact maximum in the slot it is given, the layer
tests that the layers pass slots through, the schedule test pins WHICH slot every call gets; none of them looks at the number in the
slot when its consumer runs.)

Cases: the 11 of tools/engine_schedule.py::CASES with its inputs, seeds and seeded states, the UNet and the CRNN at B = 4 and
W = 64 / 256, the UNet in eval mode with a gradient at 32x128, and the cases below in which the sharers of one slot differ in magnitude;
every case with a backward once more with the output gradient times 2^-27.  In "split_f16", with no exception list (slot_audit.violations):

  (a) every consumer's slot >= the finite abs-max of the region the launch reads, compared exactly;
  (b) slot <= 2^10 * region max (region max > 0), and a filter's scale source <= 2^10 * the filter's own maximum;
  (c) every producer leaves max(slot before, stored max) in its slot, to the bit;
  (d) every conv_igemm / conv_wgrad call the recorded call list of the same run shows with a slot has its consumer record.
In the QEA_SPLIT=bf16 and QEA_MFMA=f32 sessions every abs-max argument of every call is None (e) and the rest of the module is skipped;
the default session switches to those two modes for that one test.

Magnitude cases, measured on the fp64 oracle (oracle/model_oracle.py) on the CPU at the seeds used here, max |.| ratios as powers of two:

  concat halves    unet/train with upconv{l}.weight and .bias times 2^6 / 2^-6.  Up half : skip half of cat_4..1 is 2^5.99, 2^6.16,
                   2^6.16, 2^6.03 / 2^-6.01, 2^-6.00, 2^-5.95, 2^-6.00 (unscaled: within 2^0.31): >= 2^4 in both directions.  The halves
                   of dcat_l do NOT follow, at this or any exponent: both are the input gradient of the decoder's first conv, whose
                   BatchNorm divides the scale out again (2^0.25, 2^-0.13, 2^-0.09, 2^0.11 / 2^-0.09, 2^-0.03, 2^-0.04, 2^-0.16).  What
                   does separate them is that conv's filter: decoder{l}.dec{l}conv1.weight[:, :c] (the up half's input channels)
                   times 2^6 / 2^-6 gives dcat_4..1 up : skip = 2^6.25, 2^5.87, 2^5.91, 2^6.11 / 2^-6.09, 2^-6.03, 2^-6.04, 2^-6.16 —
                   added here as the dcat cases.
  statistics       crnn/group_sizes_3_1_2 and unet/train_bn_groups2 with the images of the first / the last group times 2^-6.  Per-group
  groups           max |dy| of the CRNN's BatchNorm1 (conv5's output gradient) then spreads 2^5.09 / 2^4.46 (unscaled 2^0.91); of
                   BatchNorm2 2^0.29 / 2^0.50, and no more at 2^-10 or 2^-14 (2^0.64, 2^0.63 / 2^0.42, 2^0.44): BatchNorm1 has divided
                   the scale out, it is not eps that holds it back, so no power of two reaches 2^4 there.  UNet: the first stage
                   (enc1conv1) spreads 2^5.53 / 2^5.99, every later one < 2^1 for the same reason.
  backward_group   crnn/replica_groups3_backward_group2 with the same per-group scaling (groups of 2): the sliced copies carry the
                   whole batch's bounds.

One defect is seeded on the device (numerically harmless: a zero slot means scale 1): ops.maxpool_fwd withholds its slot on
crnn/train_switches_off, and the audit reports the conv_igemm that reads the pooled tensor, under (a), and nothing before it.

The black-box counterpart: the backward of unet/train, crnn/train and crnn/group_sizes_3_1_2 run twice from the same forward state on
zeroed gradient buffers, with g and with 2^k g (k = -27, +6): every parameter gradient (and the CRNN's dx) of the second run is 2^k
times the first, bit for bit.  Every kernel on the path is homogeneous on its own (tests/test_operand_scale_gpu.py) or linear with
exact power-of-two scaling; a stale, zero or foreign slot breaks the equality.

pytest -s prints one row per case: the audited consumer / producer / filter records, the worst slot / region max and its launch, and
the wall time (the table of DESIGN.md section 4)."""
import contextlib
import functools
import inspect
import os
import sys
import time

import pytest
import torch

import slot_audit as A

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
try:
    import engine_schedule as E
finally:
    sys.path.pop(0)

G_SCALE = 2.0 ** -27                      # the gradient scale of tests/test_operand_scale_gpu.py


def _scaled(match, k, part=None):
    """state transform: the entries whose name `match` accepts times 2^k (part(name, tensor) -> the slice to scale, default all of it)"""
    def f(sd):
        out = dict(sd)
        for n, t in sd.items():
            if match(n):
                t = t.clone()
                (t if part is None else part(n, t)).mul_(2.0 ** k)
                out[n] = t
        return out
    return f


def _group_scaled(b0, nb, k):
    """input transform: images b0 .. b0 + nb times 2^k"""
    def f(x):
        x = x.clone()
        x[b0:b0 + nb] *= 2.0 ** k
        return x
    return f


def _variants():
    """name -> keywords of E._run (case, seed and the transforms)"""
    v = {}
    for i, case in enumerate(E.CASES):
        v[case] = dict(case=case, seed=300 + 10 * i)                                   # the seeds of E.record()
    for j, (kind, w) in enumerate((("unet", 64), ("unet", 256), ("crnn", 64), ("crnn", 256))):
        v[f"{kind}/train_b4_w{w}"] = dict(case=f"{kind}/train", seed=500 + 10 * j, width=w)
    v["unet/eval_need_grad_32x128"] = dict(case="unet/eval_grad", seed=540, spec=("unet", 4, False, True, {}, ()))
    seed = lambda case: v[case]["seed"]
    for tag, k in (("up", 6), ("down", -6)):
        v[f"unet/train/upconv_{tag}"] = dict(case="unet/train", seed=seed("unet/train"), state=_scaled(lambda n: n.startswith("upconv"), k))
        v[f"unet/train/dcat_{tag}"] = dict(case="unet/train", seed=seed("unet/train"),
                                           state=_scaled(lambda n: n.startswith("decoder") and n.endswith("conv1.weight"), k,
                                                         part=lambda n, t: t[:, :t.shape[1] // 2]))
    for case, parts in (("crnn/group_sizes_3_1_2", [(0, 3), (3, 1), (4, 2)]), ("unet/train_bn_groups2", [(0, 2), (2, 2)]),
                        ("crnn/replica_groups3_backward_group2", [(0, 2), (2, 2), (4, 2)])):
        for tag, (b0, nb) in (("first", parts[0]), ("last", parts[-1])):
            v[f"{case}/{tag}_group_small"] = dict(case=case, seed=seed(case), inputs=_group_scaled(b0, nb, -6))
    for name, kw in list(v.items()):
        if (kw.get("spec") or E.CASES[kw["case"]])[3]:                                 # every backward once more at the small gradient scale
            v[name + "/g_2^-27"] = dict(kw, out_grad=lambda g: g * G_SCALE)
    return v


VARIANTS = _variants()


@pytest.fixture(scope="module")
def split_f16():
    """the session's mode is the default one; else the module has test_other_modes_hand_out_no_slots only"""
    from qea import ops
    if ops.mfma_mode() != "split_f16":
        pytest.skip(f"abs-max slots exist in split_f16 only (this session: {ops.mfma_mode()})")


@contextlib.contextmanager
def _instruments(net, log, box, inner=contextlib.nullcontext):
    """the schedule recorder and the auditor around the same passes (`inner`: a context entered inside both)"""
    with E.recording(net, log), A.auditing() as audit:
        box.append(audit)
        with inner():
            yield


def _audited(name, inner=contextlib.nullcontext):
    box = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    log = E._run(**VARIANTS[name], around=functools.partial(_instruments, box=box, inner=inner))
    return log, box[0], time.perf_counter() - t0


def _named(entry):
    """a recorded call [name, args, kwargs] -> {parameter: recorded value}"""
    from qea import ops
    params = inspect.signature(getattr(ops, entry[0])).parameters.values()
    positional = [p.name for p in params if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    assert len(positional) == len(entry[1])
    return {**dict(zip(positional, entry[1])), **entry[2]}


def _consumer_slots(log):
    """{(call index, function, parameter)} of the consumer slots the recorded call list shows"""
    want = set()
    for i, entry in enumerate(log):
        for (fn, param), e in A.TABLE.items():
            if fn == entry[0] and e.role == "consumer" and _named(entry)[param] is not None:
                want.add((i, fn, param))
    return want


_printed = []


def _row(name, audit, seconds):
    if not _printed:
        _printed.append(True)
        print(f"\n{'case':66} consumers producers filters  worst slot/max  at{'':28} worst filter  seconds")
    c, p, f, worst, where, wf = A.summary(audit.records)
    print(f"{name:66} {c:9d} {p:9d} {f:7d} {worst:15.4g}  {where:30} {wf:12.4g} {seconds:8.2f}")


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_slots_bound_what_the_launches_read(split_f16, name):
    """(a), (b), (c), (d) of the module docstring on one case"""
    log, audit, seconds = _audited(name)
    _row(name, audit, seconds)
    assert audit.calls == [e[0] for e in log], "the auditor and the schedule recorder saw different calls"
    have = {(r.index, r.fn, r.param) for r in audit.records if r.role == "consumer"}
    want = _consumer_slots(log)
    assert want and have == want and len(have) == sum(r.role == "consumer" for r in audit.records), \
        f"(d) consumer slots in the call list without a record: {sorted(want - have)}; records without a call: {sorted(have - want)}"
    assert any(r.role == "producer" for r in audit.records) and any(r.role == "filter" for r in audit.records)
    bad = A.violations(audit.records)
    assert not bad, f"{len(bad)} of {len(audit.records)} audited slots break the contract:\n" + "\n".join(v.text for v in bad[:20])


def test_a_withheld_slot_is_seen_at_its_consumer(split_f16):
    """ops.maxpool_fwd passes its launch no slot (crnn/train_switches_off: every pool is a launch of its own): the first thing the audit
    reports is the conv_igemm that reads the first pooled tensor, under (a), with the slot still 0 and the pooled tensor's maximum."""
    from qea import ops
    pooled = []

    @contextlib.contextmanager
    def withheld():
        real = ops.maxpool_fwd                                   # (the instrumented one: the audit sees a call without a slot)

        def maxpool_fwd(x, ldx, y, ldy, B, H, W, C_, kh, kw, amax=None):
            pooled.append((y, B * (H // kh) * (W // kw), C_, ldy))
            return real(x, ldx, y, ldy, B, H, W, C_, kh, kw, amax=None)
        ops.maxpool_fwd = maxpool_fwd
        try:
            yield
        finally:
            ops.maxpool_fwd = real
    log, audit, _ = _audited("crnn/train_switches_off", inner=withheld)
    assert len(pooled) == 4 and not [r for r in audit.records if r.fn == "maxpool_fwd"]
    first_pool = audit.calls.index("maxpool_fwd")
    reader = audit.calls.index("conv_igemm", first_pool)
    bad = A.violations(audit.records)
    assert bad and tuple(bad[0][:4]) == (reader, "conv_igemm", "x_amax", "a"), "\n".join(v.text for v in bad[:5])
    rec = next(r for r in audit.records if (r.index, r.param) == (reader, "x_amax"))
    y, rows, C, ld = pooled[0]
    assert rec.before == 0.0 and rec.region == A.finite_absmax(torch.as_strided(y, (rows, C), (ld, 1))) > 0
    assert all(v.rule == "a" and v.fn in ("conv_igemm", "conv_wgrad") for v in bad), "only readers of pooled tensors are reported"


def test_other_modes_hand_out_no_slots():
    """(e): in the QEA_SPLIT=bf16 and QEA_MFMA=f32 sessions every abs-max argument of every call of every case is None; the default
    session switches to both modes itself (as tools/engine_schedule.py::record does) and holds them to the same."""
    from qea import ops
    session = ops.mfma_mode()
    try:
        for mode in (("split_bf16", "f32") if session == "split_f16" else (session,)):
            ops.set_mfma_mode(mode)
            for i, case in enumerate(E.CASES):
                for j, entry in enumerate(E._run(case, 300 + 10 * i)):
                    args = _named(entry)
                    slots = {p: args[p] for p in args if "amax" in p}
                    if args.get("pool") is not None:
                        slots["pool[3]"] = args["pool"][3]
                    assert all(s is None for s in slots.values()), f"{case}: call {j} {entry[0]} carries {slots} in mode {mode}"
    finally:
        ops.set_mfma_mode(session)


# ----------------------------------------------------------------------------- the backward is homogeneous in powers of two
def _state_tensors(o, out, seen):
    """every tensor an engine's saved context holds that is not a parameter (dicts, sequences, Acts, BatchNorm stages)"""
    from qea.act import Act
    from qea.batchnorm import Stage
    if id(o) in seen:
        return
    seen.add(id(o))
    if torch.is_tensor(o):
        if not isinstance(o, torch.nn.Parameter):
            out.append(o)
    elif isinstance(o, dict):
        for v in o.values():
            _state_tensors(v, out, seen)
    elif isinstance(o, (list, tuple)):
        for v in o:
            _state_tensors(v, out, seen)
    elif isinstance(o, Act):                                      # (no temporary containers: `seen` holds ids of live objects only)
        _state_tensors(o.t, out, seen)
        _state_tensors(o.amax, out, seen)
    elif isinstance(o, Stage):
        _state_tensors(vars(o), out, seen)


def _first_difference(a, b, f):
    """the first audited launch of run b whose operand and slot are neither those of run a (a tensor of the forward) nor f times them"""
    for r, s in zip(a, b):
        if (r.index, r.fn, r.param) != (s.index, s.fn, s.param):
            return f"the runs make different calls from call {r.index} {r.fn} / {s.index} {s.fn} on"
        if (s.region, s.after) not in ((r.region, r.after), (f * r.region, f * r.after)):
            return (f"call {r.index} {r.fn}({r.param}, {r.role}): region max {r.region!r} -> {s.region!r}, slot {r.after!r} -> {s.after!r} "
                    f"(factor {f!r})")
    return "no audited operand or slot differs by more than the factor"


@pytest.mark.parametrize("k", [-27, 6])
@pytest.mark.parametrize("case", ["unet/train", "crnn/train", "crnn/group_sizes_3_1_2"])
def test_backward_is_homogeneous_in_powers_of_two(split_f16, case, k):
    f = 2.0 ** k
    kw = VARIANTS[case]
    kind = E.CASES[case][0]
    got = {}

    def passes(net, x, kwargs):
        from qea.params import ensure_flat
        eng = net._engine()
        ensure_flat(net)
        with torch.no_grad():
            if kind == "unet":
                out, ctx = eng.forward(x.detach().contiguous(), True, True, groups=kwargs.get("bn_groups", 1))
                back = lambda g: eng.backward(ctx, g)
            else:
                out, ctx = eng.forward(x.detach().contiguous(), True, True, groups=kwargs.get("group_sizes", 1))
                ctx["grad_group"] = -1
                back = lambda g: eng.backward(ctx, g, True, True)
            g = torch.randn(out.shape, generator=torch.Generator().manual_seed(kw["seed"] + 2)).cuda()
            held = []
            _state_tensors(ctx, held, set())
            torch.cuda.synchronize()
            keep = [t.clone() for t in held]

            def run(g, audited=False):
                for t, c in zip(held, keep):                     # (the CRNN's backward overwrites the gate buffers it was handed)
                    t.copy_(c)
                net.zero_grad()
                with (A.auditing() if audited else contextlib.nullcontext()) as audit:
                    dx = back(g)
                    torch.cuda.synchronize()
                grads = {n: p.grad.clone() for n, p in net.named_parameters()}
                if dx is not None:
                    grads["dx"] = dx.clone()
                return grads, audit
            one, _ = run(g)
            two, _ = run(g * f)
            assert all(v.abs().max() > 0 for v in one.values() if v.dim() > 1), "a weight gradient of the unit-scale run is all zero"
            off = [n for n in one if not torch.equal(one[n] * f, two[n])]
            if off:
                got["first"] = _first_difference(run(g, True)[1].records, run(g * f, True)[1].records, f)
            got["off"] = off
        return out
    E._run(**kw, around=lambda net, log: contextlib.nullcontext(), passes=passes)
    assert not got["off"], (f"{len(got['off'])} gradients of the 2^{k} run are not 2^{k} times the unit run's: {got['off'][:8]}; "
                            f"first audited launch that differs: {got['first']}")
