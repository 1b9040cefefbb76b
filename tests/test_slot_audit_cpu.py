"""tests/slot_audit.py can fail: stub ops functions with the real signatures (no GPU) make one clean call sequence and one sequence per
seeded defect; every defect is reported with its call index, function and parameter, the clean sequence reports nothing.  Also: every
abs-max parameter of qea.ops has a role in the auditor's table, and conv_spec.conv_written is conv_igemm_spec's own mask."""
import functools
import inspect
import types

import numpy as np
import pytest
import torch

import conv_spec as S
import slot_audit as A


def test_every_amax_parameter_of_ops_has_a_role():
    """a new slot parameter of a public function of qea.ops cannot go unaudited; nor does the table name what ops does not have"""
    from qea import ops
    assert A.unaudited(ops) == []
    for fn, param in A.TABLE:
        assert param in inspect.signature(getattr(ops, fn)).parameters, (fn, param)
    for fn in list(A.RETURNED) + list(A.FILTER) + list(A.ANSWERS_WHETHER_FILLED):
        assert inspect.isfunction(getattr(ops, fn))
    probe = types.ModuleType("probe_ops")
    exec("def new_kernel(x, ld, out_amax=None):\n    pass\n", probe.__dict__)
    probe.new_kernel.__module__ = "probe_ops"
    assert A.unaudited(probe) == [("new_kernel", "out_amax")]


@pytest.mark.parametrize("name", sorted(S.CONV_CASES))
def test_written_mask_is_the_statements_own(name):
    _, written = S.conv_case_spec(name)
    assert np.array_equal(S.conv_written(S.conv_case(name).d, written.size), written)


# ----------------------------------------------------------------------------- stub ops
def _region(t, rows, cols):
    """what a stub reads or stores: the first `cols` channels of `rows` rows of a [rows][ld] tensor or of a channel slice of one"""
    return t.reshape(-1, t.shape[-1])[:rows, :cols]


def _raise(slot, region, how="max"):
    """a stub producer's slot update.  how: "max" (the contract), "skip" (never touched), "store" (overwritten with its own maximum)"""
    if slot is None or how == "skip":
        return
    m = region.abs().max()
    slot.copy_(torch.maximum(slot, m) if how == "max" else m)


def stub_ops(how):
    """a module of stubs with qea.ops' signatures: each `stores` what its output tensor already holds (the sequence fills the tensors)
    and updates its slots as how[function name] says (default "max")."""
    from qea import ops
    mod = types.ModuleType("stub_ops")

    def stub(name, body):
        real = getattr(ops, name)
        sig = inspect.signature(real)

        @functools.wraps(real)
        def f(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            return body(types.SimpleNamespace(**b.arguments), how.get(name, "max"))
        f.__module__ = mod.__name__
        setattr(mod, name, f)

    def conv_igemm(a, h):
        rows, cols = (4 * a.B * a.OH * a.OW, a.N // 4) if a.out_mode == S.OUT_CONVT else (a.B * a.OH * a.OW, a.N)      # (every row map
        _raise(a.y_amax, _region(a.y, rows, cols), h)                                                               # stores all rows)
        if a.pool is not None:
            _raise(a.pool[3], _region(a.pool[0], a.B * (a.OH // 2) * (a.OW // a.pool[2]), a.N), h)
    stub("conv_igemm", conv_igemm)
    stub("conv_wgrad", lambda a, h: None)
    stub("bn_apply", lambda a, h: _raise(a.amax, _region(a.a, a.M, a.C_), h))
    stub("bn_bwd", lambda a, h: _raise(a.amax, _region(a.dy, a.M, a.C_), h))
    stub("maxpool_fwd", lambda a, h: _raise(a.amax, _region(a.y, a.B * (a.H // a.kh) * (a.W // a.kw), a.C_), h))
    stub("lstm_layer_fwd_any", lambda a, h: a.mode == "seq" and (_raise(a.y_amax, a.y, h) or True))
    stub("absmax", lambda a, h: _region(a.x, a.M, a.Cc).abs().max().reshape(1) * (0.5 if h == "half" else 1.0))
    stub("filter_absmax", lambda a, h: _region(a.w, a.M, a.Cc).abs().max().reshape(1) * (2.0 ** 12 if h == "loose" else 1.0))
    return mod


def sequence(mod, consumer_slot="carried", small_group=1.0):
    """A miniature of the engines' sharing on CPU tensors, B = 2 images of 4 x 4:
      0 maxpool_fwd        8x8x8 -> p [32][8], slot s_p
      1 conv_igemm         p (s_p) -> y [32][16], no slot                      consumer
      2 filter_absmax      the scale source of call 1's filter
      3 bn_apply           group 0 of y -> skip half of cat [32][32], slot s_cat
      4 bn_apply           group 1, the same slot                              two launches raise one slot
      5 conv_igemm CONVT   d [8][8] (s_d) -> the up half of cat, slot s_cat    producer on a shared slot
      6 conv_igemm         cat (s_cat) -> z                                    consumer of both halves
      7 bn_bwd             -> dy, slot s_dy
      8 conv_wgrad         p = dy (s_dy), q = cat (s_cat)                      two consumers
      9 lstm_layer_fwd_any mode "bf3": answers False, leaves no record
     10 absmax             the fallback: its return value bounds what it was asked about
     11 conv_wgrad         p = seq (the returned tensor), q = p of call 0
    small_group: group 1's skip rows and the up half are scaled by it, so that group 0's launch alone holds the maximum of cat.
    consumer_slot: what call 1 is handed: "carried" (s_p), "zero" (a fresh slot), "half" / "loose" (s_p times 0.5 / 2^12)."""
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g)
    slot = lambda: torch.zeros(1)
    a0, p, s_p = rnd(128, 8), rnd(32, 8), slot()
    mod.maxpool_fwd(a0, 8, p, 8, 2, 8, 8, 8, 2, 2, amax=s_p)
    handed = {"carried": s_p, "zero": slot(), "half": s_p * 0.5, "loose": s_p * 2.0 ** 12}[consumer_slot]
    y, w = rnd(32, 16), rnd(16, 72)
    conv = dict(B=2, H=4, W=4, OH=4, OW=4, KH=3, KW=3, pad=(1, 1))
    mod.conv_igemm(p, w, y, Cin=8, N=16, ldx=8, ldy=16, x_amax=handed, w_src=("fwd", w), **conv)
    mod.filter_absmax(("fwd", w), w, 72, 16, 72)               # (the real conv_igemm asks from inside; the auditor takes it at any depth)
    cat, s_cat = rnd(32, 32), slot()
    cat[16:, 16:] *= small_group
    cat[:, :16] *= small_group
    skip = cat[:, 16:]
    coef = rnd(2, 16)
    for b0 in (0, 16):
        mod.bn_apply(y[b0:b0 + 16], 16, skip[b0:b0 + 16], 32, 16, 16, coef[0], coef[1], relu=True, amax=s_cat)
    d, s_d, wt = rnd(8, 8), slot(), rnd(64, 8)
    s_d.copy_(d.abs().max())
    mod.conv_igemm(d, wt, cat, B=2, H=2, W=2, Cin=8, OH=2, OW=2, N=64, KH=1, KW=1, ldx=8, ldy=32, x_amax=s_d, y_amax=s_cat, out_mode=S.OUT_CONVT)
    z = rnd(32, 16)
    mod.conv_igemm(cat, rnd(16, 288), z, Cin=32, N=16, ldx=32, ldy=16, x_amax=s_cat, **conv)
    dy, s_dy = rnd(32, 16), slot()
    mod.bn_bwd(z, 16, None, 0, y, 16, 32, 16, coef[0], coef[0], coef[1], True, None, None, dy, 16, amax=s_dy)
    mod.conv_wgrad(dy, cat, rnd(16, 288), B=2, PH=4, PW=4, QH=4, QW=4, R=16, Cc=32, KH=3, KW=3, pad=(1, 1), ldp=16, ldq=32, p_amax=s_dy, q_amax=s_cat)
    seq, s_seq = rnd(4, 2, 16), slot()
    if not mod.lstm_layer_fwd_any(rnd(4, 2, 64), rnd(4, 2, 16), seq, None, "bf3", 4, 2, y_amax=s_seq):
        s_seq = mod.absmax(seq, 16, 8, 16)
    mod.conv_wgrad(seq, p, rnd(16, 8), B=1, PH=1, PW=8, QH=1, QW=8, R=16, Cc=8, KH=1, KW=1, ldp=16, ldq=8, p_amax=s_seq, q_amax=s_p)


def audited(how=None, **kw):
    mod = stub_ops(how or {})
    with A.auditing(mod, sync=lambda: None) as audit:
        sequence(mod, **kw)
    return audit, [(v.index, v.fn, v.param, v.rule) for v in A.violations(audit.records)]


def test_clean_sequence_reports_nothing():
    audit, bad = audited()
    assert bad == []
    assert audit.calls == ["maxpool_fwd", "conv_igemm", "filter_absmax", "bn_apply", "bn_apply", "conv_igemm", "conv_igemm", "bn_bwd", "conv_wgrad",
                           "lstm_layer_fwd_any", "absmax", "conv_wgrad"]
    roles = [(r.index, r.fn, r.param, r.role) for r in audit.records]
    assert roles == [(0, "maxpool_fwd", "amax", "producer"), (1, "conv_igemm", "x_amax", "consumer"), (2, "filter_absmax", "return", "filter"),
                     (3, "bn_apply", "amax", "producer"), (4, "bn_apply", "amax", "producer"), (5, "conv_igemm", "x_amax", "consumer"),
                     (5, "conv_igemm", "y_amax", "producer"), (6, "conv_igemm", "x_amax", "consumer"), (7, "bn_bwd", "amax", "producer"),
                     (8, "conv_wgrad", "p_amax", "consumer"), (8, "conv_wgrad", "q_amax", "consumer"), (10, "absmax", "return", "returned"),
                     (11, "conv_wgrad", "p_amax", "consumer"), (11, "conv_wgrad", "q_amax", "consumer")]
    # the numbers are those of the tensors: the CONVT launch stores only the up half, the consumer of cat reads both halves
    by = {(r.index, r.param): r for r in audit.records}
    assert by[(6, "x_amax")].before == by[(6, "x_amax")].region == by[(5, "y_amax")].after
    assert by[(5, "y_amax")].region <= by[(5, "y_amax")].after and by[(4, "amax")].before == by[(3, "amax")].after
    assert A.summary(audit.records)[:3] == (7, 6, 1)


@pytest.mark.parametrize("defect, kw, how, want", [
    ("a consumer slot left at 0", dict(consumer_slot="zero"), {}, [(1, "conv_igemm", "x_amax", "a")]),
    ("a consumer slot at half the region maximum", dict(consumer_slot="half"), {}, [(1, "conv_igemm", "x_amax", "a")]),
    ("a consumer slot 2^12 above the region maximum", dict(consumer_slot="loose"), {}, [(1, "conv_igemm", "x_amax", "b")]),
    # the second group's launch stores its own, smaller maximum over the first group's: the launch itself, then both readers of cat
    ("a producer that lowers a shared slot", dict(small_group=2.0 ** -6), {"bn_apply": "store"},
     [(4, "bn_apply", "amax", "c"), (6, "conv_igemm", "x_amax", "a"), (8, "conv_wgrad", "q_amax", "a")]),
    ("a producer that skips its slot", {}, {"bn_bwd": "skip"}, [(7, "bn_bwd", "amax", "c"), (8, "conv_wgrad", "p_amax", "a")]),
    ("a fallback pass that returns half the maximum", {}, {"absmax": "half"}, [(10, "absmax", "return", "c"), (11, "conv_wgrad", "p_amax", "a")]),
    ("a filter scaled from 2^12 above its own maximum", {}, {"filter_absmax": "loose"}, [(2, "filter_absmax", "return", "b")]),
])
def test_seeded_defect_is_reported_by_name(defect, kw, how, want):
    audit, bad = audited(how, **kw)
    assert bad == want, defect
    for v in A.violations(audit.records):
        assert f"call {v.index} {v.fn}({v.param})" in v.text


def test_auditing_restores_the_module():
    mod = stub_ops({})
    before = dict(vars(mod))
    with pytest.raises(ZeroDivisionError), A.auditing(mod, sync=lambda: None):
        assert mod.conv_igemm is not before["conv_igemm"]
        1 / 0
    assert dict(vars(mod)) == before
