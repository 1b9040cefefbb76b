"""The abs-max slots of the split-fp16 launches, audited call by call while an engine runs.

In "split_f16" mode every GEMM-class launch scales its operands by a power of two read from a 4-byte slot that the operand's producer
was to fill (csrc/common.h: qea_f16_scale; qea/ops.py: AmaxPool; qea/act.py: Act.amax).  The contract: when the launch runs, the slot
is >= the largest finite magnitude of what the launch reads, and not more than 2^10 above it.

    with auditing() as audit:
        ... forward + backward ...
    audit.records            # one Record per audited slot, in call order
    violations(audit.records)

auditing() wraps the public functions of qea.ops the way tools/engine_schedule.py::recording does (a depth counter keeps the calls made
from OUTSIDE qea.ops, everything run inside SideStream.run included) and treats every abs-max parameter by its role in TABLE:

  consumer   conv_igemm x_amax, conv_wgrad p_amax / q_amax.  Before the call: synchronize, read the slot, take the finite abs-max of
             the region the launch reads, from the call's own arguments.
  producer   the slot is read before the call; after the call and a synchronize the slot and the finite abs-max of the stored region
             are recorded.  The stored region of a convolution (NHWC, TBC, the transposed-conv scatter) is conv_spec.conv_written's.
             A wrapper that answers False / None ("not taken": conv_c1_fwd_pool, the lstm_layer_*_any of a path without the fused
             abs-max) has produced nothing and leaves no record.
  returned   the tensor ops.absmax returns to an outside caller, against the region it was asked about.
  filter     the scale source ops.filter_absmax hands a filter's fp16 planes (at any depth: the engines never call it themselves),
             against the filter's own finite abs-max; the record carries the index of the outside call that asked for the planes.

Every number comes from plain torch ops (abs, isfinite, max) on strided views built from the arguments, never from ops.absmax."""
import collections
import contextlib
import functools
import inspect
import types

import torch

import conv_spec as S

LOOSE = 2.0 ** 10      # the largest looseness at which test_operand_scale_gpu.py holds the project's gates unchanged

Record = collections.namedtuple("Record", "index fn param role before after region")
# consumer: before = after = the slot when the launch starts.  producer / returned: the slot before and after.  filter: after = the
# scale source.  region: the finite abs-max of what is read (consumer, filter) / stored (producer, returned).
Violation = collections.namedtuple("Violation", "index fn param rule text")


def finite_absmax(v):
    """largest finite |v| as a Python float (exact: fp32 -> double), 0.0 where there is none"""
    a = v.detach().abs()
    a = a[torch.isfinite(a)]
    return float(a.max()) if a.numel() else 0.0


def _rows(t, rows, C, ld):
    """the [rows][C] operand with pixel stride ld that starts at t's first element"""
    return torch.as_strided(t, (rows, C), (ld, 1))


@functools.lru_cache(maxsize=64)
def _conv_mask(B, OH, OW, N, ldy, out_mode, device):
    rows, cols = (4 * B * OH * OW, N // 4) if out_mode == S.OUT_CONVT else (B * OH * OW, N)
    d = types.SimpleNamespace(B=B, OH=OH, OW=OW, N=N, ldy=ldy, out_mode=out_mode, y_guard=0, y_off=0)
    return torch.from_numpy(S.conv_written(d, (rows - 1) * ldy + cols)).to(device)


def _conv_stored(a):
    """what a conv_igemm launch stores, by conv_spec's written mask over the floats from y's first element on"""
    mask = _conv_mask(a["B"], a["OH"], a["OW"], a["N"], a["ldy"], a["out_mode"], a["y"].device)
    return torch.as_strided(a["y"], (mask.numel(),), (1,))[mask]


def _tb(t):
    """a dense [T][B][C] sequence tensor as rows"""
    return t.reshape(-1, t.shape[-1])


Entry = collections.namedtuple("Entry", "role slot region")


def _p(name):
    return lambda a: a[name]


# (function, parameter) -> Entry(role, the slot among the bound arguments `a`, the region it bounds)
TABLE = {
    ("conv_igemm", "x_amax"): Entry("consumer", _p("x_amax"), lambda a: _rows(a["x"], a["B"] * a["H"] * a["W"], a["Cin"], a["ldx"])),
    ("conv_wgrad", "p_amax"): Entry("consumer", _p("p_amax"), lambda a: _rows(a["p"], a["B"] * a["PH"] * a["PW"], a["R"], a["ldp"])),
    ("conv_wgrad", "q_amax"): Entry("consumer", _p("q_amax"), lambda a: _rows(a["q"], a["B"] * a["QH"] * a["QW"], a["Cc"], a["ldq"])),
    ("conv_igemm", "y_amax"): Entry("producer", _p("y_amax"), _conv_stored),
    # (the slot of the pooled output travels in the `pool` tuple: (pooled, ldpool, kw, slot))
    ("conv_igemm", "pool"): Entry("producer", lambda a: a["pool"][3] if a["pool"] is not None else None,
                                  lambda a: _rows(a["pool"][0], a["B"] * (a["OH"] // 2) * (a["OW"] // a["pool"][2]), a["N"], a["pool"][1])),
    ("bn_apply", "amax"): Entry("producer", _p("amax"), lambda a: _rows(a["a"], a["M"], a["C_"], a["lda"])),
    ("bn_apply_pool", "amax"): Entry("producer", _p("amax"), lambda a: _rows(a["a"], a["B"] * a["H"] * a["W"], a["C_"], a["lda"])),
    ("bn_apply_pool", "pooled_amax"): Entry("producer", _p("pooled_amax"),
                                            lambda a: _rows(a["pooled"], a["B"] * (a["H"] // a["kh"]) * (a["W"] // a["kw"]), a["C_"], a["ldp"])),
    ("bn_bwd", "amax"): Entry("producer", _p("amax"), lambda a: _rows(a["dy"], a["M"], a["C_"], a["lddy"])),       # both forms: own sums / partials
    ("bn_bwd_pool", "amax"): Entry("producer", _p("amax"), lambda a: _rows(a["dy"], a["B"] * a["H"] * a["W"], a["C_"], a["lddy"])),
    ("maxpool_fwd", "amax"): Entry("producer", _p("amax"),
                                   lambda a: _rows(a["y"], a["B"] * (a["H"] // a["kh"]) * (a["W"] // a["kw"]), a["C_"], a["ldy"])),
    ("maxpool_bwd", "amax"): Entry("producer", _p("amax"), lambda a: _rows(a["dx"], a["B"] * a["H"] * a["W"], a["C_"], a["lddx"])),
    ("conv_c1_fwd_pool", "pooled_amax"): Entry("producer", _p("pooled_amax"),
                                               lambda a: _rows(a["pooled"], a["B"] * (a["H"] // 2) * (a["W"] // 2), a["Co"], a["ldp"])),
    ("lstm_layer_fwd_any", "y_amax"): Entry("producer", _p("y_amax"), lambda a: _tb(a["y"])),
    ("lstm_layer_bwd_any", "g_amax"): Entry("producer", _p("g_amax"), lambda a: _tb(a["gates"])),      # overwritten with the gate gradients
}
RETURNED = {"absmax": lambda a: _rows(a["x"], a["M"], a["Cc"], a["ld"])}
FILTER = {"filter_absmax": lambda a: _rows(a["w"], a["M"], a["Cc"], a["ld"])}
ANSWERS_WHETHER_FILLED = ("conv_c1_fwd_pool", "lstm_layer_fwd_any", "lstm_layer_bwd_any")


def unaudited(mod):
    """the (function, parameter) pairs of mod's public functions whose parameter name contains "amax" and has no role in TABLE"""
    out = []
    for n, f in vars(mod).items():
        if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_"):
            out += [(n, p) for p in inspect.signature(f).parameters if "amax" in p and (n, p) not in TABLE]
    return out


class Audit:
    def __init__(self):
        self.records, self.calls = [], []        # calls: the name of every outside call, by index


@contextlib.contextmanager
def auditing(mod=None, sync=None):
    """Inside: every call into `mod` (default qea.ops) from outside it is audited; yields the Audit.  sync: torch.cuda.synchronize."""
    if mod is None:
        from qea import ops as mod
    sync = torch.cuda.synchronize if sync is None else sync
    audit, depth = Audit(), [0]
    saved = {n: f for n, f in vars(mod).items() if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_")}

    def wrap(name, fn):
        sig = inspect.signature(fn)
        entries = [(p, e) for (f, p), e in TABLE.items() if f == name]

        @functools.wraps(fn)
        def call(*args, **kw):
            outside = depth[0] == 0
            if not (outside or name in FILTER):
                return fn(*args, **kw)
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            a = b.arguments
            if outside:
                audit.calls.append(name)
            index = len(audit.calls) - 1
            live = [(p, e, e.slot(a)) for p, e in entries] if outside else []
            live = [(p, e, s) for p, e, s in live if s is not None]
            before = {}
            if live:
                sync()
                for p, e, s in live:
                    before[p] = float(s.item())
                    if e.role == "consumer":
                        audit.records.append(Record(index, name, p, "consumer", before[p], before[p], finite_absmax(e.region(a))))
            depth[0] += 1
            try:
                out = fn(*args, **kw)
            finally:
                depth[0] -= 1
            produced = [(p, e, s) for p, e, s in live if e.role == "producer"]
            if produced and not (name in ANSWERS_WHETHER_FILLED and not out):
                sync()
                for p, e, s in produced:
                    audit.records.append(Record(index, name, p, "producer", before[p], float(s.item()), finite_absmax(e.region(a))))
            if outside and name in RETURNED:
                sync()
                audit.records.append(Record(index, name, "return", "returned", 0.0, float(out.item()), finite_absmax(RETURNED[name](a))))
            if name in FILTER:
                sync()
                audit.records.append(Record(index, name, "return", "filter", 0.0, float(out.item()), finite_absmax(FILTER[name](a))))
            return out
        return call
    for n, f in saved.items():
        setattr(mod, n, wrap(n, f))
    try:
        yield audit
    finally:
        for n, f in saved.items():
            setattr(mod, n, f)


def violations(records, loose=LOOSE):
    """-> [Violation] in record order.  Rules:
    a  a consumer's slot (a filter's scale source) is below the finite abs-max of what the launch reads — compared exactly: a slot is
       a maximum of stored fp32 values;
    b  it is more than `loose` times above it (region max > 0);
    c  a producer left its slot below what it was, below what it stored, or at anything but max(slot before, stored max)."""
    out = []
    for r in records:
        def bad(rule, text):
            out.append(Violation(r.index, r.fn, r.param, rule, f"call {r.index} {r.fn}({r.param}): {text}"))
        if r.role in ("consumer", "filter"):
            what = "slot" if r.role == "consumer" else "scale source"
            if not r.after >= r.region:
                bad("a", f"{what} {r.after!r} < region max {r.region!r}" + (" (slot still 0)" if r.after == 0.0 else ""))
            elif r.region > 0 and r.after > loose * r.region:
                bad("b", f"{what} {r.after!r} is {r.after / r.region:.4g} x the region max {r.region!r} (cap {loose:g})")
        else:
            if r.after < r.before:
                bad("c", f"slot lowered from {r.before!r} to {r.after!r} (stored max {r.region!r})")
            elif r.after < r.region:
                bad("c", f"slot {r.after!r} < stored max {r.region!r}" + (" (slot not raised)" if r.after == r.before else ""))
            elif r.after != max(r.before, r.region):
                bad("c", f"slot {r.after!r} is not max(before {r.before!r}, stored max {r.region!r})")
    return out


def summary(records):
    """(consumer records, producer records, filter records, worst slot / region max of a consumer, "call i fn(param)" that has it,
    worst scale source / own maximum of a filter), the ratios over the records with region max > 0"""
    n = collections.Counter("producer" if r.role == "returned" else r.role for r in records)
    worst = {"consumer": (0.0, "-"), "filter": (0.0, "-")}
    for r in records:
        if r.role in worst and r.region > 0 and r.after / r.region > worst[r.role][0]:
            worst[r.role] = (r.after / r.region, f"call {r.index} {r.fn}({r.param})")
    return n["consumer"], n["producer"], n["filter"], *worst["consumer"], worst["filter"][0]
