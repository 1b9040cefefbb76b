"""The launch list of the UNet and CRNN engines: every call they make into qea.ops during one forward + backward, with its arguments,
over a fixed list of cases.  Needs a GPU.

    python tools/engine_schedule.py <commit> > tests/golden/engine_schedule.json     # pin the schedule of the engines in the tree

tests/test_engine_schedule_gpu.py re-records the cases and requires every list to equal the pinned one: a change to the host side of
the engines that claims "same behaviour, same speed" shows it as "the same calls with the same arguments in the same order".

How a call is recorded.  Every public module-level function of qea.ops is wrapped; a depth counter keeps only the calls made from
OUTSIDE qea.ops (what a wrapper calls in turn is its own business), which includes everything run inside SideStream.run.  An entry is
[name, args, kwargs] after binding to the wrapper's signature with its defaults filled in, so that a default left out and the same
value spelled out are one call.  A tensor becomes [dtype, shape, stride, storage offset, role]: role is P:/G:/B:<name> when pointer
and shape equal a named parameter, its .grad or a buffer of the model, else "".  The storage offset pins group slices, the strided
halves of the concat buffers and the order of the abs-max slots.  Numbers, bools, strings and None stand for themselves, sequences
and dicts are recorded recursively, a callable is "fn", a device its name, any other object its class name.
Stored per case: each call's name and the first 12 hex digits of the SHA-256 of its canonical JSON.

Cases: inputs [B,1,32,128] from tests/helpers.synth_images, seeded model states (oracle.model_oracle.seeded_state), each case in
split_f16 and in split_bf16 (abs-max slots are None in the latter)."""
import contextlib
import functools
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MODES = ("split_f16", "split_bf16")
# name -> (model, batch, train mode (CRNN: of its BatchNorms), input gradient / grad enabled, forward kwargs, engine switches turned off)
CASES = {
    "unet/train": ("unet", 4, True, True, {}, ()),
    "unet/train_bn_groups2": ("unet", 4, True, True, {"bn_groups": 2}, ()),
    "unet/eval_no_grad": ("unet", 4, False, False, {}, ()),
    "unet/eval_grad": ("unet", 4, False, True, {}, ()),
    "unet/train_switches_off": ("unet", 4, True, True, {}, ("FUSE_BN_POOL", "FUSE_POOL_BWD", "FUSE_BN_BWD_SUMS", "FUSE_EVAL_BN")),
    "crnn/train": ("crnn", 4, True, True, {}, ()),
    "crnn/replica_groups3": ("crnn", 6, True, True, {"replica_groups": 3}, ()),
    "crnn/replica_groups3_backward_group2": ("crnn", 6, True, True, {"replica_groups": 3, "backward_group": 2}, ()),
    "crnn/group_sizes_3_1_2": ("crnn", 6, True, True, {"group_sizes": [3, 1, 2]}, ()),
    "crnn/bn_eval_grad": ("crnn", 4, False, True, {}, ()),
    "crnn/train_switches_off": ("crnn", 4, True, True, {}, ("FUSE_POOL", "FUSE_POOL_BWD", "FUSE_C1_BWD")),
}


def _roles(model):
    import torch
    out = {}
    for tag, named in (("B:", model.named_buffers()), ("G:", ((n, p.grad) for n, p in model.named_parameters())), ("P:", model.named_parameters())):
        for n, t in named:
            if torch.is_tensor(t) and t.numel():
                out[(t.data_ptr(), tuple(t.shape))] = tag + n
    return out


def _enc(v, roles):
    import torch
    if torch.is_tensor(v):
        return [str(v.dtype), list(v.shape), list(v.stride()), v.storage_offset(), roles.get((v.data_ptr(), tuple(v.shape)), "")]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [_enc(e, roles) for e in v]
    if isinstance(v, dict):
        return {str(k): _enc(e, roles) for k, e in v.items()}
    if isinstance(v, torch.device):
        return str(v)
    return "fn" if callable(v) else type(v).__name__


@contextlib.contextmanager
def recording(model, log):
    """Inside: every call into qea.ops from outside it is appended to `log` as [name, args, kwargs]."""
    from qea import ops
    depth = [0]
    saved = {n: f for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*a, **kw):
            if depth[0] == 0:
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                roles = _roles(model)
                log.append([name, _enc(b.args, roles), _enc(b.kwargs, roles)])
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return call
    for n, f in saved.items():
        setattr(ops, n, wrap(n, f))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)


def digest(entry):
    return hashlib.sha256(json.dumps(entry, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:12]


def _run(case, seed, *, spec=None, width=128, state=None, inputs=None, out_grad=None, around=None, passes=None):
    """One forward (+ backward) of a case -> its log.  The keywords are for tests that run the same cases under other instruments
    (tests/test_slot_audit_gpu.py) and change nothing that is recorded when left alone: spec = a CASES tuple of its own, width = the
    image width, state / inputs / out_grad = a transform of the seeded state dict / the input images / the output gradient,
    around(model, log) = the context the passes run in instead of recording(model, log), passes(model, x, forward kwargs) = what runs
    there instead of one forward and one backward."""
    import torch
    import helpers as H
    from oracle import model_oracle as mo
    from qea import crnn_engine, unet_engine
    kind, B, train, grad, kwargs, off = CASES[case] if spec is None else spec
    engine = unet_engine if kind == "unet" else crnn_engine
    x = H.synth_images(B, seed, w=width)
    x = (x if inputs is None else inputs(x)).cuda()
    state = state or (lambda sd: sd)
    if kind == "unet":
        from models.model_unet import UNet
        net = UNet()
        net.load_state_dict(state(mo.seeded_state(mo.unet_state_shapes(), seed + 1)))
        net = net.cuda().train(train)
    else:
        from models.model_crnn import CRNN
        net = CRNN(95, False)
        net.load_state_dict(state(mo.seeded_state(mo.crnn_state_shapes(), seed + 1)))
        net = net.cuda().train()
        net.register_backward_hook(net.backward_hook)
        if not train:
            for m in net.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.eval()
        x.requires_grad_()
    log = []
    before = {name: getattr(engine, name) for name in off}
    try:
        for name in off:
            setattr(engine, name, False)
        with (around or recording)(net, log), torch.set_grad_enabled(grad):
            out = net(x, **kwargs) if passes is None else passes(net, x, kwargs)
            if grad and passes is None:
                g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 2))
                out.backward((g if out_grad is None else out_grad(g)).cuda())
            torch.cuda.synchronize()
    finally:
        for name, v in before.items():
            setattr(engine, name, v)
    return log


def record():
    """{"<case>/<mfma mode>": [[name, args, kwargs], ...]}"""
    from qea import ops
    out = {}
    prev = ops.mfma_mode()
    try:
        for mode in MODES:
            ops.set_mfma_mode(mode)
            for i, case in enumerate(CASES):
                out[f"{case}/{mode}"] = _run(case, 300 + 10 * i)
    finally:
        ops.set_mfma_mode(prev)
    return out


def digests(rec):
    return {k: [[e[0], digest(e)] for e in log] for k, log in rec.items()}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    d = digests(record())
    sys.stdout.write('{"recorded_at": %s,\n"cases": %s,\n"calls": {\n' % (json.dumps(sys.argv[1]), json.dumps(CASES)))
    sys.stdout.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(d.items())))
    sys.stdout.write("\n}}\n")
