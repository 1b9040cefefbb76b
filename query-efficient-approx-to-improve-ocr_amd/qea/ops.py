"""Thin tensor-level wrappers over the C ABI (include/qea_hip.h).

Every function takes CUDA (ROCm) fp32 tensors, passes raw device pointers + the current
stream to libqea_hip.so and raises on any error.  No CPU implementation exists here.
"""
import ctypes as C
import os
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import _lib, beam

OUT_NHWC, OUT_TBC, OUT_CONVT = 0, 1, 2
PROF_CONV_IGEMM, PROF_CONV_WGRAD, PROF_LSTM_STEP = 0, 1, 2

_ws = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.QeaError("qea ops need CUDA tensors (there is no CPU path)")
    if t.dtype not in (torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8):
        raise _lib.QeaError(f"unsupported dtype {t.dtype}")
    return t.data_ptr()


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream): kernels on different streams never share one.
    A buffer handed out while the current stream is capturing is baked into the graph as a raw pointer: it is noted for that capture
    (see _pin_captured) so that a later growth, which drops it from _ws, cannot hand its memory back to the allocator while a graph
    that writes it is alive (the weight-gradient side stream is persistent and runs eager steps of other shapes between replays).
    Freed, it would be handed to the next allocation on that stream, and torch.cuda.graph() empties the cache on entry, so the next
    capture would return it to the driver: the earlier graph's replays would then write unmapped memory."""
    if device.type != "cuda":
        raise _lib.QeaError("qea ops need CUDA tensors (there is no CPU path)")
    key = (device.type, device.index, _stream())
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    if torch.cuda.is_current_stream_capturing():
        _pin_captured(buf)
    return buf


_pinned = {}     # id -> workspace buffer touched by a capture made outside qea.graph.GraphedStep: kept for the process


def _pin_captured(buf):
    """GraphedStep captures (CAPTURE["pins"] set) hold their buffers for the graph's lifetime; any other capture for the process.
    Cost: at most one retained buffer per growth event of a (device, stream) entry, never a private workspace per graph."""
    pins = CAPTURE["pins"] if CAPTURE["token"] is not None else None
    (pins if pins is not None else _pinned)[id(buf)] = buf


def split_planes(x, ld, M, Cc):
    """fp32 rows [M][ld] (Cc channels used) -> the P3 pre-split format (include/qea_hip.h: qea_split_planes) as a byte tensor."""
    L = _lib.lib()
    out = torch.empty(L.qea_split_planes_bytes(M, Cc), dtype=torch.uint8, device=x.device)
    _lib.check(L.qea_split_planes(_ptr(x), ld, M, Cc, out.data_ptr(), _stream()), "qea_split_planes")
    return out


FUSE_BN_STATS = {"on": True}     # tests switch the fused statistics epilogue off to compare with the separate pass
PRESPLIT = {"on": True, "x": False}     # tests / tools: "on" = pre-split filters (default), "x" = pre-split activations too

# ---- derived forms of WEIGHTS (dgrad filter layouts, transposes, P3 planes), kept until the weights change.
# A weight tensor changes either through torch (load_state_dict, copy_: its _version moves) or through the fused Adam kernel
# (raw pointer writes: qea.optim.FusedAdam.step calls bump_weight_epoch()).  With the CRNN frozen in Phase B its derived forms
# are built once, not once per step (round 1 re-derived 390 filter layouts per step).  Inside a hipGraph capture the cache is
# scoped to that capture (see weight_cached): a replay re-derives every form from the weights it finds, once per weight epoch.
# RULE for any other writer: a write that goes through `p.data` (torch.distributed.broadcast(p.data), p.data.copy_, an EMA) or
# through a raw pointer moves neither _version nor the epoch — call bump_weight_epoch() after it (qea.graph.GraphedStep does
# after every replay, TrainerCore after the start-up broadcast, qea.params.FlatState when it re-homes the parameters).
_wcache = {}
_wepoch = [0]
WEIGHT_CACHE = {"on": True}
# token: the current GraphedStep capture; pins / flat: what that capture baked in as raw pointers (workspace buffers, the models'
# FlatStates), collected by workspace() and qea.params.ensure_flat() and kept by the GraphedStep
CAPTURE = {"token": None, "pins": None, "flat": None}


MODEL_EPOCHS = {"on": os.environ.get("QEA_MODEL_EPOCHS", "1") != "0"}   # 0: every raw-pointer writer makes ALL derived forms stale (round-3 behaviour)


def bump_weight_epoch(params=None):
    """Derived weight forms are stale from here on.  params: the parameters a raw-pointer writer has just touched — when every one of
    them lives in a flat parameter buffer, only the forms of those models go stale (the fused Adam of one model must not make
    the other model's filters be re-packed: round 4 found every form built twice per step); otherwise, or without
    params, everything."""
    if params is not None and MODEL_EPOCHS["on"]:
        from .params import flat_state_of
        seen = {}
        for p_ in params:
            fs = flat_state_of(p_, check=False)
            if fs is None:
                seen = None
                break
            seen[id(fs)] = fs
        if seen:
            for fs in seen.values():
                fs.epoch += 1
            return
    _wepoch[0] += 1


def _model_epoch(w):
    from .params import flat_state_of
    fs = flat_state_of(w, check=False)
    return fs.epoch if fs is not None else 0


def weight_cached(kind, w, build, also=(), extra=None, batch=None):
    """build() -> tensor(s) derived from the weight tensor `w` (and the tensors in `also`) only; cached per (kind, the
    tensor OBJECT) until one of them changes.  Entries die with the tensor object (weakref), so a new tensor that happens
    to reuse the address of a freed one can never hit.  `extra`: any further hashable the value depends on."""
    token = None
    if torch.cuda.is_current_stream_capturing():
        # inside a capture made by qea.graph.GraphedStep a derived form is built once per weight epoch OF THAT CAPTURE (the build
        # launches are part of the graph and run before their uses on every replay); an entry carries the capture's token, so
        # neither eager code nor another capture can ever hit it.  Any other capture caches nothing.
        token = CAPTURE["token"]
        if token is None:
            return build()
    if not WEIGHT_CACHE["on"]:
        return build()
    key = (kind, id(w))
    ver = _cache_ver(w, also, token, extra)
    hit = _wcache.get(key)
    if hit is not None and hit[0] == ver and hit[2]() is w:
        return hit[1]
    if batch is not None and BATCH_FORMS["on"] and extra is None and w.is_cuda and (w.data_ptr() & 15) == 0:
        return _batched_forms(key, w, also, batch, token)
    val = build()
    _wcache[key] = (ver, val, weakref.ref(w, lambda _r, key=key: _wcache.pop(key, None)))
    return val


# ---- derived forms of one model in ONE launch (round 4).  A form that qea_weight_forms_multi can make is described ONCE, by a FormJob.
# On a miss weight_cached hands the record of an aligned CUDA weight to _batched_forms, which registers it under its cache key and
# builds it with the multi entry — together with every other stale registered form of the SAME group whose weight lives in the same
# flat parameter buffer (= the same model), so the later requests of the step hit the cache; a weight outside a flat buffer is a launch
# of one job.  FormJob.build (the form's single entry point) runs where nothing is cached or batched: QEA_BATCH_FORMS=0, the cache off,
# a capture without a token, an unaligned or ad-hoc filter.  Groups: "flip" (flip-transposed filters) and "pack" (fragment planes; a
# pack of a flipped filter asks for the flipped filter first, which runs the flip group).
BATCH_FORMS = {"on": os.environ.get("QEA_BATCH_FORMS", "1") != "0"}
_form_jobs = {}


class FormJob:
    """plain data (no reference to the weight: a registered job must not keep its tensor alive).  kind, dims: of qea_wform_job;
    srck: what the form is made from — "self" = the weight itself, "flipT" = its flip-transposed form (dims of the 3x3 pack: N, Cin of
    the input-gradient conv), None = a tensor only the caller can derive (never batched); out: shape or byte count;
    amax: (ld, M, Cc) of the abs-max pass over the weight (srck None: over the caller's tensor), or None."""
    __slots__ = ("group", "kind", "dims", "srck", "out", "amax", "wref", "also")

    def __init__(self, group, kind, dims, srck, out, amax):
        self.group, self.kind, self.dims, self.srck, self.out, self.amax = group, kind, dims, srck, out, amax

    def parts(self, w, given=None):
        """-> (source, output, abs-max or None).  w: the model weight the form is cached with, None for an ad-hoc filter; given: the
        source where the caller holds it — required when w or srck is None, nobody else can derive it then."""
        if given is not None:
            src = given
        elif self.srck == "self":
            src = w
        else:
            assert self.srck == "flipT" and w is not None, "a form without a derivable source needs the source"
            src = flip_transposed(w, self.dims[1], self.dims[0], 3, 3)
        out = torch.empty(self.out, device=src.device) if isinstance(self.out, tuple) else torch.empty(self.out, dtype=torch.uint8, device=src.device)
        if self.amax is None:
            return src, out, None
        if w is None:
            return src, out, absmax(src, *self.amax)
        # ONE rule: of the model weight (the flipped filter holds the same elements), of the source where it is not derived by srck
        return src, out, filter_absmax((self.srck, w), w if self.srck else src, *self.amax)

    def build(self, w, given=None):
        """this form alone, through its single entry point"""
        L = _lib.lib()
        src, out, am = self.parts(w, given)
        if self.kind == 0:
            filter_flip_transpose(src, out, *self.dims)
        elif self.kind == 1:
            _lib.check(L.qea_pack_frag_planes_f16(_ptr(src), self.dims[0], self.dims[1], _ptr(am), out.data_ptr(), _stream()), "qea_pack_frag_planes_f16")
        else:
            _lib.check(L.qea_pack_frag_planes_f16_1x1(_ptr(src), self.dims[0], self.dims[1], _ptr(am), out.data_ptr(), _stream()), "qea_pack_frag_planes_f16_1x1")
        return out


def _cache_ver(w, also, token, extra=None):
    return (w.data_ptr(), w._version, _wepoch[0], _model_epoch(w), _stream(), token, extra) + tuple((id(t), t.data_ptr(), t._version, _model_epoch(t)) for t in also)


def _batched_forms(key, w, also, job, token):
    """builds `key` and every other stale registered form of its group and model; returns key's tensor"""
    from .params import flat_state_of
    job.wref, job.also = weakref.ref(w), tuple(weakref.ref(t) for t in also)
    _form_jobs[key] = job
    fs = flat_state_of(w, check=False)
    todo = [(key, w, also, job)]
    if fs is not None:
        dead = []                                            # jobs of weights that are gone: dropped here, never from a finalizer
        for k2, j2 in _form_jobs.items():                    # (a callback that edits the dict could run inside this very loop)
            w2 = j2.wref()
            also2 = tuple(r() for r in j2.also)
            if w2 is None or any(t is None for t in also2):
                dead.append(k2)
                continue
            if k2 == key or j2.group != job.group or len(todo) >= 64 or flat_state_of(w2, check=False) is not fs:
                continue
            hit = _wcache.get(k2)
            if hit is not None and hit[0] == _cache_ver(w2, also2, token) and hit[2]() is w2:
                continue
            todo.append((k2, w2, also2, j2))
        for k2 in dead:
            del _form_jobs[k2]
    jobs = (_lib.WformJob * len(todo))()
    outs, keep = [], []
    for i, (_k, wi, _a, ji) in enumerate(todo):
        src, out, am = ji.parts(wi)
        keep.append((src, am))
        outs.append(out)
        jobs[i].src, jobs[i].dst, jobs[i].amax, jobs[i].kind = src.data_ptr(), out.data_ptr(), (am.data_ptr() if am is not None else None), ji.kind
        jobs[i].a, jobs[i].b, jobs[i].c, jobs[i].d = ji.dims
    _lib.check(_lib.lib().qea_weight_forms_multi(jobs, len(todo), _stream()), "qea_weight_forms_multi")
    for (ki, wi, ai, _j), out in zip(todo, outs):
        _wcache[ki] = (_cache_ver(wi, ai, token), out, weakref.ref(wi, lambda _r, key=ki: _wcache.pop(key, None)))
    return outs[0]


def flip_transposed(w, Co, Ci, KH, KW):
    """wt[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci]: the filter of the input-gradient convolution (cached)."""
    job = FormJob("flip", 0, (Co, Ci, KH, KW), "self", (Ci, KH, KW, Co), None)
    return weight_cached(("flipT", Co, Ci, KH, KW), w, lambda: job.build(w), batch=job)


def transposed(w, R, Cc):
    """out[c][r] = w[r][c] (cached)."""
    def build():
        out = torch.empty(Cc, R, device=w.device)
        transpose2d(w, out, R, Cc)
        return out
    return weight_cached(("T", R, Cc), w, build)


def _src_cached(kind, dims, w_src, build, batch=None):
    """build() -> a form of conv_igemm's filter `w`: cached under (kind, w_src's kind, *dims) with the weight(s) w_src names until one of
    them changes; built afresh for a filter nobody named the source of (w_src None)."""
    if w_src is None:
        return build()
    return weight_cached((kind, w_src[0]) + dims, w_src[1], build, also=tuple(w_src[2]) if len(w_src) > 2 else (), batch=batch)


def _frag_planes_f16(d, kind, x, w, w_src, x_amax):
    """conv_igemm on a tile that reads the filter from fp16 fragment planes (kind 1: 3x3 LDS-halo kernel, kind 2: 1x1 LDS tile):
    points `d` at the cached planes of `w` and at the input's abs-max; returns both tensors (the caller holds them over the launch).
    The planes are batchable when `w` is a model's weight itself or its flip-transposed form (the input-gradient filter: the flipped
    filter, itself a cached form, is asked for first, which builds all stale flipped filters of the model in one launch)."""
    L = _lib.lib()
    N, Cin = d.N, d.Cin
    K = 9 * Cin if kind == 1 else Cin
    srck, amax = None, (K, N, K)
    if w_src is not None and len(w_src) == 2:
        if w_src[0] == "fwd" and w_src[1].data_ptr() == w.data_ptr():
            srck = "self"
        elif kind == 1 and w_src[0] == "flipT" and d.KH == 3 and d.KW == 3:
            srck, amax = "flipT", (9 * N, Cin, 9 * N)
    job = FormJob("pack", kind, (N, Cin, 0, 0), srck, (L.qea_pack_frag_planes_f16_bytes if kind == 1 else L.qea_pack_frag_planes_f16_1x1_bytes)(N, Cin), amax)
    frag = _src_cached("fragf16" if kind == 1 else "frag1x1", (N, Cin), w_src, lambda: job.build(w_src[1] if w_src is not None else None, w),
                       batch=job if srck else None)
    # the input's abs-max: carried by the tensor's producer (x_amax), else one pass over the input here
    xmax = x_amax if x_amax is not None else absmax(x, d.ldx, d.B * d.H * d.W, Cin)
    d.w_frag_planes, d.x_absmax = frag.data_ptr(), xmax.data_ptr()
    return frag, xmax


def _conv_desc(x, w, y, *, B, H, W, Cin, OH, OW, N, KH, KW, pad, stride, ldx, ldy, scale=None, bias=None, mask=None, ldmask=0, relu=False,
               accumulate=False, out_mode=OUT_NHWC, tile=0):
    """the qea_conv_desc of a launch, before the routing below fills in planes, abs-max slots and epilogue outputs"""
    return _lib.ConvDesc(x=_ptr(x), w=_ptr(w), y=_ptr(y), scale=_ptr(scale), bias=_ptr(bias), mask=_ptr(mask),
                         B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, N=N, KH=KH, KW=KW, pad_h=pad[0], pad_w=pad[1],
                         stride_h=stride[0], stride_w=stride[1], ldx=ldx, ldy=ldy, ldmask=ldmask,
                         relu=int(relu), accumulate=int(accumulate), out_mode=out_mode, tile=tile, x_planes=None, w_planes=None, stats=None,
                         w_frag_planes=None)


def conv_igemm(x, w, y, *, B, H, W, Cin, OH, OW, N, KH, KW, pad=(0, 0), stride=(1, 1), ldx, ldy,
               scale=None, bias=None, mask=None, ldmask=0, relu=False, accumulate=False,
               out_mode=OUT_NHWC, tile=0, x_planes=None, w_planes=None, w_src=None, want_stats=False, x_amax=None, y_amax=None, pool=None,
               bwd_stats=None):
    """x_planes / w_planes: operands already in the P3 format (a caller that uses a tensor in several launches splits it
    once); when the launch runs on a split-bf16 tile and they are not given, they are made here (one HBM pass each).
    w_src = (kind, weight tensor[, (further weight tensors)]): `w` is a function of that weight (and of the further ones) only (itself:
    kind "fwd"; its cached flip_transposed / transposed form: "flipT" / "T"; the BiLSTM's concatenated projections: "catT" of both
    directions), so its planes are cached with it until one of them changes.
    want_stats: ask for the fused BatchNorm-statistics epilogue; returns (partials [blocks][N][2] fp64, blocks) when the chosen
    kernel has it, else None (the caller then runs bn_train_stats over y).
    pool = (pooled, ldpool, kw, amax slot or None): the 2 x kw max-pool of y leaves with the epilogue (same bits as maxpool_fwd on y) —
    only for a launch conv_can_pool(...) accepted.
    bwd_stats = (y_ref, ld, stat64 [2][N], scale, shift): y (this launch's output) is the gradient entering a train-mode BatchNorm+ReLU
    whose input was y_ref: the epilogue also leaves the two reductions of that BatchNorm's backward; returns (partials, blocks) for
    bn_bwd(partials=...), or None when this launch has no such epilogue (the caller's bn_bwd then makes its own pass)."""
    L = _lib.lib()
    d = _conv_desc(x, w, y, B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, N=N, KH=KH, KW=KW, pad=pad, stride=stride, ldx=ldx, ldy=ldy, scale=scale,
                   bias=bias, mask=mask, ldmask=ldmask, relu=relu, accumulate=accumulate, out_mode=out_mode, tile=tile)
    frag = xmax = None
    wants = L.qea_conv_igemm_wants_frag_planes(C.byref(d)) if PRESPLIT["on"] else 0
    if wants == 2 and SPLIT_F16["on"] and x_planes is None and w_planes is None:
        # 1x1 GEMM on the 128-row LDS tile (tile 26, fp16 split only): filter [N][K] in fragment-order fp16 planes (cached)
        frag, xmax = _frag_planes_f16(d, 2, x, w, w_src, x_amax)
    elif wants == 1 and SPLIT_F16["on"]:
        # 3x3 layer on the split LDS-halo kernel: its filter in fragment-order planes (a few hundred KB, cached)
        frag, xmax = _frag_planes_f16(d, 1, x, w, w_src, x_amax)
    elif wants == 1:
        def build():
            out = torch.empty(L.qea_pack_frag_planes_bytes(N, Cin), dtype=torch.uint8, device=x.device)
            _lib.check(L.qea_pack_frag_planes(_ptr(w), N, Cin, out.data_ptr(), _stream()), "qea_pack_frag_planes")
            return out
        frag = _src_cached("frag", (N, Cin), w_src, build)
        d.w_frag_planes = frag.data_ptr()
    elif PRESPLIT["on"] and Cin % 16 == 0 and L.qea_conv_igemm_uses_split_bf16(C.byref(d)):
        K = KH * KW * Cin
        if N * K * 6 < (1 << 31) - 256:
            # the FILTER's planes are made once per weight update and shared by every M-tile; an activation is consumed by one
            # launch, so it is only taken pre-split when the caller has the planes anyway (PRESPLIT["x"]: tools / tests)
            if x_planes is None and PRESPLIT.get("x") and B * H * W * Cin * 6 < (1 << 31) - 256:
                x_planes = split_planes(x, ldx, B * H * W, Cin)
            f16 = SPLIT_F16["on"] and x_planes is None and w_planes is None and N * K * 4 < (1 << 31) - 256
            if w_planes is None:
                build = (lambda: split_planes_f16(w, K, N, K, w_src)) if f16 else (lambda: split_planes(w, K, N, K))
                w_planes = _src_cached("planesf16" if f16 else "planes", (N, K), w_src, build)
            d.x_planes = x_planes.data_ptr() if x_planes is not None else None
            d.w_planes = w_planes.data_ptr()
            if f16:                                       # hybrid tile on the two-way fp16 split: the activations' abs-max
                xmax = x_amax if x_amax is not None else absmax(x, ldx, B * H * W, Cin)
                d.x_absmax = xmax.data_ptr()
    if y_amax is not None:
        d.y_absmax = y_amax.data_ptr()
    if pool is not None:
        d.pool_y, d.ldpool, d.pool_kw = pool[0].data_ptr(), pool[1], pool[2]
        d.pool_absmax = pool[3].data_ptr() if pool[3] is not None else None
    partials = None
    if bwd_stats is not None and wants == 1 and d.x_absmax and FUSE_BN_STATS["on"]:
        blocks = L.qea_conv_igemm_stats_blocks(C.byref(d))
        if blocks > 0:
            partials = torch.empty(blocks + 256, N, 2, dtype=torch.float64, device=x.device)   # + QEA_BN_PARTIAL_SCRATCH_ROWS
            d.stats = partials.data_ptr()
            d.bst_y, d.ldbst, d.bst_stat64 = bwd_stats[0].data_ptr(), bwd_stats[1], bwd_stats[2].data_ptr()
            d.bst_scale, d.bst_shift = bwd_stats[3].data_ptr(), bwd_stats[4].data_ptr()
    elif want_stats and FUSE_BN_STATS["on"]:
        blocks = L.qea_conv_igemm_stats_blocks(C.byref(d))
        if blocks > 0:
            partials = torch.empty(blocks + 256, N, 2, dtype=torch.float64, device=x.device)   # + QEA_BN_PARTIAL_SCRATCH_ROWS
            d.stats = partials.data_ptr()
    _lib.check(L.qea_conv_igemm(C.byref(d), _stream()), "qea_conv_igemm")
    return (partials, partials.shape[0] - 256) if partials is not None else None


def conv_can_pool(*, B, H, W, Cin, N, kw, ldx, ldy, mask=None):
    """True when the 3x3 pad-1 layer of this shape can carry the 2 x kw max-pool that follows it in its epilogue (conv_igemm's pool=):
    the two-way fp16 split is on and the LDS-halo kernel has the instance."""
    if not (PRESPLIT["on"] and SPLIT_F16["on"] and mfma_mode() == "split_f16") or mask is not None:
        return False
    d = _conv_desc(None, None, None, B=B, H=H, W=W, Cin=Cin, OH=H, OW=W, N=N, KH=3, KW=3, pad=(1, 1), stride=(1, 1), ldx=ldx, ldy=ldy)
    return bool(_lib.lib().qea_conv_igemm_can_pool(C.byref(d), kw))


def conv_wgrad(p, q, dw, *, B, PH, PW, QH, QW, R, Cc, KH, KW, pad=(0, 0), stride=(1, 1), ldp, ldq,
               accumulate=False, splits=0, tile=0, p_amax=None, q_amax=None, dbias=None):
    """p_amax / q_amax: device scalars holding the abs-max of p / q when the caller has them (the two-way fp16 split of the
    nine-tap kernel needs both); in "split_f16" mode a missing one is computed here (one pass over the tensor).
    dbias [R]: the bias gradient (column sums of p), same `accumulate`: inside the launch where the kernel has it (the producer /
    consumer nine-tap form), else one colsum pass here."""
    L = _lib.lib()
    d = _lib.WgradDesc(p=_ptr(p), q=_ptr(q), dw=_ptr(dw), workspace=None, workspace_bytes=0,
                       B=B, PH=PH, PW=PW, QH=QH, QW=QW, R=R, C=Cc, KH=KH, KW=KW, pad_h=pad[0], pad_w=pad[1],
                       stride_h=stride[0], stride_w=stride[1], ldp=ldp, ldq=ldq, accumulate=int(accumulate),
                       splits=splits, tile=tile)
    # the library knows which kernel this descriptor routes to: the abs-max passes are paid only where that kernel reads them
    if SPLIT_F16["on"] and mfma_mode() != "f32" and L.qea_conv_wgrad_wants_absmax(C.byref(d)):
        if p_amax is None:
            p_amax = absmax(p, ldp, B * PH * PW, R)
        if q_amax is None:
            q_amax = absmax(q, ldq, B * QH * QW, Cc)
        d.p_absmax, d.q_absmax = p_amax.data_ptr(), q_amax.data_ptr()
    fused = dbias is not None and bool(L.qea_conv_wgrad_fuses_bias(C.byref(d)))
    if fused:
        d.dbias = dbias.data_ptr()
    need = L.qea_conv_wgrad_workspace_bytes(C.byref(d))
    if need:
        ws = workspace(need, p.device)
        d.workspace = ws.data_ptr()
        d.workspace_bytes = ws.numel()
    _lib.check(L.qea_conv_wgrad(C.byref(d), _stream()), "qea_conv_wgrad")
    if dbias is not None and not fused:                  # (behind the launch: a refused call leaves dbias as it found it)
        colsum(p, ldp, B * PH * PW, R, dbias, accumulate=accumulate)


# "split_f16" (default since round 3): the LDS-halo 3x3 kernels take the TWO-way fp16 split (ABI v6: three MFMAs per product,
# operands scaled by powers of two from their abs-max); every other GEMM-class launch as in "split_bf16".  QEA_SPLIT=bf16 in the
# environment keeps the three-way bf16 split everywhere.
SPLIT_F16 = {"on": os.environ.get("QEA_SPLIT", "f16").lower() != "bf16"}


def set_mfma_mode(mode):
    """"split_bf16" (default dispatch), "split_f16" (as split_bf16 with the two-way fp16 split in the LDS-halo convs) or "f32"
    (every product on the fp32 MFMA); returns the previous mode's name."""
    lib_mode = {"split_bf16": 0, "split_f16": 0, "f32": 1}[mode]
    prev_name = mfma_mode()
    prev = _lib.lib().qea_set_mfma_mode(lib_mode)
    if prev < 0:
        _lib.check(prev, "qea_set_mfma_mode")
    SPLIT_F16["on"] = mode == "split_f16"
    return prev_name


def mfma_mode():
    m = ("split_bf16", "f32")[_lib.lib().qea_set_mfma_mode(-1)]
    return "split_f16" if (m == "split_bf16" and SPLIT_F16["on"]) else m


class AmaxPool:
    """Zero-filled 4-byte slots for producer-carried abs-max values: one allocation + one memset per forward / backward pass.
    A pool lives for one pass and keeps every buffer it has handed slots out of for that long: a weight gradient pending on the side
    stream reads its slots without listing them in SideStream.run's `reads`, and every pass ends in join()."""

    def __init__(self, device, n=192, on=True):
        self.on = on
        self.buf = torch.zeros(n, device=device) if on else None
        self.full = []                                            # the buffers whose slots ran out
        self.used = 0

    def __call__(self):
        if not self.on:
            return None
        if self.used == self.buf.numel():
            self.full.append(self.buf)
            self.buf = torch.zeros(self.buf.numel(), device=self.buf.device)
            self.used = 0
        self.used += 1
        return self.buf[self.used - 1:self.used]


def amax_pool(device):
    """-> slot(): the next abs-max slot of this pass when the fp16 split is active (slot.on), else None (producers then skip the atomics)"""
    return AmaxPool(device, on=SPLIT_F16["on"] and mfma_mode() == "split_f16")


def filter_absmax(w_src, w, ld, M, Cc):
    """The abs-max a filter's fp16 planes are scaled from.  A filter that lives in a model's flat parameter buffer (qea.params)
    takes the abs-max of the WHOLE buffer, computed once per weight update for all its filters (one launch instead of one per
    filter and derived form): any bound >= the filter's own max is a valid scale source, and the fp16 pair keeps all 22 bits of
    every element down to 2^-17 of the bound, far below the spread between a model's layers."""
    from .params import flat_state_of
    fs = flat_state_of(w_src[1], check=False) if w_src is not None else None
    if fs is None or fs.total % 4 or fs.data.data_ptr() > w_src[1].data_ptr() or w_src[1].data_ptr() >= fs.data.data_ptr() + 4 * fs.total:
        return absmax(w, ld, M, Cc)
    # keyed on the version counters of ALL the model's parameters (fs.vsum, refreshed by the engines' ensure_flat() walk before
    # every forward): a torch-side write to one re-homed parameter moves that parameter's _version, not the flat buffer's, and a
    # bound taken before e.g. load_state_dict would scale the new, larger filter to inf in its h plane
    # ... and on the model's own epoch (the fused Adam writes through raw pointers and bumps only that)
    return weight_cached("flat_absmax", fs.data, lambda: absmax(fs.data, fs.total, 1, fs.total), extra=(fs.vsum, fs.epoch))


def split_planes_f16(x, ld, M, Cc, w_src=None):
    """the two-plane fp16 row format of a FILTER (qea_split_planes_f16), scaled by the power of two of its abs-max"""
    L = _lib.lib()
    out = torch.empty(L.qea_split_planes_f16_bytes(M, Cc), dtype=torch.uint8, device=x.device)
    xmax = filter_absmax(w_src, x, ld, M, Cc)
    _lib.check(L.qea_split_planes_f16(_ptr(x), ld, M, Cc, _ptr(xmax), out.data_ptr(), _stream()), "qea_split_planes_f16")
    return out


def absmax(x, ld, M, Cc):
    """device scalar: the largest finite |x| of a strided [M][Cc] tensor (one pass; the scale source of the fp16 split)"""
    out = torch.empty(1, device=x.device)
    _lib.check(_lib.lib().qea_absmax(_ptr(x), ld, M, Cc, _ptr(out), _stream()), "qea_absmax")
    return out


_overlap = {"on": None}


def set_overlap(on):
    """Switch the wgrad side stream on/off at run time (bench.py times with it on and measures per-kernel
    durations with it off, because a launch's event-to-event time otherwise includes a co-running kernel)."""
    _overlap["on"] = bool(on)


def overlap_enabled():
    if _overlap["on"] is None:
        import os
        _overlap["on"] = os.environ.get("QEA_OVERLAP", "1") != "0"
    return _overlap["on"]


class SideStream:
    """Runs weight-gradient work beside the main backward chain.  The dgrad -> BN-backward -> dgrad chain is a
    strict dependency chain with HBM-bound links, while every wgrad only needs its layer's dy: launching the
    wgrads on a second HIP stream lets the MFMA-bound wgrad kernels fill the matrix pipes while the chain's
    HBM-bound kernels run.  Set QEA_OVERLAP=0 to keep everything on one stream."""

    def __init__(self, device):
        self.side = torch.cuda.Stream(device)

    @classmethod
    def of(cls, owner, device):
        """owner's side stream on `device`, made on first use and kept as owner._side"""
        side = owner.__dict__.get("_side")
        if side is None or side.side is not None and side.side.device != device:
            side = owner._side = cls(device)
        return side

    @property
    def enabled(self):
        return overlap_enabled()

    def run(self, fn, *reads):
        """fn() is enqueued on the side stream after everything already enqueued on the current stream; `reads`
        are tensors it reads that were allocated on the current stream (kept from reuse until it has run)."""
        if not self.enabled:
            fn()
            return
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(main)
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            fn()
        for t in reads:
            if t is not None:
                t.record_stream(self.side)

    def join(self):
        if self.enabled:
            ev = torch.cuda.Event()
            ev.record(self.side)
            torch.cuda.current_stream().wait_event(ev)


def prof_enable(klass, on=True):
    _lib.check(_lib.lib().qea_prof_enable(klass, int(on)), "qea_prof_enable")


def prof_reset():
    _lib.check(_lib.lib().qea_prof_reset(), "qea_prof_reset")


def prof_read(klass):
    ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    _lib.check(_lib.lib().qea_prof_read(klass, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), "qea_prof_read")
    sp, sf = C.c_double(), C.c_double()
    _lib.check(_lib.lib().qea_prof_read_split_bf16(klass, C.byref(sp)), "qea_prof_read_split_bf16")
    _lib.check(_lib.lib().qea_prof_read_split_f16(klass, C.byref(sf)), "qea_prof_read_split_f16")
    return {"ms": ms.value, "flops": fl.value, "bytes": by.value, "launches": n.value, "flops_split_bf16": sp.value, "flops_split_f16": sf.value}


def prof_tag_halo_bf3(cin_chunk, cout_group, stats, f16=False):
    """QEA_PROF_TAG_HALO_BF3 of include/qea_hip.h (+ 5 for the two-way fp16 instantiation of the same kernel)"""
    return 24000 + (1000 if cin_chunk == 64 else 0) + cout_group + (500 if stats else 0) + (5 if f16 else 0)


def prof_read_tagged(klass, tag):
    ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    _lib.check(_lib.lib().qea_prof_read_tagged(klass, tag, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), "qea_prof_read_tagged")
    return {"ms": ms.value, "flops": fl.value, "bytes": by.value, "launches": n.value}


# ----------------------------------------------------------------------------- BN / pool / misc
def _colws(M, C_, device):
    need = _lib.lib().qea_colreduce_workspace_bytes(M, C_)
    ws = workspace(need, device)
    return ws.data_ptr(), ws.numel()


def bn_train_stats(y, ldy, M, C_, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift, stat64=None):
    wp, wn = _colws(M, C_, y.device)
    _lib.check(_lib.lib().qea_bn_train_stats(_ptr(y), ldy, M, C_, _ptr(gamma), _ptr(beta), eps, momentum,
                                             _ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(invstd),
                                             _ptr(scale), _ptr(shift), _ptr(stat64), wp, wn, _stream()), "qea_bn_train_stats")


def bn_train_stats_from_partials(partials, blocks, M, C_, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift,
                                 stat64=None):
    _lib.check(_lib.lib().qea_bn_train_stats_from_partials(_ptr(partials), blocks, M, C_, _ptr(gamma), _ptr(beta), eps, momentum,
                                                           _ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(invstd),
                                                           _ptr(scale), _ptr(shift), _ptr(stat64), _stream()),
               "qea_bn_train_stats_from_partials")


def bn_eval_coeff(C_, gamma, beta, running_mean, running_var, eps, conv_bias, mean, invstd, scale, shift):
    _lib.check(_lib.lib().qea_bn_eval_coeff(C_, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps,
                                            _ptr(conv_bias), _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift),
                                            _stream()), "qea_bn_eval_coeff")


def bn_apply(y, ldy, a, lda, M, C_, scale, shift, relu=True, amax=None):
    """amax (here and in bn_bwd / maxpool_fwd / maxpool_bwd / conv_igemm's y_amax): a zero-filled 1-element slot (AmaxPool) that receives
    the abs-max of what the launch stores — the scale source of the fp16-split launch that consumes the tensor."""
    _lib.check(_lib.lib().qea_bn_apply(_ptr(y), ldy, _ptr(a), lda, M, C_, _ptr(scale), _ptr(shift), int(relu), _ptr(amax), _stream()),
               "qea_bn_apply")


def bn_bwd(da, ldda, a, lda, y, ldy, M, C_, gamma, mean, invstd, training, dgamma, dbeta, dy, lddy, accumulate=False, stat64=None,
           relu_scale=None, relu_shift=None, amax=None, partials=None):
    """ReLU mask: pass the activation `a`, or a=None with the forward's scale/shift (mask recomputed from y, one tensor read less).
    partials = (tensor, blocks) from conv_igemm(bwd_stats=...): the reductions came with da's producer (no pass over da and y here)."""
    wp, wn = _colws(M, C_, da.device)
    if partials is not None:
        _lib.check(_lib.lib().qea_bn_bwd_from_partials(partials[0].data_ptr(), partials[1], _ptr(da), ldda, _ptr(relu_scale), _ptr(relu_shift), _ptr(y),
                                                       ldy, M, C_, _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(stat64), int(training), _ptr(dgamma),
                                                       _ptr(dbeta), int(accumulate), _ptr(dy), lddy, wp, wn, _ptr(amax), _stream()),
                   "qea_bn_bwd_from_partials")
        return
    _lib.check(_lib.lib().qea_bn_bwd(_ptr(da), ldda, _ptr(a), lda, _ptr(relu_scale), _ptr(relu_shift), _ptr(y), ldy, M, C_, _ptr(gamma), _ptr(mean),
                                     _ptr(invstd), _ptr(stat64), int(training), _ptr(dgamma), _ptr(dbeta), int(accumulate),
                                     _ptr(dy), lddy, wp, wn, _ptr(amax), _stream()), "qea_bn_bwd")


def bn_bwd_pool(da, ldda, dpool, lddp, kw, y, ldy, B, H, W, C_, gamma, mean, invstd, training, dgamma, dbeta, dy, lddy, accumulate=False,
                stat64=None, relu_scale=None, relu_shift=None, amax=None):
    """maxpool_bwd(accumulate into da) + bn_bwd in one (ABI v8): da = the skip path's gradient or None, dpool = the pooled tensor's gradient;
    winners and ReLU mask are recomputed from y (relu_scale / relu_shift required)."""
    wp, wn = _colws(B * H * W, C_, y.device)
    _lib.check(_lib.lib().qea_bn_bwd_pool(_ptr(da), ldda, _ptr(dpool), lddp, kw, _ptr(relu_scale), _ptr(relu_shift), _ptr(y), ldy, B, H, W, C_,
                                          _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(stat64), int(training), _ptr(dgamma), _ptr(dbeta),
                                          int(accumulate), _ptr(dy), lddy, wp, wn, _ptr(amax), _stream()), "qea_bn_bwd_pool")


def colsum(x, ldx, M, C_, out, accumulate=False):
    wp, wn = _colws(M, C_, x.device)
    _lib.check(_lib.lib().qea_colsum(_ptr(x), ldx, M, C_, _ptr(out), int(accumulate), wp, wn, _stream()), "qea_colsum")


def bn_apply_pool(y, ldy, a, lda, pooled, ldp, B, H, W, C_, scale, shift, kh, kw, relu=True, amax=None, pooled_amax=None):
    """bn_apply + maxpool_fwd in one pass over y (bit-identical to the two calls)"""
    _lib.check(_lib.lib().qea_bn_apply_pool(_ptr(y), ldy, _ptr(a), lda, _ptr(pooled), ldp, B, H, W, C_, _ptr(scale), _ptr(shift), int(relu), kh, kw,
                                            _ptr(amax), _ptr(pooled_amax), _stream()), "qea_bn_apply_pool")


def maxpool_fwd(x, ldx, y, ldy, B, H, W, C_, kh, kw, amax=None):
    _lib.check(_lib.lib().qea_maxpool_fwd(_ptr(x), ldx, _ptr(y), ldy, B, H, W, C_, kh, kw, _ptr(amax), _stream()), "qea_maxpool_fwd")


def conv_c1_pool_bwd(x, w, bias, dpool, lddp, dw, db, dx, B, H, W, Co, accumulate=False):
    """backward of conv1 -> ReLU -> max_pool2d(2, 2) from the pooled tensor's gradient and the 1-channel input (ABI v8): dpool is overwritten
    with its ReLU-masked values; dw / db (None: no parameter gradients), dx (None: not wanted)."""
    L = _lib.lib()
    need = L.qea_conv_c1_pool_bwd_workspace_bytes(B, H, W, Co, int(dx is not None))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
    _lib.check(L.qea_conv_c1_pool_bwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(dpool), lddp, _ptr(dw), _ptr(db), _ptr(dx), B, H, W, Co, int(accumulate),
                                      ws.data_ptr(), ws.numel(), _stream()), "qea_conv_c1_pool_bwd")


def maxpool_bwd(x, ldx, dy, lddy, dx, lddx, B, H, W, C_, kh, kw, relu_mask=False, accumulate=False, amax=None):
    _lib.check(_lib.lib().qea_maxpool_bwd(_ptr(x), ldx, _ptr(dy), lddy, _ptr(dx), lddx, B, H, W, C_, kh, kw,
                                          int(relu_mask), int(accumulate), _ptr(amax), _stream()), "qea_maxpool_bwd")


def transpose2d(src, dst, R, Cc):
    _lib.check(_lib.lib().qea_transpose2d(_ptr(src), _ptr(dst), R, Cc, _stream()), "qea_transpose2d")


def filter_flip_transpose(w, wt, Co, Ci, KH, KW):
    _lib.check(_lib.lib().qea_filter_flip_transpose(_ptr(w), _ptr(wt), Co, Ci, KH, KW, _stream()), "qea_filter_flip_transpose")


# ----------------------------------------------------------------------------- single-channel convs / head
def conv_c1_fwd(x, w, bias, y, ldy, B, H, W, Co, relu=False):
    _lib.check(_lib.lib().qea_conv_c1_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), ldy, B, H, W, Co, int(relu), _stream()),
               "qea_conv_c1_fwd")


def conv_c1_fwd_pool(x, w, bias, y, ldy, pooled, ldp, B, H, W, Co, relu=False, pooled_amax=None):
    """conv_c1_fwd + maxpool_fwd(2, 2) in one pass (bit-identical); False when the shape is not taken (the caller then runs the two)"""
    if H % 2 or W % 4 or Co not in (32, 64, 128):
        return False
    _lib.check(_lib.lib().qea_conv_c1_fwd_pool(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), ldy, _ptr(pooled), ldp, B, H, W, Co, int(relu),
                                               _ptr(pooled_amax), _stream()), "qea_conv_c1_fwd_pool")
    return True


def conv_c1_wgrad(x, dy, lddy, dw, db, B, H, W, Co, accumulate=False):
    L = _lib.lib()
    ws = workspace(L.qea_conv_c1_wgrad_workspace_bytes(B, H, W, Co), x.device)
    _lib.check(L.qea_conv_c1_wgrad(_ptr(x), _ptr(dy), lddy, _ptr(dw), _ptr(db), B, H, W, Co, int(accumulate),
                                   ws.data_ptr(), ws.numel(), _stream()), "qea_conv_c1_wgrad")


def conv_c1_dgrad(dy, lddy, w, dx, B, H, W, Co, accumulate=False):
    _lib.check(_lib.lib().qea_conv_c1_dgrad(_ptr(dy), lddy, _ptr(w), _ptr(dx), B, H, W, Co, int(accumulate), _stream()),
               "qea_conv_c1_dgrad")


def head_fwd(x, ldx, w, b, y, M, C_):
    _lib.check(_lib.lib().qea_head_fwd(_ptr(x), ldx, _ptr(w), _ptr(b), _ptr(y), M, C_, _stream()), "qea_head_fwd")


def head_bwd(x, ldx, y, dyy, w, dx, lddx, dw, db, M, C_, accumulate=False):
    L = _lib.lib()
    ws = workspace(L.qea_head_bwd_workspace_bytes(M, C_), x.device)
    _lib.check(L.qea_head_bwd(_ptr(x), ldx, _ptr(y), _ptr(dyy), _ptr(w), _ptr(dx), lddx, _ptr(dw), _ptr(db),
                              int(accumulate), M, C_, ws.data_ptr(), ws.numel(), _stream()), "qea_head_bwd")


# ----------------------------------------------------------------------------- sequence ops
def lstm_pack_whh(w_hh, packed_fwd, packed_bwd):
    _lib.check(_lib.lib().qea_lstm_pack_whh(_ptr(w_hh), _ptr(packed_fwd), _ptr(packed_bwd), _stream()), "qea_lstm_pack_whh")


def lstm_layer_fwd(gates, c, y, packed_fwd, T, B):
    _lib.check(_lib.lib().qea_lstm_layer_fwd(_ptr(gates), _ptr(c), _ptr(y), _ptr(packed_fwd), T, B, _stream()), "qea_lstm_layer_fwd")


def lstm_layer_bwd(gates, c, dy, packed_bwd, dc_scratch, T, B):
    _lib.check(_lib.lib().qea_lstm_layer_bwd(_ptr(gates), _ptr(c), _ptr(dy), _ptr(packed_bwd), _ptr(dc_scratch), T, B,
                                             _stream()), "qea_lstm_layer_bwd")


def lstm_pack_whh_split(w_hh, planes_fwd, planes_bwd):
    _lib.check(_lib.lib().qea_lstm_pack_whh_split(_ptr(w_hh), _ptr(planes_fwd), _ptr(planes_bwd), _stream()), "qea_lstm_pack_whh_split")


LSTM_SEQ = {"on": os.environ.get("QEA_LSTM", "seq") != "step"}


def lstm_mode():
    """"seq": one launch per layer pass, W_hh resident in LDS as fp16 planes (csrc/lstm_seq.hip; the default fp16-split mode);
    "bf3": one launch per step, split-bf16 recurrent GEMMs (QEA_LSTM=step, or the split-bf16 MFMA mode); "f32": QEA_MFMA=f32."""
    m = mfma_mode()
    if m == "f32":
        return "f32"
    return "seq" if (m == "split_f16" and LSTM_SEQ["on"]) else "bf3"


def lstm_packs(whf, whr):
    """(fwd pack, bwd pack, mode) of one layer's two W_hh for the CURRENT mode (lstm_mode), cached with the weights: fp16 planes +
    the two abs-max values for the one-launch layer kernels, three-plane bf16 fragments for the split-bf16 step kernels, fp32
    fragments for QEA_MFMA=f32.  A "seq" pack is the tuple (planes [2][bytes], w_absmax [2])."""
    mode = lstm_mode()
    dev = whf.device

    def pack():
        if mode == "seq":
            nb = _lib.lib().qea_lstm_seq_pack_bytes()
            pf_ = torch.empty(2, nb, dtype=torch.uint8, device=dev)
            pb_ = torch.empty(2, nb, dtype=torch.uint8, device=dev)
            # the scale source of the planes: any bound >= max |W_hh| (the model's flat abs-max when the weight lives in one: no launch)
            bounds = [filter_absmax(("fwd", wh), wh, 256, 1024, 256) for wh in (whf, whr)]
            am = torch.cat([b.reshape(1) for b in bounds])
            for d_, wh in enumerate((whf, whr)):
                _lib.check(_lib.lib().qea_lstm_seq_pack(_ptr(wh), _ptr(pf_[d_]), _ptr(pb_[d_]), _ptr(am[d_:]), _stream()), "qea_lstm_seq_pack")
            return (pf_, am), (pb_, am)
        if mode == "bf3":
            nb = _lib.lib().qea_lstm_pack_whh_split_bytes()
            pf_ = torch.empty(2, nb, dtype=torch.uint8, device=dev)
            pb_ = torch.empty(2, nb, dtype=torch.uint8, device=dev)
            for d_, wh in enumerate((whf, whr)):
                lstm_pack_whh_split(wh, pf_[d_], pb_[d_])
        else:
            pf_ = torch.empty(2, whf.numel(), device=dev)
            pb_ = torch.empty(2, whf.numel(), device=dev)
            for d_, wh in enumerate((whf, whr)):
                lstm_pack_whh(wh, pf_[d_], pb_[d_])
        return pf_, pb_
    pf, pb = weight_cached(("whh_pack", mode), whf, pack, also=(whr,))
    return pf, pb, mode


_LSTM_SEQ_LAST = {"fwd": None, "bwd": None}     # (workspace, B) of the most recent "seq" pass of each kind: see lstm_seq_timed_out


def _lstm_seq_ws(B, dev, which):
    ws = torch.empty(_lib.lib().qea_lstm_seq_workspace_bytes(B), dtype=torch.uint8, device=dev)
    _LSTM_SEQ_LAST[which] = (ws, B)
    return ws


def lstm_seq_timed_out(which):
    """True when a bounded spin of the most recent "seq" forward (which = "fwd") or backward ("bwd") ran out: the pass has then set
    the timeout word of its workspace (qea_lstm_seq_timeout_index) and poisoned its outputs with NaN.  A SYNCHRONISING device-to-host
    read of one word on the CURRENT stream (call it from the stream the pass ran on, or after that stream has been synchronised):
    for tests and diagnosis, never called from the engines, and not capturable (do not call it while a stream is capturing; after a replay it reads the word of the captured pass only if that pass was the most recent one made).  The workspace
    of the last pass of each kind stays allocated until the next one replaces it."""
    last = _LSTM_SEQ_LAST[which]
    if last is None:
        raise _lib.QeaError(f"no \"seq\" {which} pass has run in this process")
    ws, B = last
    idx = _lib.lib().qea_lstm_seq_timeout_index(B, int(which == "bwd"))
    return bool(ws.view(torch.int32)[idx].item() != 0)


def lstm_layer_fwd_any(gates, c, y, pack, mode, T, B, y_amax=None):
    """mode: "seq" / "bf3" / "f32" (True / False of the round-2 callers = "bf3" / "f32").  y_amax: a ZEROED abs-max slot; returns True
    when the pass has left the layer output's abs-max in it (the one-launch kernels), else the caller makes its own pass."""
    if os.environ.get("QEA_LSTM_TRACE"):
        print("lstm fwd", mode, T, B, flush=True)
    if mode == "seq":
        planes, am = pack
        ws = _lstm_seq_ws(B, gates.device, "fwd")
        _lib.check(_lib.lib().qea_lstm_seq_fwd(_ptr(gates), _ptr(c), _ptr(y), _ptr(planes), _ptr(am), T, B, _ptr(ws), _ptr(y_amax), _stream()), "qea_lstm_seq_fwd")
        return y_amax is not None
    elif mode is True or mode == "bf3":
        _lib.check(_lib.lib().qea_lstm_layer_fwd_split(_ptr(gates), _ptr(c), _ptr(y), _ptr(pack), T, B, _stream()), "qea_lstm_layer_fwd_split")
    else:
        lstm_layer_fwd(gates, c, y, pack, T, B)


def lstm_layer_bwd_any(gates, c, dy, pack, mode, dc_scratch, T, B, g_amax=None):
    if mode == "seq":
        planes, am = pack
        ws = _lstm_seq_ws(B, gates.device, "bwd")
        _lib.check(_lib.lib().qea_lstm_seq_bwd(_ptr(gates), _ptr(c), _ptr(dy), _ptr(planes), _ptr(am), T, B, _ptr(ws), _ptr(g_amax), _stream()), "qea_lstm_seq_bwd")
        return g_amax is not None
    elif mode is True or mode == "bf3":
        _lib.check(_lib.lib().qea_lstm_layer_bwd_split(_ptr(gates), _ptr(c), _ptr(dy), _ptr(pack), _ptr(dc_scratch), T, B, _stream()),
                   "qea_lstm_layer_bwd_split")
    else:
        lstm_layer_bwd(gates, c, dy, pack, dc_scratch, T, B)


def log_softmax_fwd(x, ldx, y, ldy, M, C_):
    _lib.check(_lib.lib().qea_log_softmax_fwd(_ptr(x), ldx, _ptr(y), ldy, M, C_, _stream()), "qea_log_softmax_fwd")


def log_softmax_bwd(g, ldg, lp, ldlp, dx, lddx, M, C_, Cpad, nan_scrub):
    _lib.check(_lib.lib().qea_log_softmax_bwd(_ptr(g), ldg, _ptr(lp), ldlp, _ptr(dx), lddx, M, C_, Cpad, int(nan_scrub),
                                              _stream()), "qea_log_softmax_bwd")


def ctc_loss(lp, ld_t, ld_n, targets, target_offsets, input_lengths, target_lengths, T, N, C_, blank, S_max, reduction,
             grad_scale, nll, loss, grad, gld_t, gld_n):
    L = _lib.lib()
    ws = workspace(L.qea_ctc_workspace_bytes(T, N, S_max), lp.device)
    _lib.check(L.qea_ctc_loss(_ptr(lp), ld_t, ld_n, _ptr(targets), _ptr(target_offsets), _ptr(input_lengths),
                              _ptr(target_lengths), T, N, C_, blank, S_max, reduction, grad_scale, _ptr(nll), _ptr(loss),
                              _ptr(grad), gld_t, gld_n, ws.data_ptr(), ws.numel(), _stream()), "qea_ctc_loss")


# ----------------------------------------------------------------------------- optimiser / jitter / selection / crops
def adam_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _lib.check(_lib.lib().qea_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, lr, beta1, beta2, eps, weight_decay, step,
                                        grad_scale, _stream()), "qea_adam_step")


def adam_step_capturable(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, coef, grad_scale=1.0):
    """step: 1-element CUDA float tensor (incremented on the device), coef: 2-element CUDA float scratch."""
    _lib.check(_lib.lib().qea_adam_step_capturable(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, lr, beta1, beta2, eps, weight_decay,
                                                   _ptr(step), _ptr(coef), grad_scale, _stream()), "qea_adam_step_capturable")


def jitter(img, sigma, out, noise_out, K, R, HW, coef, seed, offset):
    _lib.check(_lib.lib().qea_jitter(_ptr(img), _ptr(sigma), _ptr(out), _ptr(noise_out), K, R, HW, coef, seed, offset,
                                     _stream()), "qea_jitter")


def jitter_apply(img, noise, out, K, R, HW, coef):
    _lib.check(_lib.lib().qea_jitter_apply(_ptr(img), _ptr(noise), _ptr(out), K, R, HW, coef, _stream()), "qea_jitter_apply")


def topk_desc_stable(keys, n, k, idx_out):
    _lib.check(_lib.lib().qea_topk_desc_stable(_ptr(keys), n, k, _ptr(idx_out), _stream()), "qea_topk_desc_stable")


def crop_pad_gather(img, H, W, boxes, N, OH, OW, out):
    _lib.check(_lib.lib().qea_crop_pad_gather(_ptr(img), H, W, _ptr(boxes), N, OH, OW, _ptr(out), _stream()), "qea_crop_pad_gather")


def crop_pad_scatter(dout, boxes, N, OH, OW, dimg, H, W):
    _lib.check(_lib.lib().qea_crop_pad_scatter(_ptr(dout), _ptr(boxes), N, OH, OW, _ptr(dimg), H, W, _stream()), "qea_crop_pad_scatter")


def greedy_decode(scores, ld_t, ld_n, T, N, C_, blank, tokens, lengths):
    _lib.check(_lib.lib().qea_greedy_decode(_ptr(scores), ld_t, ld_n, T, N, C_, blank, _ptr(tokens), _ptr(lengths), _stream()),
               "qea_greedy_decode")


def _beam_search(name, scores, K, blank, mode=None, extra=None):
    """The one launch path of the three prefix beam searches.  name = the library function; its signature is the plain one with the
    mode's arguments between K and tokens and the mode's output column behind the scores.  Validates scores, then calls mode() (the
    wrapper's own checks; it returns the mode's arguments), allocates tokens / lengths / scores and one [N, rows] column of dtype
    `extra` where the mode has one, launches, and returns the outputs.  Nothing is launched before every check has passed."""
    who = name[len("qea_"):]
    if scores.dim() != 3 or not scores.is_cuda or scores.dtype != torch.float32:
        raise _lib.QeaError(f"{who} needs a CUDA float32 tensor [T,N,C] (there is no CPU path here: qea.beam has one)")
    if scores.stride(2) != 1:
        raise _lib.QeaError(f"{who} needs a unit class stride: make the last dimension contiguous")
    if not (0 <= scores.stride(0) < 2 ** 31 and 0 <= scores.stride(1) < 2 ** 31):
        raise _lib.QeaError(f"{who}: the T and N strides must fit 32 bits")
    T, N, C_ = scores.shape
    K = int(K)
    args = mode() if mode else ()
    rows = max(K, 1)
    out = [torch.empty(N, rows, T, dtype=torch.int32, device=scores.device), torch.empty(N, rows, dtype=torch.int32, device=scores.device),
           torch.empty(N, rows, dtype=torch.float64, device=scores.device)]
    if extra is not None:
        out.append(torch.empty(N, rows, dtype=extra, device=scores.device))
    _lib.check(getattr(_lib.lib(), name)(_ptr(scores), scores.stride(0), scores.stride(1), T, N, C_, int(blank), K, *args,
                                         *[_ptr(t) for t in out], _stream()), name)
    return tuple(out)


def ctc_beam_decode(scores, K, blank=0):
    """CTC prefix beam search (include/qea_hip.h: qea_ctc_beam_decode) of scores [T,N,C] (CUDA, float32, any T / N strides, unit class
    stride) -> (tokens int32 [N,K,T] with -1 behind every prefix, lengths int32 [N,K], scores float64 [N,K]), best first, on the
    device and without a synchronisation.  Raises QeaError for K outside 1..32, C outside 2..256, T outside 1..512, blank outside
    0..C-1."""
    return _beam_search("qea_ctc_beam_decode", scores, K, blank)


def ctc_beam_decode_lm(scores, K, table, context, blank=0):
    """The prefix beam search with a character n-gram prior fused in (include/qea_hip.h: qea_ctc_beam_decode_lm): scores as for
    ctc_beam_decode, table = the fused W [C ** context, C] (CUDA, float64, contiguous; qea.lm.CharLM.fused), context 0..2 ->
    (tokens int32 [N,K,T], lengths int32 [N,K], ctc float64 [N,K], total float64 [N,K]), best first by total, on the device and
    without a synchronisation.  Raises QeaError for what ctc_beam_decode refuses, what qea.beam.check_lm_limits refuses (context outside
    0..MAX_LM_CONTEXT, C ** (context + 1) > MAX_LM_ENTRIES) and a table of another device, dtype, layout or shape."""
    def mode():
        C_, m = scores.shape[2], int(context)
        beam.check_lm_limits(C_, m)
        if not (torch.is_tensor(table) and table.is_cuda and table.device == scores.device and table.dtype == torch.float64
                and table.is_contiguous() and tuple(table.shape) == (C_ ** m, C_)):
            raise _lib.QeaError(f"ctc_beam_decode_lm needs a contiguous CUDA float64 table [C**context, C] = {(C_ ** m, C_)} on the scores' device")
        return _ptr(table), m
    return _beam_search("qea_ctc_beam_decode_lm", scores, K, blank, mode, torch.float64)


def ctc_beam_decode_dfa(scores, K, automaton, blank=0):
    """The prefix beam search restricted to the paths of a deterministic automaton (include/qea_hip.h: qea_ctc_beam_decode_dfa): scores
    as for ctc_beam_decode, automaton = what qea.lexicon.Lexicon.device(scores.device) returns (the validated tables; nothing else
    is taken) -> (tokens int32 [N,K,T], lengths int32 [N,K], scores float64 [N,K], states int32 [N,K], -1 beyond the live count), best
    first, on the device and without a synchronisation.  The whole last beam is returned: automaton.final[state] says which ranks
    are accepted.  Raises QeaError for what ctc_beam_decode refuses, anything but a DeviceAutomaton, and one of another device, class
    count or blank."""
    def mode():
        from .lexicon import DeviceAutomaton
        a = automaton
        if not isinstance(a, DeviceAutomaton):
            raise _lib.QeaError("ctc_beam_decode_dfa takes the object Lexicon.device() returns: the tables it holds are validated")
        if a.device != scores.device:
            raise _lib.QeaError(f"ctc_beam_decode_dfa: the automaton is on {a.device}, the scores on {scores.device}")
        if a.num_classes != scores.shape[2] or a.blank != int(blank):
            raise _lib.QeaError(f"ctc_beam_decode_dfa: the automaton has {a.num_classes} classes and blank {a.blank}, "
                                f"the scores {scores.shape[2]} and {int(blank)}")
        return _ptr(a.first), _ptr(a.label), _ptr(a.child), a.num_states, a.num_edges
    return _beam_search("qea_ctc_beam_decode_dfa", scores, K, blank, mode, torch.int32)


def ctc_align(scores, targets, offsets, L_max, blank=0):
    """CTC forced alignment (include/qea_hip.h: qea_ctc_align) of scores [T,N,C] (CUDA, float32, any T / N strides, unit class stride)
    to the labels targets (int32, end to end) / offsets (int64 [N+1]), both contiguous on the scores' device; L_max >= every label length
    -> (score float64 [N], path int32 [N,T], first int32 [sum L], last int32 [sum L], char_score float64 [sum L]) on the device, one
    launch and no synchronisation (sum L is targets.numel(): nothing is read back).  Raises QeaError for what qea.align.check_limits
    refuses and for tensors of another device, dtype or layout; N = 0 launches nothing."""
    from . import align
    who = "ctc_align"
    if scores.dim() != 3 or not scores.is_cuda or scores.dtype != torch.float32:
        raise _lib.QeaError(f"{who} needs a CUDA float32 tensor [T,N,C] (there is no CPU path here: qea.align has one)")
    if scores.stride(2) != 1:
        raise _lib.QeaError(f"{who} needs a unit class stride: make the last dimension contiguous")
    if not (0 <= scores.stride(0) < 2 ** 31 and 0 <= scores.stride(1) < 2 ** 31):
        raise _lib.QeaError(f"{who}: the T and N strides must fit 32 bits")
    T, N, C_ = scores.shape
    blank, L_max = int(blank), int(L_max)
    align.check_limits(T, C_, blank, L_max, N)
    for name, t, dtype, numel in (("targets", targets, torch.int32, None), ("offsets", offsets, torch.int64, N + 1)):
        if not (torch.is_tensor(t) and t.device == scores.device and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()
                and numel in (None, t.numel())):
            raise _lib.QeaError(f"{who}: {name} must be a contiguous 1-D {dtype} tensor on the scores' device"
                                + (f" of {numel} elements" if numel else ""))
    total, dev = targets.numel(), scores.device
    score, path = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, T, dtype=torch.int32, device=dev)
    # at least one element behind every pointer: a batch of empty labels is a valid call
    first, last = (torch.empty(max(total, 1), dtype=torch.int32, device=dev) for _ in range(2))
    char_score = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    tg = targets if total else torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().qea_ctc_align(_ptr(scores), scores.stride(0), scores.stride(1), _ptr(tg), _ptr(offsets), T, N, C_, blank, L_max,
                                        _ptr(score), _ptr(path), _ptr(first), _ptr(last), _ptr(char_score), _stream()), "qea_ctc_align")
    return score, path, first[:total], last[:total], char_score[:total]


def prof_read_launches(klass, capacity=4096):
    import numpy as np
    ms = np.zeros(capacity)
    fl = np.zeros(capacity)
    n = C.c_int64()
    _lib.check(_lib.lib().qea_prof_read_launches(klass, ms.ctypes.data, fl.ctypes.data, capacity, C.byref(n)), "qea_prof_read_launches")
    k = min(n.value, capacity)
    return ms[:k], fl[:k]


def edit_distance(pred_tokens, ldp, pred_len, gt_tokens, gt_offsets, gt_len, N, out):
    _lib.check(_lib.lib().qea_edit_distance(_ptr(pred_tokens), ldp, _ptr(pred_len), _ptr(gt_tokens), _ptr(gt_offsets), _ptr(gt_len), N,
                                            _ptr(out), _stream()), "qea_edit_distance")


def facility_select(x, k):
    """Greedy facility-location ranking (include/qea_hip.h: qea_facility_select) of the rows of x [n][d] (CUDA, float64, 1 <= d <= 32):
    returns (ranking [k] int32, gains [k] float64) as HOST tensors.  Raises QeaError for k > n, d out of range and non-finite rows."""
    if x.dim() == 1:
        x = x[:, None]
    if not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2:
        raise _lib.QeaError("facility_select needs a CUDA float64 tensor [n][d] (there is no CPU path here: pruning.methods has one)")
    x = x.contiguous()
    n, d = x.shape
    L = _lib.lib()
    ranking = torch.empty(max(int(k), 1), dtype=torch.int32, device=x.device)
    gains = torch.empty(max(int(k), 1), dtype=torch.float64, device=x.device)
    nbytes = L.qea_facility_workspace_bytes(n, d)
    ws = workspace(max(nbytes, 16), x.device)
    _lib.check(L.qea_facility_select(_ptr(x), n, d, int(k), _ptr(ranking), _ptr(gains), ws.data_ptr(), _stream()), "qea_facility_select")
    out = ranking.cpu(), gains.cpu()                     # the call's one synchronisation; the flag word is read behind it
    _lib.check(L.qea_facility_status(ws.data_ptr(), _stream()), "qea_facility_select")
    return out


HISTORY_MAX_WINDOW, HISTORY_MAX_LEN, HISTORY_ATTN_MAX_TABLE = 8, 128, 12288      # QEA_HISTORY_* of include/qea_hip.h
HISTORY_ACTIVATIONS = {"sigmoid": 0, "softmax": 1, "relu": 2}
HISTORY_LAUNCHES = {"lev": 0, "attn": 0}     # launches of the two label-history kernels issued through this module (tests, tools)


def history_lev_weights(tokens, lens, count, n, W, out):
    """include/qea_hip.h: qea_history_lev_weights — tokens [n][W][128] / lens [n][W] / count [n] int32 -> out [n][W+1] fp32."""
    _lib.check(_lib.lib().qea_history_lev_weights(_ptr(tokens), _ptr(lens), _ptr(count), n, W, _ptr(out), _stream()), "qea_history_lev_weights")
    HISTORY_LAUNCHES["lev"] += 1


def history_attn_weights(char_idx, count, n, W, n_chars, embedding, wq_weight, wq_bias, coef_weight, coef_bias, pos, activation, out):
    """include/qea_hip.h: qea_history_attn_weights — char_idx [n][W][n_chars] / count [n] int32 and the HistoryAttention parameters
    (contiguous fp32) -> out [n][W+1] fp32; `activation` is one of HISTORY_ACTIVATIONS."""
    if activation not in HISTORY_ACTIVATIONS:
        raise ValueError(f"unknown attn_activation {activation!r}")
    V1, E = embedding.shape
    Dq = wq_weight.shape[0]
    _lib.check(_lib.lib().qea_history_attn_weights(_ptr(char_idx), _ptr(count), n, W, n_chars, _ptr(embedding), V1, E, _ptr(wq_weight),
                                                   _ptr(wq_bias), Dq, _ptr(coef_weight), _ptr(coef_bias), _ptr(pos),
                                                   HISTORY_ACTIVATIONS[activation], _ptr(out), _stream()), "qea_history_attn_weights")
    HISTORY_LAUNCHES["attn"] += 1


HISTORY_CTC_LAUNCHES = {"ctc": 0}            # launches of csrc/ctc_history.hip issued through this module (tests, tools)


def ctc_history_workspace_bytes(T, N, W, S_max):
    return _lib.lib().qea_ctc_history_workspace_bytes(T, N, W, S_max)


def ctc_history_loss(lp, input_lengths, lens, offs, chars, depth_n, weights, w_stride_n, w_stride_i, mean_by_length, S_max, blank=0,
                     need_grad=True):
    """include/qea_hip.h: qea_ctc_history_loss — lp [T][N][C] fp32 (last stride 1), input_lengths [N], lens / offs [N][W], chars,
    depth_n [W] int32, weights fp32 read at n * w_stride_n + i * w_stride_i -> (loss [1], grad [T][N][C] or None, nll [N][W]).
    Three launches (two without the gradient), no synchronisation."""
    T, N, C_ = lp.shape
    W = depth_n.numel()
    if lp.dtype != torch.float32 or lp.stride(2) != 1 or weights.dtype != torch.float32:
        raise _lib.QeaError("ctc_history_loss needs fp32 log-probs with a unit class stride and fp32 weights")
    if any(t.dtype != torch.int32 or not t.is_contiguous() for t in (input_lengths, lens, offs, chars, depth_n)):
        raise _lib.QeaError("ctc_history_loss needs contiguous int32 lengths, offsets, characters and depth counts")
    if input_lengths.numel() != N or lens.numel() != N * W or offs.numel() != N * W:
        raise _lib.QeaError(f"ctc_history_loss: tables of {lens.numel()} / {offs.numel()} entries for N={N}, W={W}")
    if W < 1 or (N - 1) * w_stride_n + (W - 1) * w_stride_i >= weights.untyped_storage().nbytes() // 4 - weights.storage_offset():
        raise _lib.QeaError("ctc_history_loss: the weight strides reach past the weight tensor")
    if chars.numel() == 0:
        chars = torch.zeros(1, dtype=torch.int32, device=lp.device)      # every label empty: the pointer is never read
    L = _lib.lib()
    dev = lp.device
    loss = torch.empty(1, device=dev)
    nll = torch.empty(N, W, device=dev)
    grad = torch.empty(T, N, C_, device=dev) if need_grad else None
    ws = workspace(L.qea_ctc_history_workspace_bytes(T, N, W, S_max), dev)
    _lib.check(L.qea_ctc_history_loss(_ptr(lp), lp.stride(0), lp.stride(1), _ptr(input_lengths), _ptr(lens), _ptr(offs), _ptr(chars),
                                      _ptr(depth_n), _ptr(weights), w_stride_n, w_stride_i, int(mean_by_length), T, N, C_, W, blank, S_max,
                                      _ptr(loss), _ptr(grad), N * C_ if need_grad else 0, C_ if need_grad else 0, _ptr(nll), ws.data_ptr(),
                                      ws.numel(), _stream()), "qea_ctc_history_loss")
    HISTORY_CTC_LAUNCHES["ctc"] += 3 if need_grad else 2
    return loss, grad, nll


def _tensors(who, device, *specs):
    """The tensor checks of the gather / scatter wrappers below -> the tensors' device pointers, in order.  A spec is (name, tensor,
    dtype[, element count]): every tensor is of its dtype, contiguous and on the CUDA device `device`, and has that many elements where
    a count is given, or a QeaError names the caller, the tensor and what is wrong with it.  (These wrappers sit between the device
    events of 15 us launches: one pass, no second look at a tensor that is right.)"""
    if device.type != "cuda":
        raise _lib.QeaError(f"{who} needs CUDA tensors (there is no CPU path), not {device}")
    ptrs = []
    for spec in specs:
        t = spec[1]
        if t.dtype is not spec[2] or t.device != device or not t.is_contiguous() or (len(spec) > 3 and t.numel() != spec[3]):
            raise _lib.QeaError(f"{who}: {spec[0]} must be a contiguous {spec[2]} tensor on {device}" + (f" of {spec[3]} elements" if len(spec) > 3 else "")
                                + f", not {'a' if t.is_contiguous() else 'a strided'} {t.dtype} tensor on {t.device} of {t.numel()} elements")
        ptrs.append(t.data_ptr())
    return ptrs


STRIP_ANCHORS = {"centre": 0, "left": 1}     # QEA_STRIP_ANCHOR_* of include/qea_hip.h
STRIP_LAUNCHES = {"batch": 0}                # launches of csrc/strip_batch.hip issued through this module (tests, tools)


def strip_batch(pixels, offset, h, w, idx, table, out, anchor="centre"):
    """include/qea_hip.h: qea_strip_batch — the resident store's pixels (uint8), offset (int64 [n]), h / w (int32 [n]), the device
    idx (int64 [B]) and the 256-entry fp32 table -> out [B][1][OH][OW] fp32, written whole by ONE launch on the current stream."""
    if anchor not in STRIP_ANCHORS:
        raise ValueError(f"unknown anchor {anchor!r}")
    n, B = offset.numel(), idx.numel()
    p = _tensors("strip_batch", out.device, ("pixels", pixels, torch.uint8), ("offset", offset, torch.int64), ("h", h, torch.int32, n),
                 ("w", w, torch.int32, n), ("idx", idx, torch.int64), ("table", table, torch.float32, 256), ("out", out, torch.float32))
    if out.dim() != 4 or out.shape[0] != B or out.shape[1] != 1:
        raise _lib.QeaError(f"strip_batch: out {tuple(out.shape)} for {B} indices")
    _lib.check(_lib.lib().qea_strip_batch(p[0], p[1], p[2], p[3], n, p[4], B, out.shape[2], out.shape[3], STRIP_ANCHORS[anchor], p[5], p[6],
                                          _stream()), "qea_strip_batch")
    STRIP_LAUNCHES["batch"] += 1


DOC_LAUNCHES = {"gather": 0, "scatter": 0}    # launches of csrc/doc_crops.hip issued through this module (tests, tools)


def _doc_tables(who, box, box_first, doc, strip_first, imgs, strips):
    """The argument checks the two entry points of csrc/doc_crops.hip share; -> (pointers of box, box_first, doc, strip_first, imgs and
    strips, (N, H, W), n_docs, n_boxes, (S, OH, OW))."""
    if imgs.dim() == 4 and imgs.shape[1] == 1:
        N, _, H, W = imgs.shape
    elif imgs.dim() == 3:
        N, H, W = imgs.shape
    else:
        raise _lib.QeaError(f"{who}: images {tuple(imgs.shape)} are neither [N,1,H,W] nor [N,H,W]")
    if strips.dim() != 4 or strips.shape[1] != 1:
        raise _lib.QeaError(f"{who}: strips {tuple(strips.shape)} are not [S,1,OH,OW]")
    S, _, OH, OW = strips.shape
    p = _tensors(who, imgs.device, ("box", box, torch.int32), ("box_first", box_first, torch.int32), ("doc", doc, torch.int64, N),
                 ("strip_first", strip_first, torch.int32, N + 1), ("images", imgs, torch.float32), ("strips", strips, torch.float32))
    n_docs = box_first.numel() - 1
    if box.dim() != 2 or box.shape[1] != 4 or n_docs < 1:
        raise _lib.QeaError(f"{who}: boxes {tuple(box.shape)} are not [total][4], or fewer than two box_first entries ({box_first.numel()})")
    return p, (N, H, W), n_docs, box.shape[0], (S, OH, OW)


def doc_crops_gather(imgs, box, box_first, doc, strip_first, out):
    """include/qea_hip.h: qea_doc_crops_gather — imgs [N,1,H,W] fp32, the store's box / box_first, doc (int64 [N]) and strip_first
    (int32 [N+1]) -> out [S,1,OH,OW], every strip of the step, written whole by ONE launch on the current stream."""
    (box, box_first, doc, strip_first, imgs, out), image, n_docs, n_boxes, strip = _doc_tables("doc_crops_gather", box, box_first, doc,
                                                                                              strip_first, imgs, out)
    _lib.check(_lib.lib().qea_doc_crops_gather(imgs, *image, box, box_first, n_docs, n_boxes, doc, strip_first, *strip, out, _stream()),
               "qea_doc_crops_gather")
    DOC_LAUNCHES["gather"] += 1


def doc_crops_scatter(dout, box, box_first, doc, strip_first, dimg, accumulate=False):
    """include/qea_hip.h: qea_doc_crops_scatter — dout [S,1,OH,OW] -> dimg [N,1,H,W], written whole (or added to, `accumulate`) by ONE
    launch without atomics: per pixel the sum over the covering boxes in ascending box order."""
    (box, box_first, doc, strip_first, dimg, dout), image, n_docs, n_boxes, strip = _doc_tables("doc_crops_scatter", box, box_first, doc,
                                                                                               strip_first, dimg, dout)
    _lib.check(_lib.lib().qea_doc_crops_scatter(dout, *strip, box, box_first, n_docs, n_boxes, doc, strip_first, dimg, *image,
                                                int(bool(accumulate)), _stream()), "qea_doc_crops_scatter")
    DOC_LAUNCHES["scatter"] += 1


PAGE_LAUNCHES = {"gather": 0, "scatter": 0}   # launches of csrc/page_tiles.hip issued through this module (tests, tools)


def _page_tables(who, offset, h, w, rows, cols, tiles, *more):
    """The argument checks the two entry points of csrc/page_tiles.hip share (`more`: the specs of their own tensors);
    -> (pointers of offset, h, w, rows, tiles and `more`, n_pages, (N, TH, TW))."""
    n = offset.numel()
    p = _tensors(who, tiles.device, ("offset", offset, torch.int64), ("h", h, torch.int32, n), ("w", w, torch.int32, n),
                 ("tile rows", rows, torch.int32), ("tiles", tiles, torch.float32), *more)
    if rows.dim() != 2 or rows.shape[1] != cols or tiles.dim() != 4 or tiles.shape[1] != 1 or tiles.shape[0] != rows.shape[0]:
        raise _lib.QeaError(f"{who}: tile rows {tuple(rows.shape)} (want [N][{cols}]), tiles {tuple(tiles.shape)} (want [N,1,TH,TW])")
    return p, n, (tiles.shape[0], tiles.shape[2], tiles.shape[3])


def page_tiles_gather(store, offset, h, w, rows, out, table=None):
    """include/qea_hip.h: qea_page_tiles_gather — the packed pages `store` (uint8 with the 256-entry fp32 `table`, or fp32), their element
    offset (int64 [n]) and h / w (int32 [n]), the tile rows (int32 [N][3] = page, oy, ox) -> out [N,1,TH,TW] fp32, white outside a page,
    written whole by ONE launch on the current stream."""
    _page_store("page_tiles_gather", store)
    if store.dtype == torch.uint8 and table is None:
        raise _lib.QeaError("page_tiles_gather: a uint8 store needs the 256-entry fp32 table")
    (offset, h, w, rows, out, store_p, *table_p), n, tile = _page_tables(
        "page_tiles_gather", offset, h, w, rows, 3, out, ("store", store, store.dtype),
        *([("table", table, torch.float32, 256)] if table is not None else []))
    _lib.check(_lib.lib().qea_page_tiles_gather(store_p, int(store.dtype == torch.float32), store.numel(), offset, h, w, n, rows, *tile,
                                                table_p[0] if table_p else None, out, _stream()), "qea_page_tiles_gather")
    PAGE_LAUNCHES["gather"] += 1


def page_tiles_scatter(tiles, rows, offset, h, w, out_f32=None, out_u8=None):
    """include/qea_hip.h: qea_page_tiles_scatter — tiles [N,1,TH,TW] fp32 and the tile rows (int32 [N][7] = page, oy, ox, cy0, cy1, cx0, cx1)
    -> the core of every tile pasted into the packed outputs (out_f32 fp32 and / or out_u8 uint8, one-dimensional, as large as each other)
    by ONE launch without atomics; the 8-bit value is (uint8)(min(max(x, 0), 1) * 255)."""
    outs = [(name, o, dt) for name, o, dt in (("out_f32", out_f32, torch.float32), ("out_u8", out_u8, torch.uint8)) if o is not None]
    if not outs:
        raise _lib.QeaError("page_tiles_scatter needs out_f32, out_u8 or both")
    if any(o.dim() != 1 for _, o, _ in outs):
        raise _lib.QeaError("page_tiles_scatter needs one-dimensional outputs")
    size = outs[0][1].numel()
    (offset, h, w, rows, tiles, *_), n, tile = _page_tables("page_tiles_scatter", offset, h, w, rows, 7, tiles, *(spec + (size,) for spec in outs))
    _lib.check(_lib.lib().qea_page_tiles_scatter(tiles, *tile, rows, offset, h, w, n, size, _ptr(out_f32), _ptr(out_u8), _stream()),
               "qea_page_tiles_scatter")
    PAGE_LAUNCHES["scatter"] += 1


SPREAD_WAVE_MAX_N, SPREAD_LDS4_MAX_N, SPREAD_LDS_MAX_N, SPREAD_MAX_N = 1536, 24576, 32768, 1 << 24    # QEA_SPREAD_* of include/qea_hip.h
SAMPLER_LAUNCHES = {"spread": 0, "entropy": 0}    # launches of csrc/sampling.hip issued through this module (tests, tools)
ENTROPY_NUM_CLASSES = 95                          # calc_entropy's constant (selection_utils.py:10), whatever the width of the scores


def spread_pick(est, pts):
    """include/qea_hip.h: qea_spread_pick — est [n] / pts [k] (CUDA fp32, FINITE: the caller checks) -> idx [k] int64 on the device:
    the k serial picks of the range samplers in one launch.  Nothing synchronises."""
    if not (est.is_cuda and pts.is_cuda) or est.dtype != torch.float32 or pts.dtype != torch.float32 or est.dim() != 1 or pts.dim() != 1:
        raise _lib.QeaError("spread_pick needs two one-dimensional CUDA float32 tensors (the host loop of selection_utils is the CPU path)")
    n, k = est.numel(), pts.numel()
    if not (1 <= n <= SPREAD_MAX_N and 1 <= k <= SPREAD_MAX_N):
        raise _lib.QeaError(f"spread_pick: n={n}, k={k} outside 1..{SPREAD_MAX_N}")
    est, pts = est.contiguous(), pts.contiguous()
    L = _lib.lib()
    idx = torch.empty(k, dtype=torch.int64, device=est.device)
    nbytes = L.qea_spread_pick_workspace_bytes(n)
    ws = workspace(nbytes, est.device) if nbytes else None
    _lib.check(L.qea_spread_pick(_ptr(est), n, _ptr(pts), k, _ptr(idx), ws.data_ptr() if ws is not None else None, _stream()), "qea_spread_pick")
    SAMPLER_LAUNCHES["spread"] += 1
    return idx


def seq_entropy(scores):
    """include/qea_hip.h: qea_seq_entropy — scores [T][B][C] CUDA fp32 log-probs with a unit class stride (any T and B strides: the
    CRNN's 96-column rows, a [:, a:b, :] slice) -> [B] fp32 normalised mean entropies on the device, one launch."""
    if not scores.is_cuda or scores.dtype != torch.float32 or scores.dim() != 3:
        raise _lib.QeaError("seq_entropy needs a CUDA float32 tensor [T][B][C] (selection_utils.update_entropies keeps the host path)")
    T, B, Cc = scores.shape
    if Cc > 1 and scores.stride(2) != 1 or scores.stride(0) < 0 or scores.stride(1) < 0:
        scores = scores.contiguous()
    out = torch.empty(B, dtype=torch.float32, device=scores.device)
    if T == 0 or B == 0 or Cc == 0:
        raise _lib.QeaError(f"seq_entropy: empty scores {tuple(scores.shape)}")
    _lib.check(_lib.lib().qea_seq_entropy(_ptr(scores), scores.stride(0), scores.stride(1), T, B, Cc, ENTROPY_NUM_CLASSES, _ptr(out), _stream()),
               "qea_seq_entropy")
    SAMPLER_LAUNCHES["entropy"] += 1
    return out


BINARIZE_TILE, BINARIZE_CHUNK = (32, 64), 32768             # QEA_BINARIZE_TILE_H / _W / _CHUNK of include/qea_hip.h
BINARIZE_MAX_WINDOW, BINARIZE_MAX_PAGE_PIXELS = 127, 1 << 27
BINARIZE_LAUNCHES = {"sauvola": 0, "histogram": 0, "otsu": 0}    # launches of csrc/binarize.hip issued through this module (tests, tools)

PageTable = namedtuple("PageTable", "n host_h host_w offset h w tile_first chunk_first words")


def page_table(offset, h, w, device):
    """The page table of a packed store (HOST arrays: element offset int64 [n], h / w int32 [n]) plus the two block-to-page prefix tables
    of csrc/page_store.h (32 x 64 tiles, chunks of 32768 elements), in ONE upload: -> PageTable (device pointers into one int32 tensor, which it keeps alive, and the host copies
    of h / w the entry points validate).  Page sizes are checked by the entry points, not here."""
    if torch.device(device).type != "cuda":
        raise _lib.QeaError(f"the binarisation kernels need a CUDA device (qea/binarize.py has the host path), not {device}")
    offset, h, w = (np.ascontiguousarray(np.asarray(a), dt) for a, dt in ((offset, np.int64), (h, np.int32), (w, np.int32)))
    n = offset.size
    if n < 1 or h.shape != (n,) or w.shape != (n,) or offset.shape != (n,):
        raise _lib.QeaError(f"page table: offset {offset.shape}, h {h.shape}, w {w.shape} are not three arrays of one length >= 1")
    h64, w64 = np.maximum(h.astype(np.int64), 0), np.maximum(w.astype(np.int64), 0)
    tiles = -(-h64 // BINARIZE_TILE[0]) * -(-w64 // BINARIZE_TILE[1])
    chunks = -(-(h64 * w64) // BINARIZE_CHUNK)
    if int(tiles.sum()) >= 2 ** 31 or int(chunks.sum()) >= 2 ** 31:
        raise _lib.QeaError(f"page table: {int(tiles.sum())} tiles / {int(chunks.sum())} chunks, more than 2^31 - 1 workgroups")
    first = [np.concatenate([[0], np.cumsum(c)]).astype(np.int32) for c in (tiles, chunks)]
    words = torch.from_numpy(np.concatenate([offset.view(np.int32), h, w] + first)).to(device)      # the int64 offsets lead: 8-byte aligned
    at = np.cumsum([0, 2 * n, n, n, n + 1]) * 4 + words.data_ptr()
    return PageTable(n, h, w, *(int(a) for a in at), words)


def _page_store(who, store, table=None):
    """the packed store of every page entry point: one-dimensional, uint8 or float32, on a CUDA device, and on its page table's if one is given"""
    if not torch.is_tensor(store) or store.dtype not in (torch.uint8, torch.float32) or store.dim() != 1 or not store.is_cuda:
        raise _lib.QeaError(f"{who} needs a one-dimensional uint8 or float32 CUDA store")
    if table is not None and table.words.device != store.device:
        raise _lib.QeaError(f"{who}: the page table is on {table.words.device}, the store on {store.device}")


def _page_ptrs(who, store, table, *specs):
    """ONE _tensors pass over the checked store (it adds: contiguous) and the caller's `specs` -> (the seven arguments that lead every entry
    point over a store: store, store_is_f32, store_elems, offset, h, w, n_pages; the pointers of specs)"""
    ptrs = _tensors(who, store.device, ("store", store, store.dtype), *specs)
    return (ptrs[0], int(store.dtype == torch.float32), store.numel(), table.offset, table.h, table.w, table.n), ptrs[1:]


def _page_args(who, store, table, *outs):
    """-> the nine leading arguments of the entry points that also take the host's copy of h / w; outs: (name, tensor or None, dtype), as
    large as the store"""
    _page_store(who, store, table)
    lead, _ = _page_ptrs(who, store, table, *((name, t, dt, store.numel()) for name, t, dt in outs if t is not None))
    return lead + (table.host_h.ctypes.data, table.host_w.ctypes.data)


def binarize_sauvola(store, table, window=25, k=0.2, R=128.0, out_f32=None, out_u8=None):
    """include/qea_hip.h: qea_binarize_sauvola — every page of the packed `store` (uint8 or fp32; `table`: page_table) through
    Sauvola's rule in ONE launch on the current stream: 0 / 0.0 for ink, 255 / 1.0 for background into out_u8 and / or out_f32, packed
    like the store."""
    args = _page_args("binarize_sauvola", store, table, ("out_f32", out_f32, torch.float32), ("out_u8", out_u8, torch.uint8))
    _lib.check(_lib.lib().qea_binarize_sauvola(*args, table.tile_first, int(window), float(k), float(R), _ptr(out_f32), _ptr(out_u8), _stream()),
               "qea_binarize_sauvola")
    BINARIZE_LAUNCHES["sauvola"] += 1


def otsu_histogram(store, table):
    """include/qea_hip.h: qea_otsu_histogram — launch 1 of Otsu -> the pages' grey-level counts, int32 [n][256] on the device (the entry
    point zeroes the table itself)."""
    args = _page_args("otsu_histogram", store, table)
    hist = torch.empty(table.n, 256, dtype=torch.int32, device=store.device)
    _lib.check(_lib.lib().qea_otsu_histogram(*args, table.chunk_first, hist.data_ptr(), _stream()), "qea_otsu_histogram")
    BINARIZE_LAUNCHES["histogram"] += 1
    return hist


def binarize_otsu(store, table, hist, out_f32=None, out_u8=None):
    """include/qea_hip.h: qea_binarize_otsu — launch 2 of Otsu: every workgroup derives its page's threshold from `hist` (otsu_histogram)
    and writes ink as 0 / 0.0, background as 255 / 1.0 -> the thresholds, int32 [n] on the device (-1: a page of one grey level)."""
    args = _page_args("binarize_otsu", store, table, ("out_f32", out_f32, torch.float32), ("out_u8", out_u8, torch.uint8))
    (hist_p,) = _tensors("binarize_otsu", store.device, ("hist", hist, torch.int32, table.n * 256))
    thresholds = torch.empty(table.n, dtype=torch.int32, device=store.device)
    _lib.check(_lib.lib().qea_binarize_otsu(*args, table.chunk_first, hist_p, _ptr(out_f32), _ptr(out_u8), thresholds.data_ptr(), _stream()),
               "qea_binarize_otsu")
    BINARIZE_LAUNCHES["otsu"] += 1
    return thresholds


CC_MAX_GAP = 127                                               # QEA_CC_MAX_GAP of include/qea_hip.h
# launches of csrc/components.hip issued through this module, one key per kernel (tests, tools)
COMPONENT_LAUNCHES = {"tile": 0, "border": 0, "flatten": 0, "stats": 0, "despeckle": 0, "smear": 0, "boxes": 0}


def _cc_buffer(who, store, name, t, dtype=torch.int32):
    """a working buffer packed like the store: the given one, checked, or a new one"""
    if t is None:
        return torch.empty(store.numel(), dtype=dtype, device=store.device)
    _tensors(who, store.device, (name, t, dtype, store.numel()))
    return t


def cc_label(store, table, connectivity=8, ink_max=127, ink_mask=None, labels=None, area=None):
    """include/qea_hip.h: qea_cc_label — three launches (tile, border, flatten) on the current stream -> labels, int32 packed like the
    store: an ink pixel's label is the smallest page-relative index of its component, background is -1.  `ink_mask` (uint8, packed like
    the store) replaces the ink_max threshold; `area` (int32, packed like the store) is cleared inside the pages for cc_stats."""
    args = _page_args("cc_label", store, table)
    labels = _cc_buffer("cc_label", store, "labels", labels)
    if ink_mask is not None:
        _tensors("cc_label", store.device, ("ink_mask", ink_mask, torch.uint8, store.numel()))
    if area is not None:
        _tensors("cc_label", store.device, ("area", area, torch.int32, store.numel()))
    _lib.check(_lib.lib().qea_cc_label(*args, table.tile_first, _ptr(ink_mask), int(ink_max), int(connectivity), labels.data_ptr(), _ptr(area),
                                       _stream()), "qea_cc_label")
    for key in ("tile", "border", "flatten"):
        COMPONENT_LAUNCHES[key] += 1
    return labels


def cc_stats(store, table, labels, area):
    """include/qea_hip.h: qea_cc_stats — one launch: adds every component's pixel count to area[its root]; `area` is the buffer cc_label
    cleared -> area"""
    args = _page_args("cc_stats", store, table, ("labels", labels, torch.int32), ("area", area, torch.int32))
    _lib.check(_lib.lib().qea_cc_stats(*args, table.tile_first, labels.data_ptr(), area.data_ptr(), _stream()), "qea_cc_stats")
    COMPONENT_LAUNCHES["stats"] += 1
    return area


def cc_despeckle(store, table, labels, area, min_area, out_f32=None, out_u8=None):
    """include/qea_hip.h: qea_cc_despeckle — one launch: ink of components of at least min_area pixels as 0 / 0.0, everything else as
    255 / 1.0 into out_u8 and / or out_f32, packed like the store."""
    args = _page_args("cc_despeckle", store, table, ("labels", labels, torch.int32), ("area", area, torch.int32),
                          ("out_f32", out_f32, torch.float32), ("out_u8", out_u8, torch.uint8))
    _lib.check(_lib.lib().qea_cc_despeckle(*args, table.tile_first, labels.data_ptr(), area.data_ptr(), int(min_area), _ptr(out_f32),
                                           _ptr(out_u8), _stream()), "qea_cc_despeckle")
    COMPONENT_LAUNCHES["despeckle"] += 1


def cc_smear(store, table, gap, vertical=False, ink_max=127, in_mask=None, out_mask=None):
    """include/qea_hip.h: qea_cc_smear — one launch, one direction of run-length smoothing over the ink of the store (or of `in_mask`)
    -> out_mask, uint8 1 / 0 packed like the store"""
    args = _page_args("cc_smear", store, table)
    if in_mask is not None:
        _tensors("cc_smear", store.device, ("in_mask", in_mask, torch.uint8, store.numel()))
    out_mask = _cc_buffer("cc_smear", store, "out_mask", out_mask, torch.uint8)
    _lib.check(_lib.lib().qea_cc_smear(*args, table.tile_first, _ptr(in_mask), int(ink_max), int(gap), int(bool(vertical)), out_mask.data_ptr(),
                                       _stream()), "qea_cc_smear")
    COMPONENT_LAUNCHES["smear"] += 1
    return out_mask


def cc_boxes(store, table, labels, roots, root_first):
    """include/qea_hip.h: qea_cc_boxes — one launch.  roots: the ascending page-relative roots of all pages, int32 [n] on the device, page
    p's being roots[root_first[p]:root_first[p + 1]] (root_first: int32 [pages + 1] on the device) -> int32 [n][4] = (x_min, y_min,
    x_max, y_max) of the listed components, inclusive"""
    args = _page_args("cc_boxes", store, table, ("labels", labels, torch.int32))
    n = roots.numel()
    _tensors("cc_boxes", store.device, ("roots", roots, torch.int32), ("root_first", root_first, torch.int32, table.n + 1))
    boxes = torch.empty(max(n, 1), 4, dtype=torch.int32, device=store.device)      # one spare row: an empty list still has an address
    boxes[:, :2] = 2 ** 31 - 1
    boxes[:, 2:] = -1
    roots_p = roots.data_ptr() if n else boxes.data_ptr()
    _lib.check(_lib.lib().qea_cc_boxes(*args, table.tile_first, labels.data_ptr(), roots_p, root_first.data_ptr(), n, boxes.data_ptr(), _stream()),
               "qea_cc_boxes")
    COMPONENT_LAUNCHES["boxes"] += 1
    return boxes[:n]


DESKEW_MAX_SIDE, DESKEW_MAX_SLOPE, DESKEW_MAX_GAIN = 32767, 256, 10000       # QEA_DESKEW_MAX_* of include/qea_hip.h
# launches of csrc/deskew.hip issued through this module, one key per kernel (tests, tools)
DESKEW_LAUNCHES = {"strip_sums": 0, "scores": 0, "pick": 0, "rotate": 0}


def skew_strip_sums(store, table, ink_max=127, C=None):
    """include/qea_hip.h: qea_skew_strip_sums — one launch -> C, uint8 packed like the store: page p's C[j][y], the ink pixels of row y in
    the 32-column strip j, at offset[p] + j * h[p] + y.  ink_max: an integer 0..254, or an int32 [n] tensor on the device (-1..254 per
    page, e.g. the thresholds binarize_otsu returns), which is read by the kernel, not by the host."""
    args = _page_args("skew_strip_sums", store, table)
    C = _cc_buffer("skew_strip_sums", store, "C", C, torch.uint8)
    per_page = None
    if torch.is_tensor(ink_max):
        (per_page,) = _tensors("skew_strip_sums", store.device, ("ink_max", ink_max, torch.int32, table.n))
    _lib.check(_lib.lib().qea_skew_strip_sums(*args, per_page, 0 if per_page else int(ink_max), C.data_ptr(), _stream()), "qea_skew_strip_sums")
    DESKEW_LAUNCHES["strip_sums"] += 1
    return C


def skew_scores(C, table, A=90, scores=None):
    """include/qea_hip.h: qea_skew_scores — one launch (the entry point zeroes the table itself) -> int64 [n][2 A + 1]: the differential
    projection-profile score of every candidate slope a / 1024, a = -A..A, from the strip sums C"""
    if not torch.is_tensor(C) or C.dim() != 1 or not C.is_cuda or table.words.device != C.device:
        raise _lib.QeaError("skew_scores needs the one-dimensional uint8 CUDA array skew_strip_sums filled, on the page table's device")
    _tensors("skew_scores", C.device, ("C", C, torch.uint8))
    if scores is None:
        scores = torch.empty(table.n, 2 * int(A) + 1, dtype=torch.int64, device=C.device)
    _tensors("skew_scores", C.device, ("scores", scores, torch.int64, table.n * (2 * int(A) + 1)))
    _lib.check(_lib.lib().qea_skew_scores(C.data_ptr(), C.numel(), table.offset, table.h, table.w, table.n, table.host_h.ctypes.data,
                                          table.host_w.ctypes.data, int(A), scores.data_ptr(), _stream()), "qea_skew_scores")
    DESKEW_LAUNCHES["scores"] += 1
    return scores


def skew_pick(scores, g=0, slopes=None):
    """include/qea_hip.h: qea_skew_pick — one launch.  scores: int64 [n][2 A + 1] on the device, any values -> int32 [n]: per row the a of
    the largest score (ties: the smallest |a|, then the negative one), or 0 where 100 (S_a - S_0) < g S_0"""
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] % 2 != 1:
        raise _lib.QeaError("skew_pick needs an int64 [n][2 A + 1] CUDA tensor")
    n, A = scores.shape[0], scores.shape[1] // 2
    _tensors("skew_pick", scores.device, ("scores", scores, torch.int64))
    if slopes is None:
        slopes = torch.empty(n, dtype=torch.int32, device=scores.device)
    _tensors("skew_pick", scores.device, ("slopes", slopes, torch.int32, n))
    _lib.check(_lib.lib().qea_skew_pick(scores.data_ptr(), n, A, int(g), slopes.data_ptr(), _stream()), "qea_skew_pick")
    DESKEW_LAUNCHES["pick"] += 1
    return slopes


def deskew_rotate(store, table, slopes, rot_table, interp="bilinear", fill=255, norm=None, out_f32=None, out_u8=None):
    """include/qea_hip.h: qea_deskew_rotate — ONE launch: every page of the packed store rotated about its centre by its slope
    (slopes: int32 [n] on the device, read by the kernel only) into out_u8 and / or out_f32, packed like the store.  rot_table: int32
    [2 A + 1][2] on the device (qea/deskew.py: rotation_table); norm: the 256 fp32 values an fp32 output is read through."""
    if interp not in ("bilinear", "nearest"):
        raise _lib.QeaError(f"deskew_rotate: interp={interp!r} is neither 'bilinear' nor 'nearest'")
    args = _page_args("deskew_rotate", store, table, ("out_f32", out_f32, torch.float32), ("out_u8", out_u8, torch.uint8))
    if not torch.is_tensor(rot_table) or rot_table.dim() != 2 or rot_table.shape[1] != 2 or rot_table.shape[0] % 2 != 1:
        raise _lib.QeaError("deskew_rotate: rot_table must be an int32 [2 A + 1][2] tensor")
    _tensors("deskew_rotate", store.device, ("slopes", slopes, torch.int32, table.n), ("rot_table", rot_table, torch.int32))
    if norm is not None:
        _tensors("deskew_rotate", store.device, ("norm", norm, torch.float32, 256))
    _lib.check(_lib.lib().qea_deskew_rotate(*args, table.tile_first, slopes.data_ptr(), rot_table.data_ptr(), rot_table.shape[0] // 2,
                                            int(interp == "nearest"), int(fill), _ptr(norm), _ptr(out_f32), _ptr(out_u8), _stream()),
               "qea_deskew_rotate")
    DESKEW_LAUNCHES["rotate"] += 1


# QEA_WORD_STRIP_* of include/qea_hip.h
WORD_STRIP_H, WORD_STRIP_MIN_W, WORD_STRIP_MAX_W, WORD_STRIP_MAX_BOXES, WORD_STRIP_MAX_SIDE = 32, 64, 512, 1 << 20, 32767
WORD_STRIP_LAUNCHES = {"strips": 0}          # launches of csrc/word_strips.hip issued through this module (tests, tools)


def word_strips(store, table, boxes, OW, norm, out=None):
    """include/qea_hip.h: qea_word_strips — the packed `store` (uint8 or fp32; `table`: page_table), boxes int32 [n][5] =
    (page, x0, y0, x1, y1) on the device with x1 / y1 exclusive, and norm, the 256 fp32 values a grey level is written as -> out
    [n, 1, 32, OW] fp32, written whole by ONE launch on the current stream: every box clipped to its page, copied 1:1 where it has at
    most 32 rows, shrunk to 32 rows by the exact area average where it has more, centred in OW on a white ground."""
    _page_store("word_strips", store, table)
    if not torch.is_tensor(boxes) or boxes.dim() != 2 or boxes.shape[1] != 5:
        raise _lib.QeaError("word_strips: boxes must be an int32 [n][5] tensor = (page, x0, y0, x1, y1)")
    n, OW = boxes.shape[0], int(OW)
    if OW % 16 or not WORD_STRIP_MIN_W <= OW <= WORD_STRIP_MAX_W:
        raise _lib.QeaError(f"word_strips: OW={OW} must be a multiple of 16 in {WORD_STRIP_MIN_W}..{WORD_STRIP_MAX_W}")
    if out is None:
        out = torch.empty(n, 1, WORD_STRIP_H, OW, dtype=torch.float32, device=store.device)
    if out.dim() != 4 or tuple(out.shape[:3]) != (n, 1, WORD_STRIP_H) or out.shape[3] != OW:
        raise _lib.QeaError(f"word_strips: out {tuple(out.shape)} for {n} boxes at width {OW}")
    args, (boxes_p, norm_p, out_p) = _page_ptrs("word_strips", store, table, ("boxes", boxes, torch.int32), ("norm", norm, torch.float32, 256),
                                                ("out", out, torch.float32))
    if n == 0:                                                 # nothing to write, and an empty tensor has no pointer to hand over
        return out
    _lib.check(_lib.lib().qea_word_strips(*args, boxes_p, n, OW, norm_p, out_p, _stream()), "qea_word_strips")
    WORD_STRIP_LAUNCHES["strips"] += 1
    return out


LINE_MAX_BOXES, LINE_MAX_TALL, LINE_MAX_GAP = 4096, 64, 1024       # QEA_LINE_MAX_* of include/qea_hip.h
LINE_LAUNCHES = {"group": 0}                 # launches of csrc/lines.hip issued through this module (tests, tools)
LineGroups = namedtuple("LineGroups", "line pos order line_box n_lines med")


def line_group(boxes, box_first, max_boxes, overlap=50, tall=3, gap=0):
    """include/qea_hip.h: qea_line_group — boxes int32 [N][4] = (x_min, y_min, x_max, y_max), inclusive, page after page, and box_first
    int32 [pages + 1], both on the device; max_boxes: the largest page, a host value (a page that holds more gets -1 throughout) ->
    LineGroups(line, pos, order: int32 [N]; line_box: int32 [N][4], a page's L line boxes in its first L rows and -1 in the rest; n_lines:
    int32 [pages]; med: int64 [pages]), written by ONE launch on the current stream; nothing is read back."""
    if not torch.is_tensor(boxes) or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise _lib.QeaError("line_group: boxes must be an int32 [N][4] tensor = (x_min, y_min, x_max, y_max)")
    if not torch.is_tensor(box_first) or box_first.dim() != 1 or box_first.numel() < 1:
        raise _lib.QeaError("line_group: box_first must be an int32 [pages + 1] tensor")
    dev, N, P = boxes.device, boxes.shape[0], box_first.numel() - 1
    _tensors("line_group", dev, ("boxes", boxes, torch.int32), ("box_first", box_first, torch.int32))
    line, pos, order = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    line_box = torch.empty(N, 4, dtype=torch.int32, device=dev)
    n_lines = torch.empty(P, dtype=torch.int32, device=dev)
    med = torch.empty(P, dtype=torch.int64, device=dev)
    out = LineGroups(line, pos, order, line_box, n_lines, med)
    _lib.check(_lib.lib().qea_line_group(*(t.data_ptr() if t.numel() else None for t in (boxes, box_first)), P, N, int(max_boxes), int(overlap),
                                         int(tall), int(gap), *(t.data_ptr() if t.numel() else None for t in out), _stream()), "qea_line_group")
    LINE_LAUNCHES["group"] += int(P > 0 and N > 0)
    return out
