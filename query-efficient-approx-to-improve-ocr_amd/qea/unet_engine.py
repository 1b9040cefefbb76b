"""UNet cleaner on the HIP library: explicit forward / backward kernel schedules.

Mirrors reference models/model_unet.py:49-76 (forward) and its autograd.  Everything between
the [B,1,H,W] input and the [B,1,H,W] sigmoid output stays NHWC in HBM:

  * every conv3x3 of a `_block` (model_unet.py:78-109) is one implicit-GEMM MFMA launch; its
    BatchNorm is a statistics pass (fp64 sums) + one apply(+ReLU) pass;
  * a decoder level's torch.cat((up, skip), 1) (model_unet.py:63-74) never copies: the encoder's
    second BN/ReLU writes its output into channels [c, 2c) of the level's concat buffer and the
    transposed conv scatters into channels [0, c);
  * the backward walks the same graph in reverse with dgrad = the same implicit GEMM on
    flipped/transposed filters, wgrad = the pixel-reduction MFMA kernel, accumulating straight
    into the flat gradient buffer (qea/params.py).
"""
import torch

from . import batchnorm, conv, ops
from .act import Act
from .params import ensure_flat

FUSE_EVAL_BN = True   # tests flip this to compare the fused inference epilogue with the two-pass form
FUSE_BN_BWD_SUMS = True   # tests flip this: BatchNorm1's backward reductions from the producing dgrad's epilogue (qea_conv_desc.bst_y)
FUSE_BN_POOL = True   # tests flip this: the encoder's BatchNorm apply + ReLU and its 2x2 max-pool in one pass (qea_bn_apply_pool)
FUSE_POOL_BWD = True  # tests flip this: the encoder's pool backward inside the BatchNorm2 backward (qea_bn_bwd_pool), no pass of its own


class _Block:
    """Names + channel counts of one conv-BN-ReLU x2 block."""

    def __init__(self, mod, name, cin, cout):
        self.mod, self.name, self.cin, self.cout = mod, name, cin, cout

    def key(self, i, leaf):
        kind = "conv" if leaf == "w" else "norm"
        suffix = {"w": "weight", "gamma": "weight", "beta": "bias", "rm": "running_mean", "rv": "running_var"}[leaf]
        return f"{self.mod}.{self.name}{kind}{i}.{suffix}"


class UNetEngine:
    def __init__(self, module, features=32):
        self.m = module
        f = features
        self.f = f
        self.enc = [_Block("encoder1", "enc1", 1, f), _Block("encoder2", "enc2", f, 2 * f), _Block("encoder3", "enc3", 2 * f, 4 * f),
                    _Block("encoder4", "enc4", 4 * f, 8 * f)]
        self.bott = _Block("bottleneck", "bottleneck", 8 * f, 16 * f)
        self.dec = {l: _Block(f"decoder{l}", f"dec{l}", 2 * c, c) for l, c in ((4, 8 * f), (3, 4 * f), (2, 2 * f), (1, f))}

    # ------------------------------------------------------------------ helpers
    def _conv_bn_relu(self, P, Bf, blk, i, x, cv, out, training, keep, parts, pool=None):
        """x [B,H,W,cin] -> the 3x3 layer cv -> BN -> ReLU -> out (Acts; x of the one-channel first layer: the image itself).  training,
        parts, keep: see batchnorm.forward.
        pool = the Act [B*(H/2)*(W/2)][cout]: the 2x2 max-pool of the block output (model_unet.py:52-59) leaves with the BatchNorm apply
        in ONE pass (FUSE_BN_POOL) where there is such a pass.
        -> (the batchnorm.Stage, or None where the BatchNorm rode in the conv; True when the pool left here, else the caller pools)."""
        B, H, W, cin, cout = cv.B, cv.H, cv.W, cv.Cin, cv.N
        w = P[blk.key(i, "w")]
        bn = (P[blk.key(i, "gamma")], P[blk.key(i, "beta")], Bf[blk.key(i, "rm")], Bf[blk.key(i, "rv")])
        if not training and not keep and cin != 1 and FUSE_EVAL_BN:
            # inference (Phase A's cleaner pass, validation): eval-mode BatchNorm + ReLU ride in the conv epilogue — the
            # same fused multiply-add bn_apply evaluates, so the result is bit-identical to the two-pass form
            scale, shift = batchnorm.eval_scale_shift(cout, *bn)
            fuse_pool = pool is not None and cv.can_pool(2, x, out)     # ... and so does the 2x2 max-pool behind the block
            cv.fwd(x, w, out, scale=scale, bias=shift, relu=True, pool=(pool, 2) if fuse_pool else None)
            return None, fuse_pool
        y = Act.empty(B * H * W, cout, out.t.device)
        fused = None
        if cin == 1:
            ops.conv_c1_fwd(x, w, None, y.t, y.ld, B, H, W, cout, relu=False)
        else:
            # train-mode BatchNorm: the conv's epilogue also leaves per-block fp64 column sums of y (no second pass over y)
            # (per-group statistics take the separate pass: a statistics block of the generic tile may straddle two images)
            fused = cv.fwd(x, w, y, want_stats=training and len(parts) == 1)
        return batchnorm.forward(y, out, H, W, *bn, training, parts, keep, partials=fused, pool=(pool, 2, 2) if pool is not None else None)

    # ------------------------------------------------------------------ forward
    def forward(self, x, training, need_grad, groups=1):
        """x: [B,1,H,W] contiguous CUDA fp32.  Returns (out [B,1,H,W], ctx or None).  groups: see batchnorm.partition (train mode only)."""
        fs = ensure_flat(self.m)
        P, Bf = dict(self.m.named_parameters()), dict(self.m.named_buffers())
        B, _, H, W = x.shape
        if H % 16 or W % 16:
            raise ValueError(f"UNet input {H}x{W} must be a multiple of 16 in both dimensions")
        dev = x.device
        parts = batchnorm.partition(int(groups) if training else 1, B)
        ctx = {"x": x, "B": B, "H": H, "W": W, "blocks": {}} if need_grad else None

        # every tensor a split-fp16 conv / wgrad launch will consume carries the abs-max slot its producer fills (None: that split is off)
        slot = ops.amax_pool(dev)

        def run_block(blk, xin, cin, h, w, out, pool=None):
            a1 = Act.empty(B * h * w, blk.cout, dev, slot)
            c1, c2 = (conv.Conv(B, h, w, ci, blk.cout, 3, 3, pad=(1, 1)) for ci in (cin, blk.cout))      # the block's two 3x3 layers
            bn1, _ = self._conv_bn_relu(P, Bf, blk, 1, xin, c1, a1, training, need_grad, parts)
            bn2, pooled_here = self._conv_bn_relu(P, Bf, blk, 2, a1, c2, out, training, need_grad, parts, pool)
            if need_grad:
                # (h, w: the block's plane under the keys tests/decisions.py reads; the backward reads the records)
                ctx["blocks"][blk.mod] = {"xin": xin, "c1": c1, "c2": c2, "h": h, "w": w, "a1": a1, "out": out, "bn1": bn1, "bn2": bn2,
                                          "y1": bn1.y, "y2": bn2.y}        # the conv outputs under the names the trace tools tap
            return pooled_here

        # encoder: level l has c = f*2^(l-1) channels at (H,W)/2^(l-1); its output goes to cat_l[:, c:2c]
        cats = {}
        xin, cin, h, w = x, 1, H, W                             # (the one-channel image is no record: conv_c1_* take it as it is)
        for l, blk in enumerate(self.enc, start=1):
            c = blk.cout
            cat = Act.empty(B * h * w, 2 * c, dev, slot)        # one slot for the skip half (BatchNorm apply) and the up half (transposed conv)
            cats[l] = (cat, h, w, c)
            skip = cat.cols(c, c)
            pooled = Act.empty(B * (h // 2) * (w // 2), c, dev, slot)
            if not run_block(blk, xin, cin, h, w, skip, pool=pooled if FUSE_BN_POOL else None):
                ops.maxpool_fwd(skip.t, skip.ld, pooled.t, pooled.ld, B, h, w, c, 2, 2, amax=pooled.amax)
            xin, cin, h, w = pooled, c, h // 2, w // 2
        d = Act.empty(B * h * w, self.bott.cout, dev, slot)     # (the transposed conv that consumes d is a split GEMM too)
        run_block(self.bott, xin, cin, h, w, d)
        ups = {}
        for l in (4, 3, 2, 1):
            cat, hh, ww, c = cats[l]
            # upconv_l is the adjoint of the stride-2 2x2 layer (hh, ww, c) -> (h, w, d.C), whose filter its weight [2c][2][2][c] is as it lies
            up = conv.Conv(B, hh, ww, c, d.C, 2, 2, stride=(2, 2))
            up.scatter_adjoint(d, P[f"upconv{l}.weight"], Act(cat.t, c, cat.ld, cat.amax), bias=P[f"upconv{l}.bias"])
            ups[l] = (d, up)
            d = Act.empty(B * hh * ww, c, dev, slot)
            run_block(self.dec[l], cat, 2 * c, hh, ww, d)
        out = torch.empty(B, 1, H, W, device=dev)
        ops.head_fwd(d.t, d.ld, P["conv.weight"], P["conv.bias"], out, B * H * W, d.C)
        if training:
            fs.ibuf.add_(len(parts))                            # all num_batches_tracked counters at once
        if need_grad:
            ctx.update(cats=cats, ups=ups, d1=d, out=out)
        return out, ctx

    # ------------------------------------------------------------------ backward
    def backward(self, ctx, dout):
        """dout: gradient w.r.t. the sigmoid output [B,1,H,W].  Parameter gradients are accumulated
        into the flat gradient buffer; returns None (the input image needs no gradient)."""
        fs = ensure_flat(self.m)
        fs.attach_grads()
        P = dict(self.m.named_parameters())
        G = {n: p.grad for n, p in P.items()}
        B, H, W = ctx["B"], ctx["H"], ctx["W"]
        dev = dout.device
        dout = dout.contiguous()
        side = ops.SideStream.of(self, dev)
        slot = ops.amax_pool(dev)

        def block_bwd(blk, da2, pool=None):
            """da2: grad w.r.t. the block output.  Returns grad w.r.t. the block input as a fresh [M][cin] Act (a decoder block's feeds
            the transposed conv's dgrad GEMM: it carries its slot), or None for the first encoder block.
            pool = (dpool, 2): the gradient of the block's 2x2-pooled output still has to be routed to the winners and added to da2 —
            done inside the two passes of BatchNorm2's backward (qea_bn_bwd_pool)."""
            s = ctx["blocks"][blk.mod]
            c1, c2 = s["c1"], s["c2"]
            h, w, cin, cout = c1.H, c1.W, c1.Cin, c1.N
            M = B * h * w
            dy2 = Act.empty(M, cout, dev, slot)
            dy1_amax = slot()
            batchnorm.backward(s["bn2"], da2, dy2, P[blk.key(2, "gamma")], G[blk.key(2, "gamma")], G[blk.key(2, "beta")], pool=pool)
            side.run(lambda: c2.wgrad(dy2, s["a1"], G[blk.key(2, "w")], accumulate=True), dy2.t)
            da1 = Act.empty(M, cout, dev)
            # the two reductions of BatchNorm1's backward come with da1 from the dgrad's epilogue (FUSE_BN_BWD_SUMS; train mode, one
            # statistics group, fp16 form) instead of a pass of their own over da1 and y1
            bst = s["bn1"].producer_sums() if FUSE_BN_BWD_SUMS else None
            part = c2.dgrad(dy2, P[blk.key(2, "w")], da1, bwd_stats=bst)
            dy1 = Act(torch.empty(M, cout, device=dev), amax=dy1_amax)       # (dy2 may still be read by its wgrad on the side stream)
            batchnorm.backward(s["bn1"], da1, dy1, P[blk.key(1, "gamma")], G[blk.key(1, "gamma")], G[blk.key(1, "beta")],
                               partials=part if bst is not None else None)
            if cin == 1:
                side.run(lambda: ops.conv_c1_wgrad(s["xin"], dy1.t, dy1.ld, G[blk.key(1, "w")], None, B, h, w, cout, accumulate=True), dy1.t)
                return None
            side.run(lambda: c1.wgrad(dy1, s["xin"], G[blk.key(1, "w")], accumulate=True), dy1.t)
            dxin = Act.empty(M, cin, dev, slot)
            c1.dgrad(dy1, P[blk.key(1, "w")], dxin)
            return dxin

        # head
        d1 = ctx["d1"]
        dd = Act.empty(B * H * W, d1.C, dev)
        ops.head_bwd(d1.t, d1.ld, ctx["out"], dout, P["conv.weight"], dd.t, dd.ld, G["conv.weight"], G["conv.bias"], B * H * W, d1.C, accumulate=True)

        # decoder levels 1..4: block backward gives d(cat_l); split into up-conv grad and skip grad
        dcats = {}
        for l in (1, 2, 3, 4):
            dcats[l] = block_bwd(self.dec[l], dd)
            dprev, up = ctx["ups"][l]                       # input of upconv_l: [B*h*w][dcin]; the layer upconv_l is the adjoint of
            dup = Act(dcats[l].t, up.Cin, dcats[l].ld, dcats[l].amax)                    # the up half of dcat (whose abs-max the slot of the whole tensor bounds)
            def up_grads(dup=dup, dprev=dprev, l=l, up=up):
                ops.colsum(dup.t, dup.ld, dup.nrows, dup.C, G[f"upconv{l}.bias"], accumulate=True)
                up.wgrad(dprev, dup, G[f"upconv{l}.weight"], accumulate=True)
            side.run(up_grads, dup.t)
            dd = Act.empty(B * up.OH * up.OW, up.N, dev)
            up.fwd(dup, P[f"upconv{l}.weight"], dd)
        # bottleneck, then encoder 4..1: skip grad (dcat[:, c:]) + pool backward of the deeper level
        dpool = block_bwd(self.bott, dd)
        for l in (4, 3, 2, 1):
            cat, hh, ww, c = ctx["cats"][l]
            skip, dskip = cat.cols(c, c), dcats[l].cols(c, c)
            if FUSE_POOL_BWD and ctx["blocks"][self.enc[l - 1].mod]["bn2"].single:
                # the pool backward rides in the two passes of BatchNorm2's backward: dskip is read, never rewritten
                # (one statistics group only: the grouped backward keeps the pool's own pass)
                dpool = block_bwd(self.enc[l - 1], dskip, pool=(dpool, 2))
            else:
                ops.maxpool_bwd(skip.t, skip.ld, dpool.t, dpool.ld, dskip.t, dskip.ld, B, hh, ww, c, 2, 2, relu_mask=False, accumulate=True)
                dpool = block_bwd(self.enc[l - 1], dskip)
        side.join()
        return None
