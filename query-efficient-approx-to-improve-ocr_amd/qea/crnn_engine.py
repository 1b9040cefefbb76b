"""CRNN proxy on the HIP library: explicit forward / backward kernel schedules.

Mirrors reference models/model_crnn.py:16-28 (CRNN.forward), :47-56 (Convolutional.forward) and
their autograd, including the NaN scrub of CRNN.backward_hook (:30-32).

  x [B,1,32,W] -> conv1..conv7 (NHWC, bias/ReLU fused in the GEMM epilogue, pools as separate
  HBM passes) -> conv7 writes straight into the [T,B,512] sequence layout (map_to_sequence)
  -> 2 x bidirectional LSTM (input projection = one GEMM per direction, recurrence = fused
  MFMA step kernel) -> Linear (GEMM, vocab padded to 96 columns) -> log_softmax.
"""
import torch

from . import batchnorm, conv, ops
from .act import Act
from .params import ensure_flat

FUSE_POOL = True      # tests flip this: conv1 + ReLU + pool and BatchNorm2 apply + ReLU + pool as one pass each (same bits)
HID = 256

# (name, cin, cout, relu fused in the conv epilogue, pool after (kh,kw) or None)
CONVS = (("conv2", 64, 128, True, (2, 2)), ("conv3", 128, 256, True, None), ("conv4", 256, 256, True, (2, 1)))


FUSE_POOL_BWD = True  # tests flip this: conv6's (2,1) pool backward inside BatchNorm2's backward (qea_bn_bwd_pool)
FUSE_C1_BWD = True    # tests flip this: conv1 -> ReLU -> pool backward from the pooled gradient and x alone (qea_conv_c1_pool_bwd)
KEEP_A1 = False       # tests set this: keep conv1's full-resolution activation (2.1 GB at B = 2048) although nothing in the product reads it

class CRNNEngine:
    def __init__(self, module, vocab):
        self.m = module
        self.vocab = vocab
        self.vpad = (vocab + 31) // 32 * 32
        # `convo.module.` when the backbone sits in the (never used) nn.DataParallel wrapper
        self.cp = "convo.module." if any(n.startswith("convo.module.") for n, _ in module.named_parameters()) else "convo."

    # ------------------------------------------------------------------ forward
    def forward(self, x, bn_training, need_grad, groups=1):
        """groups > 1: the batch is `groups` jitter replicas of the same strips stacked along N (replica-major).
        Batch-statistic BatchNorm is then evaluated PER REPLICA GROUP and the running statistics are updated once
        per group in order, which is exactly what `groups` sequential forward passes of the reference do
        (sharing the statistics across replicas changes the gradients by 4e-2)."""
        fs = ensure_flat(self.m)
        P = dict(self.m.named_parameters())
        Bf = dict(self.m.named_buffers())
        dev = x.device
        B, _, H, W = x.shape
        if H != 32 or W % 4:
            raise ValueError(f"CRNN input must be [B,1,32,W] with W % 4 == 0, got {H}x{W}")
        c = self.cp
        parts = batchnorm.partition(groups, B)            # groups: an int (equal groups) or per-group sample counts (ragged, round 4)
        ctx = {"x": x, "B": B, "H": H, "W": W, "parts": parts} if need_grad else None

        # every tensor a split-fp16 conv / wgrad launch consumes carries the abs-max slot its producer fills (None when that split is off)
        slot = ops.amax_pool(dev)
        # conv1 (C_in = 1) + ReLU, pool 2x2
        # (round 4: the backward rebuilds this activation from x, qea_conv_c1_pool_bwd — it is written only where something still reads it)
        keep_a1 = KEEP_A1 or (need_grad and not (FUSE_POOL and FUSE_C1_BWD)) or H % 2 or W % 8
        a1 = Act.empty(B * H * W, 64, dev) if keep_a1 else None
        h, w = H // 2, W // 2
        p1 = Act.empty(B * h * w, 64, dev, slot)
        conv1 = (P[c + "conv1.weight"], P[c + "conv1.bias"])
        # conv1 + ReLU + max-pool in one pass where the shape allows (FUSE_POOL; the same bits as the two launches)
        if not (FUSE_POOL and ops.conv_c1_fwd_pool(x, *conv1, a1.t if a1 is not None else None, 64, p1.t, p1.ld, B, H, W, 64, relu=True, pooled_amax=p1.amax)):
            if a1 is None:
                a1 = Act.empty(B * H * W, 64, dev)
            ops.conv_c1_fwd(x, *conv1, a1.t, a1.ld, B, H, W, 64, relu=True)
            ops.maxpool_fwd(a1.t, a1.ld, p1.t, p1.ld, B, H, W, 64, 2, 2, amax=p1.amax)
        acts = {"a1": a1, "p1": p1}                       # a1 None: not kept (the backward rebuilds it from x; tests: ctx["conv1_params"])
        cur = p1
        convs = {}                                        # conv2 .. conv7: each layer's geometry, stated here and reused by the backward
        for name, cin, cout, relu, pool in CONVS:
            cv = convs[name] = conv.Conv(B, h, w, cin, cout, 3, 3, pad=(1, 1))
            a = acts["a" + name[-1]] = Act.empty(B * h * w, cout, dev, slot)
            fused = False
            if pool:
                ph, pw = h // pool[0], w // pool[1]
                pt = acts["p" + name[-1]] = Act.empty(B * ph * pw, cout, dev, slot)
                # the pool behind relu(conv) leaves with the conv's epilogue where the kernel has the instance (same bits)
                fused = FUSE_POOL and pool[0] == 2 and h % 2 == 0 and cv.can_pool(pool[1], cur, a)
            cv.fwd(cur, P[c + name + ".weight"], a, bias=P[c + name + ".bias"], relu=relu, pool=(pt, pool[1]) if fused else None)
            cur = a
            if pool:
                if not fused:
                    ops.maxpool_fwd(a.t, a.ld, pt.t, pt.ld, B, h, w, cout, pool[0], pool[1], amax=pt.amax)
                cur = pt
                h, w = ph, pw
        # conv5 + BN1 + ReLU, conv6 + BN2 + ReLU (bias stays in the conv: y = conv + b is what BN sees)
        for name, bn, cin in (("conv5", "batchnorm1", 256), ("conv6", "batchnorm2", 512)):
            y = acts["y" + name[-1]] = Act.empty(B * h * w, 512, dev)     # (y: the conv output under the name the trace tools tap)
            convs[name] = conv.Conv(B, h, w, cin, 512, 3, 3, pad=(1, 1))
            convs[name].fwd(cur, P[c + name + ".weight"], y, bias=P[c + name + ".bias"])
            a = acts["a" + name[-1]] = Act.empty(B * h * w, 512, dev, slot)
            pool = None
            if name == "conv6" and FUSE_POOL:
                # BatchNorm apply + ReLU + the (2,1) max-pool behind it in one pass (bit-identical; p6 is allocated here)
                p6 = Act.empty(B * (h // 2) * w, 512, dev, slot)
                pool = (p6, 2, 1)
            acts["bn" + name[-1]], _ = batchnorm.forward(y, a, h, w, P[c + bn + ".weight"], P[c + bn + ".bias"], Bf[c + bn + ".running_mean"],
                                                         Bf[c + bn + ".running_var"], bn_training, parts, need_grad, pool=pool)
            cur = a
        if bn_training:
            fs.ibuf.add_(len(parts))                                # num_batches_tracked: one per group, as sequential calls
        seq_amax = slot()
        if not FUSE_POOL:
            p6 = Act.empty(B * (h // 2) * w, 512, dev, slot)
            ops.maxpool_fwd(cur.t, cur.ld, p6.t, p6.ld, B, h, w, 512, 2, 1, amax=p6.amax)
        acts["p6"] = p6
        if h // 2 != 2:
            raise ValueError("CRNN backbone must reduce the height to 2 before conv7")
        # conv7 2x2 pad 0 -> [B,1,T,512], written as [T][B][512]
        c7 = convs["conv7"] = conv.Conv(B, h // 2, w, 512, 512, 2, 2)
        T = c7.OW
        seq = Act(torch.empty(T, B, 512, device=dev), amax=seq_amax)
        c7.fwd(p6, P[c + "conv7.weight"], seq, bias=P[c + "conv7.bias"], out_mode=ops.OUT_TBC)

        # BiLSTM x2
        xin = seq            # the layer input: conv7 carried its abs-max for layer 0, the BiLSTM output of layer 0 carries its own
        lstm = []
        proj = conv.gemm(T * B, 512, 4 * HID)             # one direction's input projection: all steps of the layer in one GEMM
        for layer in (0, 1):
            gates = Act.empty((T, B), 2 * 4 * HID, dev)
            whf, whr = P[f"lstm.weight_hh_l{layer}"], P[f"lstm.weight_hh_l{layer}_reverse"]

            pf, pb, split = ops.lstm_packs(whf, whr)               # W_hh in per-lane MFMA fragment order, both directions, fwd + bwd forms
            for d, suf in enumerate(("", "_reverse")):
                b_ih, b_hh = P[f"lstm.bias_ih_l{layer}{suf}"], P[f"lstm.bias_hh_l{layer}{suf}"]
                bias = ops.weight_cached("lstm_bias_sum", b_ih, lambda b_ih=b_ih, b_hh=b_hh: (b_ih + b_hh).detach(), also=(b_hh,))
                proj.fwd(xin, P[f"lstm.weight_ih_l{layer}{suf}"], Act(gates.t[:, :, d * 4 * HID:], C=4 * HID), bias=bias)
            cst = Act.empty((T, B), 2 * HID, dev)
            # the layer output's abs-max: the next layer's projections / the Linear GEMM and, in the backward, the weight gradients
            # that read y take it from here — left by the one-launch layer kernel itself, else one pass
            y = Act.empty((T, B), 2 * HID, dev, slot)
            if not ops.lstm_layer_fwd_any(gates.t, cst.t, y.t, pf, split, T, B, y_amax=y.amax):
                y.amax = ops.absmax(y.t, y.ld, T * B, y.C) if slot.on else None
            lstm.append({"x": xin, "gates": gates, "c": cst, "y": y, "pb": pb, "split": split})
            xin = y
        # Linear + log_softmax (vocab padded to a multiple of 32 columns; pad columns stay 0)
        vp = self.vpad
        logits = torch.zeros(T * B, vp, device=dev)
        conv.gemm(T * B, 512, self.vocab).fwd(xin, P["linear.weight"], Act(logits, C=self.vocab), bias=P["linear.bias"])
        lp = torch.zeros(T * B, vp, device=dev)
        ops.log_softmax_fwd(logits, vp, lp, vp, T * B, self.vocab)
        out = lp.view(T, B, vp)[:, :, :self.vocab]
        if need_grad:
            # (dims: each layer's input plane under the key tests/decisions.py reads; the backward reads the records)
            dims = {"conv1": (H, W), **{name: (cv.H, cv.W) for name, cv in convs.items()}}
            ctx.update(acts=acts, convs=convs, dims=dims, lstm=lstm, lp=lp, T=T, conv1_params=conv1)
        return out, ctx

    # ------------------------------------------------------------------ backward
    def backward(self, ctx, dlp, nan_scrub, need_dx, param_grads=True):
        """dlp: gradient w.r.t. the returned log-probs [T,B,vocab].  Returns dx [B,1,H,W] or None."""
        fs = ensure_flat(self.m)
        fs.attach_grads()
        P = dict(self.m.named_parameters())
        G = {n: p.grad for n, p in P.items()}
        dev = dlp.device
        full = None
        if ctx.get("grad_group", -1) >= 0 and len(ctx["parts"]) > 1:
            # only ONE replica group receives a gradient (CRNN.forward(backward_group=g) detached the others): run the whole
            # backward on that group's samples.  Batch-major activations are row slices; the [T][B][..] sequence buffers are copied.
            full = (ctx["B"], ctx["x"])
            ctx, dlp = self._group_slice(ctx, dlp)
        B, H, W, T = ctx["B"], ctx["H"], ctx["W"], ctx["T"]
        acts, convs = ctx["acts"], ctx["convs"]
        vp, V = self.vpad, self.vocab
        c = self.cp
        TB = T * B
        side = ops.SideStream.of(self, dev)

        g = dlp.contiguous().view(TB, V)
        dlogits = Act.empty(TB, vp, dev)
        ops.log_softmax_bwd(g, V, ctx["lp"], vp, dlogits.t, vp, TB, V, vp, nan_scrub)
        slot = ops.amax_pool(dev)                                 # abs-max slots of this pass (None: the fp16 split is off)
        dlogits.amax = ops.absmax(dlogits.t, vp, TB, vp) if slot.on else None      # the split-fp16 GEMMs below want their operands' abs-max

        # Linear
        y1 = ctx["lstm"][1]["y"]
        if param_grads:
            def linear_grads():
                dwl = torch.empty(vp, 512, device=dev)
                conv.gemm(TB, 512, vp).wgrad(dlogits, y1, dwl)
                G["linear.weight"].add_(dwl[:V])
                dbl = torch.empty(vp, device=dev)
                ops.colsum(dlogits.t, vp, TB, vp, dbl)
                G["linear.bias"].add_(dbl[:V])
            side.run(linear_grads, dlogits.t)
        wlin = P["linear.weight"]

        def padded_T():
            wpad = torch.zeros(vp, 512, device=dev)
            wpad[:V].copy_(wlin)
            out = torch.empty(512, vp, device=dev)
            ops.transpose2d(wpad, out, vp, 512)
            return out
        wlT = ops.weight_cached(("padT", vp), wlin, padded_T)
        dy = Act.empty((T, B), 512, dev)
        conv.gemm(TB, vp, 512).fwd(dlogits, wlT, dy, w_src=(("padT", vp), wlin))

        # BiLSTM layers, top first
        proj = conv.gemm(TB, 512, 4 * HID)                 # one direction's input projection (its weight gradient)
        for layer in (1, 0):
            s = ctx["lstm"][layer]
            yl, xin = s["y"], s["x"]
            dc = None if s["split"] == "seq" else torch.empty(B, 2 * HID, device=dev)    # the one-launch kernels keep dc in registers
            # ONE abs-max of the gate gradients serves the four weight-gradient GEMMs and the input-gradient GEMM of the layer (a bound
            # over both directions and all steps scales every slice of the tensor): from the one-launch kernel, else one pass
            dgates = Act(s["gates"].t, amax=slot())                # the gate buffer: the layer's backward overwrites it with the gate gradients
            if not ops.lstm_layer_bwd_any(dgates.t, s["c"].t, dy.t, s["pb"], s["split"], dc, T, B, g_amax=dgates.amax):
                dgates.amax = ops.absmax(dgates.t, dgates.ld, TB, dgates.C) if slot.on else None
            if param_grads:
                def lstm_grads(layer=layer, dgates=dgates, xin=xin, yl=yl):
                    for d, suf in enumerate(("", "_reverse")):
                        dg = Act(dgates.t[:, :, d * 4 * HID:], C=4 * HID, amax=dgates.amax)
                        proj.wgrad(dg, xin, G[f"lstm.weight_ih_l{layer}{suf}"], accumulate=True)
                        db = torch.empty(4 * HID, device=dev)                  # b_ih and b_hh enter the gates as a sum: one column
                        ops.colsum(dg.t, dg.ld, TB, dg.C, db)                  # sum (a full pass over the gate gradients) serves both
                        G[f"lstm.bias_ih_l{layer}{suf}"].add_(db)
                        G[f"lstm.bias_hh_l{layer}{suf}"].add_(db)
                        if T > 1:
                            if d == 0:
                                pg, qh = dgates.rows(1, T - 1).cols(0, 4 * HID), yl.rows(0, T - 1).cols(0, HID)
                            else:
                                pg, qh = dgates.rows(0, T - 1).cols(4 * HID, 4 * HID), yl.rows(1, T - 1).cols(HID, HID)
                            conv.gemm((T - 1) * B, HID, 4 * HID).wgrad(pg, qh, G[f"lstm.weight_hh_l{layer}{suf}"], accumulate=True)
                side.run(lstm_grads)
            wf, wr = P[f"lstm.weight_ih_l{layer}"], P[f"lstm.weight_ih_l{layer}_reverse"]

            def cat_T(wf=wf, wr=wr):
                wcat = torch.cat((wf, wr), 0)                                                            # [2048][512]
                out = torch.empty(512, 8 * HID, device=dev)
                ops.transpose2d(wcat, out, 8 * HID, 512)
                return out
            wT = ops.weight_cached("catT", wf, cat_T, also=(wr,))
            # (planes of the concatenated filter: cached with BOTH directions' weights)
            if layer == 1:
                dy = Act.empty((T, B), 512, dev)
                conv.gemm(TB, 8 * HID, 512).fwd(dgates, wT, dy, w_src=("catT", wf, (wr,)))
            else:
                # rows (t,b) -> output row b*T + t : the gradient of conv7's output in its own [B,1,T,512] order
                dseq = Act.empty((B, T), 512, dev, slot)
                conv.Conv(T, 1, B, 8 * HID, 512, 1, 1).fwd(dgates, wT, dseq, w_src=("catT", wf, (wr,)), out_mode=ops.OUT_TBC)

        # conv7 (2x2, pad 0) backward
        c7, p6 = convs["conv7"], acts["p6"]
        if param_grads:
            def conv7_grads():
                ops.colsum(dseq.t, dseq.ld, B * T, 512, G[c + "conv7.bias"], accumulate=True)
                c7.wgrad(dseq, p6, G[c + "conv7.weight"], accumulate=True)
            side.run(conv7_grads, dseq.t)
        dp6 = Act.empty(B * c7.H * c7.W, 512, dev)
        c7.dgrad(dseq, P[c + "conv7.weight"], dp6)
        # pool (2,1) backward -> grad of a6 (ReLU handled by bn_bwd's mask)
        h, w = convs["conv6"].H, convs["conv6"].W            # (conv5 works on the same plane)
        da = None
        if not FUSE_POOL_BWD:
            da = Act.empty(B * h * w, 512, dev)
            ops.maxpool_bwd(acts["a6"].t, 512, dp6.t, dp6.ld, da.t, da.ld, B, h, w, 512, 2, 1, relu_mask=False)
        for name, bn, src in (("conv6", "batchnorm2", "a5"), ("conv5", "batchnorm1", "p4")):
            cv = convs[name]
            dy_ = Act.empty(B * h * w, 512, dev, slot)
            # da None: conv6's output went through the (2,1) pool only, whose backward rides in the two passes of BatchNorm2's (qea_bn_bwd_pool)
            batchnorm.backward(acts["bn" + name[-1]], da, dy_, P[c + bn + ".weight"], G[c + bn + ".weight"] if param_grads else None,
                               G[c + bn + ".bias"] if param_grads else None, pool=(dp6, 1) if da is None else None)
            if param_grads:
                def bn_conv_grads(dy_=dy_, name=name, src=src, cv=cv):
                    # (the bias gradient = column sums of dy rides with the weight gradient's staging waves where the kernel has it)
                    cv.wgrad(dy_, acts[src], G[c + name + ".weight"], accumulate=True, dbias=G[c + name + ".bias"])
                side.run(bn_conv_grads, dy_.t)
            da = Act.empty(B * h * w, cv.Cin, dev)          # (no slot: the pool backward behind it reads it, no GEMM)
            cv.dgrad(dy_, P[c + name + ".weight"], da)
        # da = grad of p4 [B,4,W/4,256]
        # conv4 (+ReLU, pool (2,1)), conv3 (+ReLU), conv2 (+ReLU, pool (2,2))
        dcur = da
        for name, cin, cout, relu, pool in reversed(CONVS):
            cv = convs[name]
            h, w = cv.H, cv.W
            M = B * h * w
            a = acts["a" + name[-1]]
            if pool:
                dyc = Act.empty(M, cout, dev, slot)
                ops.maxpool_bwd(a.t, a.ld, dcur.t, dcur.ld, dyc.t, dyc.ld, B, h, w, cout, pool[0], pool[1], relu_mask=True, amax=dyc.amax)
            else:
                dyc = dcur                                  # already masked by the producer's epilogue (which also left its abs-max)
            src = {"conv4": "a3", "conv3": "p2", "conv2": "p1"}[name]
            if param_grads:
                def conv_grads(dyc=dyc, name=name, src=src, cv=cv):
                    cv.wgrad(dyc, acts[src], G[c + name + ".weight"], accumulate=True, dbias=G[c + name + ".bias"])
                side.run(conv_grads, dyc.t)
            # conv4's input a3 is a bare ReLU output (no pool in between): fuse its mask here, and its input gradient IS conv3's output
            # gradient, so it carries a slot
            dcur = Act.empty(M, cin, dev, slot if name == "conv4" else None)
            cv.dgrad(dyc, P[c + name + ".weight"], dcur, mask=acts["a3"] if name == "conv4" else None)
        # dcur = grad of p1 [B,16,W/2,64]; conv1
        dx = None
        if FUSE_C1_BWD and H % 2 == 0 and W % 8 == 0 and (param_grads or need_dx):
            # conv1 -> ReLU -> pool backward from the pooled gradient and the 1-channel input: the activation is rebuilt (nine multiply-adds
            # per element), neither it nor its 2.1 GB gradient is read or written (dcur is overwritten with its masked values)
            if need_dx:
                dx = torch.empty(B, 1, H, W, device=dev)
            ops.conv_c1_pool_bwd(ctx["x"], P[c + "conv1.weight"], P[c + "conv1.bias"], dcur.t, dcur.ld, G[c + "conv1.weight"] if param_grads else None,
                                 G[c + "conv1.bias"] if param_grads else None, dx, B, H, W, 64, accumulate=True)
        else:
            a1 = acts["a1"].t if acts["a1"] is not None else None
            if a1 is None:                                  # (not kept by the forward: rebuild it)
                a1 = torch.empty(B * H * W, 64, device=dev)
                ops.conv_c1_fwd(ctx["x"], P[c + "conv1.weight"], P[c + "conv1.bias"], a1, 64, B, H, W, 64, relu=True)
            dy1 = torch.empty(B * H * W, 64, device=dev)
            ops.maxpool_bwd(a1, 64, dcur.t, dcur.ld, dy1, 64, B, H, W, 64, 2, 2, relu_mask=True)
            if param_grads:
                side.run(lambda: ops.conv_c1_wgrad(ctx["x"], dy1, 64, G[c + "conv1.weight"], G[c + "conv1.bias"], B, H, W, 64, accumulate=True),
                         dy1)
            if need_dx:
                dx = torch.empty(B, 1, H, W, device=dev)
                ops.conv_c1_dgrad(dy1, 64, P[c + "conv1.weight"], dx, B, H, W, 64)
        side.join()
        if full is not None and dx is not None:
            dxf = torch.zeros(full[0], 1, H, W, device=dev)
            dxf[ctx["_b0"]:ctx["_b0"] + B].copy_(dx)
            dx = dxf
        return dx

    @staticmethod
    def _group_slice(ctx, dlp):
        """The saved context and the output gradient restricted to replica group g = ctx["grad_group"].  Every slice and copy keeps its
        tensor's abs-max slot (the bound of the whole batch bounds the group)."""
        g, B = ctx["grad_group"], ctx["B"]
        b0, k = ctx["parts"][g]
        T = ctx["T"]
        sub = dict(ctx)
        sub.update(B=k, parts=[(0, k)], grad_group=-1, _b0=b0, x=ctx["x"][b0:b0 + k])
        acts = {}
        for name, a in ctx["acts"].items():
            if a is None:
                acts[name] = None
            elif isinstance(a, batchnorm.Stage):
                acts[name] = a.restricted(b0, k)
            else:
                per = a.nrows // B                                       # pixels per sample at this layer
                acts[name] = a.rows(b0 * per, k * per)
        sub["acts"] = acts
        sub["convs"] = {name: cv.with_batch(k) for name, cv in ctx["convs"].items()}
        sub["lstm"] = [{key: (Act(v.t[:, b0:b0 + k].contiguous(), amax=v.amax) if isinstance(v, Act) else v) for key, v in s.items()}
                       for s in ctx["lstm"]]
        lp = ctx["lp"]
        sub["lp"] = lp.view(T, B, -1)[:, b0:b0 + k].contiguous().view(T * k, -1)
        return sub, dlp[:, b0:b0 + k].contiguous()
