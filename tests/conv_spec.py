"""The statement of qea_conv_igemm and qea_conv_wgrad (include/qea_hip.h) in fp64, in plain loops, with every descriptor field read
the way the header words it: operands through their pixel stride and the base offset of their channel slice, pad / stride / filter
extent separately for h and w, the epilogue in the header's order, the three output row maps, OH and OW as inputs.

    conv:   y[row(b,oh,ow), n] = epilogue( sum_{kh,kw,c} x[b, oh*sh+kh-ph, ow*sw+kw-pw, c] * w[n,kh,kw,c] )      taps outside the image are 0
            epilogue: v = acc*scale[n] + bias[n];  ReLU;  v = mask[row,n] > 0 ? v : 0;  v += y_prev  (accumulate)
            rows:  NHWC m*ldy;  TBC (ow*B+b)*ldy;  CONVT n = (a,bb,co) -> y[b, 2oh+a, 2ow+bb, co] with bias[co], mask at the same pixel
    wgrad:  dw[r][kh][kw][c] (+)= sum_{b,ph,pw} p[b,ph,pw][r] * q[b, ph*sh+kh-pad_h, pw*sw+kw-pad_w][c];   dbias[r] = sum p[.][r]

Written for reading, not for speed; imports nothing of the library it checks.  tests/test_conv_spec_cpu.py holds both functions to
torch (conv2d, conv_transpose2d, autograd) in float64 and shows that every named way of getting a field wrong (PERTURBATIONS) moves
at least one case of the tables below far beyond the gates; tests/test_conv_descriptor_gpu.py holds every kernel family to them.

The operands of a case live in NaN-filled allocations (Operand): guard bands of GUARD_ROWS rows in front and behind, NaN and inf
between the channel slices, so an access outside a slice shows up in the result (a neighbour times a zero weight included) while it
never leaves the allocation.  The case tables and builders are shared by the two test files: the CPU tests speak about the very
data the device sees."""
import functools
import types

import numpy as np

OUT_NHWC, OUT_TBC, OUT_CONVT = 0, 1, 2
GUARD_ROWS = 256
CONV_GATE, WGRAD_GATE = 2e-6, 3e-5       # the project's gates (tests/test_operand_scale_gpu.py), times max |spec| of the case
BKP = 32                                 # pixels per stage of the weight-gradient gather; split chunks are rounded to it (csrc/conv_wgrad.hip)
MASK_VALUES = np.array([-1.0, -0.0, 0.0, 2.0 ** -126, 1.0, np.nan], dtype=np.float32)


class Operand:
    """[rows][width] fp32 values at buf[base + r*ld + c] of a flat NaN-filled allocation: GUARD_ROWS rows of ld floats in front and
    behind, `off` floats of each row before the slice and ld - off - width behind it (NaN, every third one inf)."""

    def __init__(self, rows, width, ld=None, off=0):
        ld = width if ld is None else ld
        assert off % 4 == 0 and off + width <= ld
        self.rows, self.width, self.ld, self.off = rows, width, ld, off
        self.guard = GUARD_ROWS * ld                              # floats in front of row 0
        self.base = self.guard + off
        self.buf = np.full((2 * GUARD_ROWS + rows) * ld, np.nan, dtype=np.float32)
        gap = np.ones(ld, dtype=bool)
        gap[off:off + width] = False
        body = self.buf[self.guard:self.guard + rows * ld].reshape(rows, ld)
        cols = np.nonzero(gap)[0][::3]
        body[:, cols] = np.inf

    def view(self):
        """the slice as a writable [rows][width] view of the allocation"""
        return self.buf[self.guard:self.guard + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.off:self.off + self.width]

    def set(self, data):
        self.view()[...] = np.asarray(data, dtype=np.float32).reshape(self.rows, self.width)
        return self

    def inside(self):
        """flat bool: the floats of the slice"""
        m = np.zeros(self.buf.shape, dtype=bool)
        m[self.guard:self.guard + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.off:self.off + self.width] = True
        return m


# ----------------------------------------------------------------------------- the statements
def conv_igemm_spec(d, x_buf, w, scale, bias, mask_buf, y_prev, perturb=None):
    """d: the descriptor fields B H W Cin OH OW N KH KW pad_h pad_w stride_h stride_w ldx ldy ldmask relu accumulate out_mode, and for
    each strided operand the floats in front of its row 0 (x_guard, y_guard, mask_guard) and the offset of its slice in a row (x_off,
    y_off, mask_off).  x_buf, mask_buf, y_prev: the flat allocations; w [N][KH][KW][Cin]; scale [N]; bias [N] ([N/4] for CONVT); any of
    scale / bias / mask_buf may be None.  -> (y: y_prev in fp64 with every stored value in place, written: flat bool of the stores).
    perturb: one of PERTURBATIONS["conv"] — the same statement with that one field misread."""
    assert perturb is None or perturb in PERTURBATIONS["conv"], perturb
    f8 = np.float64
    x_buf, w = np.asarray(x_buf, dtype=f8), np.asarray(w, dtype=f8)
    y = np.array(y_prev, dtype=f8)
    written = np.zeros(y.shape, dtype=bool)
    ph, pw, sh, sw, ldx = d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.ldx
    x_base, y_base = d.x_guard + d.x_off, d.y_guard + d.y_off
    mask_base, ldmask = (d.mask_guard + d.mask_off, d.ldmask) if mask_buf is not None else (0, 0)
    if perturb == "pad_swapped":
        ph, pw = pw, ph
    if perturb == "stride_swapped":
        sh, sw = sw, sh
    if perturb == "base_ignored":
        x_base = d.x_guard
    if perturb == "ld_as_channels":
        ldx = d.Cin
    if perturb == "mask_ldy":
        ldmask = d.ldy
    co_n = d.N // 4
    for b in range(d.B):
        for oh in range(d.OH):
            for ow in range(d.OW):
                acc = np.zeros(d.N, dtype=f8)
                for kh in range(d.KH):
                    for kw in range(d.KW):
                        if perturb == "last_tap_dropped" and (kh, kw) == (d.KH - 1, d.KW - 1):
                            continue
                        th, tw = (kw, kh) if perturb == "taps_swapped" else (kh, kw)
                        ih, iw = oh * sh + th - ph, ow * sw + tw - pw
                        if not (0 <= ih < d.H and 0 <= iw < d.W):
                            continue
                        at = x_base + ((b * d.H + ih) * d.W + iw) * ldx
                        acc += w[:, kh, kw, :] @ x_buf[at:at + d.Cin]
                m = (b * d.OH + oh) * d.OW + ow
                for n in range(d.N):
                    v = acc[n]
                    if d.out_mode == OUT_CONVT:
                        ab, co = divmod(n, co_n)
                        a, bb = (ab & 1, ab >> 1) if perturb == "convt_ab_transposed" else (ab >> 1, ab & 1)
                        row, col = (b * 2 * d.OH + 2 * oh + a) * 2 * d.OW + 2 * ow + bb, co
                        nb = n if perturb == "convt_bias_n" else co
                    else:
                        row = ow * d.B + b if (d.out_mode == OUT_TBC and perturb != "tbc_as_nhwc") else m
                        col = nb = n
                    if scale is not None:
                        v = v * f8(scale[n])
                    if bias is not None:
                        v = v + (f8(bias[nb]) if nb < len(bias) else np.nan)
                    o = y_base + row * d.ldy + col
                    if perturb == "accumulate_before_relu" and d.accumulate:
                        v = v + y[o]
                    if d.relu:
                        v = max(v, 0.0) if v == v else v
                    if mask_buf is not None:
                        v = v if mask_buf[mask_base + row * ldmask + col] > 0 else 0.0
                    if d.accumulate and perturb != "accumulate_before_relu":
                        v = v + y[o]
                    y[o] = v
                    written[o] = True
    return y, written


def conv_written(d, size):
    """flat bool [size]: the `written` of conv_igemm_spec(d, ...) from the three row maps alone, without the arithmetic, for a caller
    that needs the stored region of a launch at sizes the loops above take minutes for (tests/slot_audit.py).  Reads B OH OW N ldy
    out_mode y_guard y_off; tests/test_slot_audit_cpu.py holds it to conv_igemm_spec's own mask on every case of CONV_CASES."""
    b, oh, ow = np.meshgrid(np.arange(d.B), np.arange(d.OH), np.arange(d.OW), indexing="ij")
    if d.out_mode == OUT_CONVT:
        co_n = d.N // 4
        a, bb = np.arange(2).reshape(2, 1, 1, 1, 1), np.arange(2).reshape(1, 2, 1, 1, 1)
        row = ((b * 2 * d.OH + 2 * oh + a) * 2 * d.OW + 2 * ow + bb).reshape(-1)
        cols = co_n
    else:
        row = (ow * d.B + b if d.out_mode == OUT_TBC else (b * d.OH + oh) * d.OW + ow).reshape(-1)
        cols = d.N
    written = np.zeros(size, dtype=bool)
    written[(d.y_guard + d.y_off + row[:, None] * d.ldy + np.arange(cols)[None, :]).reshape(-1)] = True
    return written


def _walked_pixel(m, PH, PW, skip_image_carry):
    """(image, row, column) of pixel m as the gather reaches it: thread m % BKP starts at pixel m % BKP and advances BKP pixels per
    stage as eq images + er rows + dr columns with two carries (WgGather::fetch).  skip_image_carry: the eq term left out."""
    dq = BKP // PW
    dr, eq, er = BKP - dq * PW, dq // PH, dq % PH
    g = m % BKP
    b, rem = divmod(g, PH * PW)
    ph_, pw_ = divmod(rem, PW)
    for _ in range(m // BKP):
        pw_, ph_ = pw_ + dr, ph_ + er
        b += 0 if skip_image_carry else eq
        if pw_ >= PW:
            pw_, ph_ = pw_ - PW, ph_ + 1
        if ph_ >= PH:
            ph_, b = ph_ - PH, b + 1
    return b, ph_, pw_


def conv_wgrad_spec(d, p_buf, q_buf, dw_prev, perturb=None):
    """d: B PH PW QH QW R C KH KW pad_h pad_w stride_h stride_w ldp ldq accumulate splits, p_guard / p_off / q_guard / q_off as in
    conv_igemm_spec.  p_buf, q_buf: the flat allocations; dw_prev [R][KH][KW][C] (read under accumulate only).
    -> (dw [R][KH][KW][C], dbias [R] = the column sums of p), fp64.  perturb: one of PERTURBATIONS["wgrad"]."""
    assert perturb is None or perturb in PERTURBATIONS["wgrad"], perturb
    f8 = np.float64
    p_buf, q_buf = np.asarray(p_buf, dtype=f8), np.asarray(q_buf, dtype=f8)
    ph_, pw_, sh, sw, ldp, ldq = d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.ldp, d.ldq
    p_base, q_base = d.p_guard + d.p_off, d.q_guard + d.q_off
    if perturb == "pad_swapped":
        ph_, pw_ = pw_, ph_
    if perturb == "stride_swapped":
        sh, sw = sw, sh
    if perturb == "base_ignored":
        p_base, q_base = d.p_guard, d.q_guard
    if perturb == "ld_as_channels":
        ldp, ldq = d.R, d.C
    M = d.B * d.PH * d.PW
    per_split = -(-M // max(d.splits, 1))
    chunk = -(-per_split // BKP) * BKP                            # pixels per split, rounded up to whole stages
    dw = np.zeros((d.R, d.KH, d.KW, d.C), dtype=f8)
    dbias = np.zeros(d.R, dtype=f8)
    for m in range(M):
        if perturb == "split_first_row_dropped" and m >= chunk and m % chunk == 0:
            continue
        b, rem = divmod(m, d.PH * d.PW)
        y_, x_ = divmod(rem, d.PW)
        pv = p_buf[p_base + m * ldp:p_base + m * ldp + d.R]
        dbias += pv
        if perturb == "image_carry_skipped":
            b, y_, x_ = _walked_pixel(m, d.PH, d.PW, True)
        for kh in range(d.KH):
            for kw in range(d.KW):
                if perturb == "last_tap_dropped" and (kh, kw) == (d.KH - 1, d.KW - 1):
                    continue
                th, tw = (kw, kh) if perturb == "taps_swapped" else (kh, kw)
                qh, qw = y_ * sh + th - ph_, x_ * sw + tw - pw_
                if not (0 <= qh < d.QH and 0 <= qw < d.QW):
                    continue
                at = q_base + ((b * d.QH + qh) * d.QW + qw) * ldq
                qv = q_buf[at:at + d.C]
                if len(qv) < d.C:                                  # (a misread descriptor walked off the allocation)
                    qv = np.full(d.C, np.nan)
                with np.errstate(invalid="ignore"):                # (inf - inf of a perturbed read)
                    dw[:, kh, kw, :] += np.outer(pv, qv)
    if d.accumulate:
        dw += np.asarray(dw_prev, dtype=f8)
    return dw, dbias


PERTURBATIONS = {
    "conv": ("pad_swapped", "stride_swapped", "taps_swapped", "last_tap_dropped", "base_ignored", "ld_as_channels", "tbc_as_nhwc",
             "convt_ab_transposed", "convt_bias_n", "mask_ldy", "accumulate_before_relu"),
    "wgrad": ("pad_swapped", "stride_swapped", "taps_swapped", "last_tap_dropped", "base_ignored", "ld_as_channels",
              "split_first_row_dropped", "image_carry_skipped"),
}


def moved(a, b):
    """largest |a - b|; a value that is non-finite on one side only (or NaN against inf) counts as infinitely far"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        diff = np.where(same, 0.0, np.abs(a - b))
    diff[~same & ~np.isfinite(diff)] = np.inf
    return float(diff.max()) if diff.size else 0.0


# ----------------------------------------------------------------------------- conv cases
# geometry of a case; strided operands as (ld, offset of the slice); Cin = 64 unless given.  The shapes are the smallest that are
# ragged against every tile edge (BM 128 / 256, BN 32 .. 256).
_SLICES = dict(B=3, H=5, W=7, OH=5, OW=7, N=40, KH=3, KW=3, pad=(1, 1), stride=(1, 1), x=(128, 32), y=(56, 8))
EPILOGUE_SWITCHES = ("scale", "bias", "relu", "mask", "accumulate")
CONV_CASES = {
    "slices": dict(_SLICES),                                                                  # ldx / ldy on every tile
    **{f"epilogue-{s}": dict(_SLICES, mask=(48, 4) if s == "mask" else None, **{"on": (s,)}) for s in EPILOGUE_SWITCHES},
    "epilogue-all": dict(_SLICES, mask=(48, 4), on=EPILOGUE_SWITCHES),                        # branch order
    "asym": dict(B=3, H=6, W=5, OH=3, OW=7, N=40, KH=2, KW=3, pad=(0, 2), stride=(2, 1), x=(64, 0), y=(40, 0)),   # h / w never swapped
    "s2-concat": dict(B=2, H=6, W=10, OH=3, OW=5, N=72, KH=2, KW=2, pad=(0, 0), stride=(2, 2), x=(128, 64), y=(72, 0)),   # convT input gradient
    "tbc-conv7": dict(B=5, H=2, W=9, OH=1, OW=8, N=40, KH=2, KW=2, pad=(0, 0), stride=(1, 1), x=(64, 0), y=(56, 8), out_mode=OUT_TBC),
    "tbc-1x1": dict(B=7, H=1, W=11, OH=1, OW=11, N=96, KH=1, KW=1, pad=(0, 0), stride=(1, 1), x=(64, 0), y=(96, 0), out_mode=OUT_TBC,
                    on=("bias",)),                                                            # LSTM projection form: B = T, W = Bt
    "convt": dict(B=3, H=3, W=5, OH=3, OW=5, N=4 * 24, KH=1, KW=1, pad=(0, 0), stride=(1, 1), x=(64, 0), y=(48, 24), out_mode=OUT_CONVT,
                  mask=(40, 8), on=("bias", "relu", "mask")),                                 # scatter + per-co bias + mask index
}

ConvCase = types.SimpleNamespace


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """-> namespace(d, x, w, scale, bias, mask, y: Operands or None; y holds y_prev under accumulate, NaN otherwise)"""
    c = CONV_CASES[name]
    on = c.get("on", ())
    Cin, mode = c.get("Cin", 64), c.get("out_mode", OUT_NHWC)
    rng = np.random.default_rng(sorted(CONV_CASES).index(name) + 1)
    B, H, W, OH, OW, N, KH, KW = (c[k] for k in ("B", "H", "W", "OH", "OW", "N", "KH", "KW"))
    M = B * OH * OW
    yrows, ycols = (4 * M, N // 4) if mode == OUT_CONVT else (M, N)
    x = Operand(B * H * W, Cin, *c["x"]).set(rng.standard_normal((B * H * W, Cin)))
    w = Operand(N, KH * KW * Cin).set(rng.standard_normal((N, KH * KW * Cin)) / (KH * KW * Cin) ** 0.5)
    scale = Operand(1, N).set(rng.random(N) + 0.5) if "scale" in on else None
    bias = Operand(1, ycols).set(rng.standard_normal(ycols)) if "bias" in on else None
    mask = Operand(yrows, ycols, *c["mask"]).set(rng.choice(MASK_VALUES, size=(yrows, ycols))) if "mask" in on else None
    y = Operand(yrows, ycols, *c["y"])
    if "accumulate" in on:
        y.set(rng.standard_normal((yrows, ycols)))
    d = types.SimpleNamespace(B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, N=N, KH=KH, KW=KW, pad_h=c["pad"][0], pad_w=c["pad"][1],
                              stride_h=c["stride"][0], stride_w=c["stride"][1], ldx=x.ld, ldy=y.ld, ldmask=mask.ld if mask else 0,
                              relu=int("relu" in on), accumulate=int("accumulate" in on), out_mode=mode,
                              x_guard=x.guard, x_off=x.off, y_guard=y.guard, y_off=y.off,
                              mask_guard=mask.guard if mask else 0, mask_off=mask.off if mask else 0)
    return ConvCase(name=name, d=d, x=x, w=w, scale=scale, bias=bias, mask=mask, y=y)


def conv_case_spec(name, perturb=None):
    """-> (y allocation in fp64 after the launch, written) of a case"""
    return _conv_case_spec(name, perturb)


@functools.lru_cache(maxsize=None)
def _conv_case_spec(name, perturb):
    c = conv_case(name)
    d = c.d
    return conv_igemm_spec(d, c.x.buf, c.w.view().reshape(d.N, d.KH, d.KW, d.Cin), c.scale.view()[0] if c.scale else None,
                           c.bias.view()[0] if c.bias else None, c.mask.buf if c.mask else None, c.y.buf, perturb)


# ----------------------------------------------------------------------------- wgrad cases
# p / q as (ld, offset); R = 44, C = 36 unless given
WGRAD_CASES = {
    "slices": dict(B=3, PH=5, PW=7, QH=5, QW=7, KH=3, KW=3, pad=(1, 1), stride=(1, 1), p=(52, 4), q=(72, 32)),           # ldp / ldq per tile
    "asym": dict(B=3, PH=3, PW=7, QH=6, QW=5, KH=2, KW=3, pad=(0, 2), stride=(2, 1), p=(52, 4), q=(72, 32)),            # h / w never swapped
    "convt": dict(B=2, PH=3, PW=5, QH=6, QW=10, KH=2, KW=2, pad=(0, 0), stride=(2, 2), R=68, p=(68, 0), q=(72, 36)),    # p = X, q = dY: a concat half
    "linear": dict(B=1, PH=1, PW=217, QH=1, QW=217, KH=1, KW=1, pad=(0, 0), stride=(1, 1), R=96, C=64, p=(128, 0), q=(96, 0)),   # LSTM / Linear form
    "tiny-image-3x3": dict(B=70, PH=2, PW=3, QH=2, QW=3, KH=3, KW=3, pad=(1, 1), stride=(1, 1), p=(52, 4), q=(72, 32)),  # PH*PW < one stage
    "tiny-image-1x1": dict(B=70, PH=1, PW=1, QH=1, QW=1, KH=1, KW=1, pad=(0, 0), stride=(1, 1), p=(52, 4), q=(72, 32)),
    # the pixel-tile kernels (fp32 halo, nine-tap): the smallest shapes they take
    **{f"slices-{rc}-w{w_}": dict(B=2, PH=8, PW=w_, QH=8, QW=w_, KH=3, KW=3, pad=(1, 1), stride=(1, 1), R=rc, C=rc, p=(rc + 12, 4), q=(rc + 64, 32))
       for rc in (32, 64) for w_ in (16, 32)},
    # (beyond the smallest: 24 pixel tiles, so that splits = 3 is what the nine-tap kernels really run)
    "slices-64-w32-b6": dict(B=6, PH=8, PW=32, QH=8, QW=32, KH=3, KW=3, pad=(1, 1), stride=(1, 1), R=64, C=64, p=(76, 4), q=(128, 32)),
}
GENERIC_WGRAD_CASES = ("slices", "asym", "convt", "linear", "tiny-image-3x3", "tiny-image-1x1")
PIXEL_TILE_WGRAD_CASES = tuple(k for k in WGRAD_CASES if k.startswith("slices-"))


@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """-> namespace(d (splits 1, accumulate 0: the tests set both), p, q, dw_prev, db_prev)"""
    c = WGRAD_CASES[name]
    rng = np.random.default_rng(100 + sorted(WGRAD_CASES).index(name))
    R, C_ = c.get("R", 44), c.get("C", 36)
    B, PH, PW, QH, QW, KH, KW = (c[k] for k in ("B", "PH", "PW", "QH", "QW", "KH", "KW"))
    p = Operand(B * PH * PW, R, *c["p"]).set(rng.standard_normal((B * PH * PW, R)))
    q = Operand(B * QH * QW, C_, *c["q"]).set(rng.standard_normal((B * QH * QW, C_)))
    dw_prev = (rng.standard_normal((R, KH, KW, C_)) * (B * PH * PW) ** 0.5).astype(np.float32)     # the size of the gradient itself
    db_prev = (rng.standard_normal(R) * (B * PH * PW) ** 0.5).astype(np.float32)
    d = types.SimpleNamespace(B=B, PH=PH, PW=PW, QH=QH, QW=QW, R=R, C=C_, KH=KH, KW=KW, pad_h=c["pad"][0], pad_w=c["pad"][1],
                              stride_h=c["stride"][0], stride_w=c["stride"][1], ldp=p.ld, ldq=q.ld, accumulate=0, splits=1,
                              p_guard=p.guard, p_off=p.off, q_guard=q.guard, q_off=q.off)
    return types.SimpleNamespace(name=name, d=d, p=p, q=q, dw_prev=dw_prev, db_prev=db_prev)


@functools.lru_cache(maxsize=None)
def wgrad_case_spec(name, perturb=None, splits=1):
    """-> (dw, dbias) of a case WITHOUT accumulate (the prior values are added by the caller: the sum is exact in fp64)"""
    c = wgrad_case(name)
    d = types.SimpleNamespace(**vars(c.d))
    d.splits = splits
    return conv_wgrad_spec(d, c.p.buf, c.q.buf, None, perturb)
