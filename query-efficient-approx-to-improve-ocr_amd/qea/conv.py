"""One convolution layer of the UNet / CRNN schedules, stated once for its forward, its input gradient and its weight gradient: the only
place the engines reach ops.conv_igemm, ops.conv_wgrad, ops.conv_can_pool, ops.flip_transposed and ops.transposed.
A Conv is the geometry of y[b,oh,ow,n] = sum x[b, oh*s+kh-pad, ow*s+kw-pad, c] * w[n,kh,kw,c] and nothing else (no tensors); the three
launches of a layer read it, so they cannot disagree:
  dgrad  = the same implicit GEMM on the flip-transposed filter: planes and channel counts swapped, pad -> K-1-pad (stride 1 only);
  wgrad  = dw[n][kh][kw][c] = sum dy[b,oh,ow][n] * x[b, oh*s+kh-pad, ow*s+kw-pad][c]: p = dy on (OH, OW), q = x on (H, W);
  a transposed convolution (stride = kernel, pad 0) is the adjoint of a Conv and holds that Conv's filter as it lies: its forward is
  scatter_adjoint, its input gradient the Conv's fwd, its weight gradient the Conv's wgrad(dy = the adjoint's input, x = its output gradient).
Operands are records (qea/act.py: tensor, channels, pixel stride, abs-max slot); every method refuses, before any launch, one whose
channels or rows are not the layer's, and unpacks the strides and slots at the ops boundary.
Calls go through the attributes of `ops` (tools/engine_schedule.py records by replacing them)."""
from . import ops


def _out_size(size, k, pad, stride):
    steps, rest = divmod(size + 2 * pad - k, stride)
    if steps < 0 or rest:
        raise ValueError(f"a filter of {k}, pad {pad}, stride {stride}, has no whole number of positions on {size} pixels")
    return steps + 1


class Conv:
    __slots__ = ("B", "H", "W", "Cin", "N", "KH", "KW", "pad", "stride", "OH", "OW")

    def __init__(self, B, H, W, Cin, N, KH, KW, pad=(0, 0), stride=(1, 1)):
        self.B, self.H, self.W, self.Cin, self.N, self.KH, self.KW, self.pad, self.stride = B, H, W, Cin, N, KH, KW, tuple(pad), tuple(stride)
        self.OH, self.OW = _out_size(H, KH, pad[0], stride[0]), _out_size(W, KW, pad[1], stride[1])

    def with_batch(self, B):
        """the same layer on B samples (the backward of one replica group)"""
        return Conv(B, self.H, self.W, self.Cin, self.N, self.KH, self.KW, self.pad, self.stride)

    def _check(self, on_input, on_output, pooled=None, kw=1):
        """refuse a record that is not [B*H*W][Cin] on the layer's input plane, [B*OH*OW][N] on its output plane ([../(2*kw)][N]: pooled)"""
        for a, C, pixels in ((on_input, self.Cin, self.H * self.W), (on_output, self.N, self.OH * self.OW), (pooled, self.N, (self.OH // 2) * (self.OW // kw))):
            if a is not None and (a.C != C or a.nrows != self.B * pixels):
                raise ValueError(f"an operand of [{a.nrows}][{a.C}] where this layer has [{self.B * pixels}][{C}]")

    def fwd(self, x, w, y, w_src=None, pool=None, **epilogue):
        """x [B*H*W][Cin] -> y [B*OH*OW][N] (rows as out_mode says) with the filter w [N][KH][KW][Cin].  w_src: only where w is a form the
        caller derived from model weights itself (ops.conv_igemm's w_src); a model weight is its own source.  pool = (pooled Act, kw): the
        2 x kw max-pool of y leaves with the epilogue (see can_pool).  epilogue: conv_igemm's."""
        self._check(x, y, *(pool or ()))
        return ops.conv_igemm(x.t, w, y.t, B=self.B, H=self.H, W=self.W, Cin=self.Cin, OH=self.OH, OW=self.OW, N=self.N, KH=self.KH, KW=self.KW,
                              pad=self.pad, stride=self.stride, ldx=x.ld, ldy=y.ld, x_amax=x.amax, y_amax=y.amax,
                              w_src=("fwd", w) if w_src is None else w_src,
                              pool=(pool[0].t, pool[0].ld, pool[1], pool[0].amax) if pool is not None else None, **epilogue)

    def dgrad(self, dy, w, dx, mask=None, **epilogue):
        """dy [B*OH*OW][N] -> dx [B*H*W][Cin] with the layer's own filter w (its flip-transposed form is derived and cached here).
        mask: the Act on the input plane whose sign masks dx (a ReLU behind it)."""
        if self.stride != (1, 1):
            raise ValueError(f"dgrad is the stride-1 form; this layer has stride {self.stride}")
        self._check(dx, dy)
        self._check(mask, None)                                # (the mask lies on dx's plane)
        wt = ops.flip_transposed(w, self.N, self.Cin, self.KH, self.KW)
        return ops.conv_igemm(dy.t, wt, dx.t, B=self.B, H=self.OH, W=self.OW, Cin=self.N, OH=self.H, OW=self.W, N=self.Cin, KH=self.KH, KW=self.KW,
                              pad=(self.KH - 1 - self.pad[0], self.KW - 1 - self.pad[1]), ldx=dy.ld, ldy=dx.ld, x_amax=dy.amax, y_amax=dx.amax,
                              w_src=("flipT", w), mask=mask.t if mask is not None else None, ldmask=mask.ld if mask is not None else 0, **epilogue)

    def wgrad(self, dy, x, dw, **kw):
        """dw [N][KH][KW][Cin] (+)= the layer's weight gradient from dy [B*OH*OW][N] and x [B*H*W][Cin].  kw: accumulate, dbias."""
        self._check(x, dy)
        ops.conv_wgrad(dy.t, x.t, dw, B=self.B, PH=self.OH, PW=self.OW, QH=self.H, QW=self.W, R=self.N, Cc=self.Cin, KH=self.KH, KW=self.KW,
                       pad=self.pad, stride=self.stride, ldp=dy.ld, ldq=x.ld, p_amax=dy.amax, q_amax=x.amax, **kw)

    def scatter_adjoint(self, x, w, y, **epilogue):
        """The adjoint map x [B*OH*OW][N] -> y [B*H*W][Cin] with the filter w as it lies: every input pixel writes its own KH x KW output
        pixels, so it is one GEMM on w's transpose [N][KH*KW*Cin] whose epilogue scatters (OUT_CONVT, which knows the 2x2 window)."""
        if self.stride != (self.KH, self.KW) or self.pad != (0, 0) or (self.KH, self.KW) != (2, 2):
            raise ValueError(f"scatter_adjoint needs stride = kernel = (2, 2) and pad 0, got kernel {(self.KH, self.KW)}, stride {self.stride}, "
                             f"pad {self.pad}")
        self._check(y, x)
        K = self.KH * self.KW * self.Cin
        wT = ops.transposed(w, self.N, K)
        return ops.conv_igemm(x.t, wT, y.t, B=self.B, H=self.OH, W=self.OW, Cin=self.N, OH=self.OH, OW=self.OW, N=K, KH=1, KW=1,
                              ldx=x.ld, ldy=y.ld, x_amax=x.amax, y_amax=y.amax, out_mode=ops.OUT_CONVT, w_src=("T", w), **epilogue)

    def can_pool(self, kw, x, y):
        """can this layer's fwd(x, ., y) carry the 2 x kw max-pool behind it in its epilogue (fwd's pool=)?"""
        return (self.KH, self.KW, self.pad, self.stride) == (3, 3, (1, 1), (1, 1)) and \
            ops.conv_can_pool(B=self.B, H=self.H, W=self.W, Cin=self.Cin, N=self.N, kw=kw, ldx=x.ld, ldy=y.ld)


def gemm(M, K, N):
    """y [M][N] = x [M][K] . w[N][K]^T as a layer: one image of one row of M pixels, 1x1 filter"""
    return Conv(1, 1, M, K, N, 1, 1)
