"""The 3x3 kernels leave out the (tile row, kh) groups that multiply a padding row, and do not stage such a row.  A padding row must
then count exactly as a stored row of zeros does: the same image embedded in a taller all-zero image, whose tiles are interior tiles
that execute every group, gives the same bits.  With small-integer operands every product and every partial sum is exact in fp32, so a
group dropped wrongly (or multiplied twice) changes an integer: convolution and weight gradient must equal the fp64 reference exactly."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CONV_SHAPES = [
    # (H, W, Cin, Cout)
    (4, 32, 64, 128),     # top and bottom padding in one tile
    (8, 32, 128, 128),    # a top tile and a bottom tile
    (8, 32, 64, 64),      # two wave rows per tile: the flags differ per wave
    (12, 32, 64, 128),    # with an interior tile
]


def _conv(x, w, variant=None):
    """3x3 pad-1 convolution of x [B,H,W,Cin] with w [Cout,3,3,Cin] on the default route; returns y [B,H,W,Cout]."""
    from qea import ops
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    kws = dict(B=B, H=H, W=W, Cin=Cin, OH=H, OW=W, N=Cout, KH=3, KW=3, pad=(1, 1), ldx=Cin, ldy=Cout)
    if variant == "stats":
        got = ops.conv_igemm(x, w, y, want_stats=True, **kws)
        assert got is not None, "the statistics epilogue runs on this shape"
    elif variant == "pool":
        assert ops.conv_can_pool(B=B, H=H, W=W, Cin=Cin, N=Cout, kw=1, ldx=Cin, ldy=Cout)
        pooled = torch.empty(B, H // 2, W, Cout, device="cuda")
        ops.conv_igemm(x, w, y, pool=(pooled, Cout, 1, None), **kws)
        torch.cuda.synchronize()
        assert torch.equal(pooled, torch.maximum(y[:, 0::2], y[:, 1::2]))
    else:
        ops.conv_igemm(x, w, y, **kws)
    torch.cuda.synchronize()
    return y


def _embed(x, Ht, Wt, top):
    """x [B,H,W,C] at rows top.., columns 0.. of an all-zero [B,Ht,Wt,C] image"""
    B, H, W, Cc = x.shape
    big = torch.zeros(B, Ht, Wt, Cc, device=x.device)
    big[:, top:top + H, :W] = x
    return big


def _operands(B, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).cuda()
    return x, w


@pytest.mark.parametrize("H,W,Cin,Cout,variant", [s + (None,) for s in CONV_SHAPES] + [(4, 32, 64, 128, "stats"), (4, 32, 64, 128, "pool")])
def test_padding_row_equals_stored_zero_row(H, W, Cin, Cout, variant):
    x, w = _operands(3, H, W, Cin, Cout, H * 100 + Cin + Cout)
    y = _conv(x, w, variant)
    yb = _conv(_embed(x, H + 8, W, 4), w, variant)
    assert torch.isfinite(y).all()
    assert torch.equal(yb[:, 4:4 + H], y)


@pytest.mark.parametrize("H,W,Cin,Cout", [(4, 16, 128, 256), (2, 8, 256, 512)])
def test_small_image_equals_embedded_image(H, W, Cin, Cout):
    """the small-image instances (several images per tile, no zero row in LDS) against the whole-width kernel on the same image with
    stored zero neighbours; B = 5 leaves the last tile partly empty"""
    x, w = _operands(5, H, W, Cin, Cout, H + Cin)
    y = _conv(x, w)
    yb = _conv(_embed(x, 12, 32, 4), w)
    assert torch.isfinite(y).all()
    assert torch.equal(yb[:, 4:4 + H, :W], y)


def _ints(shape, g):
    return torch.randint(-4, 5, shape, generator=g).float()


@pytest.mark.parametrize("H,W,Cin,Cout", CONV_SHAPES)
def test_integer_convolution_is_exact(H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H + W + Cin + Cout)
    x, w = _ints((3, H, W, Cin), g), _ints((Cout, 3, 3, Cin), g)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), padding=1).permute(0, 2, 3, 1)
    y = _conv(x.cuda(), w.cuda())
    assert torch.equal(y.cpu().double(), ref)


def _fuses_bias(B, H, W, R, Cc):
    """whether the planner sends this weight gradient to the producer / consumer nine-tap form"""
    from qea import _lib
    d = _lib.WgradDesc(p=None, q=None, dw=None, workspace=None, workspace_bytes=0, B=B, PH=H, PW=W, QH=H, QW=W, R=R, C=Cc, KH=3, KW=3,
                       pad_h=1, pad_w=1, stride_h=1, stride_w=1, ldp=R, ldq=Cc, accumulate=0, splits=0, tile=0)
    one = torch.ones(1, device="cuda")
    d.p_absmax = d.q_absmax = one.data_ptr()
    return bool(_lib.lib().qea_conv_wgrad_fuses_bias(C.byref(d)))


@pytest.mark.parametrize("R,Cc", [(64, 64), (128, 64)])
@pytest.mark.parametrize("H,W,with_bias", [(4, 32, False), (6, 32, False), (4, 64, False), (2, 32, False), (4, 32, True)])
def test_integer_weight_gradient_is_exact(H, W, with_bias, R, Cc):
    """dY and X in {-4 .. 4}: both fp16 planes are exact (the low plane is zero), every product is exact and every partial sum stays
    below 2^24 (B * H * W <= 3 * 12 * 64 terms of at most 16), so the result equals the fp64 weight gradient whatever the order."""
    from qea import ops
    B = 3
    if (H, W) == (2, 32) and not _fuses_bias(B, H, W, R, Cc):
        pytest.skip("the planner does not route 2-row images to the nine-tap producer / consumer kernel")
    g = torch.Generator().manual_seed(H * W + R)
    dy, x = _ints((B, H, W, R), g), _ints((B, H, W, Cc), g)
    wz = torch.zeros(R, Cc, 3, 3, dtype=torch.double, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2).double(), wz, padding=1).backward(dy.permute(0, 3, 1, 2).double())
    ref = wz.grad.permute(0, 2, 3, 1).contiguous()                # [R][kh][kw][Cc]
    dw = torch.full(ref.shape, float("nan"), device="cuda")
    db = torch.full((R,), float("nan"), device="cuda") if with_bias else None
    ops.conv_wgrad(dy.cuda(), x.cuda(), dw, B=B, PH=H, PW=W, QH=H, QW=W, R=R, Cc=Cc, KH=3, KW=3, pad=(1, 1), ldp=R, ldq=Cc, dbias=db)
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu().double(), ref)
    if with_bias:
        assert torch.equal(db.cpu().double(), dy.double().sum((0, 1, 2)))
