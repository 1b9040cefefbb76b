"""The two-way fp16 split across operand SCALES (csrc/common.h: qea_f16_scale / qea_split2_f16), through qea.ops.

Every other kernel test feeds unit-scale randn data and lets ops take the abs-max itself.  Here the operands are scaled by powers of
two (bit-for-bit homogeneity), the abs-max slots are supplied by the caller and loose (the engines' concat buffers share one slot),
one tensor mixes magnitudes 2^-8 ... 2^-30 apart (each region judged against ITS OWN maximum), operands or whole 32-row tiles are
zero, and a backward chain runs at the gradient magnitude of a mean-reduced loss at B = 2048 (1e-8).  All references are fp64 on the
CPU.  No gate has an absolute floor: a tolerance is either one of the project's gates (2e-6 conv, 3e-5 wgrad, 1e-4 LSTM backward)
times the REGION's max |ref|, or the bound that follows from the per-element contract of the split

    |x - (h + l) / s|  <=  max(SPLIT_REL * |x|, SPLIT_ABS * m),     m = the bound the scale was taken from,

computed per output in fp64 (tests/test_host_logic_cpu.py::test_f16_split_contract_in_numpy checks the two constants on the CPU).
Every test runs in the session's mode (split_f16, QEA_SPLIT=bf16, QEA_MFMA=f32): the properties hold in all three.  The worst
error / gate ratio of every family is printed (pytest -s) for the table in DESIGN.md §4."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lstm_spec
from helpers import SPLIT_ABS, SPLIT_REL     # the per-element contract of qea_split2_f16 (csrc/common.h)

pytestmark = pytest.mark.gpu

CONV_GATE, WGRAD_GATE, LSTM_GATE = 2e-6, 3e-5, 1e-4     # test_filter_scale_from_the_whole_parameter_buffer, _conv_case, test_lstm_layer_fwd_bwd

WORST = {}


def _check(family, err, gate):
    """err <= gate elementwise (broadcast), no floor: where the gate is 0 the error must be 0.  Prints max err / gate and keeps the worst per family for the summary printed at the end of the module."""
    err = torch.as_tensor(err, dtype=torch.float64)
    gate = torch.as_tensor(gate, dtype=torch.float64).expand_as(err)
    assert torch.isfinite(err).all(), family
    ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    worst = ratio.max().item() if ratio.numel() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print(f"operand-scale {family}: worst error / gate = {worst:.3g}")
    assert worst <= 1.0, (family, worst)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    from qea import ops
    print(f"\noperand-scale summary, mode {ops.mfma_mode()} (lstm {ops.lstm_mode()}):")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k]:.3g}")


def _slot(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


# ----------------------------------------------------------------------------- conv forms
# name -> (B, H, W, Cin, Cout, k, pad, stride, tile, out): tile 0 takes the automatic choice (the LDS-halo kernels, the 1x1 LDS tile)
CONV_FORMS = {
    "halo32": (2, 8, 32, 32, 32, 3, 1, 1, 0, "nhwc"),          # 3x3 LDS-halo kernel, 32-channel chunks
    "halo64": (2, 12, 96, 64, 64, 3, 1, 1, 0, "nhwc"),         # 3x3 LDS-halo kernel, 64-channel chunks (16x16x32 tiles)
    "generic21": (5, 7, 9, 64, 40, 3, 1, 1, 21, "nhwc"),       # hybrid split tile, ragged M and N
    "generic22": (2, 4, 32, 512, 512, 3, 1, 1, 22, "nhwc"),    # hybrid split tile, long K
    "gemm1x1": (1, 1, 256, 64, 128, 1, 0, 1, 0, "nhwc"),       # 1x1 GEMM on the 128-row LDS tile
    "convt": (4, 4, 16, 64, 128, 1, 0, 1, 0, "convt"),         # transposed conv: 1x1 GEMM + 2x2 stride-2 scatter into a concat half
    "s2": (2, 8, 16, 64, 128, 2, 0, 2, 0, "nhwc"),             # 2x2 stride-2 conv
}


def _conv_dev(form, x, w, bias=None, relu=False, x_amax=None):
    """-> (y [B][OH][OW][C] (a copy of the written columns), y_amax slot)"""
    from qea import ops
    B, H, W, Cin, Cout, k, pad, stride, tile, out = CONV_FORMS[form]
    ya = torch.zeros(1, device="cuda")
    if out == "convt":
        c = Cout // 4
        y = torch.full((B, 2 * H, 2 * W, 2 * c), float("nan"), device="cuda")
        ops.conv_igemm(x, w, y, B=B, H=H, W=W, Cin=Cin, OH=H, OW=W, N=Cout, KH=1, KW=1, ldx=Cin, ldy=2 * c, bias=bias, relu=relu, tile=tile,
                       out_mode=ops.OUT_CONVT, x_amax=x_amax, y_amax=ya)
        assert torch.isnan(y[..., c:]).all()
        return y[..., :c].clone(), ya
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.full((B, OH, OW, Cout), float("nan"), device="cuda")
    ops.conv_igemm(x, w, y, B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, N=Cout, KH=k, KW=k, pad=(pad, pad), stride=(stride, stride), ldx=Cin, ldy=Cout,
                   bias=bias, relu=relu, tile=tile, x_amax=x_amax, y_amax=ya)
    return y, ya


def _conv_operands(form, seed=0):
    B, H, W, Cin, Cout, k, pad, stride, tile, out = CONV_FORMS[form]
    g = torch.Generator().manual_seed(seed + 17 * Cin + Cout)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, k, k, Cin, generator=g) / (k * k * Cin) ** 0.5
    bias = torch.randn(Cout // 4 if out == "convt" else Cout, generator=g)
    return x, w, bias


def _conv_ref(form, x, w, bias=None):
    """fp64 on the CPU, NHWC (not for the transposed-conv form)"""
    B, H, W, Cin, Cout, k, pad, stride, tile, out = CONV_FORMS[form]
    assert out == "nhwc"
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None if bias is None else bias.double(), stride=stride,
                    padding=pad).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _conv_case(form):
    """unit-scale operands of a form, their fp64 result and sum |w| over each output's receptive field (borders included)"""
    x, w, bias = _conv_operands(form)
    return x, w, _conv_ref(form, x, w), _conv_ref(form, torch.ones_like(x), w.abs())


# ----------------------------------------------------------------------------- wgrad forms
# name -> (B, H, W, Cin, Cout, k, pad, tile): p = dY [B][H][W][Cout], q = X [B][H][W][Cin], dw [Cout][k][k][Cin]
WGRAD_FORMS = {
    "nine23": (2, 8, 32, 128, 128, 3, 1, 23),                  # producer / consumer nine-tap form (fp16 split), 64-channel blocks
    "nine29": (2, 8, 32, 128, 128, 3, 1, 29),                  # every-wave-stages nine-tap form
    "nine23n": (2, 8, 32, 64, 32, 3, 1, 23),                   # 32-channel blocks: the bf3-shaped nine-tap kernel under tile 23
    "nine29n": (2, 8, 32, 64, 32, 3, 1, 29),
    "split20": (3, 5, 7, 36, 44, 3, 1, 20),                    # generic split tiles, ragged
    "split21": (3, 5, 7, 36, 44, 3, 1, 21),
    "split22": (3, 5, 7, 36, 44, 3, 1, 22),
    "linear": (1, 1, 217, 512, 96, 1, 0, 0),                   # dW of a linear layer: M 217, K 512, N 96
}


def _wgrad_dev(form, p, q, splits=1, dw0=None, db0=None, p_amax=None, q_amax=None):
    """-> (dw, dbias); dw0 / db0 given = accumulate onto them"""
    from qea import ops
    B, H, W, Cin, Cout, k, pad, tile = WGRAD_FORMS[form]
    acc = dw0 is not None
    dw = dw0.clone() if acc else torch.full((Cout, k, k, Cin), float("nan"), device="cuda")
    db = db0.clone() if acc else torch.full((Cout,), float("nan"), device="cuda")
    ops.conv_wgrad(p, q, dw, B=B, PH=H, PW=W, QH=H, QW=W, R=Cout, Cc=Cin, KH=k, KW=k, pad=(pad, pad), ldp=Cout, ldq=Cin, accumulate=acc,
                   splits=splits, tile=tile, p_amax=p_amax, q_amax=q_amax, dbias=db)
    return dw, db


def _wgrad_operands(form, seed=0):
    B, H, W, Cin, Cout, k, pad, tile = WGRAD_FORMS[form]
    g = torch.Generator().manual_seed(seed + 13 * Cin + Cout + tile)
    return torch.randn(B, H, W, Cout, generator=g), torch.randn(B, H, W, Cin, generator=g)


def _wgrad_ref(form, p, q):
    """fp64 torch-CPU autograd -> [Cout][k][k][Cin]"""
    B, H, W, Cin, Cout, k, pad, tile = WGRAD_FORMS[form]
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.double, requires_grad=True)
    F.conv2d(q.double().permute(0, 3, 1, 2), w, padding=pad).backward(p.double().permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _wgrad_case(form):
    """unit-scale operands, fp64 dw, and per output sum |q| (over the pixels p meets it with) and sum |p|"""
    p, q = _wgrad_operands(form)
    return p, q, _wgrad_ref(form, p, q), _wgrad_ref(form, torch.ones_like(p), q.abs()), _wgrad_ref(form, p.abs(), torch.ones_like(q))


# ----------------------------------------------------------------------------- LSTM
LSTM_SHAPES = [(4, 70), (4, 600), (3, 1300)]         # 32-row groups, ragged / 128-row forward, 32-row backward / 128-row both, ragged
LSTM_MODES = ["packs", "bf3", "f32"]                 # what ops.lstm_packs returns for the session's mode / the two step kernels


def _lstm_case(T, B):
    """-> gx [T][B][2048] (gate pre-activations), W_hh of both directions, dy [T][B][512] (unit scale), and the fp64 references for that
    dy: d loss / d gx (the gate gradients) and d loss / d c_init [B][512] (dc), from the one specification of the layer
    (tests/lstm_spec.py, cached there).  Rows (samples) never mix, so the reference for a per-sample scaled dy is the per-sample
    scaled reference."""
    return lstm_spec.unit_case_with_reference(T, B)


def _lstm_packs(mode, wh):
    """-> (fwd pack, bwd pack, mode for lstm_layer_*_any), as test_lstm_layer_fwd_bwd selects them"""
    from qea import _lib, ops
    whd = [w.cuda() for w in wh]
    if mode == "packs":
        return ops.lstm_packs(whd[0], whd[1])
    if mode == "bf3":
        nb = _lib.lib().qea_lstm_pack_whh_split_bytes()
        pf, pb = torch.empty(2, nb, dtype=torch.uint8, device="cuda"), torch.empty(2, nb, dtype=torch.uint8, device="cuda")
    else:
        pf, pb = torch.empty(2, 1024 * 256, device="cuda"), torch.empty(2, 1024 * 256, device="cuda")
    for d in range(2):
        (ops.lstm_pack_whh_split if mode == "bf3" else ops.lstm_pack_whh)(whd[d], pf[d], pb[d])
    return pf, pb, mode


class _LstmLayer:
    """the forward of one layer run once on the device; backward(dy) -> (gate gradients, dc or None, g_amax or None)"""

    def __init__(self, T, B, mode):
        from qea import ops
        gx, wh, _, _, _ = _lstm_case(T, B)
        self.T, self.B = T, B
        self.pf, self.pb, self.mode = _lstm_packs(mode, wh)
        self.acts = gx.cuda()
        self.c, y = torch.empty(T, B, 512, device="cuda"), torch.empty(T, B, 512, device="cuda")
        ops.lstm_layer_fwd_any(self.acts, self.c, y, self.pf, self.mode, T, B)

    def backward(self, dy):
        from qea import ops
        gates = self.acts.clone()
        seq = self.mode == "seq"
        dc = None if seq else torch.full((self.B, 512), float("nan"), device="cuda")
        ga = torch.zeros(1, device="cuda")
        carried = ops.lstm_layer_bwd_any(gates, self.c, dy.cuda(), self.pb, self.mode, dc, self.T, self.B, g_amax=ga)
        torch.cuda.synchronize()
        assert bool(carried) == seq
        return gates, dc, (ga if carried else None)


_per_sample = lstm_spec.per_sample     # max error and max |ref| of every sample


# ============================================================================= 1. power-of-two homogeneity, bit for bit
KS = (-40, -17, 20)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("form", list(CONV_FORMS))
def test_conv_is_homogeneous_in_powers_of_two(form, bias):
    """conv(x 2^a, w 2^b) (+ bias 2^(a+b), ReLU) == conv(x, w) 2^(a+b) BIT FOR BIT, y_amax included: every scale is a power of two, so the
    planes and accumulators of the scaled run are those of the base run and only the un-scaling differs; without scales fp32 and bf16
    carry the same exponents.  x alone, w alone, both; abs-max taken by ops and supplied by the caller."""
    x, w, b = _conv_operands(form, seed=1)
    x, w, b = x.cuda(), w.cuda(), (b.cuda() if bias else None)
    y0, a0 = _conv_dev(form, x, w, b, relu=bias)
    assert torch.isfinite(y0).all() and a0.item() > 0
    for supplied in (False, True):
        for ka, kb in [(k, 0) for k in KS] + [(0, k) for k in KS] + [(-40, 20), (20, -17), (-17, -40)]:
            xs, ws = x * 2.0 ** ka, w * 2.0 ** kb
            f = 2.0 ** (ka + kb)
            y1, a1 = _conv_dev(form, xs, ws, None if b is None else b * f, relu=bias, x_amax=xs.abs().max().reshape(1) if supplied else None)
            assert torch.equal(y1, y0 * f), (form, ka, kb, supplied)
            assert torch.equal(a1, a0 * f), (form, ka, kb, supplied)


@pytest.mark.parametrize("splits,acc", [(1, False), (1, True), (3, True)])
@pytest.mark.parametrize("form", list(WGRAD_FORMS))
def test_wgrad_is_homogeneous_in_powers_of_two(form, splits, acc):
    """wgrad(p 2^a, q 2^b) == wgrad(p, q) 2^(a+b) and dbias(p 2^a) == dbias(p) 2^a bit for bit; under accumulate the initial dw / dbias
    are scaled as well."""
    p, q = _wgrad_operands(form, seed=1)
    p, q = p.cuda(), q.cuda()
    g = torch.Generator().manual_seed(9)
    B, H, W, Cin, Cout, k, pad, tile = WGRAD_FORMS[form]
    dw0 = torch.randn(Cout, k, k, Cin, generator=g).cuda() if acc else None
    db0 = torch.randn(Cout, generator=g).cuda() if acc else None
    w_base, b_base = _wgrad_dev(form, p, q, splits, dw0, db0)
    assert torch.isfinite(w_base).all() and torch.isfinite(b_base).all()
    for supplied in (False, True):
        for ka, kb in [(-40, 0), (0, -17), (20, 0), (0, 20), (20, -40), (-17, 20)]:
            ps, qs = p * 2.0 ** ka, q * 2.0 ** kb
            f = 2.0 ** (ka + kb)
            am = dict(p_amax=ps.abs().max().reshape(1), q_amax=qs.abs().max().reshape(1)) if supplied else {}
            w1, b1 = _wgrad_dev(form, ps, qs, splits, dw0 * f if acc else None, db0 * 2.0 ** ka if acc else None, **am)
            assert torch.equal(w1, w_base * f), (form, ka, kb, supplied)
            assert torch.equal(b1, b_base * 2.0 ** ka), (form, ka, kb, supplied)


@pytest.mark.parametrize("mode", LSTM_MODES)
@pytest.mark.parametrize("T,B", LSTM_SHAPES)
def test_lstm_backward_is_homogeneous_in_powers_of_two(T, B, mode):
    """dy 2^k gives the gate gradients, dc (step kernels) and g_amax (one-launch kernel) times 2^k bit for bit: the per-tile scales of
    the exchanged gate gradients are powers of two of the tile's own abs-max.  Which quantity exists in which mode follows the API:
    the gate gradients in all; dc (the initial cell state's gradient, the dc_scratch buffer) in the step kernels "bf3" / "f32" only;
    g_amax in the one-launch kernel ("seq", what "packs" gives in split_f16 mode) only."""
    layer = _LstmLayer(T, B, mode)
    dy = _lstm_case(T, B)[2]
    g0, dc0, a0 = layer.backward(dy)
    assert torch.isfinite(g0).all()
    for k in KS:
        g1, dc1, a1 = layer.backward(dy * 2.0 ** k)
        assert torch.equal(g1, g0 * 2.0 ** k), (mode, k)
        if dc0 is not None:
            assert torch.isfinite(dc0).all() and torch.equal(dc1, dc0 * 2.0 ** k), (mode, k)
        if a0 is not None:
            assert a0.item() > 0 and torch.equal(a1, a0 * 2.0 ** k), (mode, k)


def _bn_setup(C, M, seed):
    from qea import ops
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, C, generator=g) * 2 + 0.3).cuda()
    gamma, beta = torch.randn(C, generator=g).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    coef = torch.empty(4, C, device="cuda")                     # mean, invstd, scale, shift
    st = torch.empty(2, C, device="cuda", dtype=torch.float64)
    ops.bn_train_stats(y, C, M, C, gamma, beta, 1e-5, 0.1, rm, rv, coef[0], coef[1], coef[2], coef[3], st)
    return g, y, gamma, coef, st


@pytest.mark.parametrize("C,M", [(32, 8197), (512, 777)])
def test_bn_bwd_is_homogeneous_in_powers_of_two(C, M):
    """qea_bn_bwd is linear in da with fp64 reductions and fp64 per-channel constants, rounded to fp32 once per output: dy, dgamma,
    dbeta and the abs-max slot scale exactly (ReLU mask from the activation and recomputed from y)."""
    from qea import ops
    g, y, gamma, coef, st = _bn_setup(C, M, C + M)
    a = torch.empty(M, C, device="cuda")
    ops.bn_apply(y, C, a, C, M, C, coef[2], coef[3], relu=True)
    da = torch.randn(M, C, generator=g).cuda()
    for kw in (dict(a=a, lda=C), dict(a=None, lda=0, relu_scale=coef[2], relu_shift=coef[3])):
        def run(d):
            kw_ = dict(kw)
            dg, db, dy, am = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(M, C, device="cuda"), torch.zeros(1, device="cuda")
            ops.bn_bwd(d, C, kw_.pop("a"), kw_.pop("lda"), y, C, M, C, gamma, coef[0], coef[1], True, dg, db, dy, C, stat64=st, amax=am, **kw_)
            return dy, dg, db, am
        base = run(da)
        assert all(torch.isfinite(t).all() for t in base) and base[3].item() == base[0].abs().max().item()
        for k in KS:
            for u, v in zip(run(da * 2.0 ** k), base):
                assert torch.equal(u, v * 2.0 ** k), k


@pytest.mark.parametrize("C,B,H,W,kw", [(32, 3, 4, 683, 1), (512, 3, 2, 130, 2)])
def test_bn_bwd_pool_is_homogeneous_in_powers_of_two(C, B, H, W, kw):
    """qea_bn_bwd_pool (max-pool backward inside the BatchNorm backward) in da (the skip path) and dpool together; M = 8196 / 780 rows."""
    from qea import ops
    M = B * H * W
    g, y, gamma, coef, st = _bn_setup(C, M, C + M)
    dskip = torch.randn(M, C, generator=g).cuda()
    dpool = torch.randn(B * (H // 2) * (W // kw), C, generator=g).cuda()

    def run(ds, dp, skip):
        dg, db, dy, am = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(M, C, device="cuda"), torch.zeros(1, device="cuda")
        ops.bn_bwd_pool(ds if skip else None, C if skip else 0, dp, C, kw, y, C, B, H, W, C, gamma, coef[0], coef[1], True, dg, db, dy, C, stat64=st,
                        relu_scale=coef[2], relu_shift=coef[3], amax=am)
        return dy, dg, db, am
    for skip in (True, False):
        base = run(dskip, dpool, skip)
        assert all(torch.isfinite(t).all() for t in base) and base[3].item() == base[0].abs().max().item()
        for k in KS:
            for u, v in zip(run(dskip * 2.0 ** k, dpool * 2.0 ** k, skip), base):
                assert torch.equal(u, v * 2.0 ** k), k


# ============================================================================= 2. loose and shared bounds
RATIOS = [1.0, 2.0 ** 5, 2.0 ** 10, 2.0 ** 20]


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -27])
@pytest.mark.parametrize("form", ["halo32", "halo64", "generic21", "gemm1x1"])
def test_conv_identity_filter_shows_the_split_of_every_element(form, scale):
    """An identity filter (one entry 1 per output channel, centre tap) makes y[.., n] = x[.., n % Cin] as the launch represents it:
    (h + l) / s after one fp32 rounding.  Every ELEMENT is gated by the contract itself (helpers.split_element_gate, no project gate on
    top), with the values of helpers.split_probe_values crowded around the edge of the relative regime and a power-of-two bound.
    This is the case that sees ONE bit of scale: with `se = 13 - ...` in qea_f16_scale the elements in [2^-16, 2^-15) of the bound
    come out up to 2^-22 off (emulated on the CPU in test_f16_split_contract_in_numpy), which no gate on a sum of many terms notices.
    Abs-max taken by ops and supplied; unit scale and the gradient scale 2^-27."""
    from helpers import split_element_gate, split_probe_values
    B, H, W, Cin, Cout, k, pad, stride, tile, out = CONV_FORMS[form]
    x = (split_probe_values(B * H * W * Cin, 3 + Cin) * scale).view(B, H, W, Cin)
    w = torch.zeros(Cout, k, k, Cin)
    w[torch.arange(Cout), k // 2, k // 2, torch.arange(Cout) % Cin] = 1.0
    want = x[..., torch.arange(Cout) % Cin].double()
    gate = split_element_gate(want, scale)
    for supplied in (False, True):
        y, ya = _conv_dev(form, x.cuda(), w.cuda(), x_amax=_slot(scale) if supplied else None)
        _check("conv identity, per element", (y.cpu().double() - want).abs(), gate)
        assert ya.item() > 0


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("form", ["halo32", "halo64", "generic21", "generic22", "gemm1x1"])
def test_conv_with_a_loose_input_bound(form, ratio):
    """x_amax = ratio x the true maximum (the shared slot of a concat buffer): up to 2^10 the conv gate holds unchanged (elements down
    to 2^-16 of the bound keep the relative error); at 2^20 every element is in the absolute regime, SPLIT_ABS x bound each, hence
    SPLIT_ABS x bound x sum |w| per output, on top of the gate.  The slot is read where the launch runs on the fp16 split: all five
    forms in split_f16 mode (asserted at 2^20: the result must differ from the tight-bound one), none in the other two modes, where
    the case only shows that a supplied slot does no harm."""
    from qea import ops
    x, w, ref, sum_w = _conv_case(form)
    bound = x.abs().max().item() * ratio
    y, _ = _conv_dev(form, x.cuda(), w.cuda(), x_amax=_slot(bound))
    if ratio > 2.0 ** 10 and ops.mfma_mode() == "split_f16":
        assert not torch.equal(y, _conv_dev(form, x.cuda(), w.cuda(), x_amax=_slot(bound / ratio))[0]), "x_amax was not consumed"
    err = (y.cpu().double() - ref).abs()
    gate = CONV_GATE * ref.abs().max().item()
    if ratio > 2.0 ** 10:
        gate = gate + SPLIT_ABS * bound * sum_w
    _check("conv loose bound", err, gate)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("form", ["nine23", "nine29", "nine23n", "split21"])
def test_wgrad_with_loose_operand_bounds(form, ratio):
    """p_amax / q_amax = ratio x the true maxima; the wgrad gate 3e-5 max |ref| WITHOUT an absolute term; at 2^20 the derived bound:
    each p element is off by SPLIT_ABS x bound_p, each q element by SPLIT_ABS x bound_q.  The four forms read both slots in split_f16
    mode (asserted at 2^20), none does in the other modes (ops hands the slots on to the nine-tap and generic split tiles only)."""
    from qea import ops
    p, q, ref, sum_q, sum_p = _wgrad_case(form)
    bp, bq = p.abs().max().item() * ratio, q.abs().max().item() * ratio
    dw, _ = _wgrad_dev(form, p.cuda(), q.cuda(), p_amax=_slot(bp), q_amax=_slot(bq))
    if ratio > 2.0 ** 10 and ops.mfma_mode() == "split_f16":
        assert not torch.equal(dw, _wgrad_dev(form, p.cuda(), q.cuda(), p_amax=_slot(bp / ratio), q_amax=_slot(bq / ratio))[0]), "slots not consumed"
    err = (dw.cpu().double() - ref).abs()
    gate = WGRAD_GATE * ref.abs().max().item()
    if ratio > 2.0 ** 10:
        npix = p.shape[0] * p.shape[1] * p.shape[2]
        gate = gate + SPLIT_ABS * (bp * sum_q + bq * sum_p) + SPLIT_ABS ** 2 * bp * bq * npix
    _check("wgrad loose bounds", err, gate)


# ============================================================================= 3. magnitude mixtures, region by region
MIX = [2.0 ** -8, 2.0 ** -16, 2.0 ** -24]


@pytest.mark.parametrize("r", MIX)
@pytest.mark.parametrize("form", ["halo32", "halo64", "generic22"])
def test_conv_small_half_image_is_judged_alone(form, r):
    """Columns W/2.. of every image are r times smaller.  Outputs two or more columns inside the small half see small inputs only and
    are gated against THEIR max |ref| (a gate on the whole output's maximum hides them entirely): the conv gate down to 2^-16; at
    2^-24 the inputs are in the absolute regime of the split, SPLIT_ABS x m x sum |w| per output on top.  The large half likewise."""
    x, w, _, sum_w = _conv_case(form)
    Wd = x.shape[2]
    x = x.clone()
    x[:, :, Wd // 2:] *= r
    ref = _conv_ref(form, x, w)
    y, _ = _conv_dev(form, x.cuda(), w.cuda())
    err = (y.cpu().double() - ref).abs()
    small, large = slice(Wd // 2 + 2, Wd), slice(0, Wd // 2 - 2)
    gate = CONV_GATE * ref[:, :, small].abs().max().item()
    if r < 2.0 ** -16:
        gate = gate + SPLIT_ABS * x.abs().max().item() * sum_w[:, :, small]
    _check("conv mixture, small region", err[:, :, small], gate)
    _check("conv mixture, large region", err[:, :, large], CONV_GATE * ref[:, :, large].abs().max().item())


@pytest.mark.parametrize("r", MIX)
@pytest.mark.parametrize("which", ["p", "q"])
@pytest.mark.parametrize("form", ["nine23", "nine29", "split21"])
def test_wgrad_small_channel_block_is_judged_alone(form, which, r):
    """One 32-channel block of p (of q) is r times smaller: its dw rows (columns) are gated against their own max |ref|, the rest
    against theirs."""
    p, q, _, sum_q, sum_p = _wgrad_case(form)
    p, q = p.clone(), q.clone()
    (p if which == "p" else q)[..., :32] *= r
    ref = _wgrad_ref(form, p, q)
    dw, _ = _wgrad_dev(form, p.cuda(), q.cuda())
    err = (dw.cpu().double() - ref).abs()
    if which == "p":
        es, rs, el, rl = err[:32], ref[:32], err[32:], ref[32:]
        extra = SPLIT_ABS * p.abs().max().item() * sum_q[:32]
    else:
        es, rs, el, rl = err[..., :32], ref[..., :32], err[..., 32:], ref[..., 32:]
        extra = SPLIT_ABS * q.abs().max().item() * sum_p[..., :32]
    gate = WGRAD_GATE * rs.abs().max().item()
    if r < 2.0 ** -16:
        gate = gate + extra
    _check("wgrad mixture, small block", es, gate)
    _check("wgrad mixture, large block", el, WGRAD_GATE * rl.abs().max().item())


def _lstm_arrangement(name, B):
    s = torch.ones(B, dtype=torch.float64)
    if name == "half_tile":          # inside one 32-row tile, half the samples at 2^-12
        s[32:64:2] = 2.0 ** -12
    elif name == "whole_tiles":      # whole tiles at 2^-30 and 2^+10 next to unit-scale tiles
        s[0:32] = 2.0 ** -30
        s[32:64] = 2.0 ** 10
    else:                            # a whole tile of zero dy
        s[32:64] = 0.0
    return s


@pytest.mark.parametrize("arrangement", ["half_tile", "whole_tiles", "zero_tile"])
@pytest.mark.parametrize("mode", LSTM_MODES)
@pytest.mark.parametrize("T,B", LSTM_SHAPES)
def test_lstm_backward_per_sample_scales(T, B, mode, arrangement):
    """dy scaled per sample; every sample's gate gradients (and dc) against its OWN max |ref| at the 1e-4 gate.  "whole_tiles" is
    what the per-tile scale of the exchanged gate gradients exists for: under one scale for the tensor (abs-max ~2^11, s = 2^3) the
    2^-30 tile's values lie below fp16's smallest subnormal 2^-24, both its planes are zero and its recurrent term is lost whole, an
    error of the order of the sample's own maximum.  A tile of zero dy gives exactly 0, finite,
    and leaves its neighbours within the gate.  The gate gradients are judged in every mode; dc only where it exists (step kernels
    "bf3" / "f32"); g_amax == max |gate gradient| only in "seq"."""
    _, _, dy, ref_g, ref_dc = _lstm_case(T, B)
    s = _lstm_arrangement(arrangement, B)
    layer = _LstmLayer(T, B, mode)
    gates, dc, ga = layer.backward(dy * s.float()[None, :, None])
    assert torch.isfinite(gates).all()
    rg = ref_g * s[None, :, None]
    err, top = _per_sample(gates, rg)
    _check(f"lstm bwd {arrangement}", err, LSTM_GATE * top)
    if arrangement == "zero_tile":
        assert (gates[:, 32:64] == 0).all() and (top[32:64] == 0).all()
    if dc is not None:
        err, top = _per_sample(dc, ref_dc * s[:, None])
        _check(f"lstm bwd {arrangement}", err, LSTM_GATE * top)
    if ga is not None:
        assert ga.item() == gates.abs().max().item()


# ============================================================================= 4. zeros and realistic gradient scale
@pytest.mark.parametrize("form", ["halo32", "halo64", "generic21", "gemm1x1", "convt", "s2"])
def test_conv_of_an_all_zero_input(form):
    """x == 0: the abs-max reads 0, the scale is 1, y == bias (ReLU: max(bias, 0)) or 0 exactly, y_amax accordingly"""
    from qea import ops
    x, w, bias = _conv_operands(form)
    B, H, W, Cin = x.shape
    x = torch.zeros_like(x).cuda()
    assert ops.absmax(x, Cin, B * H * W, Cin).item() == 0.0
    for supplied in (False, True):
        am = _slot(0.0) if supplied else None
        y, ya = _conv_dev(form, x, w.cuda(), x_amax=am)
        assert (y == 0).all() and ya.item() == 0.0
        y, ya = _conv_dev(form, x, w.cuda(), bias.cuda(), relu=True, x_amax=am)
        want = bias.clamp_min(0).cuda().expand_as(y)
        assert torch.equal(y, want) and ya.item() == want.max().item()


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("form", ["nine23", "nine29", "nine23n", "split21", "linear"])
def test_wgrad_of_an_all_zero_operand(form, splits):
    """p == 0 or q == 0: dw == 0 exactly (the initial value under accumulate), dbias == 0 for p == 0, nothing non-finite"""
    p, q = _wgrad_operands(form)
    p, q = p.cuda(), q.cuda()
    g = torch.Generator().manual_seed(4)
    B, H, W, Cin, Cout, k, pad, tile = WGRAD_FORMS[form]
    dw0, db0 = torch.randn(Cout, k, k, Cin, generator=g).cuda(), torch.randn(Cout, generator=g).cuda()
    for pz, qz in ((torch.zeros_like(p), q), (p, torch.zeros_like(q)), (torch.zeros_like(p), torch.zeros_like(q))):
        for supplied in (False, True):
            am = dict(p_amax=pz.abs().max().reshape(1), q_amax=qz.abs().max().reshape(1)) if supplied else {}
            dw, db = _wgrad_dev(form, pz, qz, splits, **am)
            assert (dw == 0).all() and torch.isfinite(db).all()
            if pz is not p:
                assert (db == 0).all()
            dw, db = _wgrad_dev(form, pz, qz, splits, dw0, db0, **am)
            assert torch.equal(dw, dw0)
            if pz is not p:
                assert torch.equal(db, db0)


def test_backward_chain_at_the_gradient_scale_of_a_large_batch():
    """dy = randn x 1e-8 (a mean-reduced CTC loss at B = 2048) through the LSTM backward, the input gradient (1x1 conv over the gate
    gradients, their abs-max carried by the producer where it leaves one) and the weight gradient, then a 3x3 layer's input and weight
    gradient at the same scale: every result gated RELATIVELY (an absolute 1e-6 would pass a kernel that returns zeros here)."""
    from qea import ops
    T, B, In = 4, 70, 512
    gx, wh, dy, ref_g, _ = _lstm_case(T, B)
    s = 1e-8
    layer = _LstmLayer(T, B, "packs")
    gates, _, ga = layer.backward(dy * s)
    err, top = _per_sample(gates, ref_g * float(torch.tensor(s, dtype=torch.float32)))
    _check("chain 1e-8: lstm gates", err, LSTM_GATE * top)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(T * B, In, generator=g) * 0.5
    w_ih = torch.randn(2048, In, generator=g) / In ** 0.5
    gd = gates.view(T * B, 2048)
    g64 = gd.cpu().double()                                   # the device's own gate gradients are the next operand
    dx = torch.empty(T * B, In, device="cuda")
    ops.conv_igemm(gd, w_ih.t().contiguous().cuda(), dx, B=1, H=1, W=T * B, Cin=2048, OH=1, OW=T * B, N=In, KH=1, KW=1, ldx=2048, ldy=In, x_amax=ga)
    ref = g64 @ w_ih.double()
    _check("chain 1e-8: dx", (dx.cpu().double() - ref).abs(), CONV_GATE * ref.abs().max().item())
    dw = torch.empty(2048, In, device="cuda")
    ops.conv_wgrad(gd, x.cuda(), dw, B=1, PH=1, PW=T * B, QH=1, QW=T * B, R=2048, Cc=In, KH=1, KW=1, ldp=2048, ldq=In, p_amax=ga)
    ref = g64.t() @ x.double()
    _check("chain 1e-8: dw", (dw.cpu().double() - ref).abs(), WGRAD_GATE * ref.abs().max().item())
    # a 3x3 layer: input gradient (conv of dy with a filter) and weight gradient (the nine-tap kernel), dy at 1e-8
    p, q, ref_w, _, _ = _wgrad_case("nine23")
    p = p * float(torch.tensor(s, dtype=torch.float32))
    dw3, _ = _wgrad_dev("nine23", p.cuda(), q.cuda())
    ref = _wgrad_ref("nine23", p, q)
    _check("chain 1e-8: dw", (dw3.cpu().double() - ref).abs(), WGRAD_GATE * ref.abs().max().item())
    x3, w3, _, _ = _conv_case("halo64")
    x3 = x3 * float(torch.tensor(s, dtype=torch.float32))
    y3, _ = _conv_dev("halo64", x3.cuda(), w3.cuda())
    ref = _conv_ref("halo64", x3, w3)
    _check("chain 1e-8: dx", (y3.cpu().double() - ref).abs(), CONV_GATE * ref.abs().max().item())
