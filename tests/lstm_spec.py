"""ONE fp64 specification of the bidirectional LSTM layer (hidden 256) that every arithmetic path of the library is held to:
the one-launch kernels of csrc/lstm_seq.hip ("seq") and the per-step kernels of csrc/lstm.hip ("bf3", "f32").

The layer as the kernels see it: `gates` [T][B][2048] holds the gate pre-activations x W_ih^T + b on entry (gx), column
d*1024 + gate*256 + unit, gate order i, f, g, o; direction 0 runs t = 0 .. T-1, direction 1 runs t = T-1 .. 0; h0 = c0 = 0.

    a = gx[t] + h W_hh^T,   c = sigma(a_f) c + sigma(a_i) tanh(a_g),   h = sigma(a_o) tanh(c),   y[t] = h

The forward writes y [T][B][512], c [T][B][512] and, over gx, the activations sigma(a_i), sigma(a_f), tanh(a_g), sigma(a_o); the
backward turns the activations in place into d loss / d a (the gate gradients) for a given dy = d loss / d y, and the step kernels
leave d loss / d c0 [B][512] in their dc buffer.  `reference` returns all five in fp64.  Rows (samples) never mix.

tests/test_lstm_spec_cpu.py holds this module to torch.nn.LSTM and to oracle.model_oracle.lstm_layer_dir in fp64."""
import collections
import functools

import torch

HID, GATES = 256, 1024
GATE_KINDS = ("i", "f", "g", "o")
SATURATING = (12.0, 40.0, 89.0, 200.0, 1e4)       # each exact in fp32; exp overflows fp32 from 88.73 on, 1 - sigma(x) rounds to 0 in fp32 from 17.4 on

SATURATED_SHAPES = ((4, 70), (4, 1300))         # (T, B) at which the saturated operands are used on the device and checked on the host

Spec = collections.namedtuple("Spec", "y c acts dgates dc0")


def reference(gx, wh, dy, dtype=torch.float64):
    """gx [T][B][2048], wh = the two W_hh [1024][256], dy [T][B][512] -> Spec(y, c, acts, dgates, dc0), computed in `dtype`
    (fp64: the specification; fp32: a plain fp32 implementation of it, for comparison).  A plain loop; the gradients by autograd
    (dy None: forward only, dgates and dc0 None)."""
    T, B, _ = gx.shape
    gxr = gx.to(dtype).requires_grad_()
    c0 = torch.zeros(B, 2 * HID, dtype=dtype, requires_grad=True)
    outs, cs, acts = [], [], torch.empty(T, B, 2 * GATES, dtype=dtype)
    for d in range(2):
        w = wh[d].to(dtype)
        h, c = torch.zeros(B, HID, dtype=dtype), c0[:, d * HID:(d + 1) * HID]
        ys, cl = [None] * T, [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            i, f, gg, o = (gxr[t, :, d * 1024:(d + 1) * 1024] + h @ w.t()).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            ys[t], cl[t] = h, c.detach()
            acts[t, :, d * GATES:(d + 1) * GATES] = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], dim=1).detach()
        outs.append(torch.stack(ys))
        cs.append(torch.stack(cl))
    y = torch.cat(outs, dim=2)
    if dy is None:
        return Spec(y.detach(), torch.cat(cs, dim=2), acts, None, None)
    y.backward(dy.to(dtype))
    return Spec(y.detach(), torch.cat(cs, dim=2), acts, gxr.grad, c0.grad)


def case(T, B, seed=None):
    """unit-scale operands -> gx [T][B][2048] = 0.5 randn, the two W_hh [1024][256] = randn / 16, dy [T][B][512] = randn (fp32)"""
    g = torch.Generator().manual_seed(T * 1000 + B if seed is None else seed)
    gx = torch.randn(T, B, 2048, generator=g) * 0.5
    wh = [torch.randn(1024, 256, generator=g) / 16 for _ in range(2)]
    dy = torch.randn(T, B, 512, generator=g)
    return gx, wh, dy


def saturated_case(T, B, seed=None):
    """`case`, but in every sample one eighth of the pre-activations of every gate kind (of its T x 2 x 256 places, the first eighth
    of a seeded permutation per sample and kind) are replaced by +-12, +-40, +-89, +-200, +-1e4, dealt out in turn along that
    permutation.  The other seven eighths stay at unit scale, so every sample keeps gate gradients of ordinary size."""
    gx, wh, dy = case(T, B, seed)
    g = torch.Generator().manual_seed((T * 1000 + B if seed is None else seed) + 7919)
    n = T * 2 * HID
    pick = torch.rand(B, 4, n, generator=g).argsort(dim=2)[:, :, :n // 8]                  # [B][kind][n / 8] places (t, d, unit)
    vals = torch.tensor([s * v for v in SATURATING for s in (1.0, -1.0)])
    v = vals[torch.arange(n // 8) % len(vals)].expand(B, 4, n // 8)
    view = gx.view(T, B, 2, 4, HID).permute(1, 3, 0, 2, 4).reshape(B, 4, n).clone()         # [B][kind][(t, d, unit)]
    view.scatter_(2, pick, v)
    gx = view.view(B, 4, T, 2, HID).permute(2, 0, 3, 1, 4).reshape(T, B, 2048).contiguous()
    return gx, wh, dy


@functools.lru_cache(maxsize=None)
def unit_case_with_reference(T, B):
    """-> gx, W_hh of both directions, dy, and the fp64 references for that dy: the gate gradients [T][B][2048] and
    d loss / d c0 [B][512] (the LSTM case of tests/test_operand_scale_gpu.py; small shapes only: it is kept for the session)"""
    gx, wh, dy = case(T, B)
    ref = reference(gx, wh, dy)
    return gx, wh, dy, ref.dgates, ref.dc0


def per_sample(got, ref):
    """max error and max |ref| of every sample (dim 1 of [T][B][..], dim 0 of [B][..])"""
    dims = (0, 2) if ref.dim() == 3 else (1,)
    return (got.cpu().double() - ref).abs().amax(dim=dims), ref.abs().amax(dim=dims)
