"""The fused search of DESIGN.md ("Character n-gram fusion"), written out literally in fp64 Python floats as an extension of
tests/beam_spec.py: lists only, linear searches, the candidates built in the order the specification names them, a stable sort on the
ranking score.  Independent of qea/beam.py (which it checks) and of the device kernel.  Like beam_spec.decode it reports the smallest
non-zero gap between two RANKING scores whose order decided something."""
import math

import torch

import beam_spec

NEG = -math.inf
lse, _gap = beam_spec.lse, beam_spec._gap


def start_context(C, m, blank):
    """ctx(()): the blank (BOS), m times."""
    ctx = 0
    for _ in range(m):
        ctx = ctx * C + blank
    return ctx


def decode(lp, K, W, m, blank=0):
    """lp: T rows of C float32 values, W: C**m rows of C fp64 values (NaN counts as -inf) -> (beam, gap): beam = [(prefix tuple, ctc,
    total)] best first by total, at most K entries; gap as in beam_spec.decode, over the ranking scores."""
    T, C = len(lp), len(lp[0])
    mod = C ** m
    beam = [((), 0.0, NEG, 0.0, start_context(C, m, blank))]           # (prefix, pb, pnb, lm, ctx)
    gap = math.inf
    for t in range(T):
        row = [float(v) for v in lp[t]]
        row = [NEG if v != v else v for v in row]
        tot = [lse(pb, pnb) for _, pb, pnb, _, _ in beam]
        stay_pb = [tot[i] + row[blank] for i in range(len(beam))]
        stay_pnb = [(beam[i][2] + row[beam[i][0][-1]]) if beam[i][0] else NEG for i in range(len(beam))]
        ext = []
        for i, (p, pb, pnb, lm, ctx) in enumerate(beam):
            for c in range(C):
                if c == blank:
                    continue
                v = (pb if (p and c == p[-1]) else tot[i]) + row[c]       # pnb': exactly the plain search's term
                q = p + (c,)
                j = None
                for jj in range(len(beam)):
                    if beam[jj][0] == q:
                        j = jj
                if j is None:
                    w = float(W[ctx][c])
                    w = NEG if w != w else w
                    lm2 = lm + w                                        # first lm', then the sum
                    ext.append((i, v + lm2, q, v, lm2, (ctx * C + c) % mod))
                else:
                    stay_pnb[j] = lse(stay_pnb[j], v)                   # the same prefix: the same lm and ctx, nothing else changes
        cands = []
        for i, (p, _, _, lm, ctx) in enumerate(beam):
            cands.append((lse(stay_pb[i], stay_pnb[i]) + lm, p, stay_pb[i], stay_pnb[i], lm, ctx))
            cands.extend((r, q, NEG, v, lm2, cx) for (ii, r, q, v, lm2, cx) in ext if ii == i)
        cands = [c for c in cands if c[0] > NEG]                        # not greater than -inf (a NaN too): dropped
        cands.sort(key=lambda c: -c[0])                                 # stable: equal scores keep the candidate order
        if len(cands) > K:
            gap = _gap(cands[K - 1][0], cands[K][0], gap)
        for a, b in zip(cands[:K], cands[1:K]):
            gap = _gap(a[0], b[0], gap)
        beam = [c[1:] for c in cands[:K]]
    return [(p, lse(pb, pnb), lse(pb, pnb) + lm) for p, pb, pnb, lm, _ in beam], gap


def decode_batch(scores, K, W, m, blank=0):
    """scores: a [T,N,C] float32 tensor, W: a [C**m, C] fp64 tensor or nested list -> ([beam of sample n], the smallest gap)."""
    return beam_spec.decode_batch(scores, K, W.tolist() if torch.is_tensor(W) else W, m, blank, search=decode)


def as_arrays(beams, K, T):
    """The layout of qea.ops.ctc_beam_decode_lm as nested lists: (tokens [N][K][T], lengths [N][K], ctc [N][K], total [N][K])."""
    tokens, lengths, ctc = beam_spec.as_arrays([[(p, s) for p, s, _ in b] for b in beams], K, T)
    total = [[tt for _, _, tt in b] + [NEG] * (K - len(b)) for b in beams]
    return tokens, lengths, ctc, total


def table(C, m, seed):
    """The tests' fused table: randn(C**m, C) - 1 in fp64, generator seed 1000 + seed."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(C ** m, C, generator=g, dtype=torch.float64) - 1.0


def table_sum(W, label, C, m, blank=0):
    """The sum of the table entries along a labelling, contexts BOS-padded."""
    ctx, s = start_context(C, m, blank), 0.0
    for c in label:
        s += float(W[ctx][c])
        ctx = (ctx * C + c) % (C ** m)
    return s


def forbidden_case(T, N, C, K, seed):
    """The hard-constraint input of the CPU and the GPU test: a bigram table with the pair (1, 2) at -inf and the pair (3, 3) at NaN."""
    lp = beam_spec.log_probs(T, N, C, seed)
    W = table(C, 1, seed)
    W[1, 2] = -math.inf
    W[3, 3] = float("nan")
    return lp, W


def has_forbidden_pair(prefix):
    return any((a, c) in ((1, 2), (3, 3)) for a, c in zip(prefix, prefix[1:]))
