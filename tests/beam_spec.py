"""The CTC prefix beam search of DESIGN.md ("CTC prefix beam search"), written out literally in fp64 Python floats: lists only, the
candidates built in the order the specification names them, a stable sort.  Independent of qea/beam.py (which it checks) and of the
device kernel.  It also reports the smallest non-zero gap between two scores whose order decided something, so that a test can show
its inputs are far from a near-tie that fp64 rounding could turn."""
import math

import torch

NEG = -math.inf


def lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def _gap(a, b, best):
    d = abs(a - b)
    return d if 0.0 < d < best else best


def decode(lp, K, blank=0):
    """lp: T rows of C float32 values (lists or an array) -> (beam, gap): beam = [(prefix tuple, score)] best first, at most K
    entries; gap = the smallest non-zero difference between the K-th and (K+1)-th candidate of any step and between neighbours of
    every step's beam (the last one is the result), inf if there is none."""
    T, C = len(lp), len(lp[0])
    beam = [((), 0.0, NEG)]
    gap = math.inf
    for t in range(T):
        row = [float(v) for v in lp[t]]
        row = [NEG if v != v else v for v in row]
        tot = [lse(pb, pnb) for _, pb, pnb in beam]
        # slot 0 of every entry
        stay_pb = [tot[i] + row[blank] for i in range(len(beam))]
        stay_pnb = [(beam[i][2] + row[beam[i][0][-1]]) if beam[i][0] else NEG for i in range(len(beam))]
        # the extensions, walked by (rank, class); one that is itself a beam entry is folded into that entry's slot 0
        ext = []
        for i, (p, pb, pnb) in enumerate(beam):
            for c in range(C):
                if c == blank:
                    continue
                v = (pb if (p and c == p[-1]) else tot[i]) + row[c]
                q = p + (c,)
                j = None
                for jj in range(len(beam)):
                    if beam[jj][0] == q:
                        j = jj
                if j is None:
                    ext.append((i, c, q, v))
                else:
                    stay_pnb[j] = lse(stay_pnb[j], v)
        # the candidates in order: rank ascending, slot 0 first, then the classes ascending
        cands = []
        for i, (p, _, _) in enumerate(beam):
            cands.append((lse(stay_pb[i], stay_pnb[i]), p, stay_pb[i], stay_pnb[i]))
            cands.extend((v, q, NEG, v) for (ii, c, q, v) in ext if ii == i)
        cands = [c for c in cands if c[0] != NEG]
        cands.sort(key=lambda c: -c[0])                       # stable: equal scores keep the candidate order
        if len(cands) > K:
            gap = _gap(cands[K - 1][0], cands[K][0], gap)
        beam = [(p, pb, pnb) for (_, p, pb, pnb) in cands[:K]]
        for a, b in zip(cands[:K], cands[1:K]):
            gap = _gap(a[0], b[0], gap)
    return [(p, lse(pb, pnb)) for p, pb, pnb in beam], gap


def decode_batch(scores, K, *args, search=None, **kwargs):
    """scores: a [T,N,C] float32 tensor -> ([beam of sample n], the smallest gap of all samples).  search: the per-sample decode, this
    module's unless beam_lm_spec or beam_lexicon_spec hands in its own; args, kwargs: what that one takes behind K."""
    lp = scores.detach().cpu().float().permute(1, 0, 2).tolist()
    found = [(search or decode)(rows, K, *args, **kwargs) for rows in lp]
    return [b for b, _ in found], min((g for _, g in found), default=math.inf)


def as_arrays(beams, K, T):
    """The layout of qea.ops.ctc_beam_decode: (tokens [N][K][T] with -1 padding, lengths [N][K], scores [N][K]) as nested lists."""
    tokens = [[list(p) + [-1] * (T - len(p)) for p, _ in b] + [[-1] * T] * (K - len(b)) for b in beams]
    lengths = [[len(p) for p, _ in b] + [-1] * (K - len(b)) for b in beams]
    scores = [[s for _, s in b] + [NEG] * (K - len(b)) for b in beams]
    return tokens, lengths, scores


# ---- inputs and the likelihood the scores are measured against, shared by the CPU and the GPU tests
def log_probs(T, N, C, seed, scale=2.0, blank=0):
    """log_softmax of randn * scale with the blank column raised by scale, fp32: CRNN-like rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, N, C, generator=g) * scale
    x[:, :, blank] += scale
    return torch.nn.functional.log_softmax(x, dim=2)


def ctc_log_likelihood(lp, label, blank=0):
    """log p(label | lp [T][C]) in fp64: -ctc_loss, and the sum of the blank column for the empty label."""
    if len(label) == 0:
        return lp[:, blank].double().sum().item()
    T = lp.shape[0]
    nll = torch.nn.functional.ctc_loss(lp.double()[:, None, :], torch.tensor([list(label)]), torch.tensor([T]), torch.tensor([len(label)]),
                                       blank=blank, reduction="none")
    return -nll.item()
