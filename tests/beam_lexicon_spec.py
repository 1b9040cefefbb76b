"""The automaton-constrained search of DESIGN.md ("Automaton-constrained search"), written out literally in fp64 Python floats as an
extension of tests/beam_spec.py: lists only, linear searches (over the beam and over a state's edges), the candidates built in the
order the specification names them, a stable sort.  Independent of qea/beam.py and qea/lexicon.py (which it checks) and of the device
kernel.  Like beam_spec.decode it reports the smallest non-zero gap between two scores whose order decided something.

An automaton is the tuple (first, label, child, final) of plain lists: the CSR form of the specification."""
import math
import random

import torch

import beam_spec

NEG = -math.inf
lse, _gap = beam_spec.lse, beam_spec._gap


def edge_child(aut, state, c, C, blank):
    """The child of the edge labelled c out of `state`, None when there is none.  An edge whose label is the blank or outside 0..C-1,
    or whose child is outside 0..S-1, is absent; the values of `first` are clamped to 0..E."""
    first, label, child = aut[0], aut[1], aut[2]
    S, E = len(first) - 1, len(label)
    if c == blank or not 0 <= c < C:
        return None
    lo, hi = min(max(first[state], 0), E), min(max(first[state + 1], 0), E)
    for e in range(lo, hi):
        if label[e] == c and 0 <= child[e] < S:
            return child[e]
    return None


def decode(lp, K, aut, blank=0):
    """lp: T rows of C float32 values -> (beam, gap): beam = [(prefix tuple, score, state)] best first, at most K entries; gap as in
    beam_spec.decode."""
    T, C = len(lp), len(lp[0])
    beam = [((), 0.0, NEG, 0)]                                          # (prefix, pb, pnb, state)
    gap = math.inf
    for t in range(T):
        row = [float(v) for v in lp[t]]
        row = [NEG if v != v else v for v in row]
        tot = [lse(pb, pnb) for _, pb, pnb, _ in beam]
        stay_pb = [tot[i] + row[blank] for i in range(len(beam))]
        stay_pnb = [(beam[i][2] + row[beam[i][0][-1]]) if beam[i][0] else NEG for i in range(len(beam))]
        ext = []
        for i, (p, pb, pnb, st) in enumerate(beam):
            for c in range(C):
                if c == blank:
                    continue
                nxt = edge_child(aut, st, c, C, blank)
                if nxt is None:                                         # the slot does not exist
                    continue
                v = (pb if (p and c == p[-1]) else tot[i]) + row[c]
                q = p + (c,)
                j = None
                for jj in range(len(beam)):
                    if beam[jj][0] == q:
                        j = jj
                if j is None:
                    ext.append((i, v, q, nxt))
                else:
                    stay_pnb[j] = lse(stay_pnb[j], v)                   # the same prefix: the same state
        cands = []
        for i, (p, _, _, st) in enumerate(beam):
            cands.append((lse(stay_pb[i], stay_pnb[i]), p, stay_pb[i], stay_pnb[i], st))
            cands.extend((v, q, NEG, v, nxt) for (ii, v, q, nxt) in ext if ii == i)
        cands = [c for c in cands if c[0] > NEG]
        cands.sort(key=lambda c: -c[0])                                 # stable: equal scores keep the candidate order
        if len(cands) > K:
            gap = _gap(cands[K - 1][0], cands[K][0], gap)
        for a, b in zip(cands[:K], cands[1:K]):
            gap = _gap(a[0], b[0], gap)
        beam = [c[1:] for c in cands[:K]]
    return [(p, lse(pb, pnb), st) for p, pb, pnb, st in beam], gap


def decode_batch(scores, K, aut, blank=0):
    """scores: a [T,N,C] float32 tensor -> ([beam of sample n], the smallest gap of all samples)."""
    return beam_spec.decode_batch(scores, K, aut, blank, search=decode)


def as_arrays(beams, K, T):
    """The layout of qea.ops.ctc_beam_decode_dfa as nested lists: (tokens [N][K][T], lengths [N][K], scores [N][K], states [N][K])."""
    tokens, lengths, scores = beam_spec.as_arrays([[(p, s) for p, s, _ in b] for b in beams], K, T)
    states = [[st for _, _, st in b] + [-1] * (K - len(b)) for b in beams]
    return tokens, lengths, scores, states


# ---- automata
def trie(words):
    """The trie of `words` (tuples of classes; duplicates merge, empty ones are skipped) in CSR form, states numbered breadth first with
    each state's edges by ascending class -> (first, label, child, final)."""
    kids, final = [{}], [0]
    for w in words:
        s = 0
        for c in w:
            if c not in kids[s]:
                kids[s][c] = len(kids)
                kids.append({})
                final.append(0)
            s = kids[s][c]
        if len(w):
            final[s] = 1
    order, number = [0], {0: 0}                                        # insertion numbering -> breadth-first numbering
    for s in order:
        for c in sorted(kids[s]):
            number[kids[s][c]] = len(order)
            order.append(kids[s][c])
    first, label, child = [0], [], []
    for s in order:
        for c in sorted(kids[s]):
            label.append(c)
            child.append(number[kids[s][c]])
        first.append(len(label))
    return first, label, child, [final[s] for s in order]


def accept_all(C, blank=0):
    """One state that loops on every non-blank class: the plain search."""
    classes = [c for c in range(C) if c != blank]
    return [0, len(classes)], classes, [0] * len(classes), [1]


def random_lexicon(C, blank, n_words, max_len, seed):
    """n_words words (tuples of non-blank classes) of 1..max_len tokens, seeded; duplicates may occur (the trie merges them)."""
    rng = random.Random(seed)
    classes = [c for c in range(C) if c != blank]
    return [tuple(rng.choice(classes) for _ in range(rng.randint(1, max_len))) for _ in range(n_words)]


def accepts(aut, prefix, C, blank=0):
    """Whether `prefix` is a path from state 0 that ends in an accepting state; (is a path, accepted)."""
    s = 0
    for c in prefix:
        s = edge_child(aut, s, c, C, blank)
        if s is None:
            return False, False
    return True, bool(aut[3][s])


def drop_malformed(aut, C, blank=0):
    """The automaton without the edges the specification calls absent (`first` must be well formed)."""
    first, label, child, final = aut
    S = len(first) - 1
    nf, nl, nc = [0], [], []
    for s in range(S):
        for e in range(first[s], first[s + 1]):
            if label[e] != blank and 0 <= label[e] < C and 0 <= child[e] < S:
                nl.append(label[e])
                nc.append(child[e])
        nf.append(len(nl))
    return nf, nl, nc, list(final)


def with_malformed_edges(aut, C):
    """blank = 0: state 0 gains an edge labelled with the blank in front of its edges and one labelled C behind them (both to state
    1), and the last edge of the first later state that has one gets the child S.  Three edges that are absent; the labels still
    ascend within every state."""
    first, label, child, final = aut
    S, d0 = len(final), first[1]
    label = [0] + label[:d0] + [C] + label[d0:]
    child = [1] + child[:d0] + [1] + child[d0:]
    first = [0] + [f + 2 for f in first[1:]]
    s = next(s for s in range(1, S) if first[s + 1] > first[s])
    child[first[s + 1] - 1] = S
    return first, label, child, list(final)


def tensors(aut):
    """(first, label, child) as int32 tensors; label / child hold one unused element when there is no edge (a non-null pointer)."""
    first, label, child, _ = aut
    return (torch.tensor(first, dtype=torch.int32), torch.tensor(label or [0], dtype=torch.int32), torch.tensor(child or [0], dtype=torch.int32))
