"""CTC prefix beam search on the host: the specification of include/qea_hip.h's qea_ctc_beam_decode (DESIGN.md "CTC prefix beam
search") as a numpy fp64 loop.  It decodes CPU tensors for utils.pred_to_string, and QEA_BEAM=host sends CUDA tensors through it too
(an A/B switch like QEA_SAMPLER=host); the device kernel (csrc/ctc_beam.hip) returns the same beams.

A beam entry is (prefix, pb, pnb, x): the log-probabilities of the prefix over the alignments that end in blank / in non-blank,
and x, what the mode adds to an entry (None in the plain search, (lm, ctx) in the fused one, the state in the constrained one).  The
candidates of a step are laid out as a [live, C] table: row = beam rank, column 0 = the prefix itself, column s >= 1 = the prefix
plus the s-th non-blank class.  Row-major order of that table is the candidate order, and a stable descending sort picks the next
beam, so equal scores keep that order.

With lm_table (qea_ctc_beam_decode_lm, DESIGN.md "Character n-gram fusion") an entry also carries lm, the sum of the fused-table
entries along its prefix, and ctx, the index of its last lm_context tokens (BOS = the blank index on the left).  A second [live, C]
table then holds the RANKING scores, CTC term + lm, and the sort runs on that one; pb / pnb stay pure CTC quantities.

With automaton (qea_ctc_beam_decode_dfa, DESIGN.md "Automaton-constrained search") an entry also carries a state of a deterministic
automaton over the non-blank classes; a column whose class has no edge out of the row's state is -inf, like a folded one, and an
extension takes the edge's child.  Scores are unchanged CTC quantities.
"""
import math
import os

import numpy as np
import torch

from ._lib import QeaError

MAX_K, MAX_C, MAX_T = 32, 256, 512           # the limits of qea_ctc_beam_decode
MAX_LM_CONTEXT, MAX_LM_ENTRIES = 2, 1 << 21  # and of qea_ctc_beam_decode_lm: C ** (context + 1) fp64 table entries, 16 MB
MAX_DFA_EDGES = (1 << 26) - 1                # and of qea_ctc_beam_decode_dfa: K edge lists end to end are counted in an int32
_NEG = -math.inf


def use_host():
    return os.environ.get("QEA_BEAM", "device") == "host"


def lse(a, b):
    if a == _NEG:
        return b
    if b == _NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def check_limits(T, C, K, blank):
    if not 1 <= K <= MAX_K:
        raise QeaError(f"ctc_beam_decode: K={K} outside 1..{MAX_K}")
    if not 2 <= C <= MAX_C:
        raise QeaError(f"ctc_beam_decode: C={C} outside 2..{MAX_C}")
    if not 1 <= T <= MAX_T:
        raise QeaError(f"ctc_beam_decode: T={T} outside 1..{MAX_T}")
    if not 0 <= blank < C:
        raise QeaError(f"ctc_beam_decode: blank={blank} outside 0..{C - 1}")


def check_lm_limits(C, context, table_shape=None):
    """The fused search's own limits; table_shape, where given, must be (C ** context, C)."""
    if not 0 <= context <= MAX_LM_CONTEXT:
        raise QeaError(f"ctc_beam_decode_lm: lm_context={context} outside 0..{MAX_LM_CONTEXT}")
    if C ** (context + 1) > MAX_LM_ENTRIES:
        raise QeaError(f"ctc_beam_decode_lm: a table of C^(m+1) = {C ** (context + 1)} entries, more than {MAX_LM_ENTRIES}")
    if table_shape is not None and tuple(table_shape) != (C ** context, C):
        raise QeaError(f"ctc_beam_decode_lm: the table is {tuple(table_shape)}, not [C**context, C] = {(C ** context, C)}")


def start_context(C, context, blank):
    """ctx(()): the blank, `context` times."""
    return sum(blank * C ** q for q in range(context))


def automaton_edges(automaton, C, blank):
    """automaton: a qea.lexicon.Lexicon, or any object or tuple with first / label / child -> a function state -> {class: child} of the
    edges that exist (DESIGN.md "Automaton-constrained search": a label that is the blank or outside 0..C-1 and a child outside
    0..S-1 make an edge absent, the values of `first` are clamped to 0..E), filled in state by state as the search asks."""
    if isinstance(automaton, (tuple, list)):
        first, label, child = automaton[:3]
    else:
        first, label, child = automaton.first, automaton.label, automaton.child
    first, label, child = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int64) for a in (first, label, child))
    S, E = len(first) - 1, min(len(label), len(child))
    known = {}

    def edges(state):
        if state not in known:
            lo, hi = (int(min(max(first[s], 0), E)) for s in (state, state + 1))
            out = {}
            for c, ch in zip(label[lo:hi].tolist(), child[lo:hi].tolist()):
                if c != blank and 0 <= c < C and 0 <= ch < S and c not in out:
                    out[c] = ch
            known[state] = out
        return known[state]
    return edges


def _refuse_both(lm_table, automaton):
    if lm_table is not None and automaton is not None:
        raise QeaError("ctc_beam_decode: an automaton together with an lm_table is not supported")


def decode_sample(lp, K, blank=0, lm_table=None, lm_context=0, automaton=None):
    """lp [T][C] float32 (numpy) -> [(prefix tuple, score)] of at most K entries, best first.  With lm_table (fp64 numpy
    [C ** lm_context, C]) the search is the fused one and the entries are (prefix tuple, ctc, total).  With automaton (see
    automaton_edges; not together with lm_table) the search is the constrained one and the entries are (prefix tuple, score, state)."""
    T, C = lp.shape
    _refuse_both(lm_table, automaton)
    fused, edges, start = lm_table is not None, None, None                          # start: the mode's part x of the first entry
    if automaton is not None:
        edges = automaton if callable(automaton) else automaton_edges(automaton, C, blank)
        start = 0                                                                   # x = the state
    lp = lp.astype(np.float64)
    lp[np.isnan(lp)] = _NEG
    classes = np.array([c for c in range(C) if c != blank], dtype=np.int64)          # column s of the table holds classes[s - 1]
    column = {int(c): s + 1 for s, c in enumerate(classes)}
    if fused:
        W = np.where(np.isnan(lm_table), _NEG, lm_table)
        mod = C ** lm_context
        start = (0.0, start_context(C, lm_context, blank))                         # x = (lm, ctx)
    beam = [((), 0.0, _NEG, start)]
    for t in range(T):
        row = lp[t]
        live = len(beam)
        rank = {e[0]: j for j, e in enumerate(beam)}
        tot = [lse(pb, pnb) for _, pb, pnb, _ in beam]
        stay_pb = [tot[i] + row[blank] for i in range(live)]
        stay_pnb = [beam[i][2] + row[beam[i][0][-1]] if beam[i][0] else _NEG for i in range(live)]
        table = np.empty((live, C))
        for i, (p, pb, _, x) in enumerate(beam):
            table[i, 1:] = tot[i] + row[classes]
            if p:
                table[i, column[p[-1]]] = pb + row[p[-1]]                          # a repeat of the last token needs a blank between
            if edges is not None:                                                   # a slot without an edge does not exist
                gone = np.ones(C, dtype=bool)
                gone[[column[c] for c in edges(x)]] = False
                gone[0] = False
                table[i, gone] = _NEG
        for j, (p, _, _, _) in enumerate(beam):                                     # an extension that is entry j: fold it into j
            i = rank.get(p[:-1]) if p else None
            if i is not None:
                stay_pnb[j] = lse(stay_pnb[j], float(table[i, column[p[-1]]]))
                table[i, column[p[-1]]] = _NEG
        table[:, 0] = [lse(stay_pb[i], stay_pnb[i]) for i in range(live)]
        if fused:                                                                   # ranking = CTC term + lm', lm' formed first
            lm2 = np.empty((live, C))
            with np.errstate(invalid="ignore"):
                for i, (_, _, _, (lm, ctx)) in enumerate(beam):
                    lm2[i, 0] = lm
                    lm2[i, 1:] = lm + W[ctx, classes]
                flat = (table + lm2).ravel()
        else:
            flat = table.ravel()
        flat[np.isnan(flat)] = _NEG
        order = np.argsort(-flat, kind="stable")[:K]
        nxt = []
        for idx in order.tolist():
            if flat[idx] == _NEG:
                break
            i, s = divmod(idx, C)
            p, _, _, x = beam[i]
            if s == 0:                                                              # a stay keeps the mode's part as it is
                nxt.append((p, stay_pb[i], stay_pnb[i], x))
                continue
            c = int(classes[s - 1])
            if fused:
                x = (float(lm2[i, s]), (x[1] * C + c) % mod)
            elif edges is not None:                                                 # an extension takes the edge
                x = edges(x)[c]
            nxt.append((p + (c,), _NEG, float(table[i, s]), x))
        beam = nxt
    out = []
    for p, pb, pnb, x in beam:
        score = lse(pb, pnb)
        out.append((p, score) + (() if x is None else (score + x[0],) if fused else (x,)))
    return out


def ctc_beam_decode(scores, K, blank=0, lm_table=None, lm_context=0, automaton=None):
    """scores [T,N,C] float32 (any device) -> (tokens int32 [N,K,T], lengths int32 [N,K], scores float64 [N,K]) on the CPU, in the
    layout of qea.ops.ctc_beam_decode: -1 behind every prefix, length -1 and score -inf in the rows beyond the live count.
    With lm_table (a float64 tensor or array [C ** lm_context, C]): the fused search, in the layout of qea.ops.ctc_beam_decode_lm,
    (tokens, lengths, ctc float64 [N,K], total float64 [N,K]).
    With automaton (a qea.lexicon.Lexicon, or first / label / child as attributes or a tuple; not together with lm_table): the
    constrained search, in the layout of qea.ops.ctc_beam_decode_dfa, (tokens, lengths, scores, states int32 [N,K], -1 beyond the
    live count)."""
    T, N, C = scores.shape
    K, blank, lm_context = int(K), int(blank), int(lm_context)
    check_limits(T, C, K, blank)
    _refuse_both(lm_table, automaton)
    fourth = None                                                                   # the mode's column behind the scores
    if automaton is not None:
        automaton = automaton_edges(automaton, C, blank)
        fourth = np.full((N, K), -1, dtype=np.int32)
    if lm_table is not None:
        check_lm_limits(C, lm_context, tuple(lm_table.shape))
        if torch.is_tensor(lm_table):
            lm_table = lm_table.detach().to("cpu", torch.float64).numpy()
        lm_table = np.asarray(lm_table, dtype=np.float64)
        fourth = np.full((N, K), _NEG, dtype=np.float64)
    elif lm_context:
        raise QeaError("ctc_beam_decode: lm_context without an lm_table")
    lp = scores.detach().to("cpu", torch.float32).numpy()
    tokens = np.full((N, K, T), -1, dtype=np.int32)
    lengths = np.full((N, K), -1, dtype=np.int32)
    out = np.full((N, K), _NEG, dtype=np.float64)
    for n in range(N):
        for k, (p, s, *x) in enumerate(decode_sample(lp[:, n, :], K, blank, lm_table, lm_context, automaton)):
            tokens[n, k, :len(p)] = p
            lengths[n, k], out[n, k] = len(p), s
            if x:
                fourth[n, k] = x[0]
    return tuple(torch.from_numpy(a) for a in (tokens, lengths, out, fourth) if a is not None)
