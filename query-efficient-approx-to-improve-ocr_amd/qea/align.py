"""CTC forced alignment on the host: the specification of include/qea_hip.h's qea_ctc_align (DESIGN.md "Forced alignment") as a numpy
fp64 loop over the steps, vectorised over the extended states.  It aligns CPU tensors for utils.char_spans, and QEA_ALIGN=host sends CUDA
tensors through it too (an A/B switch like QEA_BEAM=host); the device kernel (csrc/ctc_align.hip) returns the same bits, scores included:
the recursion is fp64 adds and comparisons only.

Given a label l[0..L), the extended states are s = 0..2L: the blank for even s, l[s >> 1] for odd s.  v_t(s) is the best score of a path
that is in state s at step t; a step keeps the state, moves to the next one, or (between two different characters) skips the blank
between them.  The candidates are compared in that order and the first of equal ones wins, so the alignment is unique by definition.
"""
import os

import numpy as np
import torch

from ._lib import QeaError

MAX_T, MAX_C, MAX_L = 512, 256, 127          # the limits of qea_ctc_align
_NEG = -np.inf


def use_host():
    return os.environ.get("QEA_ALIGN", "device") == "host"


def check_limits(T, C, blank, L_max, N=0):
    """What both paths refuse, before any work"""
    if N < 0:
        raise QeaError(f"ctc_align: N={N} is negative")
    if not 1 <= T <= MAX_T:
        raise QeaError(f"ctc_align: T={T} outside 1..{MAX_T}")
    if not 2 <= C <= MAX_C:
        raise QeaError(f"ctc_align: C={C} outside 2..{MAX_C}")
    if not 0 <= blank < C:
        raise QeaError(f"ctc_align: blank={blank} outside 0..{C - 1}")
    if not 0 <= L_max <= MAX_L:
        raise QeaError(f"ctc_align: L_max={L_max} outside 0..{MAX_L}")


def align_sample(lp, label, blank=0):
    """lp [T][C] float32 (numpy), label: L class indices -> (score float, path int32 [T], first int32 [L], last int32 [L],
    char_score float64 [L]); an infeasible sample gives (-inf, all -2, all -1, all -1, all -inf)."""
    T, C = lp.shape
    label = [int(c) for c in label]
    L = len(label)
    none = (_NEG, np.full(T, -2, np.int32), np.full(L, -1, np.int32), np.full(L, -1, np.int32), np.full(L, _NEG))
    if any(c < 0 or c >= C or c == blank for c in label):
        return none
    lp = lp.astype(np.float64)
    lp[~(lp < np.inf)] = _NEG                                                     # NaN and +inf
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = label
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(S, _NEG)
    v[:2] = lp[0, ext[:2]]
    back = np.zeros((T, S), np.int8)
    for t in range(1, T):
        best, kind = v.copy(), back[t]
        padded = np.concatenate(([_NEG, _NEG], v))                                 # cell s + 2 holds v(s)
        step, jump = padded[1:S + 1], np.where(skip, padded[:S], _NEG)
        for k, cand in ((1, step), (2, jump)):                                    # a later candidate wins only when strictly larger
            better = cand > best
            best[better], kind[better] = cand[better], k
        v = best + lp[t, ext]
    s = S - 2 if L >= 1 and v[S - 2] > v[S - 1] else S - 1
    score = float(v[s])
    if score == _NEG:
        return none
    path = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = s >> 1 if s & 1 else -1
        s -= int(back[t, s])
    first, last, char_score = np.empty(L, np.int32), np.empty(L, np.int32), np.empty(L)
    for k in range(L):
        steps = np.flatnonzero(path == k)
        first[k], last[k] = steps[0], steps[-1]
        acc = lp[steps[0], label[k]]
        for t in range(steps[0] + 1, steps[-1] + 1):                              # ascending, one add per step
            acc = acc + lp[t, label[k]]
        char_score[k] = acc
    return score, path, first, last, char_score


def ctc_align(scores, targets, offsets, L_max, blank=0):
    """scores [T,N,C] float32 (any device), targets: the labels end to end, offsets [N+1] -> (score float64 [N], path int32 [N,T], first
    int32 [sum L], last int32 [sum L], char_score float64 [sum L]) on the CPU, in the layout of qea.ops.ctc_align.  A label longer than
    L_max is infeasible, as on the device."""
    T, N, C = scores.shape
    blank, L_max = int(blank), int(L_max)
    check_limits(T, C, blank, L_max, N)
    lp = scores.detach().to("cpu", torch.float32).numpy()
    tg = np.asarray(targets.cpu() if torch.is_tensor(targets) else targets, dtype=np.int64).reshape(-1)
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    if len(off) != N + 1:
        raise QeaError(f"ctc_align: {len(off)} offsets for {N} samples (N + 1 wanted)")
    total = int(off[-1]) if N else 0
    score, path = np.full(N, _NEG), np.full((N, T), -2, np.int32)
    first, last, char_score = np.full(total, -1, np.int32), np.full(total, -1, np.int32), np.full(total, _NEG)
    for n in range(N):
        a, b = int(off[n]), int(off[n + 1])
        if 0 <= b - a <= L_max:
            score[n], path[n], first[a:b], last[a:b], char_score[a:b] = align_sample(lp[:, n, :], tg[a:b], blank)
    return tuple(torch.from_numpy(x) for x in (score, path, first, last, char_score))
