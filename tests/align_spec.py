"""The statement of CTC forced alignment (DESIGN.md "Forced alignment"), written literally: lists, plain loops, Python floats (fp64).
qea/align.py (numpy, vectorised over the states) and csrc/ctc_align.hip are held to it bit for bit, scores included: the recursion is
adds and comparisons only, and every add happens in the order written here.  Kept apart from qea/align.py on purpose."""
import itertools
import math

import numpy as np
import torch

NEG = -math.inf


def to_fp64(x):
    """one fp32 log-prob as the statement reads it: exactly, NaN and +inf as -inf"""
    x = float(x)
    return x if x < math.inf else NEG


def align(lp, label, blank=0):
    """lp: T rows of C numbers (fp32 values), label: L class indices -> dict(score, path [T], first [L], last [L], char_score [L])"""
    T, C = len(lp), len(lp[0])
    label = [int(c) for c in label]
    L = len(label)
    none = dict(score=NEG, path=[-2] * T, first=[-1] * L, last=[-1] * L, char_score=[NEG] * L)
    for c in label:
        if c < 0 or c >= C or c == blank:
            return none
    lp = [[to_fp64(x) for x in row] for row in lp]
    S = 2 * L + 1
    ext = [blank if s % 2 == 0 else label[s >> 1] for s in range(S)]
    skip = [s % 2 == 1 and s >= 3 and label[s >> 1] != label[(s >> 1) - 1] for s in range(S)]
    v = [NEG] * S
    v[0] = lp[0][blank]
    if L >= 1:
        v[1] = lp[0][label[0]]
    back = [[0] * S]
    for t in range(1, T):
        new, kinds = [], []
        for s in range(S):
            candidates = [v[s]]                                # stay, step, skip: in this order
            if s >= 1:
                candidates.append(v[s - 1])
            if skip[s]:
                candidates.append(v[s - 2])
            winner, kind = candidates[0], 0
            for k in range(1, len(candidates)):                # the largest; of equal ones the earliest
                if candidates[k] > winner:
                    winner, kind = candidates[k], k
            new.append(winner + lp[t][ext[s]])
            kinds.append(kind)
        v = new
        back.append(kinds)
    s = S - 1
    if L >= 1 and v[S - 2] > v[S - 1]:                         # S - 1 wins on equality
        s = S - 2
    score = v[s]
    if score == NEG:
        return none
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = (s >> 1) if s % 2 == 1 else -1
        s -= back[t][s]
    first, last, char_score = [], [], []
    for k in range(L):
        steps = [t for t in range(T) if path[t] == k]
        assert steps == list(range(steps[0], steps[-1] + 1))   # contiguous by construction
        acc = lp[steps[0]][label[k]]
        for t in steps[1:]:                                    # ascending
            acc = acc + lp[t][label[k]]
        first.append(steps[0])
        last.append(steps[-1])
        char_score.append(acc)
    return dict(score=score, path=path, first=first, last=last, char_score=char_score)


def align_batch(lp, labels, blank=0, L_max=None):
    """lp: a [T,N,C] fp32 tensor, labels: N lists -> (score float64 [N], path int32 [N,T], first int32 [sum L], last int32 [sum L],
    char_score float64 [sum L]) as numpy arrays in the layout of qea.ops.ctc_align; a label longer than L_max is infeasible"""
    T, N, _ = lp.shape
    rows = lp.permute(1, 0, 2).tolist()
    score, path, first, last, char_score = [], [], [], [], []
    for n in range(N):
        label = labels[n]
        if L_max is not None and len(label) > L_max:
            r = dict(score=NEG, path=[-2] * T, first=[-1] * len(label), last=[-1] * len(label), char_score=[NEG] * len(label))
        else:
            r = align(rows[n], label, blank)
        score.append(r["score"])
        path.append(r["path"])
        first += r["first"]
        last += r["last"]
        char_score += r["char_score"]
    return (np.asarray(score, np.float64), np.asarray(path, np.int32).reshape(N, T), np.asarray(first, np.int32), np.asarray(last, np.int32),
            np.asarray(char_score, np.float64))


def flatten(labels):
    """N lists -> (targets int32, offsets int64 [N+1]) as torch tensors"""
    offsets = [0]
    for l in labels:
        offsets.append(offsets[-1] + len(l))
    return torch.tensor([c for l in labels for c in l], dtype=torch.int32), torch.tensor(offsets, dtype=torch.int64)


def collapse(path_classes, blank):
    out, prev = [], None
    for c in path_classes:
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


def brute_force(lp, label, blank=0):
    """every one of the C^T class paths that collapses to the label, scored by the ascending sequential sum (the association order of the
    recursion) -> (best score, the paths that reach it, as class paths); (-inf, []) when none exists"""
    T, C = len(lp), len(lp[0])
    lp = [[to_fp64(x) for x in row] for row in lp]
    best, argbest = NEG, []
    for classes in itertools.product(range(C), repeat=T):
        if collapse(classes, blank) != list(label):
            continue
        acc = lp[0][classes[0]]
        for t in range(1, T):
            acc = acc + lp[t][classes[t]]
        if acc > best:
            best, argbest = acc, [classes]
        elif acc == best and acc > NEG:
            argbest.append(classes)
    return best, argbest


def log_probs(T, N, C, seed, scale=3.0):
    """[T,N,C] fp32 log-softmax of seeded noise"""
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, N, C, generator=g) * scale, dim=2)


def random_labels(N, C, lo, hi, seed, blank=0, repeats=0.3):
    """N labels of lo..hi classes without the blank; with probability `repeats` a character repeats its predecessor"""
    g = np.random.default_rng(seed)
    classes = [c for c in range(C) if c != blank]
    out = []
    for _ in range(N):
        l = []
        for _ in range(int(g.integers(lo, hi + 1))):
            if l and g.random() < repeats:
                l.append(l[-1])
            else:
                l.append(int(g.choice(classes)))
        out.append(l)
    return out


def bits(a):
    """float64 array -> its bit patterns; every -inf is the same pattern"""
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)
