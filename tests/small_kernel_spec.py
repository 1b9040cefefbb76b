"""Plain numpy / Python statements of the small kernels of csrc/ctc.hip and csrc/misc.hip: the CTC loss and gradient, the greedy
decode's argmax, Philox4x32-10 with the jitter kernel's Box-Muller, and one Adam step.  Each is written for reading, not for speed,
and imports nothing of the library it checks.  tests/test_small_kernels_cpu.py holds them to a brute force, to torch in double, to
the published Random123 answers and to oracle/path_oracle.py; tests/test_small_kernels_gpu.py holds the kernels to them.

The input builders at the end are shared by the two test files, so that the CPU tests speak about the very data the device sees."""
import collections
import itertools
import math

import numpy as np

NEG = -np.inf


# ----------------------------------------------------------------------------- CTC
def ctc_bruteforce(lp, target, Tn, blank):
    """nll of `target` under lp [>= Tn][C] by enumerating all C^Tn paths, collapsing each (merge repeats, drop blanks) and adding
    the probabilities of those that spell the target.  fp64, Tn <= 6 and C <= 4.  No path: +inf (also for Tn <= 0)."""
    lp = np.asarray(lp, dtype=np.float64)
    C = lp.shape[1]
    assert Tn <= 6 and C <= 4
    if Tn <= 0:
        return math.inf
    target = tuple(int(c) for c in target)
    terms = []
    for path in itertools.product(range(C), repeat=Tn):
        merged = [c for i, c in enumerate(path) if i == 0 or c != path[i - 1]]
        if tuple(c for c in merged if c != blank) == target:
            terms.append(math.exp(math.fsum(lp[t, c] for t, c in enumerate(path))))
    p = math.fsum(terms)
    return -math.log(p) if p > 0 else math.inf


def _lse(*xs):
    """log-sum-exp of equally shaped arrays in their own dtype; -inf where all are -inf"""
    m = xs[0]
    for x in xs[1:]:
        m = np.maximum(m, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.exp(xs[0] - m)
        for x in xs[1:]:
            acc = acc + np.exp(x - m)
        r = m + np.log(acc)
    return np.where(np.isneginf(m), m, r)


def ctc_spec(lp, target, Tn, blank, dtype=np.float64):
    """One sample.  lp [T][C] log-probs, target: L class indices, Tn: the input length (the caller clamps it to T).
    -> (nll, grad [T][C]), every operation in `dtype` (float64: the statement; float32: the same recursion as a plain fp32
    implementation would run it).  With l' the target with a blank around every character, S = 2L + 1 states:
        alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s is no blank and differs from l'_{s-2}]) + lp[t, l'_s]
        beta likewise from the end;  nll = -lse(alpha_{Tn-1}(S-1), alpha_{Tn-1}(S-2))
        grad[t, c] = exp(lp) - exp(lse_{s: l'_s = c}(alpha_t(s) + beta_t(s)) + nll - lp)      (header of csrc/ctc.hip)
    Rows t >= Tn are zero.  Tn <= 0: nll = +inf and an all-zero gradient.  An infeasible target: nll = +inf and, the formula being
    -inf + inf there, NaN rows for t < Tn.  A -inf log-prob gives NaN wherever the formula does."""
    lp = np.asarray(lp).astype(dtype)
    T, C = lp.shape
    grad = np.zeros((T, C), dtype=dtype)
    if Tn <= 0:
        return dtype(np.inf), grad
    L = len(target)
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    skip = np.zeros(S, dtype=bool)                       # state s may be entered from s - 2
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = dtype(NEG)

    def shifted(a, k):                                   # a[s - k], -inf in front
        return np.concatenate([np.full(k, ninf, dtype=dtype), a[:S - k]]) if S > k else np.full(S, ninf, dtype=dtype)

    alpha = np.full((Tn, S), ninf, dtype=dtype)
    alpha[0, 0] = lp[0, blank]
    if S > 1:
        alpha[0, 1] = lp[0, ext[1]]
    for t in range(1, Tn):
        a = alpha[t - 1]
        alpha[t] = _lse(a, shifted(a, 1), np.where(skip, shifted(a, 2), ninf)) + lp[t, ext]
    ll = alpha[Tn - 1, S - 1] if S == 1 else _lse(alpha[Tn - 1, S - 1], alpha[Tn - 1, S - 2])
    nll = dtype(-ll)

    beta = np.full((Tn, S), ninf, dtype=dtype)
    beta[Tn - 1, S - 1] = lp[Tn - 1, blank]
    if S > 1:
        beta[Tn - 1, S - 2] = lp[Tn - 1, ext[S - 2]]
    skip_to = np.zeros(S, dtype=bool)                    # state s may leave for s + 2
    skip_to[:S - 2] = skip[2:]
    for t in range(Tn - 2, -1, -1):
        b = beta[t + 1]
        b1 = shifted(b[::-1], 1)[::-1]
        b2 = np.where(skip_to, shifted(b[::-1], 2)[::-1], ninf)
        beta[t] = _lse(b, b1, b2) + lp[t, ext]

    res = np.full((Tn, C), ninf, dtype=dtype)
    ab = alpha + beta
    for s in range(S):
        res[:, ext[s]] = _lse(res[:, ext[s]], ab[:, s])
    with np.errstate(invalid="ignore", over="ignore"):
        grad[:Tn] = np.exp(lp[:Tn]) - np.exp(res + nll - lp[:Tn])
    return nll, grad


def ctc_batch_spec(lp, labels, in_len, blank, dtype=np.float64):
    """ctc_spec per sample of lp [T][N][C] -> (nll [N], grad [T][N][C]); input lengths are clamped to T as the kernel clamps them"""
    T, N, C = lp.shape
    nll = np.zeros(N, dtype=dtype)
    grad = np.zeros((T, N, C), dtype=dtype)
    for n in range(N):
        nll[n], grad[:, n] = ctc_spec(lp[:, n], labels[n], min(int(in_len[n]), T), blank, dtype)
    return nll, grad


EPS32 = 2.0 ** -24                                       # half an ulp of fp32, relative: one rounding


def gate_ratio(got, ref, gate):
    """largest |got - ref| / gate over the elements where ref is no NaN (0 / 0 counts as 0, x / 0 as inf): <= 1 passes"""
    got, ref, gate = (np.asarray(a, dtype=np.float64) for a in (got, ref, gate))
    ok = ~np.isnan(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(ok & (got != ref), np.abs(got - ref), 0.0)       # equal infinities agree
        r = np.where(err == 0, 0.0, err / gate)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def ctc_grad_gate(ref, roundings=4):
    """the device gate of a gradient [T][N][C]: roundings x 2^-24 x |ref| + 1e-11 x the sample's largest |ref| (the first term: the
    kernel rounds an fp64 evaluation to fp32, after a product with an fp32 grad_out; the second: the summation order of the fp64
    log-sum-exp).  NaN where ref is NaN; an all-NaN sample's zero rows have the gate 0."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    top = np.where(np.isnan(a), 0.0, a).max(axis=(0, 2), keepdims=True)
    return roundings * EPS32 * a + 1e-11 * top


# ----------------------------------------------------------------------------- greedy decode
def argmax_first(row):
    """index of the first NaN of `row` if it has one, otherwise of its first maximum: the rule of torch.argmax and np.argmax"""
    best = None
    for i, v in enumerate(row):
        v = float(v)
        if v != v:
            return i
        if best is None or v > float(row[best]):
            best = i
    return best


def greedy_spec(scores, blank):
    """scores [T][N][C] -> per sample the list of emitted classes: argmax_first per frame, a class is emitted when it is no blank and
    differs from the previous frame's class.  The first emitted class never looks at the previous frame (utils.py's quirk, which can
    show only where the previous class was the blank, so it changes nothing)."""
    T, N, _ = scores.shape
    out = []
    for n in range(N):
        toks, prev = [], None
        for t in range(T):
            k = argmax_first(scores[t, n])
            if k != blank and (not toks or k != prev):
                toks.append(k)
            prev = k
        out.append(toks)
    return out


# ----------------------------------------------------------------------------- Philox4x32-10 and the jitter noise
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123).  counter: 4 uint64 arrays (or ints) holding 32-bit words, key: 2
    -> 4 uint64 arrays of 32-bit words."""
    c = [np.asarray(w, dtype=np.uint64) & _LO for w in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return c


def _u01(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in fp32, as the kernel writes it: the sum rounds (to even) above 2^23"""
    return ((x >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def jitter_noise_spec(K, R, HW, sigma, seed, offset, trig_dtype=np.float64):
    """The noise of ops.jitter: -> (z, r), both [R * K][HW] in `trig_dtype`.  Pixel quad q = im * (HW / 4) + i // 4 of image
    im = r * K + k draws Philox4x32-10 at counter (q lo, q hi, offset lo, offset hi) under key (seed lo, seed hi); words (x, y) give
    elements 0 and 1 of the quad, r cos(theta) and r sin(theta) with r = sqrt(-2 log u01(x)), theta = 2 pi u01(y), and words (z, w)
    give elements 2 and 3 likewise; z = that times sigma[im].  u01 and the 2 pi u product are fp32 as in the kernel, sqrt, log, sin
    and cos are evaluated in trig_dtype (float64: the statement; float32: a plain fp32 evaluation, for comparison)."""
    nq = R * K * (HW // 4)
    q = np.arange(nq, dtype=np.uint64)
    w = philox4x32_10((q & _LO, q >> _32, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    sg = np.repeat(np.asarray(sigma, dtype=np.float32).astype(trig_dtype), HW // 4)
    z = np.empty((nq, 4), dtype=trig_dtype)
    rr = np.empty((nq, 4), dtype=trig_dtype)
    for e, (wr, wt) in ((0, (w[0], w[1])), (2, (w[2], w[3]))):
        r = np.sqrt(trig_dtype(-2.0) * np.log(_u01(wr).astype(trig_dtype)))
        th = (np.float32(6.283185307179586) * _u01(wt)).astype(trig_dtype)
        z[:, e], z[:, e + 1] = r * np.cos(th) * sg, r * np.sin(th) * sg
        rr[:, e] = rr[:, e + 1] = r
    return z.reshape(R * K, HW), rr.reshape(R * K, HW)


# ----------------------------------------------------------------------------- Adam
AdamStep = collections.namedtuple("AdamStep", "p m v g_eff update")


def adam_spec(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """One Adam step in fp64 from fp32 (p, g, m, v); `step` is the 1-based count after the increment.  The gradient is scaled first,
    then the L2 term joins it: g_eff = g * grad_scale + weight_decay * p.  -> AdamStep(p, m, v, g_eff, update), p = p_in + update.
    The hyper-parameters are used as given: pass the fp32 values the library's ABI carries."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g_eff = g * grad_scale + weight_decay * p
    m = beta1 * m + (1 - beta1) * g_eff
    v = beta2 * v + (1 - beta2) * g_eff * g_eff
    step_size = lr / (1 - beta1 ** step)
    bc2_sqrt = math.sqrt(1 - beta2 ** step)
    update = -step_size * (m / (np.sqrt(v) / bc2_sqrt + eps))
    return AdamStep(p + update, m, v, g_eff, update)


# ----------------------------------------------------------------------------- shared inputs
def log_softmax64(x):
    """fp64 log-softmax over the last axis of fp32 logits"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def repeats(label):
    return sum(1 for a, b in zip(label, label[1:]) if a == b)


TINY_LABELS = ((), (1,), (1, 1), (1, 2), (1, 2, 1), (1, 1, 2))          # "", a, aa, ab, aba, aab
TINY_TN = (1, 2, 3, 5)
TINY_BLANKS = (0, 2, 3)
TINY_IN_LEN = (6, 5, 3, 1, 0, 11)                                      # at T = 6: 11 clamps to 6, 0 has no frame


def tiny_label(label, blank):
    """the letters a, b as the first two classes that are not the blank"""
    letters = [c for c in range(4) if c != blank]
    return tuple(letters[c - 1] for c in label)


def tiny_log_probs(T, N, seed):
    """fp32 log-probs [T][N][4], the rounding of an fp64 log-softmax"""
    return log_softmax64(np.random.RandomState(seed).randn(T, N, 4).astype(np.float32) * 2).astype(np.float32)


def tiny_batch(blank):
    """every tiny label at every input length of TINY_IN_LEN, and each label once more at exactly L + repeats frames (one path) and at
    one frame fewer (infeasible) -> (labels, in_len); T = 6"""
    labels, in_len = [], []
    for lab in TINY_LABELS:
        for tn in TINY_IN_LEN:
            labels.append(tiny_label(lab, blank))
            in_len.append(tn)
        need = len(lab) + repeats(lab)
        for tn in (need, need - 1):
            if tn >= 1:
                labels.append(tiny_label(lab, blank))
                in_len.append(tn)
    return labels, np.asarray(in_len, dtype=np.int32)


B_T, B_N, B_C = 31, 70, 95


def batch_b(scale, seed=11):
    """The production-like CTC batch: T = 31, N = 70, C = 95, blank 0, label lengths 0 .. 15, some input lengths below T; sample 68 has
    L = 15 with exactly L + repeats frames (one alignment), sample 69 the same frames and one repeat more (infeasible).
    -> (logits fp32 [T][N][C], lp fp32 = the rounded fp64 log-softmax, labels, in_len)"""
    rng = np.random.RandomState(seed)
    logits = (rng.randn(B_T, B_N, B_C) * scale).astype(np.float32)
    labels = [tuple(int(c) for c in rng.randint(1, B_C, n % 16)) for n in range(B_N - 2)]
    in_len = np.full(B_N, B_T, dtype=np.int32)
    in_len[3::7] = B_T - 4
    in_len[5] = B_T + 9                                               # clamps to T
    edge = [int(c) for c in rng.permutation(np.arange(1, B_C))[:15]]
    for i in (2, 5, 6, 9, 12):                                        # five repeats
        edge[i] = edge[i - 1]
    more = list(edge)
    more[14] = more[13]                                               # a sixth
    labels += [tuple(edge), tuple(more)]
    in_len[68] = in_len[69] = 15 + repeats(edge)
    assert repeats(edge) == 5 and repeats(more) == 6
    return logits, log_softmax64(logits).astype(np.float32), labels, in_len


DECODE_T, DECODE_N = 6, 12
DECODE_C = (40, 64, 65, 95, 130)


def decode_rows(C, seed=5):
    """Score rows [6][12][C] for the greedy decode: random frames, and in sample n one frame with the n-th of these (where C has the
    classes for it): 0 a tie of classes 9 and 70 (two lanes), 1 a tie of 3 and 67 (one lane), 2 a NaN at 5, 3 a NaN at 70, 4 NaNs at 64
    and 1, 5 a NaN beside a +inf, 6 an all-NaN frame, 7 an all -inf frame, 8 a +inf, 9 a NaN at 5 in every frame, 10 ties of all
    classes, 11 nothing special.  The special values sit at the classes named when C has them, else at those classes modulo C."""
    rng = np.random.RandomState(seed + C)
    s = rng.randn(DECODE_T, DECODE_N, C).astype(np.float32)
    top = np.float32(7.5)
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def at(c):
        return c % C

    for t in (1, 4):
        s[t, 0, at(9)] = s[t, 0, at(70)] = top
        s[t, 1, at(3)] = s[t, 1, at(67)] = top
        s[t, 2, at(5)] = nan
        s[t, 3, at(70)] = nan
        s[t, 4, at(64)] = s[t, 4, at(1)] = nan
        s[t, 5, at(20)] = inf
        s[t, 5, at(33)] = nan
        s[t, 6, :] = nan
        s[t, 7, :] = -inf
        s[t, 8, at(77)] = inf
    s[2, 5, at(33)] = nan                                             # the NaN before the +inf this time
    s[2, 5, at(38)] = inf
    s[:, 9, at(5)] = nan
    s[:, 10, :] = np.float32(0.25)
    s[3, 10, :] = np.float32(-1.5)
    return s
