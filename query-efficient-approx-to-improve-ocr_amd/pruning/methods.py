"""Pruning methods with the reference's signatures (pruning/methods.py:5-23): a dict name -> CER in, the kept entries out, in
RANKING order.

`facility_location` is apricot's FacilityLocationSelection(optimizer='naive') on squared-euclidean similarities, written out:

    S[i][j] = M - sum_dd (x[i][dd] - x[j][dd])^2      (terms added in ascending dd; M = the largest squared distance of any pair)
    cur[j] = 0;  pick t = the unpicked i with the largest gain[i] = sum_j max(S[i][j], cur[j]), the LOWEST index on an exact tie;
                 cur[j] = max(cur[j], S[i][j])

backend "hip" runs it on the device (qea.ops.facility_select: S recomputed per pick, never stored), backend "cpu" is the same
definition in plain numpy fp64 (it forms the n x n matrix: 108 MB at the POS set's 3 676 documents).  Both evaluate every TERM with
the same roundings; they differ only in the order of the sum over j.  A value may be a float (the reference) or a list of floats of
one common length d <= 32 (a d-dimensional feature row)."""
import numpy as np


def topk(cer_means, num_samples):
    top_k_cers = sorted(cer_means.items(), key=lambda k: k[1], reverse=True)[:num_samples]
    return {name: cer for name, cer in top_k_cers}


def feature_rows(cer_means):
    """[n][d] float64 array of the dict's values, in the dict's order."""
    vals = list(cer_means.values())
    if not vals:
        raise ValueError("no documents to prune")
    rows = [list(v) if isinstance(v, (list, tuple)) else [v] for v in vals]
    d = len(rows[0])
    if d < 1 or any(len(r) != d for r in rows):
        raise ValueError("every document needs a feature of the same, non-zero length")
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), d)


def squared_distances(a, b):
    """[len(a)][len(b)] direct sums of squared differences, terms added in ascending dimension (as the kernel adds them)."""
    dist = np.zeros((a.shape[0], b.shape[0]))
    for dd in range(a.shape[1]):
        df = a[:, dd][:, None] - b[:, dd][None, :]
        dist += df * df
    return dist


def facility_select_cpu(x, k):
    """(ranking [k] int32, gains [k] float64) by the definition above; np.argmax returns the first of equal maxima."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    if not 1 <= k <= n:
        raise ValueError(f"k={k} outside 1..n={n}")
    if not np.isfinite(x).all():
        raise ValueError("non-finite feature (NaN or inf)")
    S = squared_distances(x, x)
    S = S.max() - S
    cur = np.zeros(n)
    free = np.ones(n, dtype=bool)
    ranking, gains = np.empty(k, dtype=np.int32), np.empty(k)
    buf = np.empty_like(S)
    for t in range(k):
        g = np.maximum(S, cur[None, :], out=buf).sum(axis=1)
        g[~free] = -np.inf
        w = int(np.argmax(g))
        ranking[t], gains[t] = w, g[w]
        free[w] = False
        np.maximum(cur, S[w], out=cur)
    return ranking, gains


def facility_select_hip(x, k):
    import torch
    from qea import ops
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    ranking, gains = ops.facility_select(torch.from_numpy(x).cuda(), k)
    return ranking.numpy(), gains.numpy()


def _default_backend():
    try:
        import torch
        return "hip" if torch.cuda.is_available() else "cpu"
    except ImportError:
        return "cpu"


def facility_location(cer_means, num_samples, backend=None):
    backend = backend or _default_backend()
    if backend not in ("hip", "cpu"):
        raise ValueError(f"backend {backend!r}: choose hip or cpu")
    x = feature_rows(cer_means)
    ranking, _ = (facility_select_hip if backend == "hip" else facility_select_cpu)(x, num_samples)
    cer_means_itms = list(cer_means.items())
    pruned_cers = dict()
    for idx in ranking:
        img_name, cer = cer_means_itms[int(idx)]
        pruned_cers[img_name] = cer
    return pruned_cers
