"""One BatchNorm(+ReLU)(+max-pool) stage of the UNet / CRNN schedules, forward and backward: the only caller of the ops.bn_* wrappers.
It owns which samples form a statistics group (partition: G sequential calls of the reference on consecutive runs of samples are one
pass here, batch statistics per group, running statistics updated once per group in order), how a stage's saved state is laid out
(Stage) and which launch serves a stage (forward / backward)."""
import torch

from . import ops

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def partition(groups, B):
    """groups: an int (equal groups) or a sequence of per-group SAMPLE counts (ragged groups: the strips of several documents in one
    pass, each document its own BatchNorm batch as in the reference's one-document-per-call loop, train_nn_patch.py:318-321)
    -> [(first sample, samples)] of every group of a batch of B."""
    if isinstance(groups, int):
        if groups < 1 or B % groups:
            raise ValueError(f"batch {B} is not a multiple of groups={groups}")
        sizes = [B // groups] * groups
    else:
        sizes = [int(v) for v in groups]
        if sum(sizes) != B or any(v <= 0 for v in sizes):
            raise ValueError(f"group sizes {sizes} do not partition the batch of {B}")
    return [(sum(sizes[:i]), n) for i, n in enumerate(sizes)]


class Stage:
    """What one BatchNorm keeps for its backward: y [B*h*w][C] (the BatchNorm's input), its statistics groups `parts` (see partition;
    the whole batch in eval mode), coef [G,4,C] (rows mean, invstd, scale, shift of every group) and stat64 [G,2,C] (the fp64
    statistics of a train-mode forward that was kept for a backward, else None)."""

    def __init__(self, y, h, w, C, parts, coef, stat64, training):
        self.y, self.h, self.w, self.C, self.parts, self.coef, self.stat64, self.training = y, h, w, C, parts, coef, stat64, training

    @property
    def single(self):
        """one statistics group?"""
        return len(self.parts) == 1

    def rows(self, t, b0, nb, per=None):
        """rows of samples b0 .. b0 + nb of a batch-major tensor (or None) with `per` rows per sample (default: this stage's h * w)"""
        per = per or self.h * self.w
        return t[b0 * per:(b0 + nb) * per] if t is not None else None

    def restricted(self, b0, nb):
        """The stage of samples b0 .. b0 + nb alone: one whole statistics group of a train-mode stage (its coefficients are that
        group's), any run of samples of an eval-mode one (its coefficients do not depend on the batch)."""
        g = self.parts.index((b0, nb)) if self.training else 0
        return Stage(self.rows(self.y, b0, nb), self.h, self.w, self.C, [(0, nb)], self.coef[g:g + 1],
                     self.stat64[g:g + 1] if self.stat64 is not None else None, self.training)

    def producer_sums(self):
        """What conv_igemm(bwd_stats=...) takes to leave the two reductions of this stage's backward with the dgrad that produces its
        `da` (then backward(partials=...)); None where there is no such form: eval mode, several groups, statistics not kept."""
        have = self.training and self.single and self.stat64 is not None
        return (self.y, self.C, self.stat64[0], self.coef[0, 2], self.coef[0, 3]) if have else None


def eval_scale_shift(C, gamma, beta, running_mean, running_var):
    """(scale, shift) of an eval-mode BatchNorm, for a conv epilogue that applies them itself"""
    coef = torch.empty(4, C, device=gamma.device)
    ops.bn_eval_coeff(C, gamma, beta, running_mean, running_var, BN_EPS, None, coef[0], coef[1], coef[2], coef[3])
    return coef[2], coef[3]


def forward(y, out, ldo, h, w, C, gamma, beta, running_mean, running_var, training, parts, keep, amax=None, partials=None, pool=None):
    """y [B*h*w][C] -> BatchNorm -> ReLU -> out (pixel stride ldo), group after group of `parts` (train mode; eval mode is one group).
    keep: the fp64 statistics are kept for a backward.  amax: abs-max slot of out.
    partials = (tensor, blocks) from conv_igemm(want_stats=True): the statistics come from the conv's epilogue, no pass over y (one
    group only: a statistics block of the generic tile may straddle two images).
    pool = (pooled, ldp, kh, kw, its abs-max slot): the kh x kw max-pool of out leaves with the apply in ONE pass.
    -> (Stage, whether the pool left with it)."""
    if not training:
        parts = [(0, sum(nb for _, nb in parts))]
    if partials is not None and len(parts) > 1:
        raise ValueError("statistics from the conv's partials cover the whole batch: one statistics group only")
    coef = torch.empty(len(parts), 4, C, device=y.device)
    stat64 = torch.empty(len(parts), 2, C, device=y.device, dtype=torch.float64) if (training and keep) else None
    st = Stage(y, h, w, C, parts, coef, stat64, training)
    for g, (b0, nb) in enumerate(parts):
        mean, invstd, scale, shift = coef[g]
        yg, s64 = st.rows(y, b0, nb), stat64[g] if stat64 is not None else None
        if not training:
            ops.bn_eval_coeff(C, gamma, beta, running_mean, running_var, BN_EPS, None, mean, invstd, scale, shift)
        elif partials is not None:
            ops.bn_train_stats_from_partials(partials[0], partials[1], nb * h * w, C, gamma, beta, BN_EPS, BN_MOMENTUM, running_mean,
                                             running_var, mean, invstd, scale, shift, s64)
        else:
            ops.bn_train_stats(yg, C, nb * h * w, C, gamma, beta, BN_EPS, BN_MOMENTUM, running_mean, running_var, mean, invstd, scale,
                               shift, s64)
        if pool is not None:
            pooled, ldp, kh, kw, pooled_amax = pool
            ops.bn_apply_pool(yg, C, st.rows(out, b0, nb), ldo, st.rows(pooled, b0, nb, (h // kh) * (w // kw)), ldp, nb, h, w, C, scale,
                              shift, kh, kw, relu=True, amax=amax, pooled_amax=pooled_amax)
        else:
            ops.bn_apply(yg, C, st.rows(out, b0, nb), ldo, nb * h * w, C, scale, shift, relu=True, amax=amax)
    return st, pool is not None


def backward(st, da, ldda, dy, gamma, dgamma, dbeta, amax=None, partials=None, pool=None):
    """BatchNorm(+ReLU) backward of stage st, group after group: da (pixel stride ldda) = the gradient of the stage's output, dy [B*h*w][C]
    receives that of its input; dgamma / dbeta are accumulated into (None: no parameter gradients).  The ReLU mask is recomputed from
    y with the forward's scale / shift: the activation is not re-read.  amax: abs-max slot of dy.
    partials = (tensor, blocks) from conv_igemm(bwd_stats=st.producer_sums()): the two reductions came with da's producer (one group).
    pool = (dpool, lddp, kw): the stage's output also went through a 2 x kw max-pool whose gradient dpool still has to be routed to the
    winners and added to da (da None: it went through the pool only) — done inside the two passes of this backward."""
    for g, (b0, nb) in enumerate(st.parts):
        mean, invstd, scale, shift = st.coef[g]
        rest = dict(accumulate=True, stat64=st.stat64[g] if st.stat64 is not None else None, relu_scale=scale, relu_shift=shift, amax=amax)
        yg, dyg = st.rows(st.y, b0, nb), st.rows(dy, b0, nb)
        if pool is not None:
            dpool, lddp, kw = pool
            ops.bn_bwd_pool(st.rows(da, b0, nb), ldda, st.rows(dpool, b0, nb, (st.h // 2) * (st.w // kw)), lddp, kw, yg, st.C, nb, st.h, st.w,
                            st.C, gamma, mean, invstd, st.training, dgamma, dbeta, dyg, st.C, **rest)
        else:
            ops.bn_bwd(st.rows(da, b0, nb), ldda, None, 0, yg, st.C, nb * st.h * st.w, st.C, gamma, mean, invstd, st.training, dgamma, dbeta,
                       dyg, st.C, partials=partials, **rest)
