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
    """What one BatchNorm keeps for its backward: y [B*h*w][C] (the BatchNorm's input, an Act), its statistics groups `parts` (see
    partition; the whole batch in eval mode), coef [G,4,C] (rows mean, invstd, scale, shift of every group) and stat64 [G,2,C] (the fp64
    statistics of a train-mode forward that was kept for a backward, else None)."""

    def __init__(self, y, h, w, parts, coef, stat64, training):
        self.y, self.h, self.w, self.C, self.parts, self.coef, self.stat64, self.training = y, h, w, y.C, parts, coef, stat64, training

    @property
    def single(self):
        """one statistics group?"""
        return len(self.parts) == 1

    def rows(self, a, b0, nb, per=None):
        """rows of samples b0 .. b0 + nb of a batch-major Act (or None) with `per` rows per sample (default: this stage's h * w); all of
        them: the Act itself"""
        per = per or self.h * self.w
        return a if a is None or (b0 == 0 and nb * per == a.nrows) else a.rows(b0 * per, nb * per)

    def restricted(self, b0, nb):
        """The stage of samples b0 .. b0 + nb alone: one whole statistics group of a train-mode stage (its coefficients are that
        group's), any run of samples of an eval-mode one (its coefficients do not depend on the batch)."""
        g = self.parts.index((b0, nb)) if self.training else 0
        return Stage(self.rows(self.y, b0, nb), self.h, self.w, [(0, nb)], self.coef[g:g + 1],
                     self.stat64[g:g + 1] if self.stat64 is not None else None, self.training)

    def producer_sums(self):
        """What conv_igemm(bwd_stats=...) takes to leave the two reductions of this stage's backward with the dgrad that produces its
        `da` (then backward(partials=...)); None where there is no such form: eval mode, several groups, statistics not kept."""
        have = self.training and self.single and self.stat64 is not None
        return (self.y.t, self.y.ld, self.stat64[0], self.coef[0, 2], self.coef[0, 3]) if have else None


def eval_scale_shift(C, gamma, beta, running_mean, running_var):
    """(scale, shift) of an eval-mode BatchNorm, for a conv epilogue that applies them itself"""
    coef = torch.empty(4, C, device=gamma.device)
    ops.bn_eval_coeff(C, gamma, beta, running_mean, running_var, BN_EPS, None, coef[0], coef[1], coef[2], coef[3])
    return coef[2], coef[3]


def forward(y, out, h, w, gamma, beta, running_mean, running_var, training, parts, keep, partials=None, pool=None):
    """y [B*h*w][C] -> BatchNorm -> ReLU -> out, group after group of `parts` (train mode; eval mode is one group); y and out are Acts,
    out's abs-max slot is filled.  keep: the fp64 statistics are kept for a backward.
    partials = (tensor, blocks) from conv_igemm(want_stats=True): the statistics come from the conv's epilogue, no pass over y (one
    group only: a statistics block of the generic tile may straddle two images).
    pool = (pooled Act, kh, kw): the kh x kw max-pool of out leaves with the apply in ONE pass (and fills pooled's slot).
    -> (Stage, whether the pool left with it)."""
    if not training:
        parts = [(0, sum(nb for _, nb in parts))]
    if partials is not None and len(parts) > 1:
        raise ValueError("statistics from the conv's partials cover the whole batch: one statistics group only")
    C = y.C
    coef = torch.empty(len(parts), 4, C, device=y.t.device)
    stat64 = torch.empty(len(parts), 2, C, device=y.t.device, dtype=torch.float64) if (training and keep) else None
    st = Stage(y, h, w, parts, coef, stat64, training)
    for g, (b0, nb) in enumerate(parts):
        mean, invstd, scale, shift = coef[g]
        yg, og, s64 = st.rows(y, b0, nb), st.rows(out, b0, nb), stat64[g] if stat64 is not None else None
        if not training:
            ops.bn_eval_coeff(C, gamma, beta, running_mean, running_var, BN_EPS, None, mean, invstd, scale, shift)
        elif partials is not None:
            ops.bn_train_stats_from_partials(partials[0], partials[1], nb * h * w, C, gamma, beta, BN_EPS, BN_MOMENTUM, running_mean,
                                             running_var, mean, invstd, scale, shift, s64)
        else:
            ops.bn_train_stats(yg.t, yg.ld, nb * h * w, C, gamma, beta, BN_EPS, BN_MOMENTUM, running_mean, running_var, mean, invstd, scale,
                               shift, s64)
        if pool is not None:
            pooled, kh, kw = pool
            pg = st.rows(pooled, b0, nb, (h // kh) * (w // kw))
            ops.bn_apply_pool(yg.t, yg.ld, og.t, og.ld, pg.t, pg.ld, nb, h, w, C, scale, shift, kh, kw, relu=True, amax=og.amax,
                              pooled_amax=pg.amax)
        else:
            ops.bn_apply(yg.t, yg.ld, og.t, og.ld, nb * h * w, C, scale, shift, relu=True, amax=og.amax)
    return st, pool is not None


def backward(st, da, dy, gamma, dgamma, dbeta, partials=None, pool=None):
    """BatchNorm(+ReLU) backward of stage st, group after group: the Act da = the gradient of the stage's output, the Act dy [B*h*w][C]
    receives that of its input (and its abs-max slot is filled); dgamma / dbeta are accumulated into (None: no parameter gradients).
    The ReLU mask is recomputed from y with the forward's scale / shift: the activation is not re-read.
    partials = (tensor, blocks) from conv_igemm(bwd_stats=st.producer_sums()): the two reductions came with da's producer (one group).
    pool = (dpool Act, kw): the stage's output also went through a 2 x kw max-pool whose gradient dpool still has to be routed to the
    winners and added to da (da None: it went through the pool only) — done inside the two passes of this backward."""
    for g, (b0, nb) in enumerate(st.parts):
        mean, invstd, scale, shift = st.coef[g]
        rest = dict(accumulate=True, stat64=st.stat64[g] if st.stat64 is not None else None, relu_scale=scale, relu_shift=shift, amax=dy.amax)
        yg, dyg, dag = st.rows(st.y, b0, nb), st.rows(dy, b0, nb), st.rows(da, b0, nb)
        if pool is not None:
            dpg = st.rows(pool[0], b0, nb, (st.h // 2) * (st.w // pool[1]))
            ops.bn_bwd_pool(dag.t if dag is not None else None, dag.ld if dag is not None else 0, dpg.t, dpg.ld, pool[1], yg.t, yg.ld, nb, st.h, st.w, st.C, gamma,
                            mean, invstd, st.training, dgamma, dbeta, dyg.t, dyg.ld, **rest)
        else:
            ops.bn_bwd(dag.t, dag.ld, None, 0, yg.t, yg.ld, nb * st.h * st.w, st.C, gamma, mean, invstd, st.training, dgamma, dbeta,
                       dyg.t, dyg.ld, partials=partials, **rest)
