"""Minibatch-subset pickers — drop-in for the reference's selection_utils.py: same factory keys
(:220-229), same `query(images, labels, num_samples, names) -> (images_sel, labels_sel, idx)` and
`update_cer(batch_cers, names)` protocol, same `.cers` / `.all_cers` attributes.

TopKCERSampler ranks on the GPU (qea_topk_desc_stable: descending CER, ties in ascending index
order) when the images live there; the reference's `torch.argsort(descending=True)` leaves the order
of tied CERs to the sort implementation, this one pins it to the stable order.

The range samplers (rangeCER, uniformEntropy) run their serial picks on the GPU too (qea_spread_pick: one launch, bit-identical to
the host loop) once the minibatch is large enough to pay for a launch and a read-back; QEA_SAMPLER=host keeps the loop.  The
entropies of uniformEntropy come from qea_seq_entropy for CUDA scores: one [B] copy back instead of [T,B,C]."""
import os
import random

import numpy as np
import torch


def calc_entropy(probs, num_classes=95):
    p = probs + 0.000001
    return -(probs * torch.log(p)).sum(dim=1) / torch.log(torch.tensor(float(num_classes)))


def update_entropies(self, crnn_scores, names):
    """The reference's update_entropies (:20-27): the normalised mean entropy of every strip's [T,C] scores into the sampler's table.
    CUDA scores: one launch and one [B] copy back (fp64 evaluation rounded once); CPU tensors: the reference's loop."""
    scores = crnn_scores.detach()
    if scores.is_cuda and scores.dtype == torch.float32 and scores.numel():
        from qea import ops
        ents = ops.seq_entropy(scores).tolist()
    else:
        probs = torch.exp(scores).cpu()
        ents = [calc_entropy(probs[:, i, :]).mean().item() for i in range(probs.shape[1])]
    self.sampler.update_entropies(ents, names)


def _known(names, table):
    return [table[n] for n in names if n in table]


def _desc_stable_topk(values, k, device):
    """indices (CPU LongTensor) of the k largest values, descending, stable."""
    n = len(values)
    if n == 0:
        return torch.zeros(0, dtype=torch.long)
    k = min(k, n)
    keys = torch.tensor(values, dtype=torch.float32)
    if device is not None and device.type == "cuda":
        from qea import ops
        out = torch.empty(k, dtype=torch.int64, device=device)
        ops.topk_desc_stable(keys.to(device), n, k, out)
        return out.cpu()
    # host path for CPU tensors: same total order (value desc, index asc)
    return torch.from_numpy(np.argsort(-keys.numpy(), kind="stable")[:k].astype(np.int64))


# Smallest n * k at which the device pick is taken.  tools/bench_samplers.py (profiles/samplers.json) times the host loop against
# upload + launch + read-back at (n, k) = (20, 19), (64, 60), (512, 486), (2048, 1945): host 0.13 / 0.37 / 3.0 / 13.8 ms, device
# 0.09 / 0.12 / 0.46 / 2.2 ms on an MI355X box.  The device path won at every measured size, so this is the smallest of them; below
# it nothing was measured and the loop stays.
SPREAD_DEVICE_MIN_NK = 20 * 19


def _spread_pick_host(est, pts):
    """the specification: the reference's loop (:52-57, :129-134)"""
    left = est.clone()
    idx = torch.zeros(pts.shape[0], dtype=torch.long)
    for i, p in enumerate(pts):
        j = torch.argmin(torch.abs(p - left))
        idx[i] = j
        left[j] = 100
    return idx


def _spread_pick(values, num_samples, rand=None, device=None):
    """The reference's range sampling (:41-57, :122-135): draw `num_samples` points uniformly over
    [min, max] of the estimates and take, without replacement, the sample nearest to each.
    `rand`: a pre-drawn uniform vector in place of torch.rand(num_samples) (tests).  `device`: where the images live; on a CUDA device,
    for finite fp32 inputs of at least SPREAD_DEVICE_MIN_NK estimate-point pairs and unless QEA_SAMPLER=host, the picks run as one
    launch (qea_spread_pick) with the same result bit for bit.  The points are drawn on the host either way."""
    est = torch.tensor(values)
    if est.shape[0] == 0:
        return torch.tensor([], dtype=torch.long)
    pts = (est.max() - est.min()) * (torch.rand(num_samples) if rand is None else rand) + est.min()
    n, k = est.shape[0], pts.shape[0]
    if (device is not None and device.type == "cuda" and os.environ.get("QEA_SAMPLER", "device") != "host" and n * k >= SPREAD_DEVICE_MIN_NK
            and est.dtype == torch.float32 and pts.dtype == torch.float32 and bool(torch.isfinite(est).all()) and bool(torch.isfinite(pts).all())):
        from qea import ops
        if n <= ops.SPREAD_MAX_N and k <= ops.SPREAD_MAX_N:
            return ops.spread_pick(est.to(device), pts.to(device)).cpu()
    return _spread_pick_host(est, pts)


def _device_of(images):
    return images.device if torch.is_tensor(images) else None


class DataSampler:
    def __init__(self, cers=None):
        self.cers = cers if cers is not None else dict()
        self.all_cers = dict()

    def query(self, images, labels, num_samples, names=None):
        raise NotImplementedError

    def update_cer(self, batch_cers, names):
        for name, cer in zip(names, batch_cers):
            if name not in self.cers:
                print(f"Sample not present - {name}")
            self.cers[name] = cer
            self.all_cers.setdefault(name, []).append(cer)

    @staticmethod
    def _take(images, labels, idx):
        return images[idx.to(images.device)], [labels[i] for i in idx.tolist()], idx


class RandomSampler(DataSampler):
    content_free = True     # the pick is a permutation draw: names, estimates and images do not enter

    def query(self, images, labels, num_samples, names=None):
        return self._take(images, labels, torch.randperm(images.shape[0])[:num_samples])


class CerRangeSampler(DataSampler):
    def __init__(self, cers, discount_factor=1):
        super().__init__(cers)
        self.discount_factor = discount_factor

    content_free = True     # the pick depends on names, CERs and RNG draws only

    def query(self, images, labels, num_samples, names):
        return self._take(images, labels, _spread_pick(_known(names, self.cers), num_samples, device=_device_of(images)))


class TopKCERSampler(DataSampler):
    def __init__(self, cers, discount_factor=1):
        super().__init__(cers)
        self.discount_factor = discount_factor

    def query(self, images, labels, num_samples, names):
        # names missing from the dict are skipped BEFORE ranking (reference :146-148), so the returned
        # indices address the compacted list exactly as the reference's do
        idx = _desc_stable_topk(_known(names, self.cers), num_samples, images.device if torch.is_tensor(images) else None)
        return self._take(images, labels, idx)

    content_free = True     # the pick depends on names / CERs only: a trainer may pick first and clean only the picked images

    def query_global(self, images, labels, num_samples_global, names, with_counts=False):
        """Data-parallel form: the reference ranks the WHOLE minibatch (train_nn_area.py:220-225); here the minibatch is sharded
        over the ranks, so the shards' CERs are all-gathered (qea.dist.global_topk: stable descending order, rank-major index
        as the tie-break = the single-process order of the concatenated minibatch) and each rank keeps the winners that live
        in its shard — possibly none.  Returns (images_sel, labels_sel, idx, k_global[, winners per rank])."""
        from qea import dist as qdist
        res = qdist.global_topk(_known(names, self.cers), num_samples_global, with_counts=with_counts)
        imgs, labs, idx = self._take(images, labels, res[0])
        return (imgs, labs, idx) + tuple(res[1:])


class UniformEntropySampler(DataSampler):
    """Range sampling over the CRNN's own uncertainty: the normalised mean entropy of a strip's scores (update_entropies), which
    needs neither black-box queries nor a --cers_ocr_path file.
    A strip without an estimate yet counts as entropy 1.0, the normalised maximum: nothing is known about it.  So the estimate list
    always has one entry per strip and the returned indices address the minibatch itself (the reference's `if name in estimates`
    compaction would index the wrong images as soon as one name is missing; it is not reproduced here).  With every name known the
    picks are exactly the reference's sampleUsingEstimates on the same RNG state.  In a first epoch every estimate is 1.0, every
    drawn point is 1.0 and the pick is the first num_samples strips of the minibatch: deterministic, no warm-up needed."""
    UNKNOWN = 1.0
    content_free = True     # the pick depends on names, entropies and RNG draws only

    def __init__(self, entropies, cers):
        super().__init__(cers)
        self.entropies = entropies if entropies is not None else dict()

    def query(self, images, labels, num_samples, names):
        est = [self.entropies.get(n, self.UNKNOWN) for n in names]
        return self._take(images, labels, _spread_pick(est, num_samples, device=_device_of(images)))

    def update_entropies(self, ents, names):
        for n, e in zip(names, ents):                    # (a first sighting is the normal case here: no "Sample not present" line)
            self.entropies[n] = e


class _GlobalSampler(DataSampler):
    def __init__(self, cers, num_samples):
        super().__init__(cers)
        self.num_samples = num_samples
        self.selected_samplenames = dict()

    def query(self, images, labels, num_samples=-1, names=None):
        idx = torch.tensor([i for i, n in enumerate(names) if n in self.selected_samplenames], dtype=torch.long)
        return self._take(images, labels, idx)


class UniformSamplerGlobal(_GlobalSampler):
    def select_samples(self):
        self.selected_samplenames.clear()
        keys = list(self.cers.keys())
        order = np.argsort(np.array(list(self.cers.values())))
        for split in np.array_split(order, self.num_samples):
            self.selected_samplenames[keys[np.random.choice(split)]] = True


class RandomSamplerGlobal(_GlobalSampler):
    def select_samples(self):
        self.selected_samplenames.clear()
        for name in random.sample(list(self.cers.keys()), self.num_samples):
            self.selected_samplenames[name] = True


_METHODS = {
    "random": RandomSampler,
    "topKCER": TopKCERSampler,
    "uniformCERglobal": UniformSamplerGlobal,
    "randomglobal": RandomSamplerGlobal,
    "rangeCER": CerRangeSampler,
    "uniformEntropy": UniformEntropySampler,
}


def datasampler_factory(sampling_method):
    return _METHODS[sampling_method]
