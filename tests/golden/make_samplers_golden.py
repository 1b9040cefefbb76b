"""Generate tests/golden/samplers.npz by RUNNING THE REFERENCE's selection_utils (CPU torch) — data only, a few KB.

    python tests/golden/make_samplers_golden.py            # needs the reference checkout (QEA_REFERENCE, default /root/reference)

Pick cases `pick<i>_*`: the estimates `est` (fp32), `k`, the uniform vector `rand` that torch.rand(k) draws under the case's seed, and the
indices the reference returns for that seed from CerRangeSampler.query (`idx_range`) and from UniformEntropySampler.query, i.e.
sampleUsingEstimates (`idx_entropy`).  Every name is in the table, so the reference's compaction changes nothing.
Entropy case: log-probs `ent_lp` [7][5][95] (one strip holds -inf entries), the fp32 values the reference's update_entropies hands to
its sampler (`ent_ref32`), the same formula evaluated in fp64 (`ent_fp64`) and the largest distance between the two (`ent_ref_dist`).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("QEA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import selection_utils as ref  # noqa: E402  (reference)


def pick_cases():
    g = np.random.RandomState(7)
    cases = [
        ("small", g.rand(5), 3),
        ("patch", g.rand(20), 19),
        ("wave", g.rand(64), 60),
        ("wave_plus", g.rand(65), 65),
        ("more_than_n", g.rand(30), 33),
        ("duplicates", np.round(g.rand(40) * 5) / 5, 30),
        ("sentinel", np.array([0.3, 100.0, 0.1, 150.0, 0.7, 99.5, 0.2, 0.9, 100.0, 0.5]), 10),
        ("constant", np.full(12, 0.25), 7),
        ("strip_batch", g.rand(300) ** 2, 285),
    ]
    return [(tag, est.astype(np.float32), k) for tag, est, k in cases]


def main():
    out = {}
    tags = []
    for i, (tag, est, k) in enumerate(pick_cases()):
        n = est.shape[0]
        names = [f"s{j}" for j in range(n)]
        table = {nm: float(e) for nm, e in zip(names, est)}
        images, labels = torch.arange(n), [str(j) for j in range(n)]
        torch.manual_seed(100 + i)
        rand = torch.rand(k)
        torch.manual_seed(100 + i)
        _, _, idx_range = ref.CerRangeSampler(dict(table)).query(images, labels, k, names)
        torch.manual_seed(100 + i)
        _, _, idx_entropy = ref.UniformEntropySampler(dict(table), {}).query(images, labels, k, names)
        tags.append(tag)
        out[f"pick{i}_est"] = est
        out[f"pick{i}_k"] = np.int64(k)
        out[f"pick{i}_seed"] = np.int64(100 + i)
        out[f"pick{i}_rand"] = rand.numpy()
        out[f"pick{i}_idx_range"] = idx_range.numpy()
        out[f"pick{i}_idx_entropy"] = idx_entropy.numpy()
    out["pick_tags"] = np.array(tags)

    torch.manual_seed(5)
    lp = torch.log_softmax(torch.randn(7, 5, 95) * 3, dim=2)
    lp[:, 1, :] = torch.log_softmax(torch.randn(7, 95) * 0.1, dim=1)           # a near-uniform strip: entropy close to 1
    lp[2, 3, 10:20] = float("-inf")
    lp[5, 3, 0] = float("-inf")
    got = {}
    holder = types.SimpleNamespace(sampler=types.SimpleNamespace(update_entropies=lambda ents, names: got.update(ents=ents)))
    ref.update_entropies(holder, lp.clone(), [f"s{j}" for j in range(5)])
    ref32 = np.array(got["ents"], dtype=np.float32)
    assert (ref32 == np.array(got["ents"])).all()                             # .item() of fp32 values: nothing lost
    p = np.exp(lp.numpy().astype(np.float64))
    fp64 = (-(p * np.log(p + 0.000001)).sum(axis=2)).mean(axis=0) / np.log(95.0)
    out["ent_lp"] = lp.numpy()
    out["ent_ref32"] = ref32
    out["ent_fp64"] = fp64
    out["ent_ref_dist"] = np.float64(np.abs(ref32.astype(np.float64) - fp64).max())
    path = os.path.join(HERE, "samplers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; reference-to-fp64 distance", out["ent_ref_dist"])


if __name__ == "__main__":
    main()
