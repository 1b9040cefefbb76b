"""The device facility-location selection (csrc/facility.hip, qea.ops.facility_select) against the reference's recorded ranking, a
numpy fp64 replay of its own sequence and the CPU backend; ties, determinism, refusals; the pruner and --pruning_artifact end to end.

Bounds.  Kernel and CPU backend evaluate every term max(M - dist, cur) with the same roundings, so two gains of one candidate differ
only by the order of a sum of n non-negative fp64 terms: relative error <= n * 2**-52 (8.2e-13 at the POS set's n = 3 676)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRUNE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pruning")
PINNED = 138          # picks of cers_pos_FL_10.json that the definition pins; later ones hang on exact ties between different CERs


def _load(name):
    with open(os.path.join(PRUNE_DIR, name)) as f:
        return json.load(f)


def _similarities(x):
    from pruning import methods
    S = methods.squared_distances(x, x)
    return S.max() - S


def _replay(x, ranking, gains, label):
    """Replays the DEVICE's sequence in numpy fp64: at every pick the gains of all candidates given the device's earlier picks.  The
    device's gain must match the replayed gain of its pick and reach the replayed maximum, both to n * 2**-52 relative."""
    n = x.shape[0]
    bound = n * 2.0 ** -52
    S = _similarities(x)
    cur = np.zeros(n)
    free = np.ones(n, dtype=bool)
    buf = np.empty_like(S)
    worst_own, worst_max = 0.0, 0.0
    failures = []
    for t, w in enumerate(ranking):
        w = int(w)
        assert 0 <= w < n and free[w], f"{label}: pick {t} = {w} is out of range or repeated"
        g = np.maximum(S, cur[None, :], out=buf).sum(axis=1)
        best = g[free].max()
        e_own = abs(gains[t] - g[w]) / g[w]
        e_max = abs(gains[t] - best) / best
        worst_own, worst_max = max(worst_own, e_own), max(worst_max, e_max)
        if (e_own > bound or e_max > bound) and len(failures) < 5:
            failures.append((t, w, float(gains[t]), float(g[w]), float(best)))
        free[w] = False
        np.maximum(cur, S[w], out=cur)
    print(f"{label}: n={n} k={len(ranking)} worst |gain - replay(own pick)| {worst_own:.3e}, worst |gain - replay max| {worst_max:.3e}, bound {bound:.3e}")
    assert not failures, f"{label}: (pick, index, device gain, replayed gain of the pick, replayed maximum) {failures}"


def test_full_pos_ranking_against_the_reference_and_its_own_replay():
    from pruning import methods
    cers = _load("cers_pos.json")
    ref = list(_load("cers_pos_FL_10.json"))
    names = list(cers)
    x = methods.feature_rows(cers)
    k = len(cers) - int(len(cers) * (10 / 100))
    assert (len(cers), k, len(ref)) == (3676, 3309, 3309)
    ranking, gains = methods.facility_select_hip(x, k)
    got = [names[int(i)] for i in ranking]
    agree = next((t for t in range(k) if got[t] != ref[t]), k)
    print(f"POS FL ranking: first {agree} names equal the reference's; {sum(a == b for a, b in zip(got, ref))} of {k} positions agree")
    assert got[:PINNED] == ref[:PINNED]
    assert len(set(int(i) for i in ranking)) == k
    _replay(x, ranking, gains, "POS d=1")


# (d, n, k, seed).  The issue's sizes are k = 750 / 750 / 257; at those no seed keeps every pick's relative gap to the runner-up above
# 1e-9 (with n points in the unit cube the gains near a maximum differ by ~n * spacing^2: the FIRST close pick came at pick 1..36 over
# seeds 0..299 for d = 1, 133..276 over seeds 0..39 for d = 8, 37..88 over seeds 0..149 for d = 32; searched on the CPU before any
# device run).  k is the longest run found, the seed the one that gives it; the 1e-9 stands and no pick inside k is skipped.  What
# the cut drops (late picks, k = n, odd n) is covered by the replay test below, which needs no gap.
SEPARATED = [(1, 1500, 36, 228), (8, 1500, 276, 22), (32, 257, 88, 28)]


def _cpu_with_gaps(x, k):
    """CPU-backend ranking and gains + the smallest relative gap between a winner and the best candidate with different features."""
    from pruning import methods
    n = x.shape[0]
    S = _similarities(x)
    cur = np.zeros(n)
    free = np.ones(n, dtype=bool)
    ranking, gains, min_gap = [], [], np.inf
    for _ in range(k):
        g = np.maximum(S, cur[None, :]).sum(axis=1)
        g[~free] = -np.inf
        w = int(np.argmax(g))
        other = free & (x != x[w]).any(axis=1)
        if other.any():
            min_gap = min(min_gap, (g[w] - g[other].max()) / g[w])
        ranking.append(w)
        gains.append(g[w])
        free[w] = False
        np.maximum(cur, S[w], out=cur)
    r2, g2 = methods.facility_select_cpu(x, k)
    assert list(r2) == ranking and list(g2) == gains            # the helper IS the CPU backend, with the gap measured on the way
    return np.asarray(ranking), np.asarray(gains), min_gap


@pytest.mark.parametrize("d,n,k,seed", SEPARATED)
def test_rankings_and_gains_equal_the_cpu_backend(d, n, k, seed):
    from pruning import methods
    x = np.random.default_rng(seed).random((n, d))
    r_cpu, g_cpu, min_gap = _cpu_with_gaps(x, k)
    print(f"d={d} n={n} k={k} seed={seed}: smallest relative gap to a different candidate {min_gap:.3e}")
    assert min_gap > 1e-9                                        # precondition: a mismatch is the kernel's fault, not a coin toss
    r_hip, g_hip = methods.facility_select_hip(x, k)
    assert list(r_hip) == list(r_cpu)
    err = np.abs(g_hip - g_cpu) / g_cpu
    print(f"d={d} n={n}: worst relative gain error {err.max():.3e}, bound {n * 2.0 ** -52:.3e}")
    assert err.max() <= n * 2.0 ** -52


@pytest.mark.parametrize("d,n,seed", [(32, 257, 28), (8, 1500, 22), (1, 1500, 228), (5, 61, 3)])
def test_every_pick_is_a_maximum_of_the_replay_up_to_k_equal_n(d, n, seed):
    """k = n, odd sizes, tiles that end inside a wave: every pick, the last included, must carry the largest replayed gain."""
    from pruning import methods
    x = np.random.default_rng(seed).random((n, d))
    ranking, gains = methods.facility_select_hip(x, n)
    assert sorted(int(i) for i in ranking) == list(range(n))
    _replay(x, ranking, gains, f"random d={d}")


@pytest.mark.parametrize("d,m", [(1, 300), (3, 300), (32, 70)])
def test_ties_go_to_the_lower_index_and_calls_repeat_bit_for_bit(d, m):
    """Every row twice (row i and row i + m: different waves and workgroups): equal features give bit-identical gains, so the
    lower index of each pair is picked first; a second call returns the same ranking and the same gains to the bit."""
    from pruning import methods
    base = np.random.default_rng(11).random((m, d))
    x = np.concatenate([base, base])
    ranking, gains = methods.facility_select_hip(x, 2 * m)
    pos = np.empty(2 * m, dtype=np.int64)
    pos[ranking] = np.arange(2 * m)
    assert sorted(int(i) for i in ranking) == list(range(2 * m))
    assert (pos[:m] < pos[m:]).all(), np.nonzero(pos[:m] >= pos[m:])[0][:8]
    # once one of each pair is in, every remaining candidate adds nothing: all gains equal, index order decides
    assert list(ranking[m:]) == sorted(int(i) for i in ranking[m:])
    r2, g2 = methods.facility_select_hip(x, 2 * m)
    assert list(r2) == list(ranking)
    assert g2.tobytes() == gains.tobytes()


def test_refusals_leave_the_device_usable():
    from pruning import methods
    from qea import ops
    from qea._lib import QeaError
    x = np.random.default_rng(5).random((40, 2))
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(QeaError, match="k=41"):
        ops.facility_select(xd, 41)
    with pytest.raises(QeaError, match="k=0"):
        ops.facility_select(xd, 0)
    with pytest.raises(QeaError, match="d=33"):
        ops.facility_select(torch.zeros(40, 33, dtype=torch.float64, device="cuda"), 4)
    with pytest.raises(QeaError):
        ops.facility_select(xd.float(), 4)                       # fp64 only
    with pytest.raises(QeaError):
        ops.facility_select(torch.from_numpy(x), 4)              # no CPU path behind the binding
    for bad in (float("nan"), float("inf")):
        for dd in (1, 2):
            xb = np.random.default_rng(6).random((40, dd))
            xb[17, dd - 1] = bad
            with pytest.raises(QeaError, match="non-finite"):
                ops.facility_select(torch.from_numpy(xb).cuda(), 4)
    with pytest.raises(QeaError, match="overflows"):
        ops.facility_select(torch.tensor([[1e200], [-1e200], [0.0]], dtype=torch.float64, device="cuda"), 2)
    # the device and the library are as before: a valid call gives the CPU backend's answer
    r_hip, g_hip = ops.facility_select(xd, 5)
    r_cpu, g_cpu = methods.facility_select_cpu(x, 5)
    assert list(r_hip.numpy()) == list(r_cpu)
    assert np.abs(g_hip.numpy() - g_cpu).max() <= 40 * 2.0 ** -52 * g_cpu.max()


def test_pruner_with_the_hip_backend_end_to_end(tmp_path, monkeypatch):
    """prune_dataset.py --backend hip on the POS fixture writes the reference's two files; an artifact pruned on the device is what
    patch_cli.py --pruning_artifact then trains on (--synthetic_size data, the HIP backend)."""
    import properties
    from pruning import prune_dataset
    from qea.cli_flags import build_parser
    from train_nn_patch import TrainNNPrep
    work = tmp_path / "pruning"
    os.makedirs(work)
    monkeypatch.chdir(work)                                      # the reference runs the pruner from pruning/
    cers = _load("cers_pos.json")
    json.dump({f"0_TOTAL_{name}": cer for name, cer in cers.items()}, open(work / "strips_pos.json", "w"))
    pruned = prune_dataset.main(["--dataset", "pos", "--cers_tess_path", str(work / "strips_pos.json"), "--prune_method", "FL", "--prune_prop", "10",
                                 "--backend", "hip"])
    art = work / properties.cer_artifacts_path
    assert sorted(f for f in os.listdir(art) if f.endswith(".json")) == ["cers_pos.json", "cers_pos_FL_10.json"]
    assert json.load(open(art / "cers_pos.json")) == cers
    on_disk = json.load(open(art / "cers_pos_FL_10.json"))
    ref = list(_load("cers_pos_FL_10.json").items())
    assert list(on_disk.items()) == list(pruned.items()) and len(on_disk) == 3309
    assert list(on_disk.items())[:PINNED] == ref[:PINNED]
    # a synthetic training set, pruned on the device, then loaded by the trainer
    from datasets.synthetic import SyntheticPatches
    n_docs = 8
    tr_set = SyntheticPatches(n_docs, seed=1)                    # what TrainNNPrep builds for --synthetic_size 8
    rng = np.random.default_rng(4)
    strips = {}
    for i in range(n_docs):
        _, boxes, name = tr_set[i]
        for s in TrainNNPrep._strip_names([b["label"] for b in boxes], name):
            strips[s] = float(rng.integers(0, 5))
    json.dump(strips, open(work / "strips_syn.json", "w"))
    kept = prune_dataset.main(["--dataset", "pos", "--cers_tess_path", str(work / "strips_syn.json"), "--prune_method", "FL", "--prune_prop", "50",
                               "--backend", "hip"])
    assert len(kept) == 4
    monkeypatch.chdir(tmp_path)                                  # the trainer runs one level up and reads pruning/cer_artifacts/
    args = build_parser("p", "").parse_args(["--exp_base_path", str(tmp_path / "exp"), "--ocr", "stub", "--epoch", "1", "--inner_limit", "1",
                                             "--synthetic_size", str(n_docs), "--pruning_artifact", "cers_pos_FL_50"])
    t = TrainNNPrep(args)
    want = sorted(i for i in range(n_docs) if f"folder1_doc_{i:05d}" in kept)
    assert len(want) == 4
    assert sorted(int(i) for i in t.loader_train.sampler.indices) == want
    assert t.train_set_size == 4
