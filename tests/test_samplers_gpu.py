"""csrc/sampling.hip on the device: qea_spread_pick against the host loop (index equality, every routing form), qea_seq_entropy against
an fp64 evaluation and the reference's recorded values, and the area trainer with --minibatch_subset uniformEntropy on the HIP path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "samplers.npz"))


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("QEA_SAMPLER", raising=False)


def _both(est, pts):
    """(device picks, host-loop picks) for fp32 CPU tensors est [n], pts [k]"""
    from qea import ops
    from selection_utils import _spread_pick_host
    got = ops.spread_pick(est.to(DEV), pts.to(DEV))
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == pts.shape
    return got.cpu().tolist(), _spread_pick_host(est, pts).tolist()


def _points(est, k, seed):
    g = torch.Generator().manual_seed(seed)
    return (est.max() - est.min()) * torch.rand(k, generator=g) + est.min()


def _estimates(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) ** 2


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025, 2048])
def test_spread_pick_equals_the_host_loop(n):
    est = _estimates(n, 10 + n)
    for k in sorted({k for k in (1, n - 1, n, n + 3) if k >= 1}):
        got, want = _both(est, _points(est, k, 1000 + k))
        assert got == want, (n, k)
        if k > n:
            assert got[n:] == [0] * (k - n)                                      # every estimate is the sentinel: index 0 repeats


def test_spread_pick_just_above_every_routing_boundary():
    """1537: four waves; 24577: sixteen waves, left in LDS; 32769: left in the workspace (and 32768, the largest LDS form)"""
    from qea import _lib, ops
    assert (ops.SPREAD_WAVE_MAX_N, ops.SPREAD_LDS4_MAX_N, ops.SPREAD_LDS_MAX_N) == (1536, 24576, 32768)
    for n, ks in ((ops.SPREAD_WAVE_MAX_N + 1, (1, 1540)), (ops.SPREAD_LDS4_MAX_N + 1, (1, 61)), (ops.SPREAD_LDS_MAX_N, (1, 61)),
                  (ops.SPREAD_LDS_MAX_N + 1, (1, 61)), (ops.SPREAD_LDS_MAX_N + 4103, (33,))):
        assert (_lib.lib().qea_spread_pick_workspace_bytes(n) > 0) == (n > ops.SPREAD_LDS_MAX_N)
        est = _estimates(n, n)
        est[-1] = -0.5                                                            # the last element (the ragged chunk) is a certain pick
        for k in ks:
            pts = _points(est, k, n + k)
            pts[0] = -0.5
            got, want = _both(est, pts)
            assert got == want and got[0] == n - 1, (n, k)


def test_spread_pick_ties_take_the_lowest_index():
    est = torch.tensor([.25, .75, .25])
    got, want = _both(est, torch.tensor([.5, .5, .5]))
    assert got == want == [0, 1, 2]
    # duplicates: many exactly equal estimates, every pick a tie between them
    est = torch.round(_estimates(300, 5) * 8) / 8
    got, want = _both(est, _points(est, 300, 6))
    assert got == want
    # a tie across every lane and every wave: equal distances everywhere, the picks walk the indices in order (one-, four- and sixteen-wave forms)
    for n in (700, 2500, 25000):
        est = torch.full((n,), .25)
        est[1::2] = .75
        got, want = _both(est, torch.full((90,), .5))
        assert got == want == list(range(90)), n


def test_spread_pick_keeps_the_reference_sentinel():
    est = torch.tensor([0.3, 100.0, 0.1, 150.0, 0.7, 99.5, 0.2, 0.9, 100.0, 0.5])
    for k in (4, 10, 13):
        got, want = _both(est, _points(est, k, k))
        assert got == want, k
    got, want = _both(est, torch.tensor([100.0, 100.0, 100.0, 100.0, 120.0, 160.0]))
    assert got == want and got[:4] == [1, 1, 1, 1]                              # an estimate equal to the sentinel stays eligible


def test_spread_pick_reference_cases(golden):
    from selection_utils import _spread_pick
    for i, tag in enumerate(golden["pick_tags"].tolist()):
        est, rand = torch.from_numpy(golden[f"pick{i}_est"]), torch.from_numpy(golden[f"pick{i}_rand"])
        pts = (est.max() - est.min()) * rand + est.min()
        got, want = _both(est, pts)
        assert got == want == golden[f"pick{i}_idx_range"].tolist(), tag
    # through the routed entry point, at a size that takes the device path
    from qea import ops
    est = _estimates(512, 3)
    rand = torch.rand(486, generator=torch.Generator().manual_seed(4))
    before = ops.SAMPLER_LAUNCHES["spread"]
    routed = _spread_pick(est.tolist(), 486, rand=rand, device=DEV)
    assert ops.SAMPLER_LAUNCHES["spread"] == before + 1 and routed.device.type == "cpu"
    assert routed.tolist() == _spread_pick(est.tolist(), 486, rand=rand).tolist()


def _fp64_entropy(lp):
    p = np.exp(lp.astype(np.float64))
    return (-(p * np.log(p + 0.000001)).sum(axis=2)).mean(axis=0) / np.log(95.0)


def _assert_one_ulp(got, want64, what):
    got = got.astype(np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want64)
    print(f"\n[gate] seq_entropy {what}: worst error {err.max():.2e}, in ulps {np.max(err / ulp):.2f} (bound 1)")
    assert (err <= ulp).all(), what


@pytest.mark.parametrize("shape", [(1, 1, 95), (7, 5, 95), (31, 65, 95)])
def test_seq_entropy_within_one_ulp_of_fp64(shape):
    from qea import ops
    T, B, C = shape
    g = torch.Generator().manual_seed(T * 100 + B)
    wide = torch.zeros(T, B, 96)
    wide[:, :, :C] = torch.log_softmax(torch.randn(T, B, C, generator=g) * torch.linspace(0.05, 6, B)[None, :, None], dim=2)
    scores = wide.to(DEV)[:, :, :C]                                              # 96-column rows, as the CRNN's
    assert scores.stride() == (B * 96, 96, 1)
    out = ops.seq_entropy(scores)
    assert out.shape == (B,) and out.dtype == torch.float32 and out.is_cuda
    want = _fp64_entropy(wide[:, :, :C].numpy())
    _assert_one_ulp(out.cpu().numpy(), want, f"{shape}")
    if B >= 5:
        sl = ops.seq_entropy(scores[:, 2:5, :])                                  # the patch trainer's per-document slices
        _assert_one_ulp(sl.cpu().numpy(), want[2:5], f"{shape} slice")
        assert torch.equal(sl, out[2:5])


def test_seq_entropy_minus_infinity_contributes_zero():
    from qea import ops
    g = torch.Generator().manual_seed(8)
    lp = torch.log_softmax(torch.randn(7, 6, 95, generator=g) * 3, dim=2)
    lp[:, 0, 5:] = float("-inf")
    lp[3, 2, :] = float("-inf")
    lp[:, 4, :] = float("-inf")                                                   # an all-zero distribution: entropy 0, not NaN
    out = ops.seq_entropy(lp.to(DEV)).cpu().numpy()
    assert np.isfinite(out).all() and out[4] == 0.0
    with np.errstate(divide="ignore"):
        _assert_one_ulp(out, _fp64_entropy(lp.numpy()), "-inf rows")


def test_seq_entropy_reference_values(golden):
    """against the reference's own fp32 numbers: within the distance the fixture records between the reference and fp64, plus one ulp"""
    import types
    from qea import ops
    from selection_utils import UniformEntropySampler, update_entropies
    lp = torch.from_numpy(golden["ent_lp"])
    out = ops.seq_entropy(lp.to(DEV)).cpu().numpy()
    _assert_one_ulp(out, golden["ent_fp64"], "fixture")
    ulp = np.spacing(np.abs(golden["ent_ref32"])).astype(np.float64)
    err = np.abs(out.astype(np.float64) - golden["ent_ref32"].astype(np.float64))
    print(f"\n[gate] seq_entropy vs the reference's fp32 values: worst {err.max():.2e} (recorded reference-to-fp64 distance {float(golden['ent_ref_dist']):.2e})")
    assert (err <= float(golden["ent_ref_dist"]) + ulp).all()
    # update_entropies routes CUDA scores through the kernel: one launch, the same values in the sampler's table
    s = UniformEntropySampler({}, {})
    names = [f"s{j}" for j in range(5)]
    before = ops.SAMPLER_LAUNCHES["entropy"]
    update_entropies(types.SimpleNamespace(sampler=s), lp.to(DEV), names)
    assert ops.SAMPLER_LAUNCHES["entropy"] == before + 1
    assert [s.entropies[n] for n in names] == out.astype(np.float64).tolist()


def _run_area(tmp, tag, monkeypatch, host):
    import selection_utils as su
    from qea import ops
    from qea.cli_flags import build_parser
    from train_nn_area import TrainNNPrep
    args = build_parser("a", "").parse_args(["--exp_base_path", str(tmp / tag), "--ocr", "stub", "--epoch", "2", "--synthetic_size", "16",
                                             "--batch_size", "8", "--minibatch_subset", "uniformEntropy", "--minibatch_subset_prop", "0.5"])
    if host:
        monkeypatch.setenv("QEA_SAMPLER", "host")
    else:
        monkeypatch.delenv("QEA_SAMPLER", raising=False)
        monkeypatch.setattr(su, "SPREAD_DEVICE_MIN_NK", 1)                        # 8 strips x 4 picks are below the routing threshold: take the kernel anyway
    t = TrainNNPrep(args)
    assert t.device.type == "cuda"
    rec, orig = [], t.sampler.query

    def spy(images, labels, k, names):
        state = torch.get_rng_state()
        rand = torch.rand(k)
        torch.set_rng_state(state)
        out = orig(images, labels, k, names)
        rec.append(dict(names=list(names), table=dict(t.sampler.entropies), k=k, rand=rand, idx=out[2].tolist()))
        return out
    t.sampler.query = spy
    launches = dict(ops.SAMPLER_LAUNCHES)
    t.train()
    used = {k: ops.SAMPLER_LAUNCHES[k] - v for k, v in launches.items()}
    return t, rec, used


def test_area_trainer_uniform_entropy_on_the_hip_path(tmp_path, monkeypatch):
    import json
    from selection_utils import _spread_pick
    t, rec, used = _run_area(tmp_path, "dev", monkeypatch, host=False)
    assert used == {"spread": 4, "entropy": 4}                                   # 2 epochs x 2 minibatches: one pick and one entropy launch each
    assert len(rec) == 4 and all(r["k"] == 4 and len(r["names"]) == 8 for r in rec)
    for r in rec[:2]:                                                             # epoch 0: nothing known -> the first k strips
        assert not (set(r["names"]) & set(r["table"])) and r["idx"] == [0, 1, 2, 3]
    for r in rec[2:]:                                                             # epoch 1: the host specification on the recorded table and draws
        assert set(r["names"]) <= set(r["table"])
        assert r["idx"] == _spread_pick([r["table"][n] for n in r["names"]], 4, rand=r["rand"]).tolist()
    table = json.load(open(os.path.join(t.cers_base_path, "entropies.json")))
    assert len(table) == 16 and all(0.0 <= v <= 1.0 for v in table.values())
    t2, rec2, used2 = _run_area(tmp_path, "host", monkeypatch, host=True)
    assert used2 == {"spread": 0, "entropy": 4}
    assert [r["idx"] for r in rec2] == [r["idx"] for r in rec] and [r["names"] for r in rec2] == [r["names"] for r in rec]
