"""The range and entropy samplers on the host: selection_utils._spread_pick against the indices recorded from the reference
(tests/golden/samplers.npz, written by tests/golden/make_samplers_golden.py), UniformEntropySampler's handling of strips without an
estimate, and both trainers running --minibatch_subset uniformEntropy on the CPU oracle backend (test_trainers_cpu.py's fixtures)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from test_trainers_cpu import _args, oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

torch.set_num_threads(4)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "samplers.npz"))


def pick_cases(g):
    for i, tag in enumerate(g["pick_tags"].tolist()):
        yield tag, {k: g[f"pick{i}_{k}"] for k in ("est", "k", "seed", "rand", "idx_range", "idx_entropy")}


def test_spread_pick_reproduces_the_recorded_reference_indices(golden):
    from selection_utils import _spread_pick
    seen = 0
    for tag, c in pick_cases(golden):
        assert (c["idx_range"] == c["idx_entropy"]).all(), tag                    # the reference's two copies of the loop agree
        idx = _spread_pick(c["est"].tolist(), int(c["k"]), rand=torch.from_numpy(c["rand"]))
        assert idx.dtype == torch.int64 and idx.tolist() == c["idx_range"].tolist(), tag
        seen += 1
    assert seen >= 8


def test_seeded_queries_reproduce_the_reference(golden):
    """query() under the recorded seed draws the recorded vector and returns the reference's indices, for both range samplers."""
    from selection_utils import CerRangeSampler, UniformEntropySampler, _spread_pick
    for tag, c in pick_cases(golden):
        n, k = c["est"].shape[0], int(c["k"])
        names = [f"s{j}" for j in range(n)]
        table = {nm: float(e) for nm, e in zip(names, c["est"])}
        images, labels = torch.arange(n), [str(j) for j in range(n)]
        torch.manual_seed(int(c["seed"]))
        assert torch.equal(torch.rand(k), torch.from_numpy(c["rand"])), tag
        for make in (lambda: CerRangeSampler(dict(table)), lambda: UniformEntropySampler(dict(table), {})):
            torch.manual_seed(int(c["seed"]))
            sel, labs, idx = make().query(images, labels, k, names)
            assert idx.tolist() == c["idx_range"].tolist(), tag
            assert sel.tolist() == idx.tolist() and labs == [str(j) for j in idx.tolist()]
            assert torch.equal(torch.rand(3), _after(int(c["seed"]), k))          # exactly k draws were consumed
        assert _spread_pick(c["est"].tolist(), k, rand=torch.from_numpy(c["rand"])).tolist() == c["idx_range"].tolist()


def _after(seed, k):
    torch.manual_seed(seed)
    torch.rand(k)
    return torch.rand(3)


def test_host_switch_and_cpu_tensors_keep_the_loop(golden, monkeypatch):
    """CPU images never reach the device path, whatever the size; a non-finite estimate never does either."""
    from selection_utils import SPREAD_DEVICE_MIN_NK, _spread_pick
    est = np.linspace(0, 1, 80).astype(np.float32)
    assert est.shape[0] * 70 >= SPREAD_DEVICE_MIN_NK
    rand = torch.rand(70)
    want = _spread_pick(est.tolist(), 70, rand=rand)
    assert _spread_pick(est.tolist(), 70, rand=rand, device=torch.device("cpu")).tolist() == want.tolist()
    monkeypatch.setenv("QEA_SAMPLER", "host")
    assert _spread_pick(est.tolist(), 70, rand=rand, device=torch.device("cuda")).tolist() == want.tolist()
    monkeypatch.delenv("QEA_SAMPLER")
    bad = est.tolist()
    bad[3] = float("inf")
    _spread_pick(bad, 70, rand=rand, device=torch.device("cuda"))                 # host loop: no CUDA call is attempted


def test_python_mirrors_the_header_thresholds():
    from qea import ops
    text = open(os.path.join(ROOT, "include", "qea_hip.h")).read()
    d = dict(re.findall(r"#define (QEA_SPREAD_\w+) (\d+)\n", text))
    assert (int(d["QEA_SPREAD_WAVE_MAX_N"]), int(d["QEA_SPREAD_LDS4_MAX_N"]), int(d["QEA_SPREAD_LDS_MAX_N"])) == \
        (ops.SPREAD_WAVE_MAX_N, ops.SPREAD_LDS4_MAX_N, ops.SPREAD_LDS_MAX_N)
    assert "#define QEA_SPREAD_MAX_N (1 << 24)" in text and ops.SPREAD_MAX_N == 1 << 24
    from qea import _lib
    L = _lib.lib()
    assert L.qea_spread_pick_workspace_bytes(ops.SPREAD_LDS_MAX_N) == 0
    assert L.qea_spread_pick_workspace_bytes(ops.SPREAD_LDS_MAX_N + 1) == (ops.SPREAD_LDS_MAX_N + 4) * 4
    assert L.qea_spread_pick(None, 1, None, 1, None, None, None) < 0 and b"null" in L.qea_last_error()
    assert L.qea_seq_entropy(None, 0, 0, 1, 1, 1, 95, None, None) < 0 and b"null" in L.qea_last_error()


def test_unknown_strips_count_as_entropy_one():
    from selection_utils import UniformEntropySampler, _spread_pick
    images, labels = torch.arange(10) * 10, [str(j) for j in range(10)]
    names = [f"s{j}" for j in range(10)]
    s = UniformEntropySampler({}, {})
    for k in (1, 4, 10):
        sel, labs, idx = s.query(images, labels, k, names)
        assert idx.tolist() == list(range(k)) and sel.tolist() == [10 * j for j in range(k)] and labs == labels[:k]
    # a partially known table: the indices address the MINIBATCH (the compacted list has 3 entries; index 7 does not exist in it)
    s = UniformEntropySampler({"s2": 0.25, "s7": 0.5, "s8": 0.75}, {})
    est = [1.0, 1.0, 0.25, 1.0, 1.0, 1.0, 1.0, 0.5, 0.75, 1.0]
    torch.manual_seed(3)
    rand = torch.rand(6)
    torch.manual_seed(3)
    sel, labs, idx = s.query(images, labels, 6, names)
    assert idx.tolist() == _spread_pick(est, 6, rand=rand).tolist()
    assert {2, 7, 8} & set(idx.tolist()) and max(idx.tolist()) > 2
    assert sel.tolist() == [10 * j for j in idx.tolist()] and labs == [labels[j] for j in idx.tolist()]
    s.update_entropies([0.125, 0.5], ["s0", "s2"])
    assert s.entropies == {"s0": 0.125, "s2": 0.5, "s7": 0.5, "s8": 0.75}


def test_update_entropies_is_the_reference_on_cpu_scores(golden):
    import types
    from selection_utils import UniformEntropySampler, update_entropies
    s = UniformEntropySampler({}, {})
    names = [f"s{j}" for j in range(5)]
    update_entropies(types.SimpleNamespace(sampler=s), torch.from_numpy(golden["ent_lp"]), names)
    got = np.array([s.entropies[n] for n in names])
    assert np.abs(got - golden["ent_ref32"].astype(np.float64)).max() <= 1e-6      # the same fp32 formula; BLAS-free, a few ulps at most
    assert np.abs(got - golden["ent_fp64"]).max() <= 1e-6 and np.isfinite(got).all()


def _spy_queries(t, rec):
    """records, for every sampler.query: the names, a copy of the table, k, the uniform vector the call is about to draw, the result"""
    orig = t.sampler.query

    def spy(images, labels, k, names):
        state = torch.get_rng_state()
        rand = torch.rand(k)
        torch.set_rng_state(state)
        out = orig(images, labels, k, names)
        rec.append(dict(names=list(names), table=dict(t.sampler.entropies), k=k, rand=rand, idx=out[2].tolist(), n_images=out[0].shape[0]))
        return out
    t.sampler.query = spy


def _check_entropy_run(t, rec, exp, seen_names, per_epoch):
    from selection_utils import _spread_pick
    table = json.load(open(exp / "cers" / "entropies.json"))
    assert set(table) == set(seen_names) and all(0.0 <= v <= 1.0 for v in table.values())
    assert table == t.sampler.entropies
    assert len(rec) == 2 * per_epoch
    for r in rec[:per_epoch]:                                                      # epoch 0: nothing known -> the first k strips
        assert not (set(r["names"]) & set(r["table"])) and r["idx"] == list(range(r["k"])) and r["n_images"] == r["k"]
    for r in rec[per_epoch:]:                                                      # epoch 1: the host specification on the recorded table and draws
        assert set(r["names"]) <= set(r["table"])
        want = _spread_pick([r["table"][n] for n in r["names"]], r["k"], rand=r["rand"])
        assert r["idx"] == want.tolist()


def test_area_trainer_runs_uniform_entropy(tmp_path):
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from train_nn_area import TrainNNPrep
    tr_set = SyntheticTextAreas(8, seed=1, include_name=True, include_index=True)
    args = _args("a", tmp_path / "exp", batch_size=4, epoch=2, minibatch_subset="uniformEntropy", minibatch_subset_prop=0.5, inner_limit=1)
    ocr = StubHelper()
    t = TrainNNPrep(args, backend=oracle_backend(), train_set=tr_set, val_set=SyntheticTextAreas(4, seed=2, include_name=True), ocr=ocr)
    assert type(t.sampler).__name__ == "UniformEntropySampler" and t.sampler.entropies is t.entropies and t.entropies == {}
    rec = []
    _spy_queries(t, rec)
    t.train()
    _check_entropy_run(t, rec, tmp_path / "exp", tr_set.names, per_epoch=2)
    assert ocr.count_calls == 2 * (2 * 2 + 4)                                      # per epoch: 2 minibatches x k=2 (+ validation: 4)
    # the table an earlier run wrote starts the next one
    args2 = _args("a", tmp_path / "exp2", batch_size=4, minibatch_subset="uniformEntropy", entropies_path=str(tmp_path / "exp" / "cers" / "entropies.json"))
    t2 = TrainNNPrep(args2, backend=oracle_backend(), train_set=tr_set, val_set=SyntheticTextAreas(4, seed=2, include_name=True), ocr=StubHelper())
    assert t2.sampler.entropies == t.sampler.entropies


def test_patch_trainer_runs_uniform_entropy(tmp_path):
    from datasets.synthetic import SyntheticPatches
    from ocr_helper.stub_helper import StubHelper
    from train_nn_patch import TrainNNPrep
    tr_set = SyntheticPatches(2, seed=1, strips=(3, 4), pad_shape=(80, 256))
    names = []
    for i in range(len(tr_set)):
        _, boxes, name = tr_set[i]
        names += TrainNNPrep._strip_names([b["label"] for b in boxes], name)
    args = _args("p", tmp_path / "exp", epoch=2, minibatch_subset="uniformEntropy", minibatch_subset_prop=0.5, inner_limit=1)
    t = TrainNNPrep(args, backend=oracle_backend(), train_set=tr_set,
                    val_set=SyntheticPatches(1, seed=2, strips=(2, 2), pad_shape=(80, 256), include_name=False), ocr=StubHelper())
    rec = []
    _spy_queries(t, rec)
    t.train()
    _check_entropy_run(t, rec, tmp_path / "exp", names, per_epoch=2)


def test_every_factory_class_is_constructed(tmp_path):
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from train_nn_area import TrainNNPrep
    tr_set = SyntheticTextAreas(4, seed=1, include_name=True, include_index=True)
    cers_path = tmp_path / "cers.json"
    json.dump({n: 0.5 for n in tr_set.names}, open(cers_path, "w"))
    for method in ("random", "topKCER", "rangeCER", "uniformEntropy", "uniformCERglobal", "randomglobal"):
        args = _args("a", tmp_path / f"exp_{method}", batch_size=2, minibatch_subset=method, cers_ocr_path=str(cers_path))
        t = TrainNNPrep(args, backend=oracle_backend(), train_set=tr_set, val_set=SyntheticTextAreas(2, seed=2, include_name=True), ocr=StubHelper())
        assert t.sampler is not None and isinstance(t.sampler.cers, dict)
    from selection_utils import CerRangeSampler, RandomSampler, TopKCERSampler, UniformEntropySampler
    assert all(c.content_free for c in (CerRangeSampler, RandomSampler, TopKCERSampler, UniformEntropySampler))


def test_area_trainer_select_before_clean_with_range_cer_is_the_same_training(tmp_path):
    """--select_before_clean with rangeCER: the pick depends on names, CERs and RNG draws only, so cleaning just the picked images
    trains the very same models (the pattern of test_area_trainer_select_before_clean_is_the_same_training)."""
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from train_nn_area import TrainNNPrep
    outs = []
    for flag in (False, True):
        tr_set = SyntheticTextAreas(8, seed=1, include_name=True, include_index=True)
        cers_path = tmp_path / f"cers{int(flag)}.json"
        json.dump({n: float(i % 5) / 4 + 0.01 * i for i, n in enumerate(tr_set.names)}, open(cers_path, "w"))
        args = _args("a", tmp_path / f"exp{int(flag)}", batch_size=4, minibatch_subset="rangeCER", minibatch_subset_prop=0.5,
                     cers_ocr_path=str(cers_path), inner_limit=2, select_before_clean=flag)
        t = TrainNNPrep(args, backend=oracle_backend(), train_set=tr_set, val_set=SyntheticTextAreas(4, seed=2, include_name=True), ocr=StubHelper())
        t.train()
        outs.append((torch.cat([p.detach().flatten() for p in t.crnn_model.parameters()]),
                     torch.cat([p.detach().flatten() for p in t.prep_model.parameters()]),
                     sorted(n for n, v in t.selected_samples.items() if v[0])))
    assert outs[0][2] == outs[1][2] and len(outs[0][2]) == 4
    assert torch.allclose(outs[0][0], outs[1][0], rtol=0, atol=2e-4) and torch.allclose(outs[0][1], outs[1][1], rtol=0, atol=1e-4)
