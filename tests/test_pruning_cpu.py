"""Dataset pruning on the CPU: the two methods against the artifacts the reference's pruner wrote (tests/golden/pruning/, copies of
its pruning/cer_artifacts/*.json), the pruner's flag surface, grouping and file names, and --pruning_artifact in the patch trainer."""
import json
import os

import pytest
import torch

PRUNE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pruning")


def _load(name):
    with open(os.path.join(PRUNE_DIR, name)) as f:
        return json.load(f)


def _num_samples(n, prop):
    return n - int(n * (prop / 100))             # prune_dataset.py:59


@pytest.mark.parametrize("prop", [10, 50])
def test_topk_equals_the_reference_artifacts(prop):
    from pruning import methods
    cers = _load("cers_pos.json")
    ref = _load(f"cers_pos_topk_{prop}.json")
    out = methods.topk(cers, _num_samples(len(cers), prop))
    assert list(out.items()) == list(ref.items())


def test_facility_location_cpu_reproduces_the_reference_ranking():
    """The first 64 picks of the reference's FL ranking (every FL artifact is a prefix of one greedy ranking), order included."""
    from pruning import methods
    cers = _load("cers_pos.json")
    ref = list(_load("cers_pos_FL_50.json").items())
    out = methods.facility_location(cers, 64, backend="cpu")
    assert list(out.items()) == ref[:64]


def test_facility_location_accepts_feature_rows_and_refuses_ragged_ones():
    from pruning import methods
    rows = {"a": [0.0, 0.0], "b": [1.0, 0.0], "c": [0.0, 0.0], "d": [5.0, 5.0]}
    out = methods.facility_location(rows, 4, backend="cpu")
    assert set(out) == set(rows) and list(out).index("a") < list(out).index("c")       # identical rows: the lower index first
    assert out["d"] == [5.0, 5.0]
    with pytest.raises(ValueError):
        methods.facility_location({"a": [0.0, 1.0], "b": [1.0]}, 1, backend="cpu")
    with pytest.raises(ValueError):
        methods.facility_location({"a": 0.0, "b": 1.0}, 3, backend="cpu")
    with pytest.raises(ValueError):
        methods.facility_location({"a": 0.0, "b": float("nan")}, 1, backend="cpu")


def test_pruner_cli_surface_matches_the_reference():
    from pruning import prune_dataset
    from qea.cli_flags import build_parser
    ref = _load("prune_reference_flags.json")["prune_dataset"]
    ap = build_parser("r", "")
    acts = {a.option_strings[0]: a for a in ap._actions if a.option_strings and a.option_strings[0] != "-h"}
    args = vars(ap.parse_args(["--cers_tess_path", "x.json"]))
    for f in ref:
        a = acts[f["flag"]]
        assert a.required == f["required"], f
        if not f["required"]:
            assert args[a.dest] == f["default"], f
        assert (a.type.__name__ if a.type else None) == f["type"], f
        assert (list(a.choices) if a.choices else None) == f["choices"], f
    extra = set(acts) - {f["flag"] for f in ref}
    assert extra == {"--backend", "--features", "--history_len"}
    assert all(acts[n].help.startswith("[new]") for n in extra)
    assert args["features"] == "mean" and args["backend"] is None and args["history_len"] == 8
    with pytest.raises(SystemExit):
        ap.parse_args([])                                                              # --cers_tess_path is required
    assert vars(prune_dataset.build_parser().parse_args(["--cers_tess_path", "x.json"])) == args
    # the trainers' surfaces are untouched by the new tag
    assert not hasattr(build_parser("p", "").parse_args([]), "prune_method")


def test_pruner_grouping_rounding_and_file_names(tmp_path, monkeypatch, capsys):
    from pruning import prune_dataset
    monkeypatch.chdir(tmp_path)
    strips = {"0_TOTAL_folderA_doc1": 0.0, "1_12.50_folderA_doc1": 1.0, "2_x_folderA_doc1": 1.0,        # 2/3 -> 0.667
              "0_a_b_folderB_doc_2": 0.25,                                                              # split("_", 2): label "a", document "b_folderB_doc_2"
              "0_CASH_folderC_doc3": 2.0, "1_VISA_folderC_doc3": 1.0,
              "0_q_folderD_doc4": 0.1, "0_q_folderE_doc5": 0.3}
    json.dump(strips, open(tmp_path / "strips.json", "w"))
    args = prune_dataset.build_parser().parse_args(["--cers_tess_path", str(tmp_path / "strips.json"), "--dataset", "pos", "--prune_prop", "40"])
    pruner = prune_dataset.DatasetPruner(args)
    means = pruner.get_image_metric()
    assert means == {"folderA_doc1": 0.667, "b_folderB_doc_2": 0.25, "folderC_doc3": 1.5, "folderD_doc4": 0.1, "folderE_doc5": 0.3}
    assert list(means) == ["folderA_doc1", "b_folderB_doc_2", "folderC_doc3", "folderD_doc4", "folderE_doc5"]
    pruned = pruner.prune(means)                                                       # 5 - int(5 * 0.4) = 3 kept
    assert list(pruned.items()) == [("folderC_doc3", 1.5), ("folderA_doc1", 0.667), ("folderE_doc5", 0.3)]
    assert "Size before pruning: 5, Size after pruning: 3" in capsys.readouterr().out
    # the whole front end: the reference's two files under properties.cer_artifacts_path
    out = prune_dataset.main(["--cers_tess_path", str(tmp_path / "strips.json"), "--dataset", "pos", "--prune_method", "FL", "--prune_prop", "40",
                              "--backend", "cpu"])
    assert sorted(os.listdir(tmp_path / "cer_artifacts")) == ["cers_pos.json", "cers_pos_FL_40.json"]
    assert json.load(open(tmp_path / "cer_artifacts" / "cers_pos.json")) == means
    on_disk = json.load(open(tmp_path / "cer_artifacts" / "cers_pos_FL_40.json"))
    assert list(on_disk.items()) == list(out.items()) and len(out) == 3 and set(out) <= set(means)


def test_pruner_history_features(tmp_path, monkeypatch):
    """[new] --features history: a trainer's all_cers.json (strip -> per-epoch CERs) -> per-document rows of the last L epoch means."""
    from pruning import prune_dataset
    from qea._lib import QeaError
    monkeypatch.chdir(tmp_path)
    hist = {"0_a_f_d1": [9.0, 1.0, 0.0], "1_b_f_d1": [9.0, 0.0, 1.0], "0_a_f_d2": [9.0, 0.5, 0.5], "0_a_f_d3": [9.0, 1.0, 1.0], "0_a_f_d4": [9.0, 0.5, 0.5]}
    json.dump(hist, open(tmp_path / "all_cers.json", "w"))
    argv = ["--cers_tess_path", str(tmp_path / "all_cers.json"), "--dataset", "pos", "--prune_method", "FL", "--prune_prop", "50", "--backend", "cpu",
            "--features", "history", "--history_len", "2"]
    pruner = prune_dataset.DatasetPruner(prune_dataset.build_parser().parse_args(argv))
    rows = pruner.get_image_metric()
    assert rows == {"f_d1": [0.5, 0.5], "f_d2": [0.5, 0.5], "f_d3": [1.0, 1.0], "f_d4": [0.5, 0.5]}
    kept = prune_dataset.main(argv)
    assert list(kept) == ["f_d1", "f_d3"]                    # the medoid first (lowest index of three identical rows), then the outlier
    with pytest.raises(QeaError):
        prune_dataset.DatasetPruner(prune_dataset.build_parser().parse_args(argv[:-6] + ["--features", "history", "--prune_method", "topk"]))


def _patch_trainer(tmp_path, **over):
    from datasets.synthetic import SyntheticPatches
    from ocr_helper.stub_helper import StubHelper
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.cli_flags import build_parser
    from qea.trainer_core import Backend
    from train_nn_patch import TrainNNPrep
    args = build_parser("p", "").parse_args(["--exp_base_path", str(tmp_path / "exp"), "--ocr", "stub", "--epoch", "1", "--inner_limit", "1"])
    for k, v in over.items():
        setattr(args, k, v)
    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    tr_set = SyntheticPatches(6, seed=1, strips=(2, 3), pad_shape=(80, 256))
    val = SyntheticPatches(1, seed=2, strips=(2, 2), pad_shape=(80, 256), include_name=False)
    return TrainNNPrep(args, backend=backend, train_set=tr_set, val_set=val, ocr=StubHelper()), tr_set


def test_pruning_artifact_is_honoured_by_the_patch_trainer(tmp_path, monkeypatch, capsys):
    """patch_cli.py --pruning_artifact NAME trains on the documents pruning/<cer_artifacts>/NAME.json names and on no others."""
    import properties
    from qea._lib import QeaError
    monkeypatch.chdir(tmp_path)
    art_dir = tmp_path / "pruning" / properties.cer_artifacts_path
    os.makedirs(art_dir)
    # SyntheticPatches(seed=1) names its documents synthetic/folder1/doc_0000i.png -> key folder1_doc_0000i
    keep = [4, 1, 3]
    json.dump({f"folder1_doc_{i:05d}": 0.5 for i in keep} | {"folder9_doc_00000": 1.0}, open(art_dir / "cers_pos_topk_50.json", "w"))
    t, tr_set = _patch_trainer(tmp_path, pruning_artifact="cers_pos_topk_50")
    assert sorted(int(i) for i in t.loader_train.sampler.indices) == [1, 3, 4]
    assert t.train_set_size == 3 and len(t.loader_train) == 3
    assert "Train Data Size - 6, Train Subset Size - 3" in capsys.readouterr().out
    seen = sorted(names[0] for _, _, names in t.loader_train)
    assert seen == [tr_set[i][2] for i in (1, 3, 4)]
    # without the flag: the whole set, as before
    t0, _ = _patch_trainer(tmp_path)
    assert sorted(int(i) for i in t0.loader_train.sampler.indices) == list(range(6))
    # an artifact that names no document of the set, and a missing one, are errors that name the file
    json.dump({"folder9_doc_00000": 1.0}, open(art_dir / "nothing.json", "w"))
    with pytest.raises(QeaError, match="nothing.json"):
        _patch_trainer(tmp_path, pruning_artifact="nothing")
    with pytest.raises(QeaError, match="absent.json"):
        _patch_trainer(tmp_path, pruning_artifact="absent")
