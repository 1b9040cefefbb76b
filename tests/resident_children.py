"""Runs of the resident-store tests that want an interpreter of their own (started by tests/test_resident_gpu.py and
tests/test_resident_cpu.py, never collected by pytest):

  graph STRIP_DIR TMP   area trainer, `--graph --resident` against `--graph` alone over three steps on the device: identical losses
                        and bit-identical weights, or a non-zero exit
  default-loaders TMP   both trainers built with the flags at their defaults on the CPU oracle backend: plain DataLoaders, and
                        datasets.resident never imported
"""
import os
import pathlib
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def graph(strip_dir, tmp):
    import resident_fixture as RF
    tmp = pathlib.Path(tmp)
    ref = RF.area_run(tmp, strip_dir, False, True, 3)
    got = RF.area_run(tmp, strip_dir, True, True, 3)
    assert len(ref[3].phase_b_graphs.graphs) >= 1 and len(got[3].phase_b_graphs.graphs) >= 1
    assert len(got[3].phase_a_graphs.graphs) >= 1
    assert got[3].loader_train.store.device.type == "cuda"
    assert got[0] == ref[0], (got[0], ref[0])
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    torch.cuda.synchronize()
    print("graph-resident-identical", got[0])


def default_loaders(tmp):
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.cli_flags import build_parser
    from qea.trainer_core import Backend
    from train_crnn import TrainCRNN
    from train_nn_area import TrainNNPrep
    torch.set_num_threads(2)
    backend = lambda: Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    tr = SyntheticTextAreas(8, seed=1, include_name=True, include_index=True)
    va = SyntheticTextAreas(4, seed=2, include_name=True)
    a = build_parser("a", "").parse_args(["--exp_base_path", os.path.join(tmp, "area"), "--ocr", "stub", "--epoch", "1", "--batch_size", "4"])
    c = build_parser("c", "").parse_args(["--crnn_model_path", os.path.join(tmp, "crnn", "model"), "--batch_size", "4"])
    assert a.resident is False and c.resident is False
    for t in (TrainNNPrep(a, backend=backend(), train_set=tr, val_set=va, ocr=StubHelper()), TrainCRNN(c, backend=backend(), train_set=tr, val_set=va)):
        assert type(t.loader_train) is torch.utils.data.DataLoader and type(t.loader_validation) is torch.utils.data.DataLoader
    assert "datasets.resident" not in sys.modules, "the flag is off, yet datasets.resident was imported"
    print("default-loaders-plain")


if __name__ == "__main__":
    {"graph": graph, "default-loaders": default_loaders}[sys.argv[1]](*sys.argv[2:])
