"""The resident strip store on the MI355X: qea_strip_batch (csrc/strip_batch.hip) against the CPU store, which
tests/test_resident_cpu.py holds against the sample loader, and the two trainers with --resident against themselves without it.
Every comparison is exact: the kernel copies table entries and the trainers' kernels are deterministic."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resident_fixture as RF

pytestmark = pytest.mark.gpu
H, W = RF.SIZE


@pytest.fixture(scope="module")
def strip_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("strips"))
    RF.write_strips(root)
    return root


@pytest.fixture(scope="module")
def stores(strip_dir):
    """(CPU store, device store) of the same directory; the CPU store's full batch is the reference every test indexes."""
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentStrips
    ds = ImgDataset(strip_dir, transform=RF.pad_transform(), include_name=True)
    return ResidentStrips(ds, RF.SIZE), ResidentStrips(ds, RF.SIZE, device="cuda")


@pytest.fixture(scope="module")
def full(stores):
    return {(ow, anchor): stores[0].batch(range(len(stores[0])), out_w=ow, anchor=anchor)
            for ow, anchor in ((128, "centre"), (128, "left"), (256, "left"), (64, "left"), (256, "centre"), (4, "left"))}


def _idx(n, B, seed):
    return torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("B", ["all", 1, 7, 300])
def test_device_batch_equals_cpu_store(stores, full, B):
    cpu, dev = stores
    n = len(cpu)
    idx = torch.arange(n) if B == "all" else _idx(n, B, 3)                     # 300 > 24: repeated indices
    from qea import ops
    before = ops.STRIP_LAUNCHES["batch"]
    got = dev.batch(idx if B != 7 else idx.tolist())                            # a CPU tensor or a host sequence
    assert ops.STRIP_LAUNCHES["batch"] == before + 1                            # one launch per batch
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(idx), 1, H, W)
    assert torch.equal(got.cpu(), full[(128, "centre")][idx])


def test_store_of_a_single_strip(tmp_path, stores):
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentStrips
    from PIL import Image
    Image.fromarray(np.arange(9 * 50, dtype=np.uint8).reshape(9, 50), mode="L").save(str(tmp_path / "0_one_x.png"))
    ds = ImgDataset(str(tmp_path), transform=RF.pad_transform())
    cpu, dev = ResidentStrips(ds, RF.SIZE), ResidentStrips(ds, RF.SIZE, device="cuda")
    assert len(dev) == 1
    assert torch.equal(dev.batch([0, 0, 0]).cpu(), cpu.batch([0, 0, 0])) and torch.equal(cpu.batch([0])[0], ds[0][0])


@pytest.mark.parametrize("out_w,anchor", [(128, "left"), (256, "left"), (64, "left"), (256, "centre")])
def test_anchor_and_width(stores, full, out_w, anchor):
    """anchor="left" at the store's width, at a wider bucket, and at 64 where the 128-wide strips are cropped; centre at 256."""
    cpu, dev = stores
    assert out_w != 64 or int(cpu.w.max()) == 128
    got = dev.batch(range(len(cpu)), out_w=out_w, anchor=anchor)
    assert tuple(got.shape) == (len(cpu), 1, H, out_w)
    assert torch.equal(got.cpu(), full[(out_w, anchor)])


def test_more_images_than_grid_rows(stores, full):
    """B above 65535 (the grid's second dimension): the workgroups walk several images each.  out_w = 4 keeps the batch at 33 MB."""
    cpu, dev = stores
    idx = _idx(len(cpu), 65535 + 70, 5)
    got = dev.batch(idx, out_w=4, anchor="left")
    assert torch.equal(got.cpu(), full[(4, "left")][idx])


def test_every_pixel_is_written(stores, full):
    cpu, dev = stores
    idx = _idx(len(cpu), 37, 7)
    out = torch.full((37, 1, H, W), float("nan"), device="cuda")
    got = dev.batch(idx, out=out)
    assert got is out and bool(torch.isfinite(out).all())
    assert torch.equal(out.cpu(), full[(128, "centre")][idx])


def test_bad_indices_never_reach_the_device(stores):
    from qea import ops
    cpu, dev = stores
    before = ops.STRIP_LAUNCHES["batch"]
    for bad in ([len(dev)], [-1]):
        with pytest.raises(ValueError):
            dev.batch(bad)
    assert ops.STRIP_LAUNCHES["batch"] == before


def test_area_trainer_resident_equals_sample_loader(tmp_path, strip_dir):
    """B = 8, two epochs of one step, inner_limit 2, TopKCER at 0.5, stub OCR: same losses, bit-identical UNet and CRNN."""
    ref = RF.area_run(tmp_path, strip_dir, False, False, 2)
    got = RF.area_run(tmp_path, strip_dir, True, False, 2)
    assert got[3].loader_train.store.device.type == "cuda"
    assert got[0] == ref[0]
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    assert got[3].ocr.count_calls == ref[3].ocr.count_calls > 0


def test_area_trainer_graph_resident_equals_graph(tmp_path, strip_dir):
    """--graph --resident against --graph alone over three steps (two eager, then the captured replays): same losses, bit-identical
    UNet and CRNN.  The two runs share a fresh interpreter of their own (tests/resident_children.py): captured graphs and the
    workspaces they pin live for the whole process, and this comparison is about the loader, not about what an earlier trainer's
    graphs leave behind for a later one's."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resident_children.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child, "graph", strip_dir, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "graph-resident-identical" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_crnn_trainer_resident_equals_sample_loader(tmp_path, strip_dir):
    """train_crnn.py without --ocr on its default datasets (<data_base_path>/textarea_dataset_{train,dev}): two steps of 8, then
    validation, with and without --resident."""
    import shutil
    import properties
    from datasets.resident import ResidentLoader
    from train_crnn import TrainCRNN, build_parser
    for d in (properties.pos_text_dataset_train, properties.pos_text_dataset_dev):
        shutil.copytree(strip_dir, str(tmp_path / "data" / d))
    res = {}
    for resident in (False, True):
        argv = ["--crnn_model_path", str(tmp_path / f"crnn{int(resident)}" / "model"), "--data_base_path", str(tmp_path / "data"),
                "--batch_size", "8", "--epoch", "1", "--train_subset", "16", "--val_subset", "8"] + (["--resident"] if resident else [])
        t = TrainCRNN(build_parser().parse_args(argv))
        assert (type(t.loader_train) is ResidentLoader) == resident and (type(t.loader_validation) is ResidentLoader) == resident
        assert t.train_set_size == 16 and t.val_set_size == 8
        losses, step = [], t.train_step

        def spy(images, labels, step=step, losses=losses):
            loss = step(images, labels)
            losses.append(loss.item())
            return loss
        t.train_step = spy
        t.train()
        assert len(losses) == 2 and all(l == l for l in losses)
        res[resident] = (losses, t.last_val_accuracy, t.last_val_cer, RF.flat(t.model))
    assert res[True][:3] == res[False][:3]
    assert torch.equal(res[True][3], res[False][3])
