"""The resident strip store (datasets/resident.py) on the CPU: its numpy form is the specification of `batch()`, so it is held
against the sample loader itself (ImgDataset + PadWhite + float32 / 255) bit for bit; the index loader against torch's DataLoader
draw by draw; the pack file, the host-side checks, the ABI entry and the command-line flags."""
import os

import numpy as np
import pytest
import torch

import resident_fixture as RF

torch.set_num_threads(4)
H, W = RF.SIZE


@pytest.fixture(scope="module")
def strip_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("strips"))
    RF.write_strips(root)
    return root


@pytest.fixture(scope="module")
def dataset(strip_dir):
    from datasets.img_dataset import ImgDataset
    return ImgDataset(strip_dir, transform=RF.pad_transform(), include_name=True, include_index=True)


@pytest.fixture(scope="module")
def reference(dataset):
    """The sample loader's items, computed once: (stacked images [n,1,32,128], labels, names)."""
    items = [dataset[i] for i in range(len(dataset))]
    return torch.stack([it[0] for it in items]), [it[1] for it in items], [it[2] for it in items]


def test_cpu_store_equals_the_sample_loader(dataset, reference):
    from datasets.resident import ResidentStrips
    images, labels, names = reference
    assert len(dataset) == RF.N_STRIPS
    store = ResidentStrips(dataset, RF.SIZE)
    assert len(store) == RF.N_STRIPS and store.device.type == "cpu"
    got = store.batch(range(len(store)))
    assert got.dtype == torch.float32 and tuple(got.shape) == (RF.N_STRIPS, 1, H, W)
    assert torch.equal(got, images)
    assert store.names == names and store.labels == labels and store.lens.tolist() == [len(l) for l in labels]
    # the files the listing drops are not in the store
    assert RF.BROKEN not in store.names and not any(n.endswith("_long.png") for n in store.names)
    # the layout: strips back to back, row-major, no padding; oversize strips were shrunk to fit
    assert store.pixels.dtype == np.uint8 and store.offset.dtype == np.int64 and store.h.dtype == np.int32 and store.w.dtype == np.int32
    sizes = store.h.astype(np.int64) * store.w
    assert store.offset.tolist() == [0] + np.cumsum(sizes)[:-1].tolist() and store.pixels.size == int(sizes.sum())
    assert int(store.h.max()) <= H and int(store.w.max()) <= W
    thumb = [i for i, n in enumerate(names) if "_40x300." in n or "_33x64." in n or "_16x200." in n or "_64x64." in n or "_12x129." in n]
    assert len(thumb) == 8 and all(store.h[i] < H or store.w[i] < W for i in thumb)
    # a CPU tensor of indices, in any order and with repeats
    pick = torch.tensor([5, 0, 5, 23])
    assert torch.equal(store.batch(pick), images[pick])


def test_left_anchor_and_crop_follow_pad_to_bucket(dataset):
    """anchor="left": column 0, centred vertically, cropped when wider than out_w — datasets.bucketing.pad_to_bucket applied to the
    strip once it is padded to the full height."""
    from datasets.bucketing import pad_to_bucket
    from datasets.resident import ResidentStrips
    store = ResidentStrips(dataset, RF.SIZE)
    for out_w in (64, 128, 256):
        got = store.batch(range(len(store)), out_w=out_w, anchor="left")
        assert tuple(got.shape) == (len(store), 1, H, out_w)
        for i in range(len(store)):
            h, w = int(store.h[i]), int(store.w[i])
            strip = torch.from_numpy(store.table[store.pixels[store.offset[i]: store.offset[i] + h * w].reshape(h, w)])
            tall = torch.ones(1, H, w)
            tall[0, (H - h) // 2: (H - h) // 2 + h] = strip
            assert torch.equal(got[i], pad_to_bucket(tall, buckets=(out_w,))), (i, out_w)


@pytest.mark.parametrize("how", ["sampler", "shuffle"])
def test_resident_loader_draws_what_the_dataloader_draws(dataset, how):
    from datasets.resident import ResidentLoader, ResidentStrips
    store = ResidentStrips(dataset, RF.SIZE)
    idx = torch.arange(len(dataset))[torch.arange(len(dataset)) % 5 != 2]          # 19 of the 24: four batches of 4, three dropped

    def loaders():
        for cls, args in ((torch.utils.data.DataLoader, (dataset,)), (ResidentLoader, (dataset, store))):
            torch.manual_seed(42)
            kw = dict(sampler=torch.utils.data.SubsetRandomSampler(idx)) if how == "sampler" else dict(shuffle=True)
            yield cls(*args, batch_size=4, drop_last=True, **kw)

    runs = []
    for loader in loaders():
        seen, states = [], []
        assert loader.dataset is dataset and len(loader) == (4 if how == "sampler" else 6)
        for _epoch in range(2):
            for images, labels, names, indices in loader:
                seen.append((images, list(labels), list(names), indices))
            states.append(torch.get_rng_state())
        runs.append((seen, states))
    (ref, ref_states), (got, got_states) = runs
    assert len(ref) == len(got) == 2 * (4 if how == "sampler" else 6)
    assert [r[2] for r in ref[:len(ref) // 2]] != [r[2] for r in ref[len(ref) // 2:]]           # the two epochs differ
    for r, g in zip(ref, got):
        assert r[2] == g[2] and r[1] == g[1]
        assert torch.equal(r[0], g[0]) and torch.equal(r[3], g[3]) and r[3].dtype == g[3].dtype
    for a, b in zip(ref_states, got_states):
        assert torch.equal(a, b)


def test_resident_loader_of_a_subset_without_names(strip_dir):
    """train_crnn.py's forms: --train_subset wraps the set in a Subset; its validation set yields (images, labels) only."""
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentLoader, ResidentStrips
    ds = ImgDataset(strip_dir, transform=RF.pad_transform())
    sub = torch.utils.data.Subset(ds, range(10))
    store = ResidentStrips(ds, RF.SIZE)
    ref = list(torch.utils.data.DataLoader(sub, batch_size=4))
    got = list(ResidentLoader(sub, store, batch_size=4))
    assert len(got) == len(ref) == 3 and len(ResidentLoader(sub, store, batch_size=4).dataset) == 10
    for r, g in zip(ref, got):
        assert len(g) == 2 and torch.equal(r[0], g[0]) and list(r[1]) == g[1]


def test_subset_indices_are_the_base_datasets(dataset):
    """include_index through a Subset: the sample loader yields ImgDataset's own index (dataset.indices[j]), so does the resident one."""
    from datasets.resident import ResidentLoader, ResidentStrips
    sub = torch.utils.data.Subset(dataset, [7, 3, 20, 11, 0])
    store = ResidentStrips(dataset, RF.SIZE)
    ref = list(torch.utils.data.DataLoader(sub, batch_size=2))
    got = list(ResidentLoader(sub, store, batch_size=2))
    assert [r[3].tolist() for r in ref] == [[7, 3], [20, 11], [0]]
    for r, g in zip(ref, got):
        assert torch.equal(r[0], g[0]) and list(r[1]) == g[1] and list(r[2]) == g[2]
        assert torch.equal(r[3], g[3]) and r[3].dtype == g[3].dtype


def test_another_transform_is_refused(strip_dir):
    """The store reproduces PadWhite(size) + float32 / 255 and never calls the dataset's transform: resident_loader compares the
    dataset's own samples with the store's and refuses a dataset that would have trained on other pixels."""
    from datasets._io import to_tensor
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentLoader, resident_loader
    from qea._lib import QeaError
    from transform_helper import PadWhite
    ok = ImgDataset(strip_dir, transform=RF.pad_transform(), include_name=True)
    assert type(resident_loader(ok, RF.SIZE, "cpu", batch_size=4)) is ResidentLoader
    inverted = ImgDataset(strip_dir, transform=lambda img: 1 - to_tensor(PadWhite(RF.SIZE)(img)), include_name=True)
    wider = ImgDataset(strip_dir, transform=lambda img: to_tensor(PadWhite((32, 256))(img)), include_name=True)
    for ds in (inverted, wider, ImgDataset(strip_dir, include_name=True)):
        with pytest.raises(QeaError, match="transform"):
            resident_loader(ds, RF.SIZE, "cpu", batch_size=4)


def test_pack_file_round_trip_and_staleness(tmp_path):
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentStrips
    root = str(tmp_path / "strips")
    RF.write_strips(root)
    ds = ImgDataset(root, transform=RF.pad_transform(), include_name=True)
    pack = str(tmp_path / "packs" / "train.npz")
    built = ResidentStrips.load_or_build(ds, RF.SIZE, pack)
    assert not built.from_pack and os.path.exists(pack)
    with np.load(pack, allow_pickle=False) as z:
        assert set(z.files) >= {"pixels", "offset", "h", "w", "names", "labels", "signature"}
        assert z["names"].tolist() == built.names and z["labels"].tolist() == built.labels
    again = ResidentStrips.load_or_build(ds, RF.SIZE, pack)
    assert again.from_pack
    for a, b in ((built.pixels, again.pixels), (built.offset, again.offset), (built.h, again.h), (built.w, again.w)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert again.names == built.names and again.labels == built.labels
    assert torch.equal(again.batch(range(len(ds))), built.batch(range(len(ds))))
    # a pack written for another target size is rejected (and replaced)
    other = ResidentStrips.load_or_build(ds, (32, 64), pack)
    assert not other.from_pack and int(other.w.max()) <= 64
    assert not ResidentStrips.load_or_build(ds, RF.SIZE, pack).from_pack            # ... so the first size rebuilds in its turn
    assert ResidentStrips.load_or_build(ds, RF.SIZE, pack).from_pack
    # one file's bytes change: stale pixels must not come back
    victim = ds.files[3]
    from PIL import Image
    w, h = Image.open(victim).size
    Image.fromarray(np.full((h, w), 7, dtype=np.uint8), mode="L").save(victim)
    st = os.stat(victim)
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))          # whatever the file system's clock granularity
    fresh = ResidentStrips.load_or_build(ds, RF.SIZE, pack)
    assert not fresh.from_pack
    assert torch.equal(fresh.batch([3]), ds[3][0][None]) and not torch.equal(fresh.batch([3]), built.batch([3]))
    assert ResidentStrips.load_or_build(ds, RF.SIZE, pack).from_pack


def test_indices_are_checked_on_the_host(dataset):
    from datasets.resident import ResidentStrips
    store = ResidentStrips(dataset, RF.SIZE)
    n = len(store)
    for bad in ([n], [-1], [0, n], torch.tensor([-1, 0])):
        with pytest.raises(ValueError):
            store.batch(bad)
    with pytest.raises(ValueError):
        store.batch([0], out_w=130)                                              # one 16-byte store per lane: out_w % 4 == 0
    with pytest.raises(ValueError):
        store.batch([0], anchor="right")


def test_memory_guard_names_the_size(dataset):
    from datasets.resident import ResidentStrips
    from qea._lib import QeaError
    with pytest.raises(QeaError, match=r"GB"):
        ResidentStrips(dataset, RF.SIZE, max_gb=1e-6)                            # 1 KB: the 24 strips hold ~40 KB
    assert ResidentStrips(dataset, RF.SIZE, max_gb=1e-3).nbytes < 1e-3 * 2 ** 30


def test_abi_entry_point():
    from qea import _lib
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    assert "qea_strip_batch" in protos and len(protos["qea_strip_batch"][1]) == 13
    L = _lib.lib()
    assert hasattr(L, "qea_strip_batch") and L.qea_version() == 9
    # refused before any launch: null pointers, and a width that is no multiple of 4
    assert L.qea_strip_batch(None, None, None, None, 1, None, 1, 32, 128, 0, None, None, None) < 0
    assert b"null" in L.qea_last_error()
    one = 16
    assert L.qea_strip_batch(one, one, one, one, 1, one, 1, 32, 130, 0, one, one, None) < 0
    assert b"multiple of 4" in L.qea_last_error()


def _oracle_backend():
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    return Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)


def test_flags_parse_and_default_to_the_sample_loaders(tmp_path, strip_dir):
    import area_cli  # noqa: F401  (the front end imports without side effects)
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentLoader
    from datasets.synthetic import SyntheticTextAreas
    from ocr_helper.stub_helper import StubHelper
    from qea._lib import QeaError
    from qea.cli_flags import build_parser
    from train_crnn import TrainCRNN
    from train_crnn import build_parser as crnn_parser
    from train_nn_area import TrainNNPrep
    for ap in (build_parser("a", ""), crnn_parser()):
        d = ap.parse_args([])
        assert d.resident is False and d.resident_pack is None and d.resident_max_gb == 8
        on = ap.parse_args(["--resident", "--resident_pack", "p.npz", "--resident_max_gb", "0.5"])
        assert on.resident is True and on.resident_pack == "p.npz" and on.resident_max_gb == 0.5
        acts = {a.option_strings[0]: a for a in ap._actions if a.option_strings}
        assert all(acts[f].help.startswith("[new]") for f in ("--resident", "--resident_pack", "--resident_max_gb"))

    def area(train, val, **over):
        a = build_parser("a", "").parse_args(["--exp_base_path", str(tmp_path / "area"), "--ocr", "stub", "--epoch", "1", "--batch_size", "4"])
        for k, v in over.items():
            setattr(a, k, v)
        return TrainNNPrep(a, backend=_oracle_backend(), train_set=train, val_set=val, ocr=StubHelper())

    def crnn(train, val, **over):
        a = crnn_parser().parse_args(["--crnn_model_path", str(tmp_path / "crnn" / "model"), "--batch_size", "4"])
        for k, v in over.items():
            setattr(a, k, v)
        return TrainCRNN(a, backend=_oracle_backend(), train_set=train, val_set=val)

    tf = RF.pad_transform()
    tr = ImgDataset(strip_dir, transform=tf, include_name=True, include_index=True)
    va = ImgDataset(strip_dir, transform=tf, include_name=True)
    for make in (area, crnn):
        t = make(tr, va)
        assert type(t.loader_train) is torch.utils.data.DataLoader and type(t.loader_validation) is torch.utils.data.DataLoader
        t = make(tr, va, resident=True, resident_pack=str(tmp_path / make.__name__ / "pack.npz"))
        assert type(t.loader_train) is ResidentLoader and type(t.loader_validation) is ResidentLoader
        assert os.path.exists(tmp_path / make.__name__ / "pack.npz") and os.path.exists(tmp_path / make.__name__ / "pack.val.npz")
        assert t.loader_train.store.device.type == "cpu" and len(t.loader_train.dataset) == RF.N_STRIPS
        with pytest.raises(QeaError, match="ImgDataset"):
            make(SyntheticTextAreas(8, seed=1, include_name=True, include_index=True), va, resident=True)
        with pytest.raises(QeaError, match="synthetic_size"):
            make(tr, va, resident=True, synthetic_size=8)
    with pytest.raises(QeaError, match="widths"):
        area(SyntheticTextAreas(8, seed=1, include_name=True, include_index=True, widths=[128] * 8), va, resident=True)
    # --train_subset of train_crnn.py: a Subset of the ImgDataset keeps its length
    t = crnn(tr, va, resident=True, train_subset=10)
    assert type(t.loader_train) is ResidentLoader and t.train_set_size == 10


def test_flag_off_never_imports_the_store(tmp_path):
    """With the flags at their defaults both trainers build plain DataLoaders and datasets.resident is not imported: checked in a
    fresh interpreter (tests/resident_children.py), since this process has imported the module long ago."""
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resident_children.py")
    r = subprocess.run([sys.executable, child, "default-loaders", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "default-loaders-plain" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
