"""The resident document store (datasets/resident.py: ResidentDocuments, ResidentDocLoader) on the CPU: its numpy form is the
specification of `batch()` and `crops()`, so it is held against what it replaces, PatchDataset's own samples, the DataLoader that
collates them and utils.get_text_stack with autograd.  Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import resident_docs_fixture as DF

H, W = DF.CANVAS
OUT = (32, 128)


@pytest.fixture(scope="module")
def doc_dir(tmp_path_factory):
    return DF.write_documents(str(tmp_path_factory.mktemp("docs")))


@pytest.fixture(scope="module")
def dataset(doc_dir):
    from datasets.patch_dataset import PatchDataset
    return PatchDataset(doc_dir, pad=True, include_name=True)


@pytest.fixture(scope="module")
def store(dataset):
    from datasets.resident import ResidentDocuments
    return ResidentDocuments(dataset)


def test_store_equals_the_dataset_samples(dataset, store):
    """batch() and the box lists against dataset[i] for every document, the two oversize ones included."""
    assert len(store) == len(DF.DOCS) and store.n_boxes.tolist() == DF.N_BOXES
    assert store.branch[DF.WIDE] == "cut" and store.branch[DF.TALL] == "cut" and store.branch.count("fit") == 6
    full = store.batch(range(len(store)))
    assert full.dtype == torch.float32 and tuple(full.shape) == (len(store), 1, H, W)
    for i in range(len(store)):
        image, boxes, path = dataset[i]
        assert torch.equal(full[i], image), i
        assert store.boxes[i] == boxes and store.paths[i] == path
    # a 10x600 document keeps source columns 44..555 on canvas rows 195..204 (PIL's negative border)
    from PIL import Image
    src = np.asarray(Image.open(store.paths[DF.WIDE]).convert("L"), dtype=np.float32) / 255.0
    assert np.array_equal(full[DF.WIDE, 0, 195:205].numpy(), src[:, 44:556])
    assert bool((full[DF.WIDE, 0, :195] == 1).all()) and bool((full[DF.WIDE, 0, 205:] == 1).all())
    # the tables: clipped boxes, prefix sums, dtypes
    assert store.pixels.dtype == np.uint8 and store.offset.dtype == np.int64 and store.h.dtype == np.int32 and store.w.dtype == np.int32
    assert store.box.dtype == np.int32 and store.box.shape == (sum(DF.N_BOXES), 4) and store.box_first.dtype == np.int32
    assert store.box_first.tolist() == np.concatenate([[0], np.cumsum(DF.N_BOXES)]).tolist()
    flat = [b for boxes in store.boxes for b in boxes]
    want = [[max(0, b["x_min"]), max(0, b["y_min"]), min(W, b["x_max"]), min(H, b["y_max"])] for b in flat]
    assert store.box.tolist() == want
    assert store.boxes[DF.PLACEHOLDER] == [{"label": store.boxes[DF.PLACEHOLDER][0]["label"], "x_min": 0, "y_min": 0, "x_max": 127, "y_max": 31,
                                            "index": 0}]
    assert store.box[store.box_first[DF.NEGATIVE]].tolist()[0] == 0 and store.boxes[DF.NEGATIVE][0]["x_min"] == -5
    # repeats and one row
    rows = [3, 3, 7, 0, 3]
    assert torch.equal(store.batch(rows), full[rows]) and torch.equal(store.batch([6]), full[6:7])
    with pytest.raises(ValueError):
        store.batch([len(store)])


def test_both_dimensions_oversize(tmp_path):
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    from PIL import Image
    from qea._lib import QeaError
    rng = np.random.RandomState(1)
    Image.fromarray(DF._pixels(rng, 30, 40), mode="L").save(tmp_path / "a_small.png")
    Image.fromarray(DF._pixels(rng, 401, 513), mode="L").save(tmp_path / "b_huge.png")
    for name in ("a_small", "b_huge"):
        json.dump(DF._as_json([(2, 2, 30, 20, "ab")], quad=False), open(tmp_path / f"{name}.json", "w"))
    with pytest.raises(QeaError, match="b_huge.png"):
        ResidentDocuments(PatchDataset(str(tmp_path), pad=True))
    # resize_images: the PIL-resized image is stored, the boxes are scaled by the dataset
    ds = PatchDataset(str(tmp_path), pad=True, resize_images=True)
    st = ResidentDocuments(ds)
    assert st.branch == ["fit", "resize"]
    for i in range(2):
        assert torch.equal(st.batch([i])[0], ds[i][0]) and st.boxes[i] == ds[i][1]
    with pytest.raises(QeaError):
        ResidentDocuments(PatchDataset(str(tmp_path), pad=False))


def test_self_check_refuses_other_pixels(dataset):
    """The store compares itself with the dataset's samples at construction: a dataset that yields anything else is refused."""
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    from qea._lib import QeaError

    class Darker(PatchDataset):
        def __getitem__(self, i):
            s = super().__getitem__(i)
            return (s[0] * 0.5,) + tuple(s[1:])

    with pytest.raises(QeaError, match="other pixels"):
        ResidentDocuments(Darker(os.path.dirname(dataset.files[0]), pad=True))


@pytest.mark.parametrize("how", ["subset_sampler", "shuffle", "sequential_keep_last"])
def test_doc_loader_draws_what_the_dataloader_draws(dataset, store, how):
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import DocBoxes, ResidentDocLoader
    idx = torch.tensor([6, 1, 0, 7, 3, 2, 4])

    def kw():
        if how == "subset_sampler":
            return dict(batch_size=2, drop_last=True, sampler=torch.utils.data.SubsetRandomSampler(idx))
        if how == "shuffle":
            return dict(batch_size=3, drop_last=False, shuffle=True)
        return dict(batch_size=3, drop_last=False)

    torch.manual_seed(7)
    theirs = [b for _ in range(2) for b in torch.utils.data.DataLoader(dataset, collate_fn=PatchDataset.collate, **kw())]
    after_theirs = torch.rand(1)
    torch.manual_seed(7)
    loader = ResidentDocLoader(dataset, store, **kw())
    ours = [b for _ in range(2) for b in loader]
    assert torch.equal(after_theirs, torch.rand(1))                              # the same use of the global generator
    assert len(ours) == len(theirs) == 2 * len(loader)
    for a, b in zip(ours, theirs):
        assert torch.equal(a[0], b[0]) and list(a[1]) == b[1] and a[2] == b[2]
        assert isinstance(a[1], DocBoxes) and a[1].store is store and [store.paths[r] for r in a[1].rows] == a[2]
        assert a[1][0] is store.boxes[a[1].rows[0]]


def test_pack_round_trip_and_rebuild(tmp_path, doc_dir):
    import shutil
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    root = str(tmp_path / "docs")
    shutil.copytree(doc_dir, root)
    ds = PatchDataset(root, pad=True, include_name=True)
    pack = str(tmp_path / "packs" / "docs.npz")
    a = ResidentDocuments.load_or_build(ds, pack)
    assert a.from_pack is False and os.path.exists(pack)
    b = ResidentDocuments.load_or_build(ds, pack)
    assert b.from_pack is True
    rows = range(len(a))
    assert torch.equal(a.batch(rows), b.batch(rows)) and a.boxes == b.boxes and np.array_equal(a.box, b.box)
    # a rewritten .json (another size) is seen by the signature: the pack is rebuilt and the new boxes are read
    path = ds.files[DF.ONE].rsplit(".", 1)[0] + ".json"
    json.dump(DF._as_json([(7, 180, 93, 211, "ab"), (3, 3, 40, 20, "cde")], quad=False), open(path, "w"))
    c = ResidentDocuments.load_or_build(ds, pack)
    assert c.from_pack is False and c.n_boxes[DF.ONE] == 2 and c.boxes[DF.ONE] == ds[DF.ONE][1]
    # the same size, another mtime
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
    assert ResidentDocuments.load_or_build(ds, pack).from_pack is False
    assert ResidentDocuments.load_or_build(ds, pack).from_pack is True
    # a foreign file in the pack's place
    open(pack, "wb").write(b"not a pack")
    assert ResidentDocuments.load_or_build(ds, pack).from_pack is False


def test_max_gb_refuses(dataset):
    from datasets.resident import ResidentDocuments, resident_documents
    from qea._lib import QeaError
    with pytest.raises(QeaError, match="resident_max_gb"):
        ResidentDocuments(dataset, max_gb=1e-4)                                  # 107 KB: passed while the second document is decoded
    with pytest.raises(QeaError, match="PatchDataset"):
        resident_documents(list(range(3)), "cpu")


def _reference_crops(store, x, rows):
    from utils import get_text_stack
    return torch.cat([get_text_stack(x[i], store.boxes[r], OUT)[0] for i, r in enumerate(rows)])


def test_numpy_crops_equal_get_text_stack(store):
    """crops() on the host against get_text_stack per document, forward and backward, on the documents whose boxes lie in the canvas.
    Overlapping boxes: the store adds in ascending box order, autograd in its own, so the gradients there are integers (sums of
    integers below 2^24 are exact in fp32 in any order); on the documents without overlaps they are real-valued."""
    from datasets.resident import DocBoxes
    from utils import get_text_stack, get_text_stacks
    g = torch.Generator().manual_seed(3)
    rows = DF.IN_CANVAS + [DF.OVERLAP, DF.CORNERS]                               # a repeated document too
    x = torch.rand(len(rows), 1, H, W, generator=g).requires_grad_()
    ours = store.crops(x, rows, *OUT)
    ref = _reference_crops(store, x, rows)
    assert tuple(ours.shape) == (int(store.n_boxes[rows].sum()), 1) + OUT and torch.equal(ours, ref)
    dout = torch.randint(-8, 9, ours.shape, generator=g).float()
    assert torch.equal(torch.autograd.grad(ours, x, dout)[0], torch.autograd.grad(ref, x, dout)[0])
    apart = [DF.PLACEHOLDER, DF.CORNERS, DF.ONE, DF.WIDE, DF.TALL]
    x = torch.rand(len(apart), 1, H, W, generator=g).requires_grad_()
    ours, ref = store.crops(x, apart, *OUT), _reference_crops(store, x, apart)
    dout = torch.randn(ours.shape, generator=g)
    assert torch.equal(ours, ref) and torch.equal(torch.autograd.grad(ours, x, dout)[0], torch.autograd.grad(ref, x, dout)[0])
    # utils.get_text_stacks: a host store loops get_text_stack, and so do plain lists
    lists = DocBoxes([store.boxes[r] for r in apart], store, apart)
    for box_lists in (lists, list(lists)):
        crops, labels = get_text_stacks(x, box_lists, OUT)
        assert torch.equal(crops, ref) and labels == [[b["label"] for b in store.boxes[r]] for r in apart]
    # a smaller target than the boxes: the floor division of an oversize crop, by odd amounts
    ours, ref = store.crops(x, apart, 8, 20), torch.cat([get_text_stack(x[i], store.boxes[r], (8, 20))[0] for i, r in enumerate(apart)])
    assert torch.equal(ours, ref)


def test_backward_spec_adds_in_ascending_box_order(store):
    """The specification itself: a pixel under three boxes gets ((0 + a) + b) + c in fp32."""
    from datasets.resident import doc_crops_backward_spec
    box = np.array([[0, 0, 4, 1]] * 3, dtype=np.int32)
    dout = np.zeros((3, 1, 4), dtype=np.float32)
    dout[:, 0, 0] = [1e8, 1.0, -1e8]
    d = doc_crops_backward_spec(dout, box, np.array([0, 3], np.int32), np.array([0]), np.array([0, 3], np.int32), 1, 4)
    assert d[0, 0, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1)) - np.float32(1e8)) == 0.0
    d = doc_crops_backward_spec(dout[::-1].copy(), box, np.array([0, 3], np.int32), np.array([0]), np.array([0, 3], np.int32), 1, 4)
    assert d[0, 0, 0] == 0.0 and doc_crops_backward_spec(dout[[0, 2, 1]].copy(), box, np.array([0, 3], np.int32), np.array([0]),
                                                         np.array([0, 3], np.int32), 1, 4)[0, 0, 0] == 1.0


def test_patch_parser_carries_the_flags():
    from qea.cli_flags import build_parser
    ap = build_parser("p", "")
    d = ap.parse_args([])
    assert d.resident is False and d.resident_pack is None and d.resident_max_gb == 8
    on = ap.parse_args(["--resident", "--resident_pack", "p.npz", "--resident_max_gb", "0.5"])
    assert on.resident is True and on.resident_pack == "p.npz" and on.resident_max_gb == 0.5
    acts = {a.option_strings[0]: a for a in ap._actions if a.option_strings}
    assert all(acts[f].help.startswith("[new]") for f in ("--resident", "--resident_pack", "--resident_max_gb"))
    assert "document" in acts["--resident"].help


def test_abi_has_the_two_entry_points():
    from qea import _lib
    protos = {name: (res, args) for name, res, args in _lib.header_prototypes()}
    assert len(protos["qea_doc_crops_gather"][1]) == 15 and len(protos["qea_doc_crops_scatter"][1]) == 16
    L = _lib.lib()
    assert hasattr(L, "qea_doc_crops_gather") and hasattr(L, "qea_doc_crops_scatter") and L.qea_version() == 9
    # refused before any launch: null pointers, OW not a multiple of 4, W not a multiple of 4 (no device needed)
    one = 16
    assert L.qea_doc_crops_gather(None, 1, 8, 8, None, None, 1, 1, None, None, 1, 4, 4, None, None) < 0
    assert L.qea_doc_crops_gather(one, 1, 8, 8, one, one, 1, 1, one, one, 1, 4, 6, one, None) < 0
    assert L.qea_doc_crops_scatter(one, 1, 4, 4, one, one, 1, 1, one, one, one, 1, 8, 6, 0, None) < 0
    assert L.qea_doc_crops_scatter(one, 1, 4, 4, one, one, 1, 1, one, one, one, 1, 8, 8, 2, None) < 0
    assert L.qea_doc_crops_scatter(one, 1, 4, 4, one, one, 1, 1, one, one, 8, 1, 8, 8, 0, None) < 0      # dimg misaligned
    assert b"16-byte" in L.qea_last_error()


def test_pack_files_hold_exactly_their_keys(tmp_path, dataset):
    """The two .npz layouts (format 1 of each): a pack written by an earlier version loads, and an earlier version loads these."""
    import resident_fixture as RF
    from datasets.img_dataset import ImgDataset
    from datasets.resident import DOC_PACK_FORMAT, PACK_FORMAT, ResidentDocuments, ResidentStrips
    assert PACK_FORMAT == 1 and DOC_PACK_FORMAT == 1
    RF.write_strips(str(tmp_path / "strips"))
    ResidentStrips.load_or_build(ImgDataset(str(tmp_path / "strips")), RF.SIZE, str(tmp_path / "strips.npz"))
    ResidentDocuments.load_or_build(dataset, str(tmp_path / "docs.npz"))
    with np.load(tmp_path / "strips.npz", allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["pixels", "offset", "h", "w", "names", "labels", "signature", "size"])
    with np.load(tmp_path / "docs.npz", allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["pixels", "offset", "h", "w", "src", "paths", "signature", "size"])
        assert z["src"].dtype == np.int32 and z["src"].tolist() == [[h, w] for h, w, _ in DF.DOCS] and z["size"].tolist() == [H, W]


def test_strip_store_and_document_store_agree(doc_dir, store):
    """The documents that fit the canvas are strips of a ResidentStrips with the canvas as its size: the two stores share the packing
    and the batch, so their batches are the same tensor."""
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentStrips
    strips = ResidentStrips(ImgDataset(doc_dir), DF.CANVAS)
    assert [os.path.basename(p) for p in store.paths] == strips.names
    fit = [i for i, how in enumerate(store.branch) if how == "fit"]
    assert len(fit) == 6
    assert torch.equal(strips.batch(fit), store.batch(fit)) and torch.equal(strips.batch(fit[::-1] + fit), store.batch(fit[::-1] + fit))


def _oracle_backend():
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    return Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)


def test_trainer_builds_the_stores_and_refuses(tmp_path):
    """patch_cli's trainer: plain DataLoader by default; with --resident the two stores (and their packs) and a ResidentDocLoader,
    also when --image_prop rebuilds the loader; refused with --synthetic_size or with a training set that is not a PatchDataset."""
    import patch_cli  # noqa: F401  (the front end imports without side effects)
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocLoader
    from datasets.synthetic import SyntheticPatches
    from ocr_helper.stub_helper import StubHelper
    from qea._lib import QeaError
    from qea.cli_flags import build_parser
    from train_nn_patch import TrainNNPrep
    root = DF.write_trainer_documents(str(tmp_path / "docs"))
    tr, va = PatchDataset(root, pad=True, include_name=True), PatchDataset(root, pad=True)

    def make(train, val, **over):
        a = build_parser("p", "").parse_args(["--exp_base_path", str(tmp_path / "exp"), "--ocr", "stub", "--epoch", "1", "--inner_limit", "1"])
        for k, v in over.items():
            setattr(a, k, v)
        return TrainNNPrep(a, backend=_oracle_backend(), train_set=train, val_set=val, ocr=StubHelper())

    t = make(tr, va)
    assert type(t.loader_train) is torch.utils.data.DataLoader and t.store_train is None and t.store_val is None
    pack = tmp_path / "packs" / "docs.npz"
    t = make(tr, va, resident=True, resident_pack=str(pack), docs_per_step=2)
    assert type(t.loader_train) is ResidentDocLoader and t.loader_train.store is t.store_train and len(t.loader_train) == 2
    assert len(t.store_train) == len(t.store_val) == 4 and t.store_train.device.type == "cpu"
    assert os.path.exists(pack) and os.path.exists(tmp_path / "packs" / "docs.val.npz")
    assert type(t._loader(t._train_idx[:2])) is ResidentDocLoader                # what --image_prop builds every epoch
    with pytest.raises(QeaError, match="synthetic_size"):
        make(tr, va, resident=True, synthetic_size=8)
    with pytest.raises(QeaError, match="PatchDataset"):
        make(SyntheticPatches(4, seed=1), va, resident=True)
