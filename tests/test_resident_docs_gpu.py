"""The resident document store on the MI355X: its batches against the CPU store (which tests/test_resident_docs_cpu.py holds against
PatchDataset's samples), qea_doc_crops_gather / qea_doc_crops_scatter (csrc/doc_crops.hip) against the per-document path they
replace and against the numpy specification, and patch_cli's trainer with --resident against itself without it.  Every comparison is
exact: the gather copies values, the scatter adds in a fixed order, and the trainers' kernels are deterministic."""
import numpy as np
import pytest
import torch

import resident_docs_fixture as DF

pytestmark = pytest.mark.gpu
H, W = DF.CANVAS
OUT = (32, 128)
FIVE = [DF.PLACEHOLDER, DF.CORNERS, DF.ONE, DF.MANY, DF.OVERLAP]                  # box counts 1 / 37 / 1 / 300 / overlapping


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """(CPU store, device store) of the fixture's eight documents."""
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    ds = PatchDataset(DF.write_documents(str(tmp_path_factory.mktemp("docs"))), pad=True, include_name=True)
    return ResidentDocuments(ds), ResidentDocuments(ds, device="cuda")


@pytest.fixture(scope="module")
def full(stores):
    return stores[0].batch(range(len(stores[0])))


def _images(n, seed):
    return torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(seed)).cuda()


def _per_document(dev, x, rows, out=OUT):
    """The path the one launch replaces: get_text_stack's CUDA branch per document, concatenated."""
    from utils import get_text_stack
    return torch.cat([get_text_stack(x[i], dev.boxes[r], out)[0] for i, r in enumerate(rows)])


@pytest.mark.parametrize("rows", ["all", [5], [3, 3, 7, 0, 6, 3, 1]])
def test_device_batch_equals_cpu_store(stores, full, rows):
    from qea import ops
    cpu, dev = stores
    rows = list(range(len(cpu))) if rows == "all" else rows
    before = ops.STRIP_LAUNCHES["batch"]
    got = dev.batch(rows)
    assert ops.STRIP_LAUNCHES["batch"] == before + 1                             # one launch per batch
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(rows), 1, H, W)
    assert torch.equal(got.cpu(), full[rows])


@pytest.mark.parametrize("rows", [[DF.ONE], FIVE, [DF.NEGATIVE, DF.WIDE, DF.TALL, DF.NEGATIVE]])
def test_gather_equals_the_per_document_path(stores, rows):
    """One launch whatever N is, bit-identical to get_text_stack's CUDA path per document; the document with a negative box
    coordinate is held against that path alone (python slicing takes another branch there)."""
    from qea import ops
    from utils import get_text_stacks
    from datasets.resident import DocBoxes
    cpu, dev = stores
    x = _images(len(rows), 11)
    ref = _per_document(dev, x, rows)
    before = dict(ops.DOC_LAUNCHES)
    got = dev.crops(x, rows, *OUT)
    assert ops.DOC_LAUNCHES == {"gather": before["gather"] + 1, "scatter": before["scatter"]}
    assert tuple(got.shape) == (int(cpu.n_boxes[rows].sum()), 1) + OUT and torch.equal(got, ref)
    # the same through utils.get_text_stacks, with the labels per document
    crops, labels = get_text_stacks(x, DocBoxes([dev.boxes[r] for r in rows], dev, rows), OUT)
    assert ops.DOC_LAUNCHES["gather"] == before["gather"] + 2 and torch.equal(crops, ref)
    assert labels == [[b["label"] for b in dev.boxes[r]] for r in rows]
    if DF.NEGATIVE not in rows:                                                  # and the numpy specification
        assert torch.equal(got.cpu(), cpu.crops(x.cpu(), rows, *OUT))
    # a target smaller than most boxes: the floor division of an oversize crop
    assert torch.equal(dev.crops(x, rows, 8, 20), _per_document(dev, x, rows, (8, 20)))


def test_gather_writes_every_element(stores):
    from qea import ops
    _, dev = stores
    x = _images(len(FIVE), 12)
    doc, first = dev.strip_tables(FIVE)
    out = torch.full((int(first[-1]), 1) + OUT, float("nan"), device="cuda")
    ops.doc_crops_gather(x, dev.box, dev.box_first, torch.from_numpy(doc).cuda(), torch.from_numpy(first).cuda(), out)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, _per_document(dev, x, FIVE))


def _tiny():
    """H=5, W=8, OH=3, OW=4: two documents; crops larger than the target by odd amounts (7x5 and 6x4 against 4x3), a box clipped to
    zero width, one smaller than the target."""
    box = np.array([[0, 0, 7, 5], [8, 1, 8, 4], [2, 1, 4, 2], [1, 0, 7, 4], [0, 0, 8, 5]], dtype=np.int32)
    box_first = np.array([0, 3, 5], dtype=np.int32)
    doc = np.array([1, 0, 1], dtype=np.int64)
    first = np.array([0, 2, 5, 7], dtype=np.int32)
    return box, box_first, doc, first


def test_tiny_direct_call_against_the_specification():
    from datasets.resident import doc_crops_backward_spec, doc_crops_spec
    from qea import ops
    box, box_first, doc, first = _tiny()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 1, 5, 8, generator=g)
    up = lambda a: torch.from_numpy(a).cuda()
    out = torch.full((7, 1, 3, 4), float("nan"), device="cuda")
    ops.doc_crops_gather(x.cuda(), up(box), up(box_first), up(doc), up(first), out)
    spec = doc_crops_spec(x.numpy()[:, 0], box, box_first, doc, first, 3, 4)
    assert np.array_equal(out.cpu().numpy()[:, 0], spec)
    assert bool((out[3] == 1).all())                                             # the zero-width box: all white
    assert np.array_equal(spec[2, :, :], x.numpy()[1, 0, 1:4, 2:6])              # 7x5 -> 4x3: columns 2..5 (the extra one lost left), rows 1..3
    dout = torch.randn(7, 1, 3, 4, generator=g)
    dimg = torch.full((3, 1, 5, 8), float("nan"), device="cuda")
    ops.doc_crops_scatter(dout.cuda(), up(box), up(box_first), up(doc), up(first), dimg)
    assert np.array_equal(dimg.cpu().numpy()[:, 0], doc_crops_backward_spec(dout.numpy()[:, 0], box, box_first, doc, first, 5, 8))
    with pytest.raises(Exception):
        ops.doc_crops_gather(x.cuda(), up(box), up(box_first), up(doc), up(first[:-1].copy()), out)


def _scatter(dev, dout, rows, dimg=None, accumulate=False):
    from qea import ops
    doc, first = dev.strip_tables(rows)
    if dimg is None:
        dimg = torch.full((len(rows), 1, H, W), float("nan"), device="cuda")     # no prior fill is needed: every element is written
    ops.doc_crops_scatter(dout, dev.box, dev.box_first, torch.from_numpy(doc).cuda(), torch.from_numpy(first).cuda(), dimg, accumulate)
    return dimg


def _old_scatter(dev, dout, rows):
    """memset + qea_crop_pad_scatter (atomicAdd) per document: the backward of the per-document path."""
    from qea import ops
    res, a = [], 0
    for r in rows:
        n = len(dev.boxes[r])
        dimg = torch.zeros(1, H, W, device="cuda")
        ops.crop_pad_scatter(dout[a:a + n].contiguous(), dev.box[int(dev._host_box_first[r]): int(dev._host_box_first[r]) + n].contiguous(), n,
                             OUT[0], OUT[1], dimg, H, W)
        res.append(dimg)
        a += n
    return torch.stack(res)


def test_scatter_adds_in_ascending_box_order(stores):
    """Real-valued gradients on the five documents (overlaps inside an LDS chunk and across the chunk border of the 300-box document):
    bit-identical to the numpy fp32 sum in ascending box order, twice; accumulate; one launch."""
    from datasets.resident import doc_crops_backward_spec
    from qea import ops
    cpu, dev = stores
    rows = FIVE + [DF.MANY]
    doc, first = cpu.strip_tables(rows)
    g = torch.Generator().manual_seed(21)
    dout = torch.randn(int(first[-1]), 1, *OUT, generator=g)
    spec = doc_crops_backward_spec(dout.numpy()[:, 0], cpu.box, cpu.box_first, doc, first, H, W)
    before = dict(ops.DOC_LAUNCHES)
    a = _scatter(dev, dout.cuda(), rows)
    assert ops.DOC_LAUNCHES == {"gather": before["gather"], "scatter": before["scatter"] + 1}
    assert bool(torch.isfinite(a).all())                                         # the NaN fill is gone everywhere
    assert np.array_equal(a.cpu().numpy()[:, 0], spec)
    assert torch.equal(_scatter(dev, dout.cuda(), rows), a)                      # fixed by the inputs
    covered = torch.from_numpy(doc_crops_backward_spec(np.ones_like(dout.numpy()[:, 0]), cpu.box, cpu.box_first, doc, first, H, W))
    assert int((covered > 1).sum()) > 1000 and bool((a.cpu()[:, 0][covered == 0] == 0).all())
    # accumulate adds the same sum to what dimg holds
    base = torch.randn(len(rows), 1, H, W, generator=g)
    got = _scatter(dev, dout.cuda(), rows, dimg=base.cuda().clone(), accumulate=True)
    assert np.array_equal(got.cpu().numpy()[:, 0], doc_crops_backward_spec(dout.numpy()[:, 0], cpu.box, cpu.box_first, doc, first, H, W,
                                                                           dimg=base.numpy()[:, 0]))
    # boxes that do not overlap: the old memset + atomic scatter, bit for bit, with real-valued gradients
    apart = [DF.CORNERS, DF.ONE, DF.WIDE, DF.TALL, DF.PLACEHOLDER]
    d = torch.randn(int(cpu.n_boxes[apart].sum()), 1, *OUT, generator=g).cuda()
    assert torch.equal(_scatter(dev, d, apart), _old_scatter(dev, d, apart))


def test_scatter_integer_gradients_equal_the_atomic_scatter(stores):
    """Integer gradients in -8..8: sums are exact in any order, so the overlapping documents must equal memset + atomicAdd."""
    cpu, dev = stores
    rows = [DF.OVERLAP, DF.MANY, DF.NEGATIVE]
    g = torch.Generator().manual_seed(22)
    dout = torch.randint(-8, 9, (int(cpu.n_boxes[rows].sum()), 1) + OUT, generator=g).float().cuda()
    assert torch.equal(_scatter(dev, dout, rows), _old_scatter(dev, dout, rows))


def test_autograd_through_get_text_stacks(stores):
    """The autograd function: the gradient of the one-launch crops is the scatter's, one launch, and equals the per-document
    path's on integer gradients."""
    from qea import ops
    _, dev = stores
    x = _images(len(FIVE), 13).requires_grad_()
    crops = dev.crops(x, FIVE, *OUT)
    dout = torch.randint(-8, 9, crops.shape, generator=torch.Generator().manual_seed(23)).float().cuda()
    before = ops.DOC_LAUNCHES["scatter"]
    got, = torch.autograd.grad(crops, x, dout)
    assert ops.DOC_LAUNCHES["scatter"] == before + 1
    ref, = torch.autograd.grad(_per_document(dev, x, FIVE), x, dout)
    assert torch.equal(got, ref) and torch.equal(got, _scatter(dev, dout, FIVE))


@pytest.mark.parametrize("docs_per_step", [1, 2])
def test_patch_trainer_resident_equals_sample_loader(tmp_path, docs_per_step):
    """patch_cli --resident against itself without it: 4 documents, 2 epochs, --inner_limit 2, topKCER at 0.5, stub OCR.  The boxes
    of this folder do not overlap, so the atomic scatter of the run without the flag is exact too and every kernel on both paths is
    order-fixed: the same logged numbers, the same black-box calls, bit-identical UNet and CRNN."""
    from qea import ops
    doc_dir = DF.write_trainer_documents(str(tmp_path / "docs"))
    res = {}
    for resident in (False, True):
        before = dict(ops.DOC_LAUNCHES)
        res[resident] = DF.patch_run(tmp_path, doc_dir, resident, docs_per_step)
        used = {k: ops.DOC_LAUNCHES[k] - before[k] for k in before}
        if resident:
            steps = 2 * (4 // docs_per_step)
            assert used == {"gather": 2 * steps + 2 * 4, "scatter": steps}, used  # Phase A, Phase B and validation; Phase B's backward
        else:
            assert used == {"gather": 0, "scatter": 0}
    (rows0, calls0, unet0, crnn0, _), (rows1, calls1, unet1, crnn1, _) = res[False], res[True]
    assert rows0 == rows1 and calls0 == calls1 and calls0 > 0
    assert torch.equal(unet0, unet1) and torch.equal(crnn0, crnn1)
