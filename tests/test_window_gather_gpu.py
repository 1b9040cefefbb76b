"""The window gather (csrc/window_gather.h) on the MI355X through its three kernels, by direct `ops` calls of a few hundred elements, each
bit for bit against the specification in the tree: strip_batch_spec and doc_crops_spec (datasets/resident.py), tiles_gather_spec
(qea/pages.py).  Edge phase: the window's edges on every position inside a quad, empty windows, sources larger than the output.  Tail:
a quad count that is no multiple of the workgroup.  Guards: table entries past the lengths the call names give white images.  Every
output is prefilled with NaN, so an element nobody wrote shows up as well.  (grid.y's stride over more than 65535 images:
tests/test_resident_gpu.py::test_more_images_than_grid_rows, which runs the shared body.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OH, OW = 3, 12
SIZES = [(h, w) for h in range(1, 6) for w in range(1, 14)]            # source heights 1..5, widths 1..13
TAIL = (5, 260)                                                        # 325 quads: one full workgroup and a partial one


def _up(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _packed(sizes, dtype, seed):
    """items of `sizes` in one store, three junk elements between them and an odd first offset -> (store, offset, h, w)"""
    rng = np.random.RandomState(seed)
    offset, off = [], 1
    for h, w in sizes:
        offset.append(off)
        off += h * w + 3
    store = rng.randint(0, 256, off).astype(np.uint8) if dtype == np.uint8 else (rng.rand(off) * 1.5 - 0.25).astype(np.float32)
    return store, np.asarray(offset, np.int64), np.asarray([s[0] for s in sizes], np.int32), np.asarray([s[1] for s in sizes], np.int32)


# ------------------------------------------------------------------------------------------------ strips
def _strips(sizes, rows, oh, ow, anchor, n=None):
    """ops.strip_batch on the first n table entries (views of the whole tables) -> (device result, specification on ALL entries)"""
    from datasets.resident import norm_table, strip_batch_spec
    from qea import ops
    pixels, offset, h, w = _packed(sizes, np.uint8, 3)
    n = len(sizes) if n is None else n
    rows = np.asarray(rows, np.int64)
    out = _nan(len(rows), 1, oh, ow)
    ops.strip_batch(_up(pixels), _up(offset)[:n], _up(h)[:n], _up(w)[:n], _up(rows), _up(norm_table()), out, anchor)
    return out.cpu().numpy(), strip_batch_spec(pixels, offset, h, w, norm_table(), rows, oh, ow, anchor)


@pytest.mark.parametrize("anchor", ["centre", "left"])
def test_edge_phase_strips(anchor):
    sizes = SIZES + [(2, 0), (0, 0)]                                   # and two strips without a pixel
    got, want = _strips(sizes, range(len(sizes)), OH, OW, anchor)
    assert np.array_equal(got, want)
    assert bool((want[-2:] == 1).all()) and bool((want[:-2] != 1).any())


def test_tail_strips():
    got, want = _strips([(5, 260), (7, 300), (3, 259), (1, 1), (4, 257)], [4, 0, 1, 2, 3, 0], *TAIL, "centre")
    assert np.array_equal(got, want)


def test_guard_strips():
    """Six strips in the tables, four named to the call: indices 4 and 5 are out of range for the call and inside the allocations."""
    rows = [0, 4, 3, 5, 1, 2, 5]
    got, want = _strips([(3, 9), (2, 12), (5, 13), (1, 4), (3, 11), (2, 7)], rows, OH, OW, "centre", n=4)
    bad = np.asarray(rows) >= 4
    assert bool((want[bad] != 1).any())                                # the specification on all six does show them
    want[bad] = 1
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ crops
def _crops(imgs, box, box_first, doc, first, oh, ow, n_docs=None, n_boxes=None):
    """ops.doc_crops_gather on the first n_docs / n_boxes table entries (views of the whole tables) -> (device result, specification
    on ALL entries)"""
    from datasets.resident import doc_crops_spec
    from qea import ops
    n_docs = len(box_first) - 1 if n_docs is None else n_docs
    n_boxes = len(box) if n_boxes is None else n_boxes
    out = _nan(int(first[-1]), 1, oh, ow)
    ops.doc_crops_gather(_up(imgs)[:, None], _up(box)[:n_boxes], _up(box_first)[:n_docs + 1], _up(doc), _up(first), out)
    return out.cpu().numpy()[:, 0], doc_crops_spec(imgs, box, box_first, doc, first, oh, ow)


def test_edge_phase_crops():
    """A box of every size in an 8 x 16 image: OW - cw runs from 11 to -1 and OH - ch from 2 to -2, the odd negative ones (the floor
    division) included; an empty box; three documents of 20, 1 and 45 boxes taken in another order."""
    H, W = 8, 16
    box = [[(3 * w + h) % (W - w + 1), (w + h) % (H - h + 1)] for h, w in SIZES]
    box = np.asarray([[x, y, x + w, y + h] for (x, y), (h, w) in zip(box, SIZES)] + [[5, 2, 5, 4]], np.int32)
    box_first = np.asarray([0, 20, 21, 66], np.int32)
    doc, first = np.asarray([2, 0, 1], np.int64), np.asarray([0, 45, 65, 66], np.int32)
    imgs = np.random.RandomState(4).rand(3, H, W).astype(np.float32)
    got, want = _crops(imgs, box, box_first, doc, first, OH, OW)
    assert np.array_equal(got, want)
    assert bool((want[44] == 1).all()) and bool((want[:44] != 1).any(axis=(1, 2)).all())      # strip 44 is the empty box


def test_tail_crops():
    H, W = 8, 272
    box = np.asarray([[0, 0, 272, 8], [3, 1, 262, 6], [10, 2, 11, 3], [5, 0, 264, 5]], np.int32)
    imgs = np.random.RandomState(5).rand(2, H, W).astype(np.float32)
    got, want = _crops(imgs, box, np.asarray([0, 3, 4], np.int32), np.asarray([1, 0], np.int64), np.asarray([0, 1, 4], np.int32), *TAIL)
    assert np.array_equal(got, want)


def test_guard_crops():
    """Four documents with ten boxes in the tables, two documents and five boxes named to the call.  White: the strips of documents 2
    and 3, boxes 5 and 6 of document 1, and a fourth strip of the three-box document 0 (box 3 exists, but is document 1's)."""
    H, W = 8, 16
    box = np.asarray([[1 + i, i % 3, 9 + i % 6, 4 + i % 4] for i in range(10)], np.int32)
    box_first = np.asarray([0, 3, 7, 9, 10], np.int32)
    doc, first = np.asarray([1, 2, 0, 3], np.int64), np.asarray([0, 4, 6, 10, 11], np.int32)
    imgs = np.random.RandomState(6).rand(4, H, W).astype(np.float32)
    got, want = _crops(imgs, box, box_first, doc, first, OH, OW, n_docs=2, n_boxes=5)
    bad = [2, 3, 4, 5, 9, 10]
    assert bool((want != 1).any(axis=(1, 2)).all())                    # the specification on the whole tables shows all eleven
    want[bad] = 1
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ pages
def _tiles(sizes, dtype, rows, th, tw, n_pages=None):
    """ops.page_tiles_gather on the first n_pages table entries (views of the whole tables) -> (device result, specification on ALL)"""
    from qea import ops
    from qea.pages import norm_table, tiles_gather_spec
    store, offset, h, w = _packed(sizes, dtype, 7)
    n_pages = len(sizes) if n_pages is None else n_pages
    rows = np.asarray(rows, np.int32)
    out = _nan(len(rows), 1, th, tw)
    ops.page_tiles_gather(_up(store), _up(offset)[:n_pages], _up(h)[:n_pages], _up(w)[:n_pages], _up(rows), out,
                          norm_table().cuda() if dtype == np.uint8 else None)
    return out.cpu(), tiles_gather_spec(torch.from_numpy(store), offset, h, w, rows, th, tw)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_edge_phase_pages(dtype):
    """A page of every size, each cut at ox in -3..3 and oy in -2..2: 2275 tiles of 3 x 12 in one launch."""
    rows = [(p, oy, ox) for p in range(len(SIZES)) for oy in range(-2, 3) for ox in range(-3, 4)]
    got, want = _tiles(SIZES, dtype, rows, OH, OW)
    assert torch.equal(got, want)
    assert bool((want == 1).flatten(1).all(1).any()) and bool((want != 1).any())              # some windows are empty


def test_tail_pages():
    got, want = _tiles([(6, 300), (5, 259)], np.uint8, [(0, 0, 0), (0, -1, 37), (1, 1, -2), (0, 3, 45), (1, 0, 0)], *TAIL)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_guard_pages(dtype):
    """Four pages in the tables, two named to the call: tiles of pages 2 and 3 are white, their neighbours right."""
    rows = [(0, 0, 0), (2, 0, 0), (1, -1, 2), (3, 1, -1), (1, 0, 0)]
    got, want = _tiles([(3, 12), (4, 9), (3, 13), (5, 12)], dtype, rows, OH, OW, n_pages=2)
    assert bool((want != 1).flatten(1).any(1).all())
    want[[1, 3]] = 1
    assert torch.equal(got, want)
