"""The shared lookups of csrc/page_store.h on the MI355X: ONE hand-built store, with junk before the first page and between the pages,
goes through every tile- or chunk-mapped entry point of csrc/binarize.hip, components.hip and deskew.hip, and every result is compared
bit for bit with the product's host path on the same pages; what lies between the pages keeps its sentinel.  The five pages hit every edge
of the 32 x 64 tiling and of the prefix search: 1 x 1, exactly one tile, 2 x 2 ragged tiles, one tile row of four columns, and a page three
pixels wide; the 33 x 65 page runs alone as well (n_pages = 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (32, 64), (33, 65), (5, 200), (70, 3)]
A, SLOPES = 90, [0, 37, -90, 5, 0]
U8, F32, I32 = 0x5A, -7.0, -77               # the sentinels


def _store(shapes, dtype, seed=23):
    """-> (store, offset, h, w): the pages at offsets 5, +7 junk elements after each page; junk and pages are random"""
    g = torch.Generator().manual_seed(seed)
    offset, off = [], 5
    for h, w in shapes:
        offset.append(off)
        off += h * w + 7
    store = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8) if dtype == torch.uint8 else torch.rand(off, generator=g) * 1.5 - 0.25
    return store, np.asarray(offset, np.int64), np.asarray([s[0] for s in shapes], np.int32), np.asarray([s[1] for s in shapes], np.int32)


def _packed(n, offset, arrays, sentinel, dtype):
    """what a kernel must leave in an output of n elements prefilled with `sentinel`: the arrays at the offsets, the sentinel elsewhere"""
    want = torch.full((n,), sentinel, dtype=dtype)
    for o, a in zip(offset, arrays):
        a = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).reshape(-1)
        want[int(o):int(o) + a.numel()] = a.to(dtype)
    return want


@pytest.mark.parametrize("shapes", [SHAPES, SHAPES[2:3]], ids=["five_pages", "one_page"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_every_family_finds_the_same_pages_and_tiles(dtype, shapes):
    from qea import ops
    from qea.binarize import binarize_pages, otsu_thresholds
    from qea.components import _smear_host, despeckle_pages, label_pages, page_components
    from qea.deskew import _strip_sums_host, deskew_pages, rotation_table
    from qea.pages import norm_table, quantise_u8
    host_store, offset, h, w = _store(shapes, dtype)
    n, slopes = host_store.numel(), SLOPES[:len(shapes)] if len(shapes) > 1 else [37]
    pages = [host_store[int(o):int(o) + int(a) * int(b)].view(int(a), int(b)) for o, a, b in zip(offset, h, w)]
    v8 = [(p if dtype == torch.uint8 else quantise_u8(p)).numpy() for p in pages]
    store = host_store.cuda()
    table = ops.page_table(offset, h, w, store.device)
    assert table.n == len(shapes) and offset[0] == 5

    def fresh(sentinel, dt):
        return torch.full((n,), sentinel, dtype=dt, device="cuda")

    def same(got, arrays, sentinel, what):
        assert torch.equal(got.cpu(), _packed(n, offset, arrays, sentinel, got.dtype)), what

    for window in (3, 25):                                     # Sauvola: the tile lookup with a one-pixel and a 12-pixel halo
        u8, f32 = fresh(U8, torch.uint8), fresh(F32, torch.float32)
        ops.binarize_sauvola(store, table, window, 0.2, 128.0, out_f32=f32, out_u8=u8)
        same(u8, binarize_pages(pages, "sauvola", window=window, out="u8"), U8, f"sauvola {window} u8")
        same(f32, binarize_pages(pages, "sauvola", window=window, out="float"), F32, f"sauvola {window} float")

    u8, f32 = fresh(U8, torch.uint8), fresh(F32, torch.float32)   # Otsu: the chunk lookup
    hist = ops.otsu_histogram(store, table)
    assert np.array_equal(hist.cpu().numpy(), np.stack([np.bincount(v.reshape(-1), minlength=256) for v in v8]))
    thresholds = ops.binarize_otsu(store, table, hist, out_f32=f32, out_u8=u8)
    assert torch.equal(thresholds.cpu(), otsu_thresholds(pages))
    same(u8, binarize_pages(pages, "otsu", out="u8"), U8, "otsu u8")
    same(f32, binarize_pages(pages, "otsu", out="float"), F32, "otsu float")

    for conn in (4, 8):                                        # components: label (three kernels), stats, despeckle, boxes
        labels, area = fresh(I32, torch.int32), fresh(I32, torch.int32)
        ops.cc_label(store, table, conn, 127, labels=labels, area=area)
        ops.cc_stats(store, table, labels, area)
        same(labels, label_pages(pages, conn, 127), I32, f"labels {conn}")
        tables = page_components(pages, conn, 127)
        want_area = []
        for t, (a, b) in zip(tables, shapes):
            full = np.zeros(a * b, np.int32)
            full[t[:, 0].numpy()] = t[:, 1].numpy()
            want_area.append(full)
        same(area, want_area, I32, f"area {conn}")
        u8, f32 = fresh(U8, torch.uint8), fresh(F32, torch.float32)
        ops.cc_despeckle(store, table, labels, area, 3, out_f32=f32, out_u8=u8)
        same(u8, despeckle_pages(pages, 3, conn, 127, out="u8"), U8, f"despeckle {conn} u8")
        same(f32, despeckle_pages(pages, 3, conn, 127, out="float"), F32, f"despeckle {conn} float")
        roots = torch.cat([t[:, 0] for t in tables]).to(torch.int32).cuda()
        first = torch.tensor(np.concatenate([[0], np.cumsum([len(t) for t in tables])]), dtype=torch.int32).cuda()
        assert torch.equal(ops.cc_boxes(store, table, labels, roots, first).cpu(), torch.cat([t[:, 2:] for t in tables])), f"boxes {conn}"

    for vertical in (False, True):                             # smear: the tile with its halo along either axis
        mask = ops.cc_smear(store, table, 5, vertical, 127, out_mask=fresh(U8, torch.uint8))
        same(mask, [_smear_host(v <= 127, 0 if vertical else 5, 5 if vertical else 0).astype(np.uint8) for v in v8], U8, f"smear {vertical}")

    C = ops.skew_strip_sums(store, table, 127, C=fresh(U8, torch.uint8))      # page p's ceil(w / 32) x h counts lead its elements
    same(C, [_strip_sums_host(v, 127) for v in v8], U8, "strip sums")

    rot = torch.from_numpy(rotation_table(A)).cuda()           # rotate: given slopes, 0 (the identity) among them
    given = torch.tensor(slopes, dtype=torch.int32).cuda()
    for interp in ("bilinear", "nearest"):
        u8, f32 = fresh(U8, torch.uint8), fresh(F32, torch.float32)
        ops.deskew_rotate(store, table, given, rot, interp, 255, norm=norm_table().cuda(), out_f32=f32, out_u8=u8)
        same(u8, deskew_pages(pages, A, interp=interp, out="u8", slopes=slopes)[0], U8, f"rotate {interp} u8")
        same(f32, deskew_pages(pages, A, interp=interp, out="float", slopes=slopes)[0], F32, f"rotate {interp} float")
    assert torch.equal(store.cpu(), host_store)                # nothing wrote to the store
