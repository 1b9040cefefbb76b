"""Connected components of the ink of ragged page lists (csrc/components.hip): labels, component tables, the area filter that follows a
classic binariser (despeckle), and word boxes by run-length smearing, which give clean_cli.py the <name>.json files PatchDataset reads.

The statement (tests/components_spec.py spells it out; DESIGN.md "Connected components" says why it is exact and why it terminates).  A
page is read as 8-bit grey exactly as binarize_pages reads it; a pixel is ink iff v8 <= ink_max (0..254, default 127).
  * Labels, connectivity 4 or 8: an ink pixel's label is the smallest row-major index y * w + x within its page over the pixels of its
    component (int32: pages are capped at 2^27 pixels), background is -1.  No scheduling order enters.
  * Component table, per page: int32 [n, 6] = (root, area, x_min, y_min, x_max, y_max), inclusive, rows ascending by root: reading order
    by each component's first pixel.
  * Despeckle: 0 where the pixel is ink and its component has at least min_area (>= 1) pixels, else 255 / 1.0.
  * Smear: along rows with gap gx, a background pixel becomes ink iff its row has ink at distance a >= 1 to the left and b >= 1 to the
    right with a + b - 1 <= gx; then along columns with gy on that result; a gap of 0 skips its pass; gaps 0..127.
  * Word boxes, per page: int32 [n, 4] = (x_min, y_min, x_max, y_max), inclusive, of the 8-connected components of the smeared page with
    a smeared area >= min_area, ascending by root.  Smearing fills only between ink, so a box also bounds the original ink inside it.
All of it is integer work: the device, the host path below and the statement agree bit for bit.

CUDA pages (or a CUDA `device`) run the kernels over the packed store: label = three launches, stats, despeckle, each smear direction and
boxes one launch each, a fixed sequence whatever the pages hold.  The despeckle path never synchronises; the table and box functions read
the per-page component counts back, once, to size their results.  CPU tensors run the host path: row runs, the links between runs of
neighbouring rows, and pointer jumping over the runs, all in numpy.
"""
import numpy as np
import torch

from .pages import _check_out, host_pages, is_int, open_store, pack_host, pack_ink_host, packed_result, unpack_pages

MAX_GAP, MAX_PAGE_PIXELS = 127, 1 << 27


def check_params(connectivity=8, ink_max=127, min_area=1, gap_x=0, gap_y=0):
    """ValueError for parameters outside the statement's ranges, before any work"""
    if not is_int(connectivity) or connectivity not in (4, 8):
        raise ValueError(f"connectivity={connectivity!r}: 4 or 8")
    if not is_int(ink_max) or not 0 <= ink_max <= 254:
        raise ValueError(f"ink_max={ink_max!r}: an integer in 0..254")
    if not is_int(min_area) or min_area < 1 or min_area >= 2 ** 31:
        raise ValueError(f"min_area={min_area!r}: an integer >= 1")
    for name, g in (("gap_x", gap_x), ("gap_y", gap_y)):
        if not is_int(g) or not 0 <= g <= MAX_GAP:
            raise ValueError(f"{name}={g!r}: an integer in 0..{MAX_GAP}")


# ---------------------------------------------------------------------------------------------------------------- the host path
def _runs(ink):
    """bool [h, w] -> the maximal row runs of ink in row-major order: (row, start, end) with end exclusive"""
    d = np.diff(np.pad(ink, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    row, start = np.nonzero(d == 1)
    return row, start, np.nonzero(d == -1)[1]


def _run_labels(ink, connectivity):
    """-> (row, start, end, label): label = the page-relative index of the first pixel of the smallest run of the run's component"""
    h, w = ink.shape
    row, start, end = _runs(ink)
    n, K, c = row.size, w + 2, int(connectivity == 8)
    lab = np.arange(n)
    if n:
        # run j of row r touches the runs i of row r - 1 with end_i > start_j - c and start_i < end_j + c; runs of a row are disjoint
        # and ascending, so those are one range of the row-major order, found by two searches over keys row * K + position
        first = np.searchsorted(row * K + end, (row - 1) * K + start - c, side="right")
        last = np.searchsorted(row * K + start, (row - 1) * K + end + c, side="left")
        count = np.maximum(last - first, 0)
        begin = np.concatenate([[0], np.cumsum(count)[:-1]])
        b = np.repeat(np.arange(n), count)                     # the links (a, b): run a of the row above touches run b
        a = np.repeat(first - begin, count) + np.arange(b.size)
        # the links of one run are one segment of a list sorted by that run: its minimum is one reduceat (np.minimum.at is far slower)
        runs_b = np.flatnonzero(count)
        begin_b = begin[runs_b]
        by_a = np.argsort(a, kind="stable")
        runs_a, begin_a = np.unique(a[by_a], return_index=True)
        while a.size:                                          # hook every link to the smaller label, then jump; labels only fall
            m = np.minimum(lab[a], lab[b])
            new = lab.copy()
            new[runs_b] = np.minimum(new[runs_b], np.minimum.reduceat(m, begin_b))
            new[runs_a] = np.minimum(new[runs_a], np.minimum.reduceat(m[by_a], begin_a))
            new = new[new]
            if np.array_equal(new, lab):
                break
            lab = new
    return row, start, end, (row * w + start)[lab]


def _labels_host(ink, connectivity):
    row, start, end, label = _run_labels(ink, connectivity)
    out = np.full(ink.shape, -1, np.int32)
    out.reshape(-1)[np.flatnonzero(ink)] = np.repeat(label, end - start)
    return out


def _table_of_runs(row, start, end, label):
    roots, inv = np.unique(label, return_inverse=True)
    t = np.empty((roots.size, 6), np.int64)
    t[:, 0] = roots
    t[:, 1] = np.bincount(inv, weights=end - start, minlength=roots.size)
    t[:, 2:4] = np.iinfo(np.int64).max
    t[:, 4:] = -1
    np.minimum.at(t[:, 2], inv, start)
    np.minimum.at(t[:, 3], inv, row)
    np.maximum.at(t[:, 4], inv, end - 1)
    np.maximum.at(t[:, 5], inv, row)
    return t.astype(np.int32), inv


def _despeckle_host(ink, min_area, connectivity):
    """-> bool [h, w]: the ink of components of at least min_area pixels"""
    row, start, end, label = _run_labels(ink, connectivity)
    table, inv = _table_of_runs(row, start, end, label)
    keep = np.zeros(ink.shape, bool)
    keep.reshape(-1)[np.flatnonzero(ink)] = np.repeat(table[inv, 1] >= min_area, end - start)
    return keep


def _smear_rows(ink, gap):
    if gap == 0:
        return ink
    h, w = ink.shape
    row, start, end = _runs(ink)
    fill = np.flatnonzero((row[1:] == row[:-1]) & (start[1:] - end[:-1] <= gap))
    delta = np.zeros((h, w + 1), np.int32)
    np.add.at(delta, (row[fill], end[fill]), 1)
    np.add.at(delta, (row[fill], start[fill + 1]), -1)
    return ink | (np.cumsum(delta, 1)[:, :w] > 0)


def _smear_host(ink, gap_x, gap_y):
    return np.ascontiguousarray(_smear_rows(np.ascontiguousarray(_smear_rows(ink, gap_x).T), gap_y).T)


def _boxes_host(ink, gap_x, gap_y, min_area):
    table, _ = _table_of_runs(*_run_labels(_smear_host(ink, gap_x, gap_y), 8))
    return np.ascontiguousarray(table[table[:, 1] >= min_area, 2:])


def _host_inks(pk, ink_max):
    return (v <= ink_max for v in host_pages(pk))


# ---------------------------------------------------------------------------------------------------------------- the device path
def despeckle_store(store, table, min_area, connectivity=8, ink_max=127, out="float"):
    """The device sequence over a packed store that is already on the device (binarize_pages hands its result over without unpacking):
    label (3 launches), stats, apply -> the packed result.  Nothing synchronises."""
    from . import ops
    area = torch.empty(store.numel(), dtype=torch.int32, device=store.device)
    labels = ops.cc_label(store, table, connectivity, ink_max, area=area)
    ops.cc_stats(store, table, labels, area)
    res, outs = packed_result(store.numel(), out, store.device)
    ops.cc_despeckle(store, table, labels, area, min_area, **outs)
    return res


def despeckle_store_host(pk, min_area, connectivity=8, ink_max=127, out="float"):
    """the same over a packed store on the host"""
    return pack_ink_host(pk, (_despeckle_host(ink, min_area, connectivity) for ink in _host_inks(pk, ink_max)), out)


def _device_tables(pk, store, table, labels, area, min_area):
    """labels and areas on the device -> per page int32 [n, 6] of the components with area >= min_area.  One read of the per-page counts;
    the roots themselves are found without another: the k-th listed root is where the running count reaches k + 1."""
    from . import ops
    dev = store.device
    running = torch.cumsum(area >= min_area, 0, dtype=torch.int32)
    ends = torch.from_numpy((pk.offset + pk.h.astype(np.int64) * pk.w.astype(np.int64) - 1)).to(dev)
    root_first = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), running[ends]])
    first = root_first.cpu().tolist()                          # the one read: sizes the result
    n = first[-1]
    at = torch.searchsorted(running, torch.arange(1, n + 1, dtype=torch.int32, device=dev))
    page = torch.searchsorted(root_first[1:].contiguous(), torch.arange(n, dtype=torch.int32, device=dev), right=True)
    roots = (at - torch.from_numpy(pk.offset).to(dev)[page]).to(torch.int32)
    boxes = ops.cc_boxes(store, table, labels, roots, root_first)
    rows = torch.cat([roots[:, None], area[at][:, None], boxes], 1)
    return [rows[a:b] for a, b in zip(first[:-1], first[1:])]


def _open(pages, device):
    return open_store(pages, device, max_pixels=MAX_PAGE_PIXELS)      # labels are int32 indices into a page


# ---------------------------------------------------------------------------------------------------------------- the interface
def label_pages(pages, connectivity=8, ink_max=127, device=None):
    """pages as for binarize_pages -> a list of int32 [h, w]: the smallest page-relative index of each ink pixel's component, -1 for
    background; on `device` if given, else where the pages are"""
    check_params(connectivity, ink_max)
    pk, dev, store, table = _open(pages, device)
    if dev.type == "cuda":
        from . import ops
        res = ops.cc_label(store, table, connectivity, ink_max)
    else:
        res = pack_host(pk, [_labels_host(ink, connectivity) for ink in _host_inks(pk, ink_max)], torch.int32)
    return [v.view(v.shape[-2], v.shape[-1]) for v in unpack_pages(res, pk)]


def page_components(pages, connectivity=8, ink_max=127, device=None):
    """-> per page int32 [n, 6] = (root, area, x_min, y_min, x_max, y_max), inclusive, rows ascending by root"""
    check_params(connectivity, ink_max)
    pk, dev, store, table = _open(pages, device)
    if dev.type == "cuda":
        from . import ops
        area = torch.empty(store.numel(), dtype=torch.int32, device=dev)
        labels = ops.cc_label(store, table, connectivity, ink_max, area=area)
        ops.cc_stats(store, table, labels, area)
        return _device_tables(pk, store, table, labels, area, 1)
    return [torch.from_numpy(_table_of_runs(*_run_labels(ink, connectivity))[0]) for ink in _host_inks(pk, ink_max)]


def despeckle_pages(pages, min_area, connectivity=8, ink_max=127, out="float", device=None):
    """-> pages as binarize_pages returns them (0 / 255 uint8 for out="u8", 0.0 / 1.0 fp32 for out="float"): ink of components of at least
    min_area pixels stays ink, everything else is background.  min_area = 1 only binarises at ink_max."""
    _check_out(out)
    check_params(connectivity, ink_max, min_area)
    pk, dev, store, table = _open(pages, device)
    if dev.type == "cuda":
        res = despeckle_store(store, table, min_area, connectivity, ink_max, out)
    else:
        res = despeckle_store_host(pk, min_area, connectivity, ink_max, out)
    return unpack_pages(res, pk)


def word_boxes(pages, gap_x=8, gap_y=0, min_area=16, ink_max=127, device=None):
    """-> per page int32 [n, 4] = (x_min, y_min, x_max, y_max), inclusive: the bounding boxes of the 8-connected components of the page
    smeared by gap_x along rows and then gap_y along columns, whose smeared area is at least min_area, in ascending root order"""
    check_params(8, ink_max, min_area, gap_x, gap_y)
    pk, dev, store, table = _open(pages, device)
    if dev.type == "cuda":
        from . import ops
        mask = None
        if gap_x:
            mask = ops.cc_smear(store, table, gap_x, False, ink_max)
        if gap_y:
            mask = ops.cc_smear(store, table, gap_y, True, ink_max, in_mask=mask)
        area = torch.empty(store.numel(), dtype=torch.int32, device=dev)
        labels = ops.cc_label(store, table, 8, ink_max, ink_mask=mask, area=area)
        ops.cc_stats(store, table, labels, area)
        return [t[:, 2:].contiguous() for t in _device_tables(pk, store, table, labels, area, min_area)]
    return [torch.from_numpy(_boxes_host(ink, gap_x, gap_y, min_area)) for ink in _host_inks(pk, ink_max)]
