"""Whole pages of any size through the eval-mode UNet, tile by tile (csrc/page_tiles.hip).

In eval mode the UNet is a LOCAL function of its input: BatchNorm is an affine map folded into the conv epilogue and nothing looks at the
batch.  A page can therefore be cleaned in tiles, and the stitched result IS the whole-page pass — provided every pixel that is kept sees,
inside its tile, everything it sees on the page.

HALO = 96.  Through the deepest path an output pixel reaches 2 + 4 + 8 + 16 px through the 3x3 convs of the four decoder blocks (two convs
each at strides 1, 2, 4, 8), 32 px through the bottleneck (two convs at stride 16) and 16 + 8 + 4 + 2 px through the encoder blocks: 92 px of
3x3 reach, plus the alignment of the 2x2 pools and transposed convs, which makes single pixels reach up to 102 px (measured with the fp64
oracle: one flipped column of a 16x640 strip changes outputs 226..429 around columns 327/328).  The pools and transposed convs snap to the
16-px grid of the deepest level; with every tile origin and every core boundary on a multiple of 16 the alignment term drops out and 96 px
(the next multiple of 16 above 92) is enough, while 80 is not (stitched against whole, fp64 oracle, f = 8):

    shape            tile  halo  max difference
    16x640 strip     320    64   7.6e-3
    16x640 strip     320    80   1.3e-3
    16x640 strip     320    96   0.0
    16x640 strip     320   112   0.0
    437x531 page     320    96   2.3e-15   (2 x 3 tiles)
    437x531 page     320    80   1.06e-2
    33x900 page      208    96   1.7e-15   (1 x 45 tiles, core step 16)

The plan of one axis (plan_axis): the page length L is padded with white (1.0) at the right / bottom only to Lp = ceil(L / 16) * 16.
Lp <= T: one tile at 0 of size Lp, core [0, Lp).  Otherwise tiles of size T: the first at origin 0 with core [0, T - HALO); each next
origin is + (T - 2 * HALO), its core runs from the previous core's end to origin + T - HALO; once origin + T >= Lp the last tile sits at
Lp - T and its core runs to Lp.  Tile sides on the page edge coincide with the tile's own edge, so the convs' zero padding falls where the
whole-page pass has it — which is why the first origin is 0 and the last Lp - T, not a centred layout.  The 2-D plan is the product of the
two axes.  The result is therefore: the eval-mode pass over the page padded with white to the next multiple of 16 at the right and
bottom, cropped back to h x w.

clean_pages is the device path: pages packed into one store, all tiles of all pages planned on the host, grouped by tile shape so that
tiles of different pages share passes, cut by ONE launch per chunk (qea_page_tiles_gather), sent through the model's own eval-mode no-grad
forward, pasted by ONE launch per chunk (qea_page_tiles_scatter).  clean_pages_spec is the same plan in plain torch around any callable:
the specification of the two kernels (tiles_gather_spec / tiles_scatter_spec) and of the stitching, and the host backend's path.
"""
from collections import namedtuple

import numpy as np
import torch

from ._lib import QeaError

HALO = 96

# Default pixels per UNet pass.  What the engine's eval-mode no-grad forward (qea/unet_engine.py) keeps alive per INPUT pixel at f = 32,
# counted at its peak inside decoder1's second conv: the four concat buffers, which live for the whole pass (level l: 2c fp32 channels at
# 1/4^(l-1) of the pixels = 256 + 128 + 64 + 32 B), decoder2's output (64 channels at 1/4: 64 B), decoder1's first activation and its
# output (32 channels each: 128 + 128 B), input and output (4 + 4 B): 808 B, call it 1 KiB with the allocator's rounding.  2^23 pixels are
# 8 GiB of working set, eight 1024 x 1024 tiles per pass — and the pixel count of the benchmark's 2048 strips of 32 x 128, the largest pass
# the engine's kernels are exercised at.
MAX_TILE_PIXELS = 1 << 23


def _check_tile(T, halo):
    if T % 16 or T < 2 * halo + 16:
        raise ValueError(f"tile side {T} must be a multiple of 16 and at least 2 * {halo} + 16 = {2 * halo + 16}")


def plan_axis(L, T, halo=HALO):
    """-> [(origin, size, core0, core1)] of one axis of length L with tiles of at most T (the module docstring has the rule).  Origins, sizes
    and core bounds are multiples of 16; the cores partition [0, Lp), Lp = L rounded up to a multiple of 16."""
    L, T = int(L), int(T)
    _check_tile(T, halo)
    if L < 1:
        raise ValueError(f"page side {L} < 1")
    Lp = (L + 15) // 16 * 16
    if Lp <= T:
        return [(0, Lp, 0, Lp)]
    plan, o, c0 = [], 0, 0
    while o + T < Lp:
        plan.append((o, T, c0, o + T - halo))
        c0 = o + T - halo
        o += T - 2 * halo
    plan.append((Lp - T, T, c0, Lp))
    return plan


def plan_tiles(h, w, tile, halo=HALO):
    """-> (TH, TW, [(oy, ox, cy0, cy1, cx0, cx1)]): the tiles of an h x w page, row after row; all have the size TH x TW."""
    ys, xs = plan_axis(h, tile[0], halo), plan_axis(w, tile[1], halo)
    return ys[0][1], xs[0][1], [(oy, ox, cy0, cy1, cx0, cx1) for oy, _, cy0, cy1 in ys for ox, _, cx0, cx1 in xs]


Packed = namedtuple("Packed", "store offset h w dims")     # store: 1-D tensor; offset int64 / h / w int32 numpy [n]; dims: each page's dim()


def pack_pages(pages):
    """A list of [h, w] uint8 pages, or of [h, w] / [1, h, w] floating pages (one kind per call), of any sizes -> Packed: the pages
    back to back in one store of their dtype, on the device of the first page."""
    if not len(pages):
        raise ValueError("no pages")
    flat, hs, ws, dims = [], [], [], []
    for i, p in enumerate(pages):
        if not torch.is_tensor(p):
            p = torch.as_tensor(p)
        if p.dim() == 3 and p.shape[0] == 1 and p.dtype != torch.uint8:
            q = p[0]
        elif p.dim() == 2:
            q = p
        else:
            raise ValueError(f"page {i}: {tuple(p.shape)} {p.dtype} is neither [h, w] uint8 nor [h, w] / [1, h, w] floating")
        if (flat and q.dtype != flat[0].dtype) or not (q.dtype == torch.uint8 or q.is_floating_point()) or q.numel() == 0:
            raise ValueError(f"page {i}: {tuple(p.shape)} {p.dtype}; pages are all uint8 or all of one floating type, and not empty")
        flat.append(q.reshape(-1))
        hs.append(q.shape[0])
        ws.append(q.shape[1])
        dims.append(p.dim())
    sizes = np.asarray(hs, np.int64) * np.asarray(ws, np.int64)
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return Packed(torch.cat(flat), offset, np.asarray(hs, np.int32), np.asarray(ws, np.int32), dims)


def unpack_pages(store, pk):
    """the pages of a store packed like `pk`, as views with the dims the caller's pages had"""
    out = []
    for o, h, w, d in zip(pk.offset, pk.h, pk.w, pk.dims):
        v = store[int(o):int(o) + int(h) * int(w)].view(int(h), int(w))
        out.append(v[None] if d == 3 else v)
    return out


# ---- the Python side of a packed store, shared by qea/binarize.py, components.py, deskew.py and reading.py (csrc/page_store.h is the
# device and library side)
def is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_page_sizes(pages, max_side=None, max_pixels=None):
    """QeaError for a page with a side over max_side or more than max_pixels (a power of two) pixels; None: no such bound.  Runs before
    anything is packed or copied and looks at nothing but .shape."""
    for i, p in enumerate(pages):
        shape = tuple(getattr(p, "shape", ()))
        if len(shape) < 2:
            continue
        h, w = int(shape[-2]), int(shape[-1])
        over = ([f"a side over {max_side}"] if max_side and max(h, w) > max_side else []) + \
               ([f"more than 2^{int(max_pixels).bit_length() - 1} pixels"] if max_pixels and h * w > max_pixels else [])
        if over:
            raise QeaError(f"page {i}: {h} x {w} has " + " and ".join(over))


def _device_store(pk, dev):
    """the store as the kernels read it: 8-bit as it is, anything floating as fp32"""
    return pk.store.to(dev) if pk.store.dtype == torch.uint8 else pk.store.to(dev, torch.float32)


def open_store(pages, device=None, max_side=None, max_pixels=None):
    """check_page_sizes and pack_pages, then the store where the work runs -> (pk, dev, store, table).  dev is `device` if given, else
    where the pages are.  On a CUDA dev, store is the device store and table its ops.page_table; on the host, pk.store is moved to the
    CPU, store is pk.store and table is None."""
    check_page_sizes(pages, max_side, max_pixels)
    pk = pack_pages(pages)
    dev = torch.device(device) if device is not None else pk.store.device
    if dev.type != "cuda":
        pk = pk._replace(store=pk.store.cpu())
        return pk, dev, pk.store, None
    from . import ops
    return pk, dev, _device_store(pk, dev), ops.page_table(pk.offset, pk.h, pk.w, dev)


def host_page(pk, p):
    """page p of a packed host store as the statements read it: uint8 numpy [h, w] (a view of an 8-bit store, quantise_u8 of a floating one)"""
    o, h, w = int(pk.offset[p]), int(pk.h[p]), int(pk.w[p])
    page = pk.store[o:o + h * w].view(h, w)
    return (page if page.dtype == torch.uint8 else quantise_u8(page)).numpy()


def host_pages(pk):
    """all of them, one after the other"""
    return (host_page(pk, p) for p in range(len(pk.h)))


def pack_host(pk, arrays, dtype):
    """one numpy array per page, of the page's size -> a host tensor of `dtype` packed like pk.store"""
    res = torch.empty(pk.store.numel(), dtype=dtype)
    for o, a in zip(pk.offset, arrays):
        res[int(o):int(o) + a.size] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    return res


def pack_ink_host(pk, inks, out):
    """one bool array per page -> the packed binarised result: 0 where it is set (ink), 255 for out="u8" / 1.0 for "float" elsewhere"""
    hi, dtype = (np.uint8(255), torch.uint8) if out == "u8" else (np.float32(1.0), torch.float32)
    return pack_host(pk, (np.where(ink, hi.dtype.type(0), hi) for ink in inks), dtype)      # in the result's type: no 8-byte detour


def packed_result(n, out, device):
    """-> (res, kw): the packed result of n elements for out="u8" / "float" on `device`, and the out_u8= / out_f32= keyword that hands it
    to a wrapper of qea/ops.py"""
    res = torch.empty(n, dtype=torch.uint8 if out == "u8" else torch.float32, device=device)
    return res, {"out_u8" if out == "u8" else "out_f32": res}


def require_eval(model, who):
    if getattr(model, "training", False) or any(m.training for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)):
        raise ValueError(f"{who} needs the model in eval mode: with batch statistics a result depends on what shares its pass")


def plan_groups(hs, ws, tile, halo=HALO):
    """All tiles of all pages, grouped by tile shape: -> {(TH, TW): int32 [n][7] = (page, oy, ox, cy0, cy1, cx0, cx1)}, shapes in sorted
    order, the tiles of a shape page after page."""
    groups = {}
    for p, (h, w) in enumerate(zip(hs, ws)):
        TH, TW, rows = plan_tiles(int(h), int(w), tile, halo)
        groups.setdefault((TH, TW), []).extend((p,) + r for r in rows)
    return {k: np.asarray(groups[k], np.int32).reshape(-1, 7) for k in sorted(groups)}


def norm_table():
    """float32(p) / 255 for the 256 byte values, rounded once on the host (datasets/resident.py: norm_table)"""
    from datasets.resident import norm_table as table
    return torch.from_numpy(table())


def quantise_u8(x):
    """The 8-bit rule of qea_page_tiles_scatter: (uint8)(min(max(x, 0), 1) * 255) in fp32, truncated — what ToPILImage makes of a float
    tensor, and what the OCR engines and save_img see.  NaN gives 0."""
    x = x.float()
    return (torch.where(x != x, torch.zeros_like(x), x).clamp(0, 1) * 255).to(torch.uint8)


def tiles_gather_spec(store, offset, h, w, rows, TH, TW, table=None):
    """Specification of qea_page_tiles_gather in torch slicing: rows [N][>= 3] = (page, oy, ox, ...) -> [N, 1, TH, TW], white outside a page.
    A uint8 store goes through `table` (default norm_table()) and gives fp32; a floating store keeps its dtype."""
    if store.dtype == torch.uint8:
        table = (norm_table() if table is None else table).to(store.device)
    tiles = []
    for r in np.asarray(rows):
        p, oy, ox = int(r[0]), int(r[1]), int(r[2])
        ph, pw, off = int(h[p]), int(w[p]), int(offset[p])
        page = store[off:off + ph * pw].view(ph, pw)
        t = torch.ones(TH, TW, dtype=torch.float32 if store.dtype == torch.uint8 else store.dtype, device=store.device)
        y0, y1, x0, x1 = max(oy, 0), min(oy + TH, ph), max(ox, 0), min(ox + TW, pw)
        if y0 < y1 and x0 < x1:
            src = page[y0:y1, x0:x1]
            t[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = table[src.long()] if store.dtype == torch.uint8 else src
        tiles.append(t)
    return torch.stack(tiles)[:, None]


def tiles_scatter_spec(tiles, rows, offset, h, w, out_f=None, out_u8=None):
    """Specification of qea_page_tiles_scatter: tiles [N, 1, TH, TW], rows [N][7] -> the core of every tile, cut to the tile and to the page,
    copied into the packed outputs (out_f of the tiles' dtype and / or out_u8 by quantise_u8), one copy_ per tile."""
    TH, TW = tiles.shape[2], tiles.shape[3]
    for t, r in zip(tiles, np.asarray(rows)):
        p, oy, ox, cy0, cy1, cx0, cx1 = (int(v) for v in r)
        ph, pw, off = int(h[p]), int(w[p]), int(offset[p])
        y0, y1, x0, x1 = max(cy0, oy, 0), min(cy1, oy + TH, ph), max(cx0, ox, 0), min(cx1, ox + TW, pw)
        if y0 >= y1 or x0 >= x1:
            continue
        src = t[0, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        if out_f is not None:
            out_f[off:off + ph * pw].view(ph, pw)[y0:y1, x0:x1].copy_(src)
        if out_u8 is not None:
            out_u8[off:off + ph * pw].view(ph, pw)[y0:y1, x0:x1].copy_(quantise_u8(src))


def _check_out(out):
    if out not in ("float", "u8"):
        raise ValueError(f"out={out!r}: 'float' or 'u8'")


def clean_pages_spec(forward, pages, tile, halo=HALO, out="float", max_tile_pixels=None):
    """The tiled pass in plain torch around any callable forward([n, 1, TH, TW]) -> [n, 1, TH, TW] (the model's eval-mode pass, the
    fp64 oracle): pages as for clean_pages -> a list of the same sizes; floating results keep the dtype forward returns.  `halo` is an
    argument only so that a test can show a seam with too small a one."""
    _check_out(out)
    pk = pack_pages(pages)
    res = None
    for (TH, TW), rows in plan_groups(pk.h, pk.w, tile, halo).items():
        step = len(rows) if not max_tile_pixels else max(1, int(max_tile_pixels) // (TH * TW))
        for i in range(0, len(rows), step):
            y = forward(tiles_gather_spec(pk.store, pk.offset, pk.h, pk.w, rows[i:i + step], TH, TW))
            if res is None:
                res = torch.empty(pk.store.numel(), dtype=torch.uint8 if out == "u8" else y.dtype, device=y.device)
            tiles_scatter_spec(y, rows[i:i + step], pk.offset, pk.h, pk.w, **{"out_u8" if out == "u8" else "out_f": res})
    return unpack_pages(res, pk)


def clean_pages(model, pages, tile=(1024, 1024), max_tile_pixels=None, out="float"):
    """pages: a list of [h, w] uint8 tensors (8-bit grey, read as p / 255) or of [h, w] / [1, h, w] float tensors, of any sizes ->
    a list of the same sizes on the model's device: for every page the model's eval-mode pass over the page padded with white to the
    next multiple of 16 at the right and bottom, cropped back (fp32 for out="float", quantise_u8 of it for out="u8").
    tile = (TH, TW): the largest tile, each side a multiple of 16 and at least 2 * HALO + 16 = 208; the default keeps 61 % of an interior
    tile as core (the training canvas 400 x 512 would keep 25 %).  max_tile_pixels: pixels per UNet pass (default MAX_TILE_PIXELS; at
    least one tile runs per pass).  A model on the host (the oracle backend) runs clean_pages_spec."""
    from . import ops
    _check_out(out)
    for T in tile:
        _check_tile(int(T), HALO)
    require_eval(model, "clean_pages")
    budget = int(max_tile_pixels) if max_tile_pixels else MAX_TILE_PIXELS
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        with torch.no_grad():
            return clean_pages_spec(lambda x: model(x.to(dev)), pages, tile, out=out, max_tile_pixels=budget)
    pk = pack_pages(pages)
    store = _device_store(pk, dev)
    table = norm_table().to(dev) if store.dtype == torch.uint8 else None
    offset, h, w = (torch.from_numpy(a).to(dev) for a in (pk.offset, pk.h, pk.w))
    groups = plan_groups(pk.h, pk.w, tile)
    rows7 = torch.from_numpy(np.concatenate(list(groups.values()))).to(dev)          # every table of the call in one upload
    rows3 = rows7[:, :3].contiguous()
    res, outs = packed_result(store.numel(), out, dev)
    first = 0
    with torch.no_grad():
        for (TH, TW), rows in groups.items():
            step = max(1, budget // (TH * TW))
            for i in range(first, first + len(rows), step):
                n = min(step, first + len(rows) - i)
                x = torch.empty(n, 1, TH, TW, device=dev)
                ops.page_tiles_gather(store, offset, h, w, rows3[i:i + n], x, table)
                y = model(x).contiguous()
                ops.page_tiles_scatter(y, rows7[i:i + n], offset, h, w, **outs)
            first += len(rows)
    return unpack_pages(res, pk)
