"""[new] Strip datasets kept resident: every file of an ImgDataset is decoded ONCE, its 8-bit grey pixels packed into one flat
buffer, and each minibatch is built from that buffer by one gather / white-pad / normalise pass (--resident of area_cli.py and
train_crnn.py).

The per-sample path this replaces runs, for every image of every epoch, Image.open -> convert("L") -> PadWhite (thumbnail of oversize
strips, ImageOps.expand) -> float32 / 255 -> torch.stack -> a pageable host-to-device copy.  The store keeps exactly what that path
has BEFORE the pad (the decode and the thumbnail stay in PIL, so the pixels are the loader's), and `batch()` reproduces the rest:

  ResidentStrips(dataset, size, device)   pixels (flat uint8, strips row-major without padding), offset int64 [n], h / w int32 [n];
                                          on the host: names (basenames), labels (ImgDataset.__getitem__'s rule), lens
      .batch(idx, out_w=None, anchor="centre") -> fp32 [B,1,H,out_w] on the store's device, bit-identical to
                                          torch.stack([dataset[i][0] for i in idx]) under the PadWhite((H, W)) + float32 / 255 transform
      device="cuda"   arrays on the GPU, one launch of qea_strip_batch (csrc/strip_batch.hip) per batch, nothing synchronises
      device="cpu"    numpy arrays and a numpy gather: the specification, and the path of the CPU tests
  ResidentStrips.load_or_build(dataset, size, pack_path)   the same through one .npz pack file with a signature of the file list
  ResidentLoader      a torch DataLoader over the INDICES (same sampler arguments, so the same batches, order and RNG draws as the
                      loader it replaces) whose batches come out as (images on the device, labels, names[, indices])

The same for the document flow (--resident of patch_cli.py), whose sample path also re-reads and re-parses every document's .json:

  ResidentDocuments(dataset, device)      a PatchDataset's documents as the dataset has them before its white pad (pixels / offset /
                                          h / w as above) and, per document, the box dicts of the dataset's own coord_loader; box
                                          int32 [total][4] (clipped to the canvas) and box_first int32 [n+1] on the device
      .batch(rows)                        fp32 [N,1,400,512] = torch.stack([dataset[i][0] for i in rows]): qea_strip_batch again
      .crops(images, rows, oh, ow)        ALL boxes of those documents cut out of `images` and centred on white: one launch forward
                                          and one order-fixed launch without atomics backward (csrc/doc_crops.hip); numpy on the host
  ResidentDocuments.load_or_build         the pack file; its signature also covers every .json
  ResidentDocLoader                       the index DataLoader again; yields [images, DocBoxes (box lists that name store and rows), paths]

Both stores are a _PackedStore (the packed pixels, their upload, the pack file, the index checks and the batch) and both loaders an
_IndexLoader; a store adds its decode, its signature, what it knows per item and its self-check.
"""
import hashlib
import json
import os
import time

import numpy as np
import torch
from PIL import Image

import properties
from datasets._io import ascii_label
from datasets.img_dataset import ImgDataset, _label_of
from qea._lib import QeaError

PACK_FORMAT = 1
ANCHORS = ("centre", "left")


def norm_table():
    """The loader's normalisation of the 256 byte values: float32(p) / 255, rounded once in fp32 on the host."""
    return np.arange(256, dtype=np.float32) / np.float32(255)


def _size(size):
    h, w = (size, size) if isinstance(size, int) else size
    return int(h), int(w)


def _label(path):
    """ImgDataset.__getitem__'s label of a file."""
    label = ascii_label(_label_of(path))
    return properties.empty_char if len(label) > properties.max_char_len else label


def _decode(path, H, W):
    """The loader's calls up to, not including, the pad: the grey image, shrunk by PadWhite's thumbnail rule when it exceeds (H, W)."""
    img = Image.open(path).convert("L")
    if img.size[0] > W or img.size[1] > H:
        img.thumbnail((W, H))
    return np.asarray(img, dtype=np.uint8)


def _stat_rows(files, with_json=False):
    """[relative name, byte size, st_mtime_ns] of every file (and of its .json), in listing order."""
    root = os.path.commonpath([os.path.dirname(os.path.abspath(f)) for f in files]) if files else ""
    rows = []
    for f in files:
        for g in (f, f.rsplit(".", 1)[0] + ".json") if with_json else (f,):
            st = os.stat(g)
            rows.append([os.path.relpath(os.path.abspath(g), root), st.st_size, st.st_mtime_ns])
    return rows


def _signature(files, H, W):
    """sha256 over the format version, the target size and (relative name, byte size, st_mtime_ns) of every file, in listing order."""
    return hashlib.sha256(json.dumps({"format": PACK_FORMAT, "size": [H, W], "files": _stat_rows(files)}).encode()).hexdigest()


class _PackedStore:
    """What the resident stores share.  Items (strips, documents) as 8-bit grey, row-major, back to back: pixels (flat uint8), offset
    int64 [n], h / w int32 [n] and the 256-entry table, numpy arrays on a host store and tensors on a device store; `_host` keeps the host
    arrays a pack file holds (PACKED names them), nbytes their pixels.  A subclass sets H, W and n, and names what else its pack file
    holds in _pack_extras()."""
    PACKED = ("pixels", "offset", "h", "w")

    def _open(self, device, max_gb):
        self.device = torch.device(device)
        if self.device.type not in ("cpu", "cuda"):
            raise QeaError(f"{type(self).__name__}: device {device!r} is neither cpu nor cuda")
        self.max_gb = float(max_gb)

    def __len__(self):
        return self.n

    def _guard(self, nbytes):
        if nbytes > self.max_gb * 2 ** 30:
            raise QeaError(f"the resident pack needs more than {nbytes / 2 ** 30:.3f} GB, above the limit of {self.max_gb:g} GB "
                           "(--resident_max_gb)")

    def _pack(self, decoded):
        """(pixels, offset, h, w) of an iterator of decoded uint8 [h, w] arrays."""
        chunks, offset, h, w, total = [], [], [], [], 0
        for a in decoded:
            offset.append(total)
            h.append(a.shape[0])
            w.append(a.shape[1])
            chunks.append(a.reshape(-1))
            total += a.size
            self._guard(total)                                                # refuse as soon as the limit is passed, not after the decode
        pixels = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
        return pixels, np.array(offset, dtype=np.int64), np.array(h, dtype=np.int32), np.array(w, dtype=np.int32)

    def _place(self, host, **tables):
        """Keeps the host arrays `host` (in PACKED order) for the pack file; pixels, offset, h, w, the table and `tables` become the
        store's attributes, on a device store as tensors (an empty array as one zero: every pointer is valid)."""
        self._guard(host[0].size)
        self._host, self.nbytes = tuple(host), int(host[0].size)
        arrays = dict(zip(_PackedStore.PACKED, host), table=norm_table(), **tables)
        if self.device.type == "cuda":
            from qea import _lib
            _lib.lib()                                                        # a missing kernel is an error here, not at the first batch
            arrays = {k: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.device) for k, a in arrays.items()}
        vars(self).update(arrays)

    # ---- the pack file ----
    @classmethod
    def _load_or_build(cls, n, pack_path, sig, make):
        """make(packed) through the pack file: `packed` holds the PACKED arrays of a pack whose signature is `sig` and that lists n items,
        None otherwise (no such file, an unreadable or foreign one, another signature); the store built from None overwrites the pack."""
        packed = None
        if pack_path and os.path.exists(pack_path):
            try:
                with np.load(pack_path, allow_pickle=False) as z:
                    if str(z["signature"]) == sig and len(z["offset"]) == n:
                        packed = tuple(z[k] for k in cls.PACKED)
            except (OSError, ValueError, KeyError):
                packed = None                                                 # unreadable or foreign file: rebuild
        store = make(packed)
        store.from_pack = packed is not None
        if packed is None and pack_path:
            store.save(pack_path, sig)
        return store

    def save(self, pack_path, signature=None):
        tmp = f"{pack_path}.tmp{os.getpid()}"
        os.makedirs(os.path.dirname(os.path.abspath(pack_path)), exist_ok=True)
        with open(tmp, "wb") as f:
            np.savez(f, **dict(zip(self.PACKED, self._host)), **self._pack_extras(), signature=np.array(signature or ""),
                     size=np.array([self.H, self.W], dtype=np.int32))
        os.replace(tmp, pack_path)

    # ---- batches ----
    def _rows(self, rows, what, noun="rows", device_tensor=True):
        """`rows` (a host sequence, an array or a tensor) as int64 [B], checked against 0..n-1: ValueError before any launch."""
        who = f"{type(self).__name__}.{what}"
        if isinstance(rows, torch.Tensor):
            if rows.is_cuda and not device_tensor:
                raise ValueError(f"{who}: idx is a host sequence or a CPU tensor")
            rows = rows.cpu().numpy()
        rows = np.ascontiguousarray(np.asarray(list(rows) if not isinstance(rows, np.ndarray) else rows).reshape(-1)).astype(np.int64, copy=False)
        if rows.size == 0:
            raise ValueError(f"{who}: no {noun}")
        if int(rows.min()) < 0 or int(rows.max()) >= self.n:
            raise ValueError(f"{who}: {noun} {int(rows.min())}..{int(rows.max())} outside 0..{self.n - 1}")
        return rows

    def _batch(self, rows, OH, OW, anchor="centre", out=None):
        """fp32 [B,1,OH,OW] on the store's device: item rows[b] on white, centred vertically and, by `anchor`, centred or at column 0,
        clipped to OH x OW.  Device store: one launch of qea_strip_batch.  Host store: numpy, the specification."""
        shape = (rows.size, 1, OH, OW)
        if self.device.type == "cuda":
            from qea import ops
            # a fresh pinned block per call: the caching host allocator hands it out again only after the copy below has run, so
            # neither a wait nor a second buffer is needed
            pinned = torch.empty(rows.size, dtype=torch.int64, pin_memory=True)
            pinned.numpy()[:] = rows
            d_rows = pinned.to(self.device, non_blocking=True)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
            ops.strip_batch(self.pixels, self.offset, self.h, self.w, d_rows, self.table, out, anchor)
            return out
        res = torch.from_numpy(strip_batch_spec(self.pixels, self.offset, self.h, self.w, self.table, rows, OH, OW, anchor))
        if out is not None:
            out.copy_(res)
            return out
        return res


def strip_batch_spec(pixels, offset, h, w, table, rows, OH, OW, anchor="centre"):
    """numpy specification of qea_strip_batch: the packed items `rows` -> fp32 [B,1,OH,OW]."""
    res = np.ones((len(rows), 1, OH, OW), dtype=np.float32)
    for b, s in enumerate(rows):
        sh, sw = int(h[s]), int(w[s])
        hh, ww = min(sh, OH), min(sw, OW)
        top = (OH - hh) // 2
        left = 0 if anchor == "left" else (OW - ww) // 2
        item = pixels[offset[s]: offset[s] + sh * sw].reshape(sh, sw)
        res[b, 0, top:top + hh, left:left + ww] = table[item[:hh, :ww]]
    return res


class ResidentStrips(_PackedStore):
    def __init__(self, dataset, size, device="cpu", max_gb=8.0, _packed=None):
        if not isinstance(dataset, ImgDataset):
            raise QeaError(f"ResidentStrips packs an ImgDataset, not a {type(dataset).__name__}")
        self.H, self.W = _size(size)
        self._open(device, max_gb)
        files = list(dataset.files)
        self.n = len(files)
        self.names = [os.path.basename(f) for f in files]
        self.labels = [_label(f) for f in files]
        self.lens = np.array([len(l) for l in self.labels], dtype=np.int32)
        t0 = time.perf_counter()
        host = self._pack(_decode(f, self.H, self.W) for f in files) if _packed is None else _packed
        self.build_seconds = time.perf_counter() - t0
        self._place(host)

    @classmethod
    def load_or_build(cls, dataset, size, pack_path, device="cpu", max_gb=8.0):
        """The store of `dataset` through the pack file at `pack_path` (.npz: pixels, offset, h, w, names, labels, signature).  A pack
        whose signature is not this dataset's (a file added, removed, resized or rewritten, another target size or format) is never
        used: the store is rebuilt from the files and the pack overwritten."""
        return cls._load_or_build(len(dataset.files), pack_path, _signature(dataset.files, *_size(size)),
                                  lambda packed: cls(dataset, size, device=device, max_gb=max_gb, _packed=packed))

    def _pack_extras(self):
        return dict(names=np.array(self.names, dtype=str), labels=np.array(self.labels, dtype=str))

    def batch(self, idx, out_w=None, anchor="centre", out=None):
        """fp32 [B,1,H,out_w] (out_w defaults to W) on the store's device; `out` (optional) receives it.  anchor="centre": PadWhite's
        placement, left = dw // 2, top = dh // 2.  anchor="left": column 0, centred vertically, a strip wider than out_w cropped to its
        first out_w columns (datasets.bucketing.pad_to_bucket).  Indices are checked on the host: ValueError before any launch."""
        if anchor not in ANCHORS:
            raise ValueError(f"unknown anchor {anchor!r}")
        idx = self._rows(idx, "batch", noun="indices", device_tensor=False)
        OW = self.W if out_w is None else int(out_w)
        if OW < 4 or OW % 4:
            raise ValueError(f"ResidentStrips.batch: out_w={OW} must be a positive multiple of 4")
        shape = (idx.size, 1, self.H, OW)
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device.type != self.device.type
                                or not out.is_contiguous()):
            raise ValueError(f"ResidentStrips.batch: out must be a contiguous fp32 {shape} tensor on {self.device}")
        return self._batch(idx, self.H, OW, anchor, out)


class _Indices(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class _IndexLoader:
    """The DataLoader of `dataset`, whose items sit in `store`, with the sampling left to torch: a DataLoader over the indices
    0..len(dataset)-1 with the caller's batch_size / drop_last / sampler / shuffle draws the same index batches, in the same order and
    with the same use of the global generator, as one over the samples.  A subclass turns each index batch into the sample loader's."""

    def __init__(self, dataset, store, loader_kw):
        if loader_kw.get("num_workers") or "collate_fn" in loader_kw or "batch_sampler" in loader_kw:
            raise QeaError(f"{type(self).__name__} takes batch_size, drop_last and sampler or shuffle only")
        self.dataset, self.store = dataset, store
        self._indices = torch.utils.data.DataLoader(_Indices(len(dataset)), **loader_kw)
        self.batch_size, self.sampler = self._indices.batch_size, self._indices.sampler

    def __len__(self):
        return len(self._indices)


class ResidentLoader(_IndexLoader):
    """The index loader of an ImgDataset, or of a Subset of one, whose strips sit in `store`: each index batch becomes the list the
    sample loader collates: [images (on the store's device), labels, names (if include_name), indices (if include_index)]."""

    def __init__(self, dataset, store, **loader_kw):
        base, self._remap = dataset, None
        if isinstance(dataset, torch.utils.data.Subset):
            base, self._remap = dataset.dataset, np.asarray(list(dataset.indices), dtype=np.int64)
        if not isinstance(base, ImgDataset) or [os.path.basename(f) for f in base.files] != store.names:
            raise QeaError("ResidentLoader: the store was not built from this dataset")
        super().__init__(dataset, store, loader_kw)
        self.include_name, self.include_index = base.include_name, base.include_index

    def __iter__(self):
        for indices in self._indices:                                         # int64 [B], as default_collate makes of the samples' idx
            rows = indices.numpy() if self._remap is None else self._remap[indices.numpy()]
            out = [self.store.batch(rows), [self.store.labels[i] for i in rows]]
            if self.include_name:
                out.append([self.store.names[i] for i in rows])
            if self.include_index:                                            # ImgDataset's own index: through a Subset, the base row
                out.append(indices if self._remap is None else torch.from_numpy(rows))
            yield out


def resident_args(args, what):
    """The --resident_pack / --resident_max_gb arguments of resident_loader for one of a trainer's two sets."""
    pack = getattr(args, "resident_pack", None)
    if pack and what.startswith("validation"):
        root, ext = os.path.splitext(pack)
        pack = f"{root}.val{ext}"
    return dict(pack_path=pack, max_gb=getattr(args, "resident_max_gb", 8))


def resident_loader(dataset, size, device, pack_path=None, max_gb=8.0, what="dataset", **loader_kw):
    """--resident: the ResidentLoader that replaces DataLoader(dataset, **loader_kw).  The store reproduces ONE transform, the
    trainers' PadWhite(size) + float32 / 255, and never calls the dataset's: the dataset's own first and last samples are therefore
    compared with the store's here, and a dataset whose transform yields anything else is refused.  Refuses what has no resident form."""
    base = dataset.dataset if isinstance(dataset, torch.utils.data.Subset) else dataset
    if getattr(base, "widths", None) is not None:
        raise QeaError(f"--resident: the {what} has per-sample widths (the bucketed path); the resident store builds fixed-width batches")
    if not isinstance(base, ImgDataset):
        raise QeaError(f"--resident needs an ImgDataset (or a Subset of one) as {what}, not a {type(base).__name__}")
    if pack_path:
        store = ResidentStrips.load_or_build(base, size, pack_path, device=device, max_gb=max_gb)
    else:
        store = ResidentStrips(base, size, device=device, max_gb=max_gb)
    for i in sorted({0, len(store) - 1} - {-1}):
        theirs, ours = base[i][0], store.batch([i])[0].cpu()
        if not torch.is_tensor(theirs) or theirs.shape != ours.shape or not torch.equal(theirs, ours):
            raise QeaError(f"--resident: the {what}'s transform does not give PadWhite(({store.H}, {store.W})) followed by float32 / 255 "
                           f"(sample {i} differs from the resident batch); the store would train on other pixels")
    return ResidentLoader(dataset, store, **loader_kw)


# ----------------------------------------------------------------------------- documents (patch_cli.py --resident)
DOC_PACK_FORMAT = 1


def _doc_geometry(dataset, path, w, h):
    """PatchDataset.__getitem__'s (top, left, sx, sy) of a w x h document and the branch it takes: "fit", "cut" (oversize in one
    dimension: ImageOps.expand with a negative border keeps the central pixels) or "resize"."""
    H, W = dataset.size
    if h <= H or w <= W:
        return (H - h) // 2, (W - w) // 2, 1, 1, "cut" if (h > H or w > W) else "fit"
    if dataset.resize_images:
        return 0, 0, W / w, H / h, "resize"
    raise QeaError(f"--resident: {path} is {h}x{w}, larger than the {H}x{W} canvas in both dimensions, and the dataset does not resize: "
                   "its sample is an unpadded image that no batch can hold")


def _decode_doc(dataset, path):
    """The dataset's decode of one document up to, not including, the white pad -> (uint8 [h', w'], source (h, w))."""
    H, W = dataset.size
    image = Image.open(path).convert("L")
    w, h = image.size
    top, left, _, _, how = _doc_geometry(dataset, path, w, h)
    if how == "resize":
        return np.asarray(image.resize((W, H), Image.BILINEAR), dtype=np.uint8), (h, w)
    a = np.asarray(image, dtype=np.uint8)
    if how == "cut":                                  # the slice a negative border leaves: source rows -top .. -top+H-1 (columns alike)
        y0, x0 = max(0, -top), max(0, -left)
        a = a[y0:y0 + H, x0:x0 + W]
    return np.ascontiguousarray(a), (h, w)


def _doc_signature(dataset):
    """_signature's rows of every image AND of its .json, with the canvas and the dataset's resize flag."""
    return hashlib.sha256(json.dumps({"format": DOC_PACK_FORMAT, "size": list(dataset.size), "resize": bool(dataset.resize_images),
                                      "files": _stat_rows(list(dataset.files), with_json=True)}).encode()).hexdigest()


class DocBoxes(list):
    """The box lists of a batch of documents (what PatchDataset.collate yields as its second entry) that also says where they came
    from: `store` (a ResidentDocuments) and `rows` (the store row of each document), so utils.get_text_stacks can cut all their strips
    from the store's device tables.  Indexing and iterating it give the plain lists."""

    def __init__(self, lists, store, rows):
        super().__init__(lists)
        self.store, self.rows = store, [int(r) for r in rows]


class ResidentDocuments(_PackedStore):
    """Every document of a PatchDataset (pad=True) decoded ONCE: pixels as the dataset has them before the white pad, boxes as its
    coord_loader returns them.  batch(rows) is torch.stack([dataset[i][0] for i in rows]) bit for bit; crops(images, rows, oh, ow)
    cuts all boxes of those documents out of `images`.  device="cpu": numpy tables and the numpy specification of both."""
    PACKED = _PackedStore.PACKED + ("src",)           # src int32 [n][2]: the (h, w) of every source image

    def __init__(self, dataset, device="cpu", max_gb=8.0, _packed=None):
        from datasets.patch_dataset import PatchDataset
        if not isinstance(dataset, PatchDataset):
            raise QeaError(f"ResidentDocuments packs a PatchDataset, not a {type(dataset).__name__}")
        if not dataset.pad:
            raise QeaError("ResidentDocuments needs a PatchDataset with pad=True: unpadded documents have no common canvas")
        self.dataset = dataset
        self.H, self.W = dataset.size
        self._open(device, max_gb)
        self.paths = list(dataset.files)
        self.n = len(self.paths)
        if not self.n:
            raise QeaError("ResidentDocuments: the dataset lists no document")
        t0 = time.perf_counter()
        if _packed is None:
            src = []                                                          # the source sizes, noted as _pack walks the documents

            def decoded():
                for f in self.paths:
                    a, hw = _decode_doc(dataset, f)
                    src.append(hw)
                    yield a
            _packed = self._pack(decoded()) + (np.array(src, dtype=np.int32).reshape(-1, 2),)
        self.boxes, self.branch = [], []
        for f, (sh, sw) in zip(self.paths, _packed[4].tolist()):
            top, left, sx, sy, how = _doc_geometry(dataset, f, sw, sh)
            self.boxes.append(dataset.coord_loader(f, top, left, sx, sy))     # filtering, shifting and the placeholder stay the dataset's
            self.branch.append(how)
        self.n_boxes = np.array([len(b) for b in self.boxes], dtype=np.int32)
        box_first = np.zeros(self.n + 1, dtype=np.int32)
        np.cumsum(self.n_boxes, out=box_first[1:])
        # get_text_stack's clipping of its CUDA branch
        box = np.array([[max(0, b["x_min"]), max(0, b["y_min"]), min(self.W, b["x_max"]), min(self.H, b["y_max"])]
                        for boxes in self.boxes for b in boxes], dtype=np.int32).reshape(-1, 4)
        self.build_seconds = time.perf_counter() - t0
        self._place(_packed, box=box, box_first=box_first)
        self._host_box, self._host_box_first = box, box_first
        self._self_check()

    def _self_check(self):
        """The store against the dataset's own samples: the first and the last document and every one stored through an oversize
        branch (the cut and the resize are re-done here, not taken from PIL's pad)."""
        rows = sorted({0, self.n - 1} | {i for i, how in enumerate(self.branch) if how != "fit"})
        for i in rows:
            sample = self.dataset[i]
            ours = self.batch([i])[0].cpu()
            if not torch.is_tensor(sample[0]) or sample[0].shape != ours.shape or not torch.equal(sample[0], ours):
                raise QeaError(f"--resident: document {self.paths[i]} comes out of the store with other pixels than out of the dataset")
            if sample[1] != self.boxes[i]:
                raise QeaError(f"--resident: document {self.paths[i]} comes out of the store with other boxes than out of the dataset")

    @classmethod
    def load_or_build(cls, dataset, pack_path, device="cpu", max_gb=8.0):
        """The store of `dataset` through the pack file at `pack_path` (.npz: pixels, offset, h, w, src, paths, signature).  A pack
        whose signature is not this dataset's (an image or a .json added, removed, resized or rewritten, another canvas or format) is
        never used: the store is rebuilt from the files and the pack overwritten.  Boxes are not packed: they are read from the
        .json files by the dataset's coord_loader either way."""
        return cls._load_or_build(len(dataset.files), pack_path, _doc_signature(dataset),
                                  lambda packed: cls(dataset, device=device, max_gb=max_gb, _packed=packed))

    def _pack_extras(self):
        return dict(paths=np.array(self.paths, dtype=str))

    def batch(self, rows):
        """fp32 [N,1,H,W] on the store's device: documents `rows` centred on the white canvas, the dataset's own samples bit for bit.
        On the device one launch of qea_strip_batch (OH = H, OW = W, centre anchor)."""
        return self._batch(self._rows(rows, "batch"), self.H, self.W)

    def strip_tables(self, rows):
        """(doc int64 [N], strip_first int32 [N+1]) of a step on documents `rows`, as host arrays."""
        rows = self._rows(rows, "crops")
        first = np.zeros(rows.size + 1, dtype=np.int32)
        np.cumsum(self.n_boxes[rows], out=first[1:])
        return rows, first

    def labels(self, rows):
        """[[label of every box] per document]: the second result of get_text_stack, per document."""
        return [[b["label"] for b in self.boxes[int(r)]] for r in rows]

    def crops(self, images, rows, oh, ow):
        """All boxes of documents `rows` cut out of images [N,1,H,W] (image n = document rows[n]) and centred on white oh x ow:
        [S,1,oh,ow], document after document, box after box; differentiable in `images`.  Device store: one launch forward
        (qea_doc_crops_gather) and one backward (qea_doc_crops_scatter, no atomics).  Host store: the numpy specification."""
        doc, first = self.strip_tables(rows)
        if images.dim() != 4 or images.shape[0] != doc.size or tuple(images.shape[1:]) != (1, self.H, self.W):
            raise ValueError(f"ResidentDocuments.crops: images {tuple(images.shape)} for {doc.size} documents on a {self.H}x{self.W} canvas")
        if ow < 4 or ow % 4:
            raise ValueError(f"ResidentDocuments.crops: ow={ow} must be a positive multiple of 4")
        if self.device.type == "cuda":
            if not images.is_cuda:
                raise ValueError("ResidentDocuments.crops: a device store cuts device images")
            # doc and strip_first in ONE pinned block and one non-blocking copy (fresh per call, see _PackedStore._batch)
            N = doc.size
            pinned = torch.empty(8 * N + 4 * (N + 1), dtype=torch.uint8, pin_memory=True)
            pinned[:8 * N].view(torch.int64).numpy()[:] = doc
            pinned[8 * N:].view(torch.int32).numpy()[:] = first
            dev = pinned.to(images.device, non_blocking=True)
            from utils import _DocCrops
            return _DocCrops.apply(images, self, dev[:8 * N].view(torch.int64), dev[8 * N:].view(torch.int32), int(first[-1]), int(oh), int(ow))
        if images.is_cuda:
            raise ValueError("ResidentDocuments.crops: a host store cuts host images")
        return _DocCropsHost.apply(images, self._host_box, self._host_box_first, doc, first, int(oh), int(ow))


def doc_crops_spec(imgs, box, box_first, doc, first, oh, ow):
    """numpy specification of qea_doc_crops_gather: imgs fp32 [N,H,W] -> [S,oh,ow]."""
    N, H, W = imgs.shape
    out = np.ones((int(first[-1]), oh, ow), dtype=np.float32)
    for n in range(N):
        for j in range(int(first[n + 1] - first[n])):
            x0, y0, x1, y1 = (int(v) for v in box[box_first[doc[n]] + j])
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
            cw, ch = x1 - x0, y1 - y0
            left, top = (ow - cw) // 2, (oh - ch) // 2
            for oy in range(max(0, top), min(oh, top + ch)):
                a, b = max(0, left), min(ow, left + cw)
                if b > a:
                    out[first[n] + j, oy, a:b] = imgs[n, y0 + oy - top, x0 + a - left: x0 + b - left]
    return out


def doc_crops_backward_spec(dout, box, box_first, doc, first, H, W, dimg=None):
    """numpy specification of qea_doc_crops_scatter: dout fp32 [S,oh,ow] -> [N,H,W]; every pixel is the fp32 sum, in ascending box
    order from 0, of the dout elements that read it, added to `dimg` when that is given (accumulate)."""
    S, oh, ow = dout.shape
    N = len(doc)
    acc = np.zeros((N, H, W), dtype=np.float32)
    for n in range(N):
        for j in range(int(first[n + 1] - first[n])):
            x0, y0, x1, y1 = (int(v) for v in box[box_first[doc[n]] + j])
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
            cw, ch = x1 - x0, y1 - y0
            left, top = (ow - cw) // 2, (oh - ch) // 2
            a, b = max(0, left), min(ow, left + cw)
            for oy in range(max(0, top), min(oh, top + ch)):
                if b > a:
                    acc[n, y0 + oy - top, x0 + a - left: x0 + b - left] += dout[first[n] + j, oy, a:b]
    return acc if dimg is None else (dimg + acc).astype(np.float32)


class _DocCropsHost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, box, box_first, doc, first, oh, ow):
        ctx.tables = (box, box_first, doc, first, images.shape)
        return torch.from_numpy(doc_crops_spec(images.detach().numpy()[:, 0], box, box_first, doc, first, oh, ow))[:, None]

    @staticmethod
    def backward(ctx, dout):
        box, box_first, doc, first, shape = ctx.tables
        d = doc_crops_backward_spec(dout.contiguous().numpy()[:, 0], box, box_first, doc, first, shape[2], shape[3])
        return torch.from_numpy(d)[:, None], None, None, None, None, None, None


class ResidentDocLoader(_IndexLoader):
    """The index loader of a PatchDataset whose documents sit in `store`: the same index batches as
    DataLoader(dataset, collate_fn=PatchDataset.collate, ...).  Each batch is [images on the store's device, DocBoxes (the box lists,
    with the store and the rows), paths (if include_name)]."""

    def __init__(self, dataset, store, **loader_kw):
        if store.dataset is not dataset and list(dataset.files) != store.paths:
            raise QeaError("ResidentDocLoader: the store was not built from this dataset")
        super().__init__(dataset, store, loader_kw)
        self.include_name = dataset.include_name

    def __iter__(self):
        for indices in self._indices:
            rows = indices.numpy().reshape(-1)
            out = [self.store.batch(rows), DocBoxes([self.store.boxes[i] for i in rows], self.store, rows)]
            if self.include_name:
                out.append([self.store.paths[i] for i in rows])
            yield out


def resident_documents(dataset, device, pack_path=None, max_gb=8.0, what="dataset"):
    """--resident of patch_cli.py: the ResidentDocuments of `dataset` (through the pack file when one is named).  The store checks
    itself against the dataset's own samples at construction.  Refuses what has no resident form."""
    from datasets.patch_dataset import PatchDataset
    if not isinstance(dataset, PatchDataset):
        raise QeaError(f"--resident needs a PatchDataset as {what}, not a {type(dataset).__name__}")
    if pack_path:
        return ResidentDocuments.load_or_build(dataset, pack_path, device=device, max_gb=max_gb)
    return ResidentDocuments(dataset, device=device, max_gb=max_gb)
