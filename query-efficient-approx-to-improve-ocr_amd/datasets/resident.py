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


def _signature(files, H, W):
    """sha256 over the format version, the target size and (relative name, byte size, st_mtime_ns) of every file, in listing order."""
    root = os.path.commonpath([os.path.dirname(os.path.abspath(f)) for f in files]) if files else ""
    rows = []
    for f in files:
        st = os.stat(f)
        rows.append([os.path.relpath(os.path.abspath(f), root), st.st_size, st.st_mtime_ns])
    return hashlib.sha256(json.dumps({"format": PACK_FORMAT, "size": [H, W], "files": rows}).encode()).hexdigest()


class ResidentStrips:
    def __init__(self, dataset, size, device="cpu", max_gb=8.0, _packed=None):
        if not isinstance(dataset, ImgDataset):
            raise QeaError(f"ResidentStrips packs an ImgDataset, not a {type(dataset).__name__}")
        self.H, self.W = _size(size)
        self.device = torch.device(device)
        if self.device.type not in ("cpu", "cuda"):
            raise QeaError(f"ResidentStrips: device {device!r} is neither cpu nor cuda")
        self.max_gb = float(max_gb)
        files = list(dataset.files)
        self.n = len(files)
        self.names = [os.path.basename(f) for f in files]
        self.labels = [_label(f) for f in files]
        self.lens = np.array([len(l) for l in self.labels], dtype=np.int32)
        t0 = time.perf_counter()
        if _packed is None:
            pixels, offset, h, w = self._pack(files)
        else:
            pixels, offset, h, w = _packed
            self._guard(pixels.size)
        self.build_seconds = time.perf_counter() - t0
        self.nbytes = int(pixels.size)
        self._host = (pixels, offset, h, w)                                   # what a pack file holds
        table = norm_table()
        if self.device.type == "cuda":
            from qea import _lib
            _lib.lib()                                                        # a missing kernel is an error here, not at the first batch
            up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.device)
            self.pixels, self.offset, self.h, self.w, self.table = up(pixels), up(offset), up(h), up(w), up(table)
        else:
            self.pixels, self.offset, self.h, self.w, self.table = pixels, offset, h, w, table

    def __len__(self):
        return self.n

    def _guard(self, nbytes):
        if nbytes > self.max_gb * 2 ** 30:
            raise QeaError(f"the resident pack needs more than {nbytes / 2 ** 30:.3f} GB, above the limit of {self.max_gb:g} GB "
                           "(--resident_max_gb)")

    def _pack(self, files):
        chunks, total = [], 0
        offset = np.zeros(len(files), dtype=np.int64)
        h = np.zeros(len(files), dtype=np.int32)
        w = np.zeros(len(files), dtype=np.int32)
        for i, f in enumerate(files):
            a = _decode(f, self.H, self.W)
            offset[i], h[i], w[i] = total, a.shape[0], a.shape[1]
            chunks.append(a.reshape(-1))
            total += a.size
            self._guard(total)                                                # refuse as soon as the limit is passed, not after the decode
        pixels = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
        return pixels, offset, h, w

    # ---- the pack file ----
    @classmethod
    def load_or_build(cls, dataset, size, pack_path, device="cpu", max_gb=8.0):
        """The store of `dataset` through the pack file at `pack_path` (.npz: pixels, offset, h, w, names, labels, signature).  A pack
        whose signature is not this dataset's (a file added, removed, resized or rewritten, another target size or format) is never
        used: the store is rebuilt from the files and the pack overwritten."""
        H, W = _size(size)
        sig = _signature(dataset.files, H, W)
        packed = None
        if pack_path and os.path.exists(pack_path):
            try:
                with np.load(pack_path, allow_pickle=False) as z:
                    if str(z["signature"]) == sig and len(z["offset"]) == len(dataset.files):
                        packed = (z["pixels"], z["offset"], z["h"], z["w"])
            except (OSError, ValueError, KeyError):
                packed = None                                                 # unreadable or foreign file: rebuild
        store = cls(dataset, size, device=device, max_gb=max_gb, _packed=packed)
        store.from_pack = packed is not None
        if packed is None and pack_path:
            store.save(pack_path, sig)
        return store

    def save(self, pack_path, signature=None):
        pixels, offset, h, w = self._host
        tmp = f"{pack_path}.tmp{os.getpid()}"
        os.makedirs(os.path.dirname(os.path.abspath(pack_path)), exist_ok=True)
        with open(tmp, "wb") as f:
            np.savez(f, pixels=pixels, offset=offset, h=h, w=w, names=np.array(self.names, dtype=str), labels=np.array(self.labels, dtype=str),
                     signature=np.array(signature or ""), size=np.array([self.H, self.W], dtype=np.int32))
        os.replace(tmp, pack_path)

    # ---- batches ----
    def _indices(self, idx):
        if isinstance(idx, torch.Tensor):
            if idx.is_cuda:
                raise ValueError("ResidentStrips.batch: idx is a host sequence or a CPU tensor")
            idx = idx.numpy()
        idx = np.ascontiguousarray(np.asarray(list(idx) if not isinstance(idx, np.ndarray) else idx).reshape(-1)).astype(np.int64, copy=False)
        if idx.size == 0:
            raise ValueError("ResidentStrips.batch: no indices")
        if int(idx.min()) < 0 or int(idx.max()) >= self.n:
            raise ValueError(f"ResidentStrips.batch: indices {int(idx.min())}..{int(idx.max())} outside 0..{self.n - 1}")
        return idx

    def batch(self, idx, out_w=None, anchor="centre", out=None):
        """fp32 [B,1,H,out_w] (out_w defaults to W) on the store's device; `out` (optional) receives it.  anchor="centre": PadWhite's
        placement, left = dw // 2, top = dh // 2.  anchor="left": column 0, centred vertically, a strip wider than out_w cropped to its
        first out_w columns (datasets.bucketing.pad_to_bucket).  Indices are checked on the host: ValueError before any launch."""
        if anchor not in ANCHORS:
            raise ValueError(f"unknown anchor {anchor!r}")
        idx = self._indices(idx)
        OW = self.W if out_w is None else int(out_w)
        if OW < 4 or OW % 4:
            raise ValueError(f"ResidentStrips.batch: out_w={OW} must be a positive multiple of 4")
        shape = (idx.size, 1, self.H, OW)
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device.type != self.device.type
                                or not out.is_contiguous()):
            raise ValueError(f"ResidentStrips.batch: out must be a contiguous fp32 {shape} tensor on {self.device}")
        if self.device.type == "cuda":
            from qea import ops
            # a fresh pinned block per call: the caching host allocator hands it out again only after the copy below has run, so
            # neither a wait nor a second buffer is needed
            pinned = torch.empty(idx.size, dtype=torch.int64, pin_memory=True)
            pinned.numpy()[:] = idx
            d_idx = pinned.to(self.device, non_blocking=True)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
            ops.strip_batch(self.pixels, self.offset, self.h, self.w, d_idx, self.table, out, anchor)
            return out
        res = np.ones(shape, dtype=np.float32)
        for b, s in enumerate(idx):
            h, w = int(self.h[s]), int(self.w[s])
            hh, ww = min(h, self.H), min(w, OW)
            top = (self.H - hh) // 2
            left = 0 if anchor == "left" else (OW - ww) // 2
            strip = self.pixels[self.offset[s]: self.offset[s] + h * w].reshape(h, w)
            res[b, 0, top:top + hh, left:left + ww] = self.table[strip[:hh, :ww]]
        res = torch.from_numpy(res)
        if out is not None:
            out.copy_(res)
            return out
        return res


class _Indices(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class ResidentLoader:
    """The DataLoader of `dataset` (an ImgDataset, or a Subset of one, whose strips sit in `store`) with the sampling left to torch:
    a DataLoader over the indices 0..len(dataset)-1 with the caller's batch_size / drop_last / sampler / shuffle draws the same index
    batches, in the same order and with the same use of the global generator, as one over the samples; each index batch then becomes
    the list the sample loader collates: [images (on the store's device), labels, names (if include_name), indices (if include_index)]."""

    def __init__(self, dataset, store, **loader_kw):
        base, self._remap = dataset, None
        if isinstance(dataset, torch.utils.data.Subset):
            base, self._remap = dataset.dataset, np.asarray(list(dataset.indices), dtype=np.int64)
        if not isinstance(base, ImgDataset) or [os.path.basename(f) for f in base.files] != store.names:
            raise QeaError("ResidentLoader: the store was not built from this dataset")
        if loader_kw.get("num_workers") or "collate_fn" in loader_kw or "batch_sampler" in loader_kw:
            raise QeaError("ResidentLoader takes batch_size, drop_last and sampler or shuffle only")
        self.dataset, self.store = dataset, store
        self.include_name, self.include_index = base.include_name, base.include_index
        self._indices = torch.utils.data.DataLoader(_Indices(len(dataset)), **loader_kw)
        self.batch_size, self.sampler = self._indices.batch_size, self._indices.sampler

    def __len__(self):
        return len(self._indices)

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
