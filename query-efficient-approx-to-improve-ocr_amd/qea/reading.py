"""Reading word boxes with the CRNN (csrc/word_strips.hip): the last stage of the page pipeline behind deskew, the binarisers, the
components and the word boxes.  A box of any height becomes a 32-row strip of a CRNN width, the strips of a group of pages go through
the CRNN bucket by bucket, and the existing decoders (utils.pred_to_string: greedy, beam, n-gram fused, lexicon constrained) turn the
scores into strings.

The statement (tests/word_strips_spec.py spells it out in plain loops; DESIGN.md "Word strips" says why it is exact).  A page is read
as 8-bit grey exactly as binarize_pages reads it; a box is (page, x0, y0, x1, y1) with x1 / y1 EXCLUSIVE; OW % 16 == 0, 64..512; OH = 32.
  * Clip the box to its page; cw = x1 - x0, ch = y1 - y0.  cw <= 0, ch <= 0 or a page index outside the list: an all-white strip.
  * ch <= 32: crop + pad as utils.padder: centred with Python floor division, an oversize width cut (the extra pixel is lost on the
    left), bytes through norm_table(): bit for bit utils.get_text_stack(image, boxes, (32, OW)).
  * ch > 32: shrink by ch / 32 in both axes by the exact area average, all lengths in units of 1 / 32 source pixel: sw = ceil(32 cw / ch)
    columns; scaled row oy covers [oy ch, (oy + 1) ch), scaled column j covers [j ch, (j + 1) ch) cut to [0, 32 cw); source row r is
    [32 r, 32 r + 32), source column c likewise; wy(oy, r) and wx(j, c) are the integer overlap lengths; S = sum wy wx p(y0 + r, x0 + c),
    Area = ch min(ch, 32 cw - j ch), q = (2 S + Area) // (2 Area) in 0..255, value norm_table()[q]; the sw columns are centred in OW by the
    rule above.
All of it is integer work: the device, the host path below and the statement agree bit for bit.

CUDA pages (or a CUDA `device`) run the kernel over the packed store, ONE launch per call of word_strips; CPU tensors run the host path:
the same statement with the two weight matrices of a box written out and multiplied in numpy.
"""
from collections import namedtuple

import numpy as np
import torch

from .pages import host_page, is_int, norm_table, open_store, require_eval

OH, MIN_W, MAX_W = 32, 64, 512                    # QEA_WORD_STRIP_H / _MIN_W / _MAX_W of include/qea_hip.h
MAX_SIDE, MAX_BOXES = 32767, 1 << 20              # QEA_WORD_STRIP_MAX_SIDE / _MAX_BOXES
STRIP_PIXELS = 65536                              # strips x width per CRNN pass: 512 strips of 128 columns, 128 of 512
MAX_BEAM = 32                                     # the beam kernels' limit (utils.beam_decode)

Plan = namedtuple("Plan", "sw bucket cut passes")  # int32 [n], int32 [n], bool [n], [(OW, int64 box indices)]


def default_buckets():
    from datasets.bucketing import BUCKETS
    return BUCKETS


def _check_width(width):
    if not is_int(width) or width % 16 or not MIN_W <= width <= MAX_W:
        raise ValueError(f"width={width!r}: a multiple of 16 in {MIN_W}..{MAX_W}")


def check_params(buckets=None, strip_pixels=STRIP_PIXELS, beam=0, nbest=1):
    """ValueError for parameters outside the statement's ranges, before any work -> the buckets as a tuple"""
    buckets = default_buckets() if buckets is None else buckets
    if not isinstance(buckets, (tuple, list)) or not len(buckets):
        raise ValueError(f"buckets={buckets!r}: a non-empty ascending tuple of widths")
    for b in buckets:
        _check_width(b)
    if any(a >= b for a, b in zip(buckets[:-1], buckets[1:])):
        raise ValueError(f"buckets={buckets!r}: strictly ascending")
    if not is_int(strip_pixels) or strip_pixels < 1:
        raise ValueError(f"strip_pixels={strip_pixels!r}: an integer >= 1")
    if not is_int(beam) or not 0 <= beam <= MAX_BEAM:
        raise ValueError(f"beam={beam!r}: an integer in 0..{MAX_BEAM} (0 = greedy)")
    if not is_int(nbest) or not 1 <= nbest <= max(beam, 1):
        raise ValueError(f"nbest={nbest!r}: an integer in 1..beam (1 with the greedy decode)")
    return tuple(int(b) for b in buckets)


def _box_table(boxes):
    """-> int32 numpy [n, 5]; values outside int32 are refused, not wrapped"""
    b = boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
    if b.size == 0:
        return np.zeros((0, 5), np.int32)
    if b.ndim != 2 or b.shape[1] != 5 or b.dtype.kind not in "iu":
        raise ValueError(f"boxes {b.shape} {b.dtype}: an integer table [n, 5] = (page, x0, y0, x1, y1), x1 / y1 exclusive")
    if len(b) > MAX_BOXES:
        raise ValueError(f"{len(b)} boxes, more than 2^20 per call")
    b = b.astype(np.int64)
    if ((b < -2 ** 31) | (b >= 2 ** 31)).any():
        raise ValueError("boxes: values outside int32")
    return np.ascontiguousarray(b, np.int32)


def box_table(boxes_per_page):
    """per page an integer table [n_p, 4] = (x_min, y_min, x_max, y_max), INCLUSIVE (components.word_boxes) -> the int32 table [n, 5] =
    (page, x0, y0, x1, y1) with x1 / y1 exclusive, page after page"""
    rows = [np.zeros((0, 5), np.int64)]
    for p, b in enumerate(boxes_per_page):
        b = (b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).reshape(-1, 4).astype(np.int64)
        rows.append(np.concatenate([np.full((len(b), 1), p, np.int64), b[:, :2], b[:, 2:] + 1], 1))
    return _box_table(np.concatenate(rows))


def _geometry(boxes, hs, ws):
    """The clip and the scaled width of every box, in int64 -> (x0, y0, cw, ch, sw); an empty box has cw = ch = sw = 0"""
    b = boxes.astype(np.int64).reshape(-1, 5)
    hs, ws = np.asarray(hs, np.int64).reshape(-1), np.asarray(ws, np.int64).reshape(-1)
    known = (b[:, 0] >= 0) & (b[:, 0] < len(hs))
    p = np.where(known, b[:, 0], 0)
    H, W = (np.where(known, a[p], 0) if len(a) else np.zeros(len(b), np.int64) for a in (hs, ws))
    x0, y0 = np.maximum(b[:, 1], 0), np.maximum(b[:, 2], 0)
    cw, ch = np.minimum(b[:, 3], W) - x0, np.minimum(b[:, 4], H) - y0
    empty = (cw <= 0) | (ch <= 0)
    cw, ch = np.where(empty, 0, cw), np.where(empty, 0, ch)
    sw = np.where(ch <= OH, cw, (32 * cw + ch - 1) // np.maximum(ch, 1))
    return x0, y0, cw, ch, sw


def strip_plan(boxes, hs, ws, buckets=None, strip_pixels=STRIP_PIXELS):
    """Host-only integer work.  boxes: [n, 5] = (page, x0, y0, x1, y1), exclusive; hs / ws: the pages' sizes -> Plan: per box its strip
    width sw (cw where ch <= 32, ceil(32 cw / ch) above, 0 for an empty box), its bucket (the smallest that holds sw; the last one, with
    cut = True, when none does) and cut; and the passes [(OW, box indices)]: the buckets in ascending order, within a bucket the boxes in
    table order, chopped into passes of at most max(1, strip_pixels // OW) strips."""
    buckets = check_params(buckets, strip_pixels)
    sw = _geometry(_box_table(boxes), hs, ws)[4]
    widths = np.asarray(buckets, np.int64)
    bucket = widths[np.minimum(np.searchsorted(widths, sw, side="left"), len(widths) - 1)]
    passes = []
    for OW in buckets:
        idx = np.flatnonzero(bucket == OW)
        step = max(1, int(strip_pixels) // OW)
        passes.extend((OW, idx[i:i + step]) for i in range(0, len(idx), step))
    return Plan(sw.astype(np.int32), bucket.astype(np.int32), sw > widths[-1], passes)


# ---------------------------------------------------------------------------------------------------------------- the host path
def _shrink_host(crop):
    """uint8 [ch, cw], ch > 32 -> uint8 [32, sw]: the area average of the statement as Wy @ crop @ Wx.  The products run in fp64, where
    they are exact: every entry and every partial sum is a non-negative integer of at most 255 ch^2 < 2.8e11 < 2^53."""
    ch, cw = crop.shape
    sw = (32 * cw + ch - 1) // ch
    ya, r = np.arange(OH, dtype=np.int64)[:, None] * ch, 32 * np.arange(ch, dtype=np.int64)[None, :]
    Wy = np.clip(np.minimum(r + 32, ya + ch) - np.maximum(r, ya), 0, None)                  # [32, ch]
    xa, c = np.arange(sw, dtype=np.int64)[None, :] * ch, 32 * np.arange(cw, dtype=np.int64)[:, None]
    xb = np.minimum(xa + ch, 32 * cw)
    Wx = np.clip(np.minimum(c + 32, xb) - np.maximum(c, xa), 0, None)                       # [cw, sw]
    S = (Wy.astype(np.float64) @ crop.astype(np.float64) @ Wx.astype(np.float64)).astype(np.int64)
    area = ch * (xb - xa)                                                                  # [1, sw]
    return ((2 * S + area) // (2 * area)).astype(np.uint8)


def _strips_host(pk, boxes, OW):
    """-> fp32 numpy [n, 1, 32, OW]"""
    norm = norm_table().numpy()
    out = np.ones((len(boxes), 1, OH, OW), np.float32)
    x0, y0, cw, ch, _ = _geometry(boxes, pk.h, pk.w)
    pages = {}
    for i in np.flatnonzero(ch > 0):
        p = int(boxes[i, 0])
        if p not in pages:                                     # only the pages that have a box are read
            pages[p] = host_page(pk, p)
        crop = pages[p][y0[i]:y0[i] + ch[i], x0[i]:x0[i] + cw[i]]
        levels = crop if ch[i] <= OH else _shrink_host(crop)
        rows, cols = levels.shape
        top, left = (OH - rows) // 2, (OW - cols) // 2                                     # Python floor division; rows <= 32
        c0, c1 = max(0, -left), min(cols, OW - left)
        out[i, 0, top:top + rows, left + c0:left + c1] = norm[levels[:, c0:c1]]
    return out


# ---------------------------------------------------------------------------------------------------------------- the interface
class _Cutter:
    """The pages of a call packed once, on the device or on the host; strips(boxes, OW) cuts any subset of boxes at any width."""

    def __init__(self, pages, device):
        self.pk, self.dev, self.store, self.table = open_store(pages, device, max_side=MAX_SIDE)
        if self.dev.type == "cuda":
            self.norm = norm_table().to(self.dev)

    def strips(self, boxes, OW):
        if self.dev.type == "cuda":
            from . import ops
            return ops.word_strips(self.store, self.table, torch.from_numpy(boxes).to(self.dev), OW, self.norm)
        return torch.from_numpy(_strips_host(self.pk, boxes, OW))


def word_strips(pages, boxes, width, device=None):
    """pages: a list of [h, w] uint8 tensors or of [h, w] / [1, h, w] floating tensors, of any sizes (as for binarize_pages); boxes: an
    integer table [n, 5] = (page, x0, y0, x1, y1), x1 / y1 exclusive -> fp32 [n, 1, 32, width], on `device` if given, else where the pages
    are: every box as the statement's strip.  On a CUDA device: one launch."""
    _check_width(width)
    return _Cutter(pages, device).strips(_box_table(boxes), int(width))


def char_boxes(first, last, x0, cw, ch, sw, OW):
    """Pure integer host code: the character spans of ONE box (first / last: per character the CRNN steps it occupies, as utils.char_spans
    returns them) and that box's geometry (x0: its clipped left edge on the page, cw x ch: its clipped size, sw: its strip width from
    strip_plan, OW: the width of the pass it was read in) -> per character (x_min, x_max) in page coordinates, x_max EXCLUSIVE as in the
    written JSON.
    Step t of the CRNN is column t of conv7.  Along the width the layers are (the CRNN's layer list): conv1 3x3 pad 1, pool 2x2,
    conv2 3x3 pad 1, pool 2x2, conv3..conv6 3x3 pad 1 with the pools (2, 1) behind conv4 and conv6, which halve the height only, and conv7
    2x2 without padding.  So a pooled column p covers strip columns [4 p, 4 p + 4), conv7 column t reads pooled columns t and t + 1, T = OW / 4 - 1,
    and step t is centred on strip columns [4 t, 4 t + 8).  Its cell is the central half [4 t + 2, 4 t + 6): the cells of neighbouring steps
    touch and tile [2, OW - 2).  A character on steps first..last owns strip columns [4 first + 2, 4 last + 6).
    The strip holds the box's sw columns from left = (OW - sw) // 2 on (Python floor division as _strips_host centres them; negative for
    a cut strip), one strip column being m / 32 page columns with m = max(ch, 32):
        a = clamp(4 first + 2 - left, 0, sw - 1)    b = clamp(4 last + 6 - left, a + 1, sw)
        x_min = x0 + (a m) // 32                    x_max = x0 + min(cw, (b m + 31) // 32)
    For ch <= 32 that is the shift by x0 - left.  A character the alignment put into the padding is clamped to the box's nearest column:
    every box lies inside [x0, x0 + cw], is at least one column wide, and x_min does not decrease along the word."""
    x0, cw, ch, sw, OW = (int(v) for v in (x0, cw, ch, sw, OW))
    if cw < 1 or ch < 1 or sw < 1:
        raise ValueError(f"char_boxes: an empty box (cw={cw}, ch={ch}, sw={sw}) has no characters")
    left, m = (OW - sw) // 2, max(ch, OH)
    out = []
    for f, l in zip(first, last):
        a = min(max(4 * int(f) + 2 - left, 0), sw - 1)
        b = min(max(4 * int(l) + 6 - left, a + 1), sw)
        out.append((x0 + (a * m) // 32, x0 + min(cw, (b * m + 31) // 32)))
    return out


def read_pages(model, pages, boxes_per_page, index_to_char, buckets=None, strip_pixels=STRIP_PIXELS, beam=0, nbest=1, lm=None,
               lm_weight=1.0, lm_bonus=0.0, lexicon=None, forward=None, chars=False):
    """pages as for word_strips; boxes_per_page: per page an integer table [n_p, 4] = (x_min, y_min, x_max, y_max), INCLUSIVE, as
    components.word_boxes returns them -> (texts, cut) for beam = 0 and (texts, scores, cut) for beam > 0: per page the list of what the
    CRNN reads in that page's box order (strings, or lists of nbest strings), the scores as utils.pred_to_string(return_scores=True)
    gives them in the same nesting, and the number of boxes whose strip is wider than the last bucket and lost its sides.
    The work follows strip_plan: one word_strips call (one launch) per non-empty bucket, one CRNN forward per pass, on the model's device;
    decoding is utils.pred_to_string unchanged (beam, nbest, lm, lm_weight, lm_bonus, lexicon are its arguments).  forward: the callable
    that maps a pass [b, 1, 32, OW] to its scores [T, b, C]; the default is the model itself.
    chars=True: the best string of every box is also aligned to the scores of the same pass (utils.char_spans: one more launch per pass)
    and the result gains, in front of cut, per page and box a list of (char, x_min, x_max, mean_logp): the character's columns on the page
    (char_boxes; x_max exclusive) and the mean of its log-probs over its steps.  An empty string, an empty box and an infeasible alignment
    give an empty list.  index_to_char must then be one-to-one (ValueError otherwise)."""
    from utils import _check_beam_arguments, char_spans, pred_to_string
    buckets = check_params(buckets, strip_pixels, beam, nbest)
    _check_beam_arguments("read_pages", beam, lm, lexicon)
    require_eval(model, "read_pages")
    if len(boxes_per_page) != len(pages):
        raise ValueError(f"{len(boxes_per_page)} box tables for {len(pages)} pages")
    table = box_table(boxes_per_page)
    param = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    cutter = _Cutter(pages, param.device if param is not None else None)
    plan = strip_plan(table, cutter.pk.h, cutter.pk.w, buckets, strip_pixels)
    forward = model if forward is None else forward
    texts, scores, spans = [None] * len(table), [None] * len(table), [None] * len(table)
    if chars:
        char_to_index = {c: i for i, c in index_to_char.items()}
        if len(char_to_index) != len(index_to_char):
            raise ValueError("read_pages(chars=True): index_to_char maps several classes to one character")
        x0, _, cw, ch, _ = _geometry(table, cutter.pk.h, cutter.pk.w)
    strips, width, done = None, None, 0
    with torch.no_grad():
        for OW, idx in plan.passes:
            if OW != width:                                    # the first pass of a bucket cuts all of the bucket's strips
                strips, width, done = cutter.strips(table[plan.bucket == OW], OW), OW, 0
            s = forward(strips[done:done + len(idx)])
            done += len(idx)
            labels = [""] * len(idx)
            if beam:
                got, sc = pred_to_string(s, labels, index_to_char, beam=int(beam), nbest=int(nbest), return_scores=True, lm=lm,
                                         lm_weight=lm_weight, lm_bonus=lm_bonus, lexicon=lexicon)
            else:
                got, sc = pred_to_string(s, labels, index_to_char), labels
            for i, t, v in zip(idx.tolist(), got, sc):
                texts[i], scores[i] = t, v
            if chars:
                best = [t if isinstance(t, str) else t[0] for t in got]
                for i, text, (score, lo, hi, cs) in zip(idx.tolist(), best, char_spans(s, best, char_to_index)):
                    spans[i] = []
                    if text and score > -np.inf and plan.sw[i] > 0:
                        cols = char_boxes(lo, hi, x0[i], cw[i], ch[i], plan.sw[i], OW)
                        spans[i] = [(c, a, b, float(v) / (int(h) - int(l) + 1)) for c, (a, b), v, l, h in zip(text, cols, cs, lo, hi)]
    first = np.searchsorted(table[:, 0], np.arange(len(pages) + 1)).tolist()      # the table is page after page
    per_page = lambda values: [values[a:b] for a, b in zip(first[:-1], first[1:])]
    cut = int(plan.cut.sum())
    out = (per_page(texts), per_page(scores)) if beam else (per_page(texts),)
    return out + ((per_page(spans), cut) if chars else (cut,))
