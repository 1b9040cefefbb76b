"""Packing of label histories for the device weight tables (csrc/history.hip) and the choice between the device kernels and the
host loops of label_tracking/tracking_methods.py.

A history is `tracked_labels[name]`, oldest label first; the generators look at its last `window` labels, most recent first.
`LabelPacker.pack(tracked_labels, img_names)` returns one int32 host array laid out as

    [count: n] [lens: n * W] [rows: n * W * row_len]

(`lens` only for the Levenshtein packer), in pinned memory when a GPU is present, so the whole call is one host-to-device copy.
The encoded row of a label is cached BY THE STRING ITSELF: a step appends one label per strip, so all but n of the n * W rows of
the next call are already there, and a key that is the string cannot go stale whatever happens to the history lists.  Nothing
here needs a GPU."""
import os

import numpy as np
import torch

MAX_WINDOW = 8            # QEA_HISTORY_MAX_WINDOW
LEV_MAX_LEN = 128         # QEA_HISTORY_MAX_LEN
ATTN_MAX_TABLE = 12288    # QEA_HISTORY_ATTN_MAX_TABLE
CACHE_ROWS = 1 << 16      # the cache is emptied at the start of a call that finds more rows than this (32 MB of Levenshtein rows)


def host_forced():
    """QEA_HISTORY_WEIGHTS=host keeps the generators' host loops on a GPU too (A/B runs)"""
    return os.environ.get("QEA_HISTORY_WEIGHTS", "device") == "host"


def route(device, window, packed=True, table_floats=0, params_on_device=True):
    """'device' or 'host' for one gen_weights call.  `device`: the generator's torch.device (or its type string); `packed`: False
    when the packer refused the call (a word longer than the kernel's row, or a call the host path itself answers with an exception:
    it then raises there); `table_floats`: (V + 1 + window) * Dq of the attention scorer."""
    kind = device if isinstance(device, str) else torch.device(device).type
    if kind != "cuda" or host_forced():
        return "host"
    if window < 1 or window > MAX_WINDOW or not packed or table_floats > ATTN_MAX_TABLE or not params_on_device:
        return "host"
    return "device"


class LabelPacker:
    """Base: a growing [rows][row_len] int32 table of encoded labels, row 0 = the row of a missing word."""
    row_len = 0
    with_lens = False

    def __init__(self, window):
        self.window = int(window)
        self._pinned = None
        self._event = None
        self.clear()

    def clear(self):
        self._ids = {}
        self._rows = np.full((64, self.row_len), self.missing_row(), dtype=np.int32)     # unused tails keep the missing-word value
        self._lens = np.zeros(64, dtype=np.int32)
        self._used = 1

    def missing_row(self):
        return 0

    def encode(self, label):
        """int32 array of at most row_len entries, or None when the device kernel cannot take this label"""
        raise NotImplementedError

    def _row_of(self, label):
        i = self._ids.get(label)
        if i is None:
            enc = self.encode(label)
            if enc is None:
                return None
            if self._used == len(self._rows):
                self._rows = np.concatenate([self._rows, np.full_like(self._rows, self.missing_row())])
                self._lens = np.concatenate([self._lens, np.zeros_like(self._lens)])
            i = self._used
            if len(enc):
                self._rows[i, :len(enc)] = enc
                self._lens[i] = len(enc)
            self._ids[label] = i
            self._used += 1
        return i

    def sizes(self, n):
        """element offsets of (count, lens, rows, end) in the packed array"""
        W = self.window
        o_lens = n
        o_rows = o_lens + (n * W if self.with_lens else 0)
        return 0, o_lens, o_rows, o_rows + n * W * self.row_len

    def _buffer(self, total):
        if not torch.cuda.is_available():
            return np.empty(total, dtype=np.int32), None
        if self._event is not None:
            self._event.synchronize()                 # the copy out of the pinned buffer of the previous call has finished
            self._event = None
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1 << 16), dtype=torch.int32, pin_memory=True)
        t = self._pinned[:total]
        return t.numpy(), t

    def pack(self, tracked_labels, img_names):
        """-> (host int32 array, the pinned tensor it views or None), or None when some label cannot go to the device"""
        if self._used > CACHE_ROWS:
            self.clear()
        n, W = len(img_names), self.window
        ids, count = [], []
        known, pad = self._ids, [0] * W
        for name in img_names:
            hist = tracked_labels.get(name)
            if hist:
                recent = hist[:-W - 1:-1]
                for label in recent:
                    i = known.get(label)
                    if i is None:
                        i = self._row_of(label)
                        if i is None:
                            return None
                    ids.append(i)
                ids += pad[len(recent):]
                count.append(len(recent))
            else:
                ids += pad
                count.append(0)
        ids = np.array(ids, dtype=np.int64)
        o_count, o_lens, o_rows, total = self.sizes(n)
        host, pinned = self._buffer(total)
        host[o_count:o_lens] = count
        if self.with_lens:
            np.take(self._lens, ids.reshape(-1), out=host[o_lens:o_rows], mode="clip")
        np.take(self._rows, ids.reshape(-1), axis=0, out=host[o_rows:total].reshape(n * W, self.row_len), mode="clip")
        return host, pinned

    def unpack(self, host, n):
        """views (count [n], lens [n][W] or None, rows [n][W][row_len]) of a packed array"""
        o_count, o_lens, o_rows, total = self.sizes(n)
        lens = host[o_lens:o_rows].reshape(n, self.window) if self.with_lens else None
        return host[o_count:o_lens], lens, host[o_rows:total].reshape(n, self.window, self.row_len)

    def to_device(self, packed, device):
        """one host-to-device copy of a packed call; the pinned buffer is reused once the copy has finished"""
        host, pinned = packed
        dev = torch.empty(len(host), dtype=torch.int32, device=device)
        dev.copy_(pinned if pinned is not None else torch.from_numpy(host), non_blocking=True)
        if pinned is not None:
            self._event = torch.cuda.Event()
            self._event.record()
        return dev


class LevenshteinPacker(LabelPacker):
    """rows of Unicode code points (the generator compares raw characters), with lengths"""
    row_len = LEV_MAX_LEN
    with_lens = True

    def encode(self, label):
        if len(label) > LEV_MAX_LEN:
            return None
        return np.frombuffer(label.encode("utf-32-le", "surrogatepass"), dtype="<i4")


class AttentionPacker(LabelPacker):
    """rows as tracking_utils.str_to_tensor builds them: char_to_index of each character, padded with len(char_set)"""

    def __init__(self, window, char_to_index):
        import properties
        self.row_len = properties.max_char_len
        self.pad = len(properties.char_set)
        self.char_to_index = char_to_index
        super().__init__(window)

    def missing_row(self):
        return self.pad

    def encode(self, label):
        idx = [self.char_to_index[c] for c in label]            # KeyError for a character outside the set, as on the host path
        if len(idx) > self.row_len:
            return None                                         # str_to_tensor fails on the ragged rows: the host path raises
        return np.asarray(idx, dtype=np.int32).reshape(-1)


# ----------------------------------------------------------------------------- the weighted CTC loss over the history (csrc/ctc_history.hip)
CTC_MAX_LABEL = 127       # 2 L + 1 <= 256 states


def ctc_steps_forced():
    """QEA_HISTORY_CTC=steps keeps tracking_utils.weighted_ctc_loss's loop over the depths on a GPU too (A/B runs)"""
    return os.environ.get("QEA_HISTORY_CTC", "fused") == "steps"


def ctc_route(scores, loss_weights, window, max_label, loss_fn):
    """'fused' (one qea_ctc_history_loss call) or 'steps' (one CTC evaluation per history depth) for one weighted_ctc_loss call.
    `max_label`: the longest label of the call; `loss_fn`: the CTC module the loop would call (primary_loss_fn for decaying
    weights, primary_loss_fn_sample_wise otherwise).  Callable without a GPU."""
    from .loss import CTCLoss
    if ctc_steps_forced() or not (torch.is_tensor(scores) and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3):
        return "steps"
    if not (torch.is_tensor(loss_weights) and loss_weights.is_cuda and loss_weights.dtype == torch.float32 and not loss_weights.requires_grad):
        return "steps"
    if window < 1 or window > MAX_WINDOW or max_label > CTC_MAX_LABEL or not isinstance(loss_fn, CTCLoss):
        return "steps"
    return "fused"


class TargetBatchPacker:
    """`target_batches` of tracking_utils.generate_ctc_target_batches ([targets, target sizes, strip indices] per history depth)
    -> one int32 array  [depth_n: W] [lens: n * W] [offs: n * W] [chars: total] [input_lengths: n]  (the last block only when the
    input lengths are handed over as a host tensor), pinned when a GPU is present, so the whole call is one host-to-device copy.
    lens is -1 where a strip has no label at a depth; offs points into chars.  The index list of a depth may be any set of distinct
    strips: nothing assumes that a deeper list is a subset of a shallower one."""
    _buffer = LabelPacker._buffer
    to_device = LabelPacker.to_device

    def __init__(self):
        self._pinned = None
        self._event = None

    @staticmethod
    def sizes(n, W, total, with_input_lengths=False):
        """element offsets of (depth_n, lens, offs, chars, input_lengths, end) in the packed array"""
        o_lens = W
        o_offs = o_lens + n * W
        o_chars = o_offs + n * W
        o_in = o_chars + total
        return 0, o_lens, o_offs, o_chars, o_in, o_in + (n if with_input_lengths else 0)

    def pack(self, target_batches, n, input_lengths=None):
        """-> (host int32 array, the pinned tensor it views or None, W, total characters, longest label), or None for batches the
        fused call does not take (an index outside 0..n-1 or listed twice, sizes that do not match: the loop answers those)"""
        W = len(target_batches)
        parts = []
        for target, target_size, idx in target_batches:
            tg = torch.as_tensor(target).reshape(-1).numpy().astype(np.int32, copy=False)
            ts = torch.as_tensor(target_size).reshape(-1).numpy().astype(np.int64, copy=False)
            ix = np.asarray(idx, dtype=np.int64).reshape(-1)
            if len(ts) != len(ix) or len(ix) == 0 or ts.min() < 0 or int(ts.sum()) != len(tg):
                return None
            if ix.min() < 0 or ix.max() >= n or len(np.unique(ix)) != len(ix):
                return None
            parts.append((tg, ts, ix))
        if input_lengths is not None and len(input_lengths) != n:
            return None
        total = sum(len(tg) for tg, _, _ in parts)
        o_depth, o_lens, o_offs, o_chars, o_in, end = self.sizes(n, W, total, input_lengths is not None)
        host, pinned = self._buffer(end)
        lens = host[o_lens:o_offs].reshape(n, W)
        offs = host[o_offs:o_chars].reshape(n, W)
        lens.fill(-1)
        offs.fill(0)
        base, longest = 0, 0
        for i, (tg, ts, ix) in enumerate(parts):
            host[o_depth + i] = len(ix)
            lens[ix, i] = ts
            offs[ix, i] = base + np.cumsum(ts) - ts
            host[o_chars + base:o_chars + base + len(tg)] = tg
            base += len(tg)
            longest = max(longest, int(ts.max()))
        if input_lengths is not None:
            host[o_in:end] = torch.as_tensor(input_lengths).reshape(-1).numpy()
        return host, pinned, W, total, longest

    def unpack(self, host, n, W, total):
        """views (depth_n [W], lens [n][W], offs [n][W], chars [total], the rest) of a packed array or device tensor"""
        o_depth, o_lens, o_offs, o_chars, o_in, _ = self.sizes(n, W, total)
        return host[o_depth:o_lens], host[o_lens:o_offs].reshape(n, W), host[o_offs:o_chars].reshape(n, W), host[o_chars:o_in], host[o_in:]
