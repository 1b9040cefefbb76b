"""Character n-gram language model for the fused CTC prefix beam search (DESIGN.md "Character n-gram fusion"; the reference has no
language model).  CharLM holds logp [C ** m, C] fp64 with m = order - 1 context tokens; the search reads the fused table
W = alpha * logp + beta (CharLM.fused), formed here in fp64, and only ever adds its entries.

The context index follows the kernel's: ctx(p) = sum_q tok_q * C ** (m - 1 - q) over the last m tokens of the prefix, padded on the left
with BOS, which is represented by the blank index (it never occurs inside a prefix); ctx(p + c) = (ctx(p) * C + c) mod C ** m.
"""
import numpy as np
import torch

from . import beam as _beam
from ._lib import QeaError


class CharLM:
    def __init__(self, logp, order, add_k, blank, vocabulary):
        self.logp = np.ascontiguousarray(logp, dtype=np.float64)
        self.order, self.add_k, self.blank = int(order), float(add_k), int(blank)
        self.vocabulary = [str(c) for c in vocabulary]                 # class index -> character
        C = len(self.vocabulary)
        if not 1 <= self.order <= _beam.MAX_LM_CONTEXT + 1:
            raise QeaError(f"CharLM: order={self.order} outside 1..{_beam.MAX_LM_CONTEXT + 1}")
        if not 0 <= self.blank < C:
            raise QeaError(f"CharLM: blank={self.blank} outside 0..{C - 1}")
        _beam.check_lm_limits(C, self.context, self.logp.shape)
        self._fused = {}

    @property
    def context(self):
        """m: the number of context tokens, order - 1."""
        return self.order - 1

    @property
    def num_classes(self):
        return len(self.vocabulary)

    @staticmethod
    def _vocabulary(char_to_index):
        C = len(char_to_index)
        vocabulary = [None] * C
        for ch, i in char_to_index.items():
            if not 0 <= i < C or vocabulary[i] is not None:
                raise QeaError("CharLM: char_to_index must map onto 0..C-1 one to one")
            vocabulary[i] = ch
        return vocabulary

    @classmethod
    def from_labels(cls, labels, char_to_index, order=2, add_k=0.1, blank=0):
        """Counts count[ctx][c] over all positions of all labels (the context of the first characters is BOS-padded) and smooths:
        P(c | ctx) = (count[ctx][c] + add_k) / (sum_c' count[ctx][c'] + add_k * (C - 1)) over the C - 1 non-blank classes; logp's blank
        column is 0.  A label with a character outside the map (or the blank's own character) raises.  There is NO end-of-word
        term: the model says nothing about where a label stops, so it favours short readings; the bonus beta of fused() is the
        length control."""
        vocabulary = cls._vocabulary(char_to_index)
        C, m = len(vocabulary), int(order) - 1
        if not 1 <= int(order) <= _beam.MAX_LM_CONTEXT + 1:
            raise QeaError(f"CharLM: order={order} outside 1..{_beam.MAX_LM_CONTEXT + 1}")
        if not 0 <= int(blank) < C:
            raise QeaError(f"CharLM: blank={blank} outside 0..{C - 1}")
        if not add_k > 0:
            raise QeaError(f"CharLM: add_k={add_k} must be positive (an unseen context would have no distribution)")
        _beam.check_lm_limits(C, m)
        mod = C ** m
        count = np.zeros((mod, C), dtype=np.float64)
        start = _beam.start_context(C, m, int(blank))
        for label in labels:
            ctx = start
            for ch in label:
                c = char_to_index.get(ch)
                if c is None or c == blank:
                    raise QeaError(f"CharLM: label {label!r} has the character {ch!r}, which is not a non-blank class")
                count[ctx, c] += 1
                ctx = (ctx * C + c) % mod
        logp = np.log((count + add_k) / (count.sum(axis=1, keepdims=True) + add_k * (C - 1)))
        logp[:, int(blank)] = 0.0
        lm = cls(logp, order, add_k, blank, vocabulary)
        lm.count = count
        return lm

    def check_vocabulary(self, char_to_index):
        if self._vocabulary(char_to_index) != self.vocabulary:
            raise QeaError("CharLM: the model was built for another vocabulary")

    def save(self, path):
        """One .npz: logp, order, add_k, blank and the vocabulary (written to exactly `path`)."""
        with open(path, "wb") as f:
            np.savez(f, logp=self.logp, order=np.int64(self.order), add_k=np.float64(self.add_k), blank=np.int64(self.blank),
                     vocabulary=np.array(self.vocabulary))

    @classmethod
    def load(cls, path, char_to_index=None):
        """The model save() wrote; with char_to_index, a model built for another vocabulary raises."""
        with np.load(path, allow_pickle=False) as z:
            lm = cls(z["logp"], int(z["order"]), float(z["add_k"]), int(z["blank"]), z["vocabulary"].tolist())
        if char_to_index is not None:
            lm.check_vocabulary(char_to_index)
        return lm

    def fused(self, alpha=1.0, beta=0.0, device="cpu"):
        """W = alpha * logp + beta as a contiguous fp64 tensor [C ** m, C] on `device`, formed on the host in fp64 and cached per
        (alpha, beta, device)."""
        device = torch.device(device)
        key = (float(alpha), float(beta), str(device))
        if key not in self._fused:
            with np.errstate(invalid="ignore"):
                W = float(alpha) * self.logp + float(beta)
            self._fused[key] = torch.from_numpy(np.ascontiguousarray(W)).to(device)
        return self._fused[key]
