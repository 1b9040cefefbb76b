"""Lexicons for the automaton-constrained CTC prefix beam search (DESIGN.md "Automaton-constrained search"; the reference has no
lexicon).  A Lexicon is a deterministic automaton over the non-blank classes in CSR form: first [S+1], label [E] (strictly ascending
within a state, never the blank), child [E], final [S]; state 0 is the start.  Lexicon.from_words builds the trie of a word list,
Lexicon.from_automaton takes any automaton of that form (a pattern such as "digits and a decimal point").  Every statement of the
specification is validated here, on the host, once: qea.ops.ctc_beam_decode_dfa takes only what Lexicon.device() returns, which is
how the device tables are known to be valid.
"""
import numpy as np
import torch

from . import beam as _beam
from ._lib import QeaError


class DeviceAutomaton:
    """The validated tables of a Lexicon on one device: first / label / child int32, final uint8.  label and child hold one unused
    element when there is no edge, so that their pointers are never null.  Made by Lexicon.device() only."""

    def __init__(self, lexicon, device):
        pad = lambda a: a if len(a) else np.zeros(1, dtype=np.int32)       # noqa: E731
        self.first = torch.from_numpy(lexicon.first).to(device)
        self.label = torch.from_numpy(pad(lexicon.label)).to(device)
        self.child = torch.from_numpy(pad(lexicon.child)).to(device)
        self.final = torch.from_numpy(lexicon.final).to(device)
        self.num_states, self.num_edges = lexicon.num_states, lexicon.num_edges
        self.num_classes, self.blank = lexicon.num_classes, lexicon.blank
        self.device = self.first.device


class Lexicon:
    def __init__(self, first, label, child, final, vocabulary, blank=0, num_words=None, num_empty=0):
        """Validates every statement of the specification; use from_words or from_automaton."""
        self.vocabulary = [str(c) for c in vocabulary]                 # class index -> character
        self.blank = int(blank)
        C = len(self.vocabulary)
        if not 2 <= C <= _beam.MAX_C:
            raise QeaError(f"Lexicon: {C} classes, outside 2..{_beam.MAX_C}")
        if not 0 <= self.blank < C:
            raise QeaError(f"Lexicon: blank={self.blank} outside 0..{C - 1}")
        arrays = []
        for name, a in (("first", first), ("label", label), ("child", child), ("final", final)):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iub"):
                raise QeaError(f"Lexicon: {name} must be a one-dimensional integer array")
            a = a.astype(np.int64)
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise QeaError(f"Lexicon: {name} does not fit 32 bits")
            arrays.append(a)
        first, label, child, final = arrays
        S, E = len(first) - 1, len(label)
        if S < 1:
            raise QeaError("Lexicon: first needs S + 1 >= 2 entries (at least the start state)")
        if E > _beam.MAX_DFA_EDGES:
            raise QeaError(f"Lexicon: {E} edges, more than {_beam.MAX_DFA_EDGES}")
        if len(child) != E or len(final) != S:
            raise QeaError(f"Lexicon: {E} labels, {len(child)} children, {S} states, {len(final)} final marks")
        if first[0] != 0 or first[S] != E or (np.diff(first) < 0).any():
            raise QeaError("Lexicon: first must start at 0, not decrease and end at the number of edges")
        if E and (label.min() < 0 or label.max() >= C or (label == self.blank).any()):
            raise QeaError(f"Lexicon: an edge label is the blank or outside 0..{C - 1}")
        if E and (child.min() < 0 or child.max() >= S):
            raise QeaError(f"Lexicon: an edge's child is outside 0..{S - 1}")
        if E > 1:
            same_state = np.ones(E - 1, dtype=bool)
            inner = first[1:-1]
            same_state[inner[(inner > 0) & (inner < E)] - 1] = False   # edge e and e + 1 belong to different states
            if (np.diff(label)[same_state] <= 0).any():
                raise QeaError("Lexicon: the labels of a state's edges must ascend strictly")
        if S and ((final != 0) & (final != 1)).any():
            raise QeaError("Lexicon: final holds 0 or 1 per state")
        self.first, self.label, self.child = (np.ascontiguousarray(a, dtype=np.int32) for a in (first, label, child))
        self.final = np.ascontiguousarray(final, dtype=np.uint8)
        self.num_words = None if num_words is None else int(num_words)
        self.num_empty = int(num_empty)                                # empty strings from_words skipped
        self._device = {}

    @property
    def num_classes(self):
        return len(self.vocabulary)

    @property
    def num_states(self):
        return len(self.first) - 1

    @property
    def num_edges(self):
        return len(self.label)

    @staticmethod
    def _vocabulary(char_to_index):
        C = len(char_to_index)
        vocabulary = [None] * C
        for ch, i in char_to_index.items():
            if not 0 <= i < C or vocabulary[i] is not None:
                raise QeaError("Lexicon: char_to_index must map onto 0..C-1 one to one")
            vocabulary[i] = ch
        return vocabulary

    @classmethod
    def from_words(cls, words, char_to_index, blank=0):
        """The trie of `words`: states in breadth-first order (a state's children by ascending class), duplicates merged, empty
        strings skipped and counted (num_empty); num_words counts the distinct words.  A character outside the non-blank classes
        raises."""
        vocabulary = cls._vocabulary(char_to_index)
        blank = int(blank)
        kids, final, empty = [{}], [0], 0
        for w in words:
            if len(w) == 0:
                empty += 1
                continue
            s = 0
            for ch in w:
                c = char_to_index.get(ch)
                if c is None or c == blank:
                    raise QeaError(f"Lexicon: word {w!r} has the character {ch!r}, which is not a non-blank class")
                nxt = kids[s].get(c)
                if nxt is None:
                    nxt = kids[s][c] = len(kids)
                    kids.append({})
                    final.append(0)
                s = nxt
            final[s] = 1
        order, number = [0], {0: 0}
        for s in order:                                                # grows while it is walked: breadth first
            for c in sorted(kids[s]):
                number[kids[s][c]] = len(order)
                order.append(kids[s][c])
        first, label, child = [0], [], []
        for s in order:
            for c in sorted(kids[s]):
                label.append(c)
                child.append(number[kids[s][c]])
            first.append(len(label))
        return cls(np.array(first, dtype=np.int64), np.array(label, dtype=np.int64), np.array(child, dtype=np.int64),
                   np.array([final[s] for s in order], dtype=np.int64), vocabulary, blank, num_words=sum(final), num_empty=empty)

    @classmethod
    def from_automaton(cls, first, label, child, final, vocabulary, blank=0):
        """Any deterministic automaton in the specification's form; raises QeaError for every statement it breaks."""
        return cls(first, label, child, final, vocabulary, blank)

    def step(self, state, c):
        """The child of the edge labelled c out of `state`, -1 when there is none."""
        lo, hi = int(self.first[state]), int(self.first[state + 1])
        e = lo + int(np.searchsorted(self.label[lo:hi], c))
        return int(self.child[e]) if e < hi and self.label[e] == c else -1

    def accepts(self, tokens):
        """Whether the class sequence `tokens` is a path from the start that ends in an accepting state."""
        s = 0
        for c in tokens:
            s = self.step(s, int(c))
            if s < 0:
                return False
        return bool(self.final[s])

    def accepts_string(self, text, char_to_index):
        return all(ch in char_to_index for ch in text) and self.accepts([char_to_index[ch] for ch in text])

    def check_vocabulary(self, char_to_index):
        if self._vocabulary(char_to_index) != self.vocabulary:
            raise QeaError("Lexicon: the lexicon was built for another vocabulary")

    def save(self, path):
        """One .npz: the four tables, blank, num_words (-1: unknown), num_empty and the vocabulary (written to exactly `path`)."""
        with open(path, "wb") as f:
            np.savez(f, first=self.first, label=self.label, child=self.child, final=self.final, blank=np.int64(self.blank),
                     num_words=np.int64(-1 if self.num_words is None else self.num_words), num_empty=np.int64(self.num_empty),
                     vocabulary=np.array(self.vocabulary))

    @classmethod
    def load(cls, path, char_to_index=None):
        """The lexicon save() wrote, validated again; with char_to_index, one built for another vocabulary raises."""
        with np.load(path, allow_pickle=False) as z:
            words = int(z["num_words"])
            lex = cls(z["first"], z["label"], z["child"], z["final"], z["vocabulary"].tolist(), int(z["blank"]),
                      num_words=None if words < 0 else words, num_empty=int(z["num_empty"]))
        if char_to_index is not None:
            lex.check_vocabulary(char_to_index)
        return lex

    def device(self, dev):
        """The validated tables on `dev` (a DeviceAutomaton), uploaded once and cached per device."""
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._device:
            self._device[key] = DeviceAutomaton(self, dev)
        return self._device[key]
