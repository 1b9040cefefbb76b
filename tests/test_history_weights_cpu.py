"""CPU side of the device label-history weight tables (csrc/history.hip): the library exports the two entry points, qea.history
packs histories into the arrays the kernels read, its cache cannot go stale, and the routing between the kernels and the host loops
can be asked without a GPU."""
import json
import os
import types

import numpy as np
import torch

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _history(fx):
    return json.loads(str(fx["history_json"])), [str(s) for s in fx["names"]], int(fx["window"])


def test_library_exports_history_entry_points():
    from qea import _lib
    declared = {name for name, _, _ in _lib.header_prototypes()}
    L = _lib.lib()
    for name in ("qea_history_lev_weights", "qea_history_attn_weights"):
        assert name in declared, name
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "qea_hip.h")).read()
    assert "tracking_methods.py:63-101" in text and "tracking_methods.py:26-59" in text and "model_attention.py:7-38" in text
    # refused before any launch
    assert L.qea_history_lev_weights(None, None, None, 1, 1, None, None) < 0
    assert b"null" in L.qea_last_error()


def test_levenshtein_packing_of_the_fixture_history():
    from qea import history
    hist, names, W = _history(H.golden("tracking_f3.npz"))
    pk = history.LevenshteinPacker(W)
    host, _ = pk.pack(hist, names)
    count, lens, tokens = pk.unpack(host, len(names))
    assert tokens.shape == (len(names), W, 128) and tokens.dtype == np.int32
    for r, name in enumerate(names):
        recent = hist[name][-W:][::-1] if name in hist else []
        assert count[r] == len(recent)
        for i in range(W):
            word = recent[i] if i < len(recent) else ""
            assert lens[r, i] == len(word)
            assert tokens[r, i, :len(word)].tolist() == [ord(c) for c in word]
    assert (count == 0).any() and (count == W).any()          # the fixture has an unknown strip and a full window


def test_attention_packing_equals_str_to_tensor():
    import properties
    import tracking_utils as tu
    from qea import history
    hist, names, W = _history(H.golden("tracking_f3.npz"))
    pk = history.AttentionPacker(W, H.C2I)
    host, _ = pk.pack(hist, names)
    count, lens, idx = pk.unpack(host, len(names))
    assert lens is None and idx.shape == (len(names), W, properties.max_char_len)
    self = types.SimpleNamespace(char_to_index=H.C2I, window_size=W, device=torch.device("cpu"))
    for r, name in enumerate(names):
        recent = hist[name][-W:][::-1] if name in hist else []
        assert count[r] == len(recent)
        assert np.array_equal(idx[r], tu.str_to_tensor(self, recent).numpy()), name


def test_unknown_names_long_histories_and_code_points():
    from qea import history
    hist = {"a": ["one", "two", "three", "four", "five"], "b": ["Zoë €", "日本語"], "c": []}
    pk = history.LevenshteinPacker(3)
    host, _ = pk.pack(hist, ["missing", "a", "b", "c"])
    count, lens, tokens = pk.unpack(host, 4)
    assert count.tolist() == [0, 3, 2, 0]
    words = lambda r: ["".join(chr(c) for c in tokens[r, i, :lens[r, i]]) for i in range(count[r])]
    assert words(1) == ["five", "four", "three"]              # the most recent W labels, most recent first
    assert words(2) == ["日本語", "Zoë €"]
    assert tokens[2, 0, :3].tolist() == [0x65E5, 0x672C, 0x8A9E] and tokens[2, 1, 4] == 0x20AC
    assert lens[0].tolist() == [0, 0, 0] and lens[3].tolist() == [0, 0, 0]


def test_cache_has_no_stale_rows_after_a_label_is_appended():
    import tracking_utils as tu
    from qea import history
    fx = H.golden("tracking_f3.npz")
    hist, names, W = _history(fx)
    self = types.SimpleNamespace(tracked_labels=hist)
    for make in (lambda: history.LevenshteinPacker(W), lambda: history.AttentionPacker(W, H.C2I)):
        pk = make()
        first = pk.pack(self.tracked_labels, names)[0].copy()
        assert np.array_equal(first, make().pack(self.tracked_labels, names)[0])
        again = pk.pack(self.tracked_labels, names)[0].copy()
        assert np.array_equal(first, again)                   # same arrays from the cache
        rows_before = pk._used
        tu.add_labels_to_history(self, names, [str(s) for s in fx["current"]])
        after = pk.pack(self.tracked_labels, names)[0].copy()
        assert np.array_equal(after, make().pack(self.tracked_labels, names)[0])      # equals a packer that never saw the old state
        assert not np.array_equal(after, first)
        assert pk._used - rows_before <= len(names)           # only the appended labels were encoded
        # the same name with a different history of the same length: a key that is the string itself cannot go stale
        swapped = {n: [l[::-1] + "x" for l in v] for n, v in self.tracked_labels.items()}
        assert np.array_equal(pk.pack(swapped, names)[0], make().pack(swapped, names)[0])
        self.tracked_labels = json.loads(str(fx["history_json"]))


def test_fallback_routing_without_a_gpu(monkeypatch):
    from label_tracking.tracking_methods import weightgenerator_factory
    from qea import history
    monkeypatch.delenv("QEA_HISTORY_WEIGHTS", raising=False)
    cuda = torch.device("cuda")
    assert history.route(cuda, 5) == "device" and history.route(cuda, 8) == "device"
    assert history.route(cuda, 9) == "host"
    assert history.route(torch.device("cpu"), 5) == "host"
    assert history.route(cuda, 5, packed=False) == "host"
    assert history.route(cuda, 5, table_floats=history.ATTN_MAX_TABLE + 1) == "host"
    hist = {"a": ["x" * 128, "abc"], "b": ["y" * 129]}
    lev = lambda w, dev: weightgenerator_factory("levenshtein")(types.SimpleNamespace(window_size=w), dev)
    assert lev(5, cuda).select_path(hist, ["a"])[0] == "device"           # 128 characters fit
    assert lev(5, cuda).select_path(hist, ["a", "b"]) == ("host", None)   # one 129-character word sends the whole call to the host
    assert lev(9, cuda).select_path(hist, ["a"]) == ("host", None)
    assert lev(5, torch.device("cpu")).select_path(hist, ["a"]) == ("host", None)
    assert history.AttentionPacker(3, H.C2I).pack({"a": ["z" * 101]}, ["a"]) is None      # str_to_tensor fails there: host path raises
    try:
        history.AttentionPacker(3, H.C2I).pack({"a": ["日"]}, ["a"])
        raise AssertionError("no KeyError")
    except KeyError:
        pass
    monkeypatch.setenv("QEA_HISTORY_WEIGHTS", "host")
    assert history.route(cuda, 5) == "host"
    assert lev(5, cuda).select_path(hist, ["a"]) == ("host", None)
