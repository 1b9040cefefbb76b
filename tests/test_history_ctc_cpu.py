"""CPU side of the label-history weighted CTC loss evaluated in one device pass (csrc/ctc_history.hip): the library exports the
entry points, qea.history packs `target_batches` into the arrays the kernels read, and the routing between the fused call and the
loop over the depths can be asked without a GPU."""
import os
import types

import numpy as np
import torch

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(labels, idx):
    """one entry of generate_ctc_target_batches: [targets, target sizes, strip indices]"""
    y = torch.tensor([H.C2I[c] for c in "".join(labels)], dtype=torch.int)
    return [y, torch.tensor([len(l) for l in labels], dtype=torch.int), list(idx)]


def _plain(target_batches, n):
    """the packed tables by a plain Python construction: label (as a list of indices) or None per (strip, depth)"""
    table = [[None] * len(target_batches) for _ in range(n)]
    for i, (y, ys, idx) in enumerate(target_batches):
        y, pos = y.tolist(), 0
        for j, L in zip(idx, ys.tolist()):
            table[j][i] = y[pos:pos + L]
            pos += L
    return table


BATCHES = [
    _batch(["abc", "", "zz", "hello world!", "q"], [0, 1, 2, 3, 4]),        # an empty label
    _batch(["ab", "xyz"], [1, 3]),
    _batch(["k", "mn", "o"], [0, 3, 5]),                                      # not a subset of the shallower list: 0 and 5 are new
]


def test_library_exports_history_ctc_entry_points():
    from qea import _lib
    declared = {name for name, _, _ in _lib.header_prototypes()}
    L = _lib.lib()
    for name in ("qea_ctc_history_loss", "qea_ctc_history_workspace_bytes"):
        assert name in declared, name
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "qea_hip.h")).read()
    assert "tracking_utils.py:59-75" in text
    assert L.qea_version() == 9
    assert L.qea_ctc_history_workspace_bytes(31, 9, 3, 25) == (2 * 31 * 25 + 2) * 9 * 3 * 8
    assert L.qea_ctc_history_workspace_bytes(31, 0, 3, 25) == 0
    # refused before any launch
    args = [None, 0, 0] + [None] * 6 + [0, 1, 0, 31, 9, 95, 3, 0, 25] + [None, None, 0, 0, None, None, 0, None]
    assert L.qea_ctc_history_loss(*args) < 0
    assert b"null" in L.qea_last_error()


def test_packer_round_trips_hand_made_batches():
    from qea import history
    n = 7
    pk = history.TargetBatchPacker()
    host, _, W, total, longest = pk.pack(BATCHES, n)
    assert (W, total, longest) == (3, sum(len(b[0]) for b in BATCHES), 12)
    assert host.dtype == np.int32 and len(host) == history.TargetBatchPacker.sizes(n, W, total)[-1]
    first = host.copy()
    depth_n, lens, offs, chars, rest = pk.unpack(host, n, W, total)
    assert depth_n.tolist() == [len(b[2]) for b in BATCHES] == [5, 2, 3]
    assert lens.shape == offs.shape == (n, W) and len(rest) == 0
    want = _plain(BATCHES, n)
    for j in range(n):
        for i in range(W):
            if want[j][i] is None:
                assert lens[j, i] == -1 and offs[j, i] == 0, (j, i)
            else:
                assert lens[j, i] == len(want[j][i]), (j, i)
                assert chars[offs[j, i]:offs[j, i] + lens[j, i]].tolist() == want[j][i], (j, i)
    assert lens[1, 0] == 0                                      # the empty label is present, not absent
    assert lens[6].tolist() == [-1, -1, -1]                     # a strip without any label
    assert lens[5].tolist() == [-1, -1, 1] and lens[0].tolist() == [3, -1, 1]     # non-nested depths
    # a second call reuses the buffer and gives the same array; input lengths ride at the end
    again = pk.pack(BATCHES, n, torch.tensor([31, 30, 29, 28, 5, 1, 0], dtype=torch.int))
    assert np.array_equal(again[0][:len(first)], first)
    assert pk.unpack(again[0], n, W, total)[4].tolist() == [31, 30, 29, 28, 5, 1, 0]


def test_packer_of_the_product_batches_and_refusals():
    import tracking_utils as tu
    from qea import history
    hist = {"a": ["one", "two", "three"], "b": ["x"], "c": [], "d": ["", "rr"]}
    names = ["a", "b", "c", "d", "a2"]
    hist["a2"] = ["p", "q"]
    self = types.SimpleNamespace(char_to_index=H.C2I, window_size=3, tracked_labels=hist)
    batches = tu.generate_ctc_target_batches(self, names)
    pk = history.TargetBatchPacker()
    host, _, W, total, longest = pk.pack(batches, len(names))
    depth_n, lens, offs, chars, _ = pk.unpack(host, len(names), W, total)
    assert depth_n.tolist() == [len(b[2]) for b in batches] == [4, 3, 1]
    for j, name in enumerate(names):
        for i in range(W):
            if i < len(hist[name]):
                word = hist[name][-(i + 1)]
                assert chars[offs[j, i]:offs[j, i] + lens[j, i]].tolist() == [H.C2I[c] for c in word]
            else:
                assert lens[j, i] == -1
    assert longest == 5
    # what the fused call does not take goes back to the loop
    assert pk.pack([_batch(["a", "b"], [0, 0])], 3) is None                    # a strip listed twice at one depth
    assert pk.pack([_batch(["a", "b"], [0, 3])], 3) is None                    # an index outside the batch
    assert pk.pack([_batch(["a", "b"], [0])], 3) is None                       # sizes that do not match
    assert pk.pack(BATCHES, 7, torch.tensor([31, 31], dtype=torch.int)) is None


def test_routing_without_a_gpu(monkeypatch):
    import tracking_utils as tu
    from qea import history
    from qea.loss import CTCLoss
    monkeypatch.delenv("QEA_HISTORY_CTC", raising=False)
    scores = torch.randn(31, 7, 95).log_softmax(2)
    w = torch.ones(3)
    assert history.ctc_route(scores, w, 3, 12, CTCLoss()) == "steps"           # CPU tensors
    meta = torch.empty(31, 7, 95, device="meta")
    assert history.ctc_route(meta, w, 3, 12, CTCLoss()) == "steps"
    assert history.MAX_WINDOW == 8 and history.CTC_MAX_LABEL == 127
    assert not history.ctc_steps_forced()
    monkeypatch.setenv("QEA_HISTORY_CTC", "steps")
    assert history.ctc_steps_forced()
    monkeypatch.delenv("QEA_HISTORY_CTC")
    # the public function on CPU tensors with torch's CTCLoss runs the reference's loop (decaying and sample-wise)
    pred = torch.full((7,), 31, dtype=torch.int)
    self = types.SimpleNamespace(window_size=3, weightgen_method="decaying", primary_loss_fn=torch.nn.CTCLoss(),
                                 primary_loss_fn_sample_wise=torch.nn.CTCLoss(reduction="none"))
    got = tu.weighted_ctc_loss(self, scores.double(), pred, BATCHES, torch.tensor([1.0, 0.7, 0.49]))
    want = sum(wi * torch.nn.functional.ctc_loss(scores.double()[:, idx, :], y, pred[idx], ys)
               for wi, (y, ys, idx) in zip([1.0, 0.7, 0.49], BATCHES))
    assert abs(got.item() - want.item()) <= 1e-6 * abs(want.item())
    assert not hasattr(self, "_ctc_packer")                                    # the loop was taken before anything was packed
