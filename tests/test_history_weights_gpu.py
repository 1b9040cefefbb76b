"""The label-history weight tables built on the device (csrc/history.hip through the generators of
label_tracking/tracking_methods.py): the reference's tables, the host generators at size, one launch per call, the fall-backs, and
the area trainer end to end."""
import copy
import json
import math
import types

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

ACTIVATIONS = ("sigmoid", "softmax", "relu")


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("QEA_HISTORY_WEIGHTS", raising=False)


def _generator(method, window, device, **kw):
    from label_tracking.tracking_methods import weightgenerator_factory
    args = types.SimpleNamespace(window_size=window, **kw)
    return weightgenerator_factory(method)(args, torch.device(device), H.C2I)


def test_levenshtein_reference_table():
    fx = H.golden("tracking_f3.npz")
    names, wg, self = H.f3_setup(fx, "levenshtein", torch.device("cuda"))
    assert wg.select_path(self.tracked_labels, names)[0] == "device"
    w = wg.gen_weights(self.tracked_labels, names)
    assert w.is_cuda and w.dtype == torch.float32 and w.shape == (len(names), int(fx["window"]) + 1)
    assert np.allclose(w.cpu().numpy(), fx["weights|levenshtein"], rtol=0, atol=0)


def test_attention_reference_tables():
    fx = H.golden("tracking_f3.npz")
    names, wg, self = H.f3_setup(fx, "self_attention", torch.device("cuda"))
    assert wg.select_path(self.tracked_labels, names)[0] == "device"
    worst = {}
    for act, key in (("sigmoid", "weights|self_attention"), ("softmax", "weights|self_attention_softmax"), ("relu", "weights|self_attention_relu")):
        wg.attention_model.activation = act
        w = wg.gen_weights(self.tracked_labels, names).cpu().numpy()
        worst[act] = float(np.abs(w - fx[key]).max())
        print(f"\n[gate] device attention table vs the reference's, {act}: worst error {worst[act]:.2e} (bound 1e-6)")
        assert np.allclose(w, fx[key], rtol=0, atol=1e-6), (act, worst[act])


def _lev_histories(n=2048, W=5, seed=11):
    """seeded histories over a three-letter alphabet (equal, near-equal and disjoint words all occur) with the corner cases planted"""
    rng = np.random.RandomState(seed)
    alphabets = ["abc", "abc", "xyz", "ab€"]

    def word():
        kind = rng.randint(0, 10)
        if kind == 0:
            return ""
        if kind == 1:
            return "".join(rng.choice(list("abc"), 100))
        return "".join(rng.choice(list(alphabets[rng.randint(0, 4)]), rng.randint(1, 9)))

    hist, names = {}, []
    for r in range(n):
        name = f"s{r}"
        names.append(name)
        depth = [0, 1, 2, 5, 3, 4, 7, 5][r % 8]
        if depth == 0:
            if r % 16 == 0:
                hist[name] = []                                    # known name, no labels yet; the others are unknown names
            continue
        if r % 8 == 7 and r % 3 == 0:
            hist[name] = [word()] * depth                          # all words identical
        elif r % 8 == 3 and r % 5 == 0:
            base = word() or "abc"
            hist[name] = [base[:-1] + rng.choice(list("abz")) for _ in range(depth)]     # near-equal words
        else:
            hist[name] = [word() for _ in range(depth)]
    return hist, names


def test_levenshtein_at_size_is_bit_equal_to_the_host_generator():
    W = 5
    hist, names = _lev_histories(2048, W)
    recent = [hist.get(nm, [])[-W:] for nm in names]
    counts = np.array([len(r) for r in recent])
    for c in (0, 1, 2, 5):
        assert (counts == c).sum() >= 50, (c, (counts == c).sum())
    words = [w for r in recent for w in r]
    assert sum(w == "" for w in words) >= 20
    assert sum(len(w) == 100 for w in words) >= 20
    assert sum(len(r) >= 2 and len(set(r)) == 1 for r in recent) >= 20
    assert max(len(w) for w in words) <= 128
    dev = _generator("levenshtein", W, "cuda")
    assert dev.select_path(hist, names)[0] == "device"             # no fall-back in this test
    got = dev.gen_weights(hist, names)
    want = _generator("levenshtein", W, "cpu").gen_weights(hist, names)
    diff = (got.cpu() - want).abs().max().item()
    print(f"\n[gate] device Levenshtein table, n=2048 W=5, vs the host generator: worst difference {diff:.1e} (must be 0)")
    assert torch.equal(got.cpu(), want)


def _fp64_scorer_table(model, hist, names, W):
    """the same HistoryAttention evaluated in fp64 on the CPU, strip by strip, as the host generator does"""
    import tracking_utils as tu
    m = copy.deepcopy(model).cpu().double()
    self = types.SimpleNamespace(char_to_index=H.C2I, window_size=W, device=torch.device("cpu"))
    w = torch.zeros(len(names), W + 1, dtype=torch.float64)
    w[:, 0] = 1
    with torch.no_grad():
        for r, nm in enumerate(names):
            h = hist[nm][-W:][::-1] if nm in hist else []
            if h:
                w[r, 1:len(h) + 1] = m(tu.str_to_tensor(self, h))[:len(h)]
    return w


def test_attention_at_size_against_fp64():
    n, W = 2048, 5
    rng = np.random.RandomState(5)
    chars = H.CHAR_SET[1:]
    hist, names = {}, []
    for r in range(n):
        names.append(f"s{r}")
        depth = rng.randint(0, 8)
        if depth:
            hist[names[-1]] = ["".join(rng.choice(chars, rng.randint(0, 26))) for _ in range(depth)]
    torch.manual_seed(7)
    wg = _generator("self_attention", W, "cuda", query_dim=32, emb_dim=256, attn_activation="sigmoid")
    with torch.no_grad():
        wg.attention_model.positional_encodings.copy_(torch.normal(0, 0.5, (W, 256)))
    assert wg.select_path(hist, names)[0] == "device"
    for act in ACTIVATIONS:
        wg.attention_model.activation = act
        got = wg.gen_weights(hist, names).cpu().double()
        want = _fp64_scorer_table(wg.attention_model, hist, names, W)
        err = (got - want).abs().max().item()
        print(f"\n[gate] device attention table, n=2048 W=5 E=256 Dq=32, {act}: worst error against fp64 {err:.2e} (bound 1e-6)")
        assert err <= 1e-6, (act, err)
        assert (got[:, 1:].abs().sum(dim=1) > 0).sum().item() == sum(1 for nm in names if hist.get(nm))


@pytest.mark.parametrize("method", ["levenshtein", "self_attention"])
def test_one_launch_per_call(method, monkeypatch):
    from models.model_attention import HistoryAttention
    from qea import ops
    key = "lev" if method == "levenshtein" else "attn"
    calls = []
    real_forward = HistoryAttention.forward
    monkeypatch.setattr(HistoryAttention, "forward", lambda self, x: calls.append(1) or real_forward(self, x))
    wg = _generator(method, 5, "cuda")
    for n in (32, 2048):
        hist, names = _lev_histories(n, 5, seed=n)
        hist = {k: [w.replace("€", "e")[:100] for w in v] for k, v in hist.items()}
        before = dict(ops.HISTORY_LAUNCHES)
        w = wg.gen_weights(hist, names)
        assert w.shape == (n, 6)
        after = dict(ops.HISTORY_LAUNCHES)
        assert after[key] - before[key] == 1, (n, before, after)
        other = "attn" if key == "lev" else "lev"
        assert after[other] == before[other]
    assert not calls                                               # the torch module is not evaluated on the device path


def test_fallbacks_on_the_device():
    hist = {"a": ["abc", "abd", "x" * 129], "b": ["same", "same"], "c": ["q"]}
    names = ["a", "b", "c", "unknown"]
    dev = _generator("levenshtein", 3, "cuda")
    assert dev.select_path(hist, names) == ("host", None)
    got = dev.gen_weights(hist, names)
    assert got.is_cuda
    assert torch.equal(got.cpu(), _generator("levenshtein", 3, "cpu").gen_weights(hist, names))
    wide = _generator("levenshtein", 9, "cuda")
    assert torch.equal(wide.gen_weights(hist, names).cpu(), _generator("levenshtein", 9, "cpu").gen_weights(hist, names))
    att = _generator("self_attention", 3, "cuda")
    with pytest.raises(KeyError):
        att.gen_weights({"a": ["ok", "日本"]}, ["a"])
    cpu_att = _generator("self_attention", 3, "cpu")
    with pytest.raises(KeyError):
        cpu_att.gen_weights({"a": ["ok", "日本"]}, ["a"])
    for g in (att, cpu_att):                                       # a 101-character word: the same exception type on both paths
        with pytest.raises(ValueError):
            g.gen_weights({"a": ["ok", "z" * 101]}, ["a"])


def test_host_switch_keeps_the_loops(monkeypatch):
    from qea import ops
    monkeypatch.setenv("QEA_HISTORY_WEIGHTS", "host")
    hist, names = _lev_histories(32, 5, seed=3)
    before = dict(ops.HISTORY_LAUNCHES)
    w = _generator("levenshtein", 5, "cuda").gen_weights(hist, names)
    assert ops.HISTORY_LAUNCHES == before and w.is_cuda
    assert torch.equal(w.cpu(), _generator("levenshtein", 5, "cpu").gen_weights(hist, names))


@pytest.mark.parametrize("method", ["levenshtein", "self_attention"])
def test_area_trainer_uses_the_device_tables(tmp_path, method, monkeypatch):
    import train_nn_area
    from datasets.synthetic import SyntheticTextAreas
    from qea import ops
    from qea.cli_flags import build_parser
    tr = SyntheticTextAreas(16, seed=3, include_name=True, include_index=True)
    cers_path = tmp_path / "cers.json"
    json.dump({n: 0.5 for n in tr.names}, open(cers_path, "w"))
    args = build_parser("a", "").parse_args(["--exp_base_path", str(tmp_path / "exp"), "--ocr", "stub", "--epoch", "2", "--inner_limit_skip",
                                             "--window_size", "3", "--weightgen_method", method, "--batch_size", "8", "--inner_limit", "2",
                                             "--minibatch_subset", "topKCER", "--minibatch_subset_prop", "0.5", "--cers_ocr_path", str(cers_path)])
    t = train_nn_area.TrainNNPrep(args, train_set=tr, val_set=SyntheticTextAreas(8, seed=4, include_name=True))
    wg = t.loss_wghts_gnrtr
    seen, losses = [], []
    real_gen = wg.gen_weights

    def spy_gen(tracked_labels, img_names):
        w = real_gen(tracked_labels, img_names)
        seen.append((copy.deepcopy(tracked_labels), list(img_names), w.detach().cpu().clone()))
        return w

    real_loss = train_nn_area.weighted_ctc_loss

    def spy_loss(*a, **k):
        loss = real_loss(*a, **k)
        losses.append(loss.detach())
        return loss

    monkeypatch.setattr(wg, "gen_weights", spy_gen)
    monkeypatch.setattr(train_nn_area, "weighted_ctc_loss", spy_loss)
    key = "lev" if method == "levenshtein" else "attn"
    before = ops.HISTORY_LAUNCHES[key]
    t.train()
    assert seen and ops.HISTORY_LAUNCHES[key] - before == len(seen)          # every table came from the kernel
    assert max(len(v) for snap, _, _ in seen for v in snap.values()) >= 1    # the second epoch saw real histories
    worst = 0.0
    for snap, names, w in seen:
        if method == "levenshtein":
            want = _generator("levenshtein", 3, "cpu").gen_weights(snap, names)
            assert torch.equal(w, want)
        else:
            host = wg._gen_weights_host(snap, names).cpu()
            err = (w - host).abs().max().item()
            worst = max(worst, err)
            assert err <= 1e-6, err
    print(f"\n[gate] trainer tables, {method}: {len(seen)} calls, worst difference from the host generator {worst:.2e}")
    assert losses and all(math.isfinite(float(l)) for l in losses)
