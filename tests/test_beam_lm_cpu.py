"""The CTC prefix beam search with a character n-gram prior fused in, without a GPU: the literal specification (tests/beam_lm_spec.py)
against the plain search and the CTC likelihood, the host loop (qea/beam.py) against the specification, hard constraints, a hand-made
tip, qea.lm.CharLM, the pred_to_string / eval_crnn / lm_cli interface and the refusals."""
import math

import numpy as np
import pytest
import torch

import beam_lm_spec
import beam_spec
import helpers as H
from beam_checks import same_scores as _same_scores


def _host(lp, K, W, m, blank=0):
    from qea import beam as host
    return host.ctc_beam_decode(lp, K, blank, W, m)


@pytest.mark.parametrize("m", [0, 1, 2])
def test_zero_table_is_the_plain_search(m):
    """W = 0: the specification and the host loop return beam_spec.decode's beams exactly, ctc bit-equal to the plain scores and
    total == ctc."""
    T, N, C, K = 7, 6, 5, 4
    lp = beam_spec.log_probs(T, N, C, seed=2)
    plain, _ = beam_spec.decode_batch(lp, K)
    W = torch.zeros(C ** m, C, dtype=torch.float64)
    fused, _ = beam_lm_spec.decode_batch(lp, K, W, m)
    assert [[(p, s) for p, s, _ in b] for b in fused] == plain
    assert all(s == tt for b in fused for _, s, tt in b)
    wt, wl, ws = beam_spec.as_arrays(plain, K, T)
    tokens, lengths, ctc, total = _host(lp, K, W, m)
    assert tokens.tolist() == wt and lengths.tolist() == wl
    from qea import beam as host
    assert torch.equal(ctc, host.ctc_beam_decode(lp, K)[2]) and torch.equal(total, ctc)
    assert _same_scores(ctc.tolist(), ws)


def test_exhaustive_scores_are_the_likelihood_and_the_table_sum():
    """C = 3, T = 5, K = 32 holds every live labelling: ctc is its CTC log-likelihood, total - ctc the sum of the table entries along
    it (both within 1e-9), total does not increase with rank."""
    T, N, C, K, m = 5, 8, 3, 32, 2
    lp = beam_spec.log_probs(T, N, C, seed=16)
    W = beam_lm_spec.table(C, m, 1)
    seen = 0
    for n in range(N):
        beam, _ = beam_lm_spec.decode(lp[:, n].tolist(), K, W.tolist(), m)
        assert len({p for p, _, _ in beam}) == len(beam)
        for p, ctc, total in beam:
            assert abs(ctc - beam_spec.ctc_log_likelihood(lp[:, n], p)) <= 1e-9, (n, p)
            assert abs((total - ctc) - beam_lm_spec.table_sum(W, p, C, m)) <= 1e-9, (n, p)
        assert all(a[2] >= b[2] for a, b in zip(beam, beam[1:]))
        seen += len(beam)
    assert seen >= 150


@pytest.mark.parametrize("T,C,K,m,blank", [(7, 5, 4, 2, 0), (7, 5, 4, 1, 4), (6, 4, 8, 2, 3), (31, 95, 8, 1, 0), (5, 3, 32, 2, 0), (9, 6, 6, 0, 0)])
def test_host_loop_equals_the_spec(T, C, K, m, blank):
    """qea/beam.py's fused path returns the specification's beams: same prefixes in the same order, both scores within
    1e-12 * max(1, |s|)."""
    N = 5
    lp = beam_spec.log_probs(T, N, C, seed=200 + T, blank=blank)
    W = beam_lm_spec.table(C, m, 200 + T)
    want, _ = beam_lm_spec.decode_batch(lp, K, W, m, blank)
    tokens, lengths, ctc, total = _host(lp, K, W, m, blank)
    assert tokens.shape == (N, K, T) and tokens.dtype == torch.int32 and lengths.shape == (N, K) and lengths.dtype == torch.int32
    assert ctc.shape == total.shape == (N, K) and ctc.dtype == total.dtype == torch.float64
    wt, wl, wc, wtot = beam_lm_spec.as_arrays(want, K, T)
    assert tokens.tolist() == wt and lengths.tolist() == wl
    assert _same_scores(ctc.tolist(), wc) and _same_scores(total.tolist(), wtot)
    assert all(blank not in p for b in want for p, _, _ in b)
    if (T, C, K) == (5, 3, 32):
        dead = lengths == -1
        assert dead.any() and (ctc[dead] == -math.inf).all() and (total[dead] == -math.inf).all()


def test_hard_constraints():
    """A table entry of -inf and a NaN entry never appear as adjacent tokens of a returned prefix, in the specification and in the
    host loop; with every extension forbidden the live count drops below K."""
    T, N, C, K = 7, 20, 5, 8
    lp, W = beam_lm_spec.forbidden_case(T, N, C, K, 21)
    beams, _ = beam_lm_spec.decode_batch(lp, K, W, 1)
    assert not any(beam_lm_spec.has_forbidden_pair(p) for b in beams for p, _, _ in b)
    tokens, lengths, ctc, total = _host(lp, K, W, 1)
    wt, wl, _, _ = beam_lm_spec.as_arrays(beams, K, T)
    assert tokens.tolist() == wt and lengths.tolist() == wl and not torch.isnan(total).any()
    plain, _ = beam_spec.decode_batch(lp, K)
    assert any(beam_lm_spec.has_forbidden_pair(p) for b in plain for p, _ in b)            # the constraint did something
    # only the empty prefix and "1" can live: two entries, the other ranks are padding
    W = torch.full((C, C), -math.inf, dtype=torch.float64)
    W[0, 1] = -0.5
    beams, _ = beam_lm_spec.decode_batch(lp, K, W, 1)
    assert all(sorted(p for p, _, _ in b) == [(), (1,)] for b in beams)
    tokens, lengths, ctc, total = _host(lp, K, W, 1)
    assert ((lengths >= 0).sum(dim=1) == 2).all() and (total[lengths < 0] == -math.inf).all()


class _TinyLM:
    """The three-class model of the hand-made tip: duck-typed like qea.lm.CharLM."""
    num_classes, blank, context, order = 3, 0, 1, 2

    def fused(self, alpha, beta, device):
        logp = torch.zeros(3, 3, dtype=torch.float64)
        logp[0, 2] = 1.0                                    # W[BOS][b] - W[BOS][a] = 1 at weight 1
        return (alpha * logp + beta).to(device)


def test_a_hand_made_tip():
    """T = 1, classes {blank, a, b} with probabilities (0.2, 0.41, 0.39): the plain beam reads "a"; a table that favours b after BOS
    by 1 tips the fused search to "b"; at weight 0 it reads "a" again."""
    from utils import pred_to_string
    i2c = {0: "-", 1: "a", 2: "b"}
    lp = torch.log(torch.tensor([[[0.2, 0.41, 0.39]]]))
    assert pred_to_string(lp, [""], i2c, beam=4) == ["a"]
    assert pred_to_string(lp, [""], i2c, beam=4, lm=_TinyLM()) == ["b"]
    assert pred_to_string(lp, [""], i2c, beam=4, lm=_TinyLM(), lm_weight=0.0) == ["a"]
    strings, total = pred_to_string(lp, [""], i2c, beam=4, lm=_TinyLM(), nbest=3, return_scores=True)
    assert strings == [["b", "a", ""]]
    assert total[0] == pytest.approx([math.log(0.39) + 1.0, math.log(0.41), math.log(0.2)], abs=1e-6)


# ---- qea.lm.CharLM
_VOCAB = {"-": 0, "a": 1, "b": 2, "c": 3}
_LABELS = ["ab", "abc", "b"]


def _check_rows(lm, k):
    p = np.exp(lm.logp)
    p[:, lm.blank] = 0.0
    assert np.allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    want = (lm.count + k) / (lm.count.sum(axis=1, keepdims=True) + 3 * k)
    want[:, 0] = 0.0
    assert np.allclose(p, want, rtol=1e-15, atol=0) and (lm.logp[:, 0] == 0.0).all()


def test_charlm_counts_and_probabilities():
    from qea.lm import CharLM
    k = 0.1
    uni = CharLM.from_labels(_LABELS, _VOCAB, order=1, add_k=k)
    assert uni.logp.shape == (1, 4) and uni.count.tolist() == [[0, 2, 3, 1]]
    assert math.exp(uni.logp[0, 2]) == pytest.approx((3 + k) / (6 + 3 * k), rel=1e-14)
    bi = CharLM.from_labels(_LABELS, _VOCAB, order=2, add_k=k)
    want = np.zeros((4, 4))
    want[0, 1], want[0, 2], want[1, 2], want[2, 3] = 2, 1, 2, 1          # BOS a x2, BOS b, a b x2, b c
    assert bi.logp.shape == (4, 4) and (bi.count == want).all()
    assert math.exp(bi.logp[1, 2]) == pytest.approx((2 + k) / (2 + 3 * k), rel=1e-14)
    assert math.exp(bi.logp[3, 1]) == pytest.approx(1 / 3, rel=1e-14)     # an unseen context is uniform
    tri = CharLM.from_labels(_LABELS, _VOCAB, order=3, add_k=k)
    want = np.zeros((16, 4))
    want[0 * 4 + 0, 1], want[0 * 4 + 0, 2] = 2, 1                         # (BOS, BOS) a x2, (BOS, BOS) b
    want[0 * 4 + 1, 2] = 2                                                # (BOS, a) b x2: the BOS padding is visible here
    want[1 * 4 + 2, 3] = 1                                                # (a, b) c
    assert tri.logp.shape == (16, 4) and (tri.count == want).all() and tri.context == 2
    for lm in (uni, bi, tri):
        _check_rows(lm, k)
    # another blank: the BOS rows move with it
    last = CharLM.from_labels(["ab"], {"a": 0, "b": 1, "-": 2}, order=2, add_k=k, blank=2)
    assert last.count[2, 0] == 1 and last.count[0, 1] == 1 and last.count.sum() == 2 and (last.logp[:, 2] == 0.0).all()
    from qea._lib import QeaError
    for bad in (lambda: CharLM.from_labels(["abd"], _VOCAB), lambda: CharLM.from_labels(["a-"], _VOCAB),
                lambda: CharLM.from_labels(_LABELS, _VOCAB, order=4), lambda: CharLM.from_labels(_LABELS, _VOCAB, order=0),
                lambda: CharLM.from_labels(_LABELS, _VOCAB, add_k=0.0)):
        with pytest.raises(QeaError):
            bad()


def test_charlm_save_load_and_fused(tmp_path):
    from qea._lib import QeaError
    from qea.lm import CharLM
    lm = CharLM.from_labels(_LABELS, _VOCAB, order=3, add_k=0.25)
    path = str(tmp_path / "model.lm")
    lm.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["add_k", "blank", "logp", "order", "vocabulary"]
    back = CharLM.load(path, _VOCAB)
    assert (back.logp == lm.logp).all() and (back.order, back.add_k, back.blank, back.vocabulary) == (3, 0.25, 0, ["-", "a", "b", "c"])
    assert CharLM.load(path).vocabulary == lm.vocabulary
    with pytest.raises(QeaError):
        CharLM.load(path, {"-": 0, "a": 1, "c": 2, "b": 3})
    with pytest.raises(QeaError):
        CharLM.load(path, {"-": 0, "a": 1, "b": 2})
    W = lm.fused(0.5, 0.25, "cpu")
    assert W.dtype == torch.float64 and W.shape == (16, 4) and W.is_contiguous()
    assert torch.equal(W, torch.from_numpy(0.5 * lm.logp + 0.25))
    assert lm.fused(0.5, 0.25, "cpu") is W and lm.fused(0.5, 0.5, "cpu") is not W


# ---- interface
def _synthetic_lm(order=2):
    from qea.lm import CharLM
    return CharLM.from_labels(H.synth_labels(64, 5), H.C2I, order=order, add_k=0.1)


def test_pred_to_string_interface():
    """lm without beam raises; beam without lm is today's output; with lm the strings are the fused specification's and the scores
    its totals; batch_cers refuses lm without beam as well."""
    from qea._lib import QeaError
    from utils import batch_cers, pred_to_string
    T, N, C, K = 12, 6, 95, 4
    lp = beam_spec.log_probs(T, N, C, seed=31)
    labels = [""] * N
    lm = _synthetic_lm()
    with pytest.raises(QeaError):
        pred_to_string(lp, labels, H.I2C, lm=lm)
    with pytest.raises(QeaError):
        batch_cers(lp, labels, H.C2I, lm=lm)
    plain, _ = beam_spec.decode_batch(lp, K)
    assert pred_to_string(lp, labels, H.I2C, beam=K) == pred_to_string(lp, labels, H.I2C, beam=K, lm=None, lm_weight=3.0, lm_bonus=1.0) \
        == ["".join(H.I2C[i] for i in b[0][0]) for b in plain]
    want, _ = beam_lm_spec.decode_batch(lp, K, lm.fused(0.7, 0.3, "cpu"), 1)
    strings, total = pred_to_string(lp, labels, H.I2C, beam=K, lm=lm, lm_weight=0.7, lm_bonus=0.3, return_scores=True)
    assert strings == ["".join(H.I2C[i] for i in b[0][0]) for b in want]
    assert all(abs(a - b[0][2]) <= 1e-12 * max(1.0, abs(a)) for a, b in zip(total, want))
    lists = pred_to_string(lp, labels, H.I2C, beam=K, lm=lm, lm_weight=0.7, lm_bonus=0.3, nbest=3)
    assert [l[0] for l in lists] == strings and all(len(l) == 3 for l in lists)
    with pytest.raises(QeaError):                              # a model over another number of classes
        pred_to_string(lp[:, :, :50], labels, H.I2C, beam=K, lm=lm)


def test_the_flags_are_on_eval_crnn_only():
    from qea.cli_flags import build_parser
    ap = build_parser("e", "")
    act = {a.option_strings[0]: a for a in ap._actions if a.option_strings}
    for flag, default, ty in (("--lm", None, None), ("--lm_weight", 1.0, float), ("--lm_bonus", 0.0, float)):
        assert act[flag].help.startswith("[new]") and act[flag].default == default and act[flag].type is ty
    args = ap.parse_args(["--beam", "4", "--lm", "x.npz", "--lm_weight", "0.5"])
    assert (args.lm, args.lm_weight, args.lm_bonus) == ("x.npz", 0.5, 0.0)
    for tag in "cvpanr":
        ns = vars(build_parser(tag, "").parse_args(["--cers_tess_path", "x"] if tag == "r" else
                                                   ["--in_dir", "a", "--out_dir", "b"] if tag == "n" else []))
        assert not {"lm", "lm_weight", "lm_bonus"} & set(ns)


def test_eval_crnn_reports_the_lm_numbers(tmp_path):
    """EvalCRNN --beam 4 --lm on the oracle CRNN (CPU tensors: the host loop): exactly five more keys than --beam 4 alone, the same
    count; --lm without --beam is refused."""
    import lm_cli
    from datasets.synthetic import SyntheticTextAreas
    from eval_crnn import EvalCRNN, build_parser
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.lm import CharLM
    from qea.trainer_core import Backend
    from utils import pred_to_string
    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    model = OracleCRNN(95, False, seed=3).eval()
    torch.save(model, tmp_path / "crnn_ckpt")
    path = str(tmp_path / "chars.npz")
    built = lm_cli.main(["--dataset", "vgg", "--synthetic_size", "40", "--order", "3", "--add_k", "0.5", "--out", path])
    lm = CharLM.load(path, H.C2I)                              # lm_cli.py --synthetic_size writes a loadable file
    assert lm.order == 3 and lm.add_k == 0.5 and (lm.logp == built.logp).all() and lm.logp.shape == (95 * 95, 95)
    va = SyntheticTextAreas(4, seed=2)
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--dataset", "vgg", "--batch_size", "2", "--ocr", "stub"]
    beam = EvalCRNN(build_parser().parse_args(argv + ["--beam", "4"]), backend=backend, dataset=va).eval()
    assert sorted(beam) == ["beam", "count", "crnn_accuracy", "crnn_cer", "crnn_correct", "crnn_mean_log_score", "greedy_disagreements"]
    res = EvalCRNN(build_parser().parse_args(argv + ["--beam", "4", "--lm", path, "--lm_weight", "0.8", "--lm_bonus", "0.5"]),
                   backend=backend, dataset=va).eval()
    assert sorted(set(res) - set(beam)) == ["crnn_mean_total_score", "lm_bonus", "lm_disagreements", "lm_order", "lm_weight"]
    assert (res["lm_order"], res["lm_weight"], res["lm_bonus"], res["beam"], res["count"]) == (3, 0.8, 0.5, 4, 4)
    with torch.no_grad():                                     # the loader's batches of two
        lp = torch.cat([model(torch.stack([va[i][0] for i in (0, 1)])), model(torch.stack([va[i][0] for i in (2, 3)]))], dim=1)
    strings, total = pred_to_string(lp, [""] * 4, H.I2C, beam=4, lm=lm, lm_weight=0.8, lm_bonus=0.5, return_scores=True)
    plain = pred_to_string(lp, [""] * 4, H.I2C, beam=4)
    assert res["crnn_mean_total_score"] == pytest.approx(sum(total) / 4, rel=1e-9)
    assert res["lm_disagreements"] == sum(a != b for a, b in zip(strings, plain)) and 0 <= res["lm_disagreements"] <= 4
    # crnn_mean_log_score stays the CTC log-probability of the chosen readings: total minus the table entries along them
    ctc = [t - beam_lm_spec.table_sum(lm.fused(0.8, 0.5, "cpu"), [H.C2I[c] for c in s], 95, 2) for s, t in zip(strings, total)]
    assert res["crnn_mean_log_score"] == pytest.approx(sum(ctc) / 4, rel=1e-9)
    with pytest.raises(ValueError):
        EvalCRNN(build_parser().parse_args(argv + ["--lm", path]), backend=backend, dataset=va)


def test_refusals():
    from qea import beam as host
    from qea._lib import QeaError
    lp = torch.zeros(4, 2, 5)
    ok = torch.zeros(25, 5, dtype=torch.float64)
    host.ctc_beam_decode(lp, 2, 0, ok, 2)
    for bad in (lambda: host.ctc_beam_decode(lp, 2, 0, torch.zeros(125, 5, dtype=torch.float64), 3),          # m = 3
                lambda: host.ctc_beam_decode(lp, 2, 0, ok, -1),
                lambda: host.ctc_beam_decode(torch.zeros(2, 1, 129), 2, 0, torch.zeros(1, 129, dtype=torch.float64), 2),   # C^3 > 2^21
                lambda: host.ctc_beam_decode(lp, 2, 0, ok, 1),                                                   # [25,5] is no bigram table
                lambda: host.ctc_beam_decode(lp, 2, 0, torch.zeros(5, 25, dtype=torch.float64), 2),
                lambda: host.ctc_beam_decode(lp, 2, 0, None, 1),
                lambda: host.ctc_beam_decode(lp, 33, 0, ok, 2)):
        with pytest.raises(QeaError):
            bad()
    host.check_lm_limits(128, 2)
    host.check_lm_limits(256, 1)
    with pytest.raises(QeaError):
        host.check_lm_limits(256, 2)
