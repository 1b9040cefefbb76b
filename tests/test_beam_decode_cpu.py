"""CTC prefix beam search without a GPU: the specification (tests/beam_spec.py) against the CTC likelihood itself, the host loop
(qea/beam.py) against the specification, the pred_to_string interface on CPU tensors, hand-made cases, and the eval_crnn flag."""
import math

import pytest
import torch
import torch.nn.functional as F

import beam_spec
import helpers as H
from beam_checks import same_scores as _same_scores


_log_probs, _ctc_log_likelihood = beam_spec.log_probs, beam_spec.ctc_log_likelihood


def test_spec_scores_are_the_ctc_likelihoods():
    """C = 3, T = 4, K = 32 holds every labelling there is (at most 31 prefixes): each score is that labelling's CTC log-likelihood
    within 1e-9, and rank 0 is the most likely one."""
    lp = _log_probs(4, 20, 3, seed=11)
    seen = 0
    for n in range(20):
        beam, _ = beam_spec.decode(lp[:, n].tolist(), 32)
        assert 1 <= len(beam) <= 31 and len({p for p, _ in beam}) == len(beam)
        want = [_ctc_log_likelihood(lp[:, n], p) for p, _ in beam]
        for (p, s), w in zip(beam, want):
            assert abs(s - w) <= 1e-9, (n, p, s, w)
        assert beam[0][1] == max(s for _, s in beam) and want[0] == max(want)
        assert all(a[1] >= b[1] for a, b in zip(beam, beam[1:]))
        seen += len(beam)
    assert seen >= 300


@pytest.mark.parametrize("T,C,K", [(7, 5, 4), (31, 95, 8), (5, 3, 32)])
def test_host_loop_equals_the_spec(T, C, K):
    """qea/beam.py returns the specification's beams: same prefixes in the same order, scores within 1e-12 * max(1, |s|)."""
    from qea import beam as host
    N = 6
    lp = _log_probs(T, N, C, seed=100 + T)
    want, _ = beam_spec.decode_batch(lp, K)
    tokens, lengths, scores = host.ctc_beam_decode(lp, K)
    assert tokens.shape == (N, K, T) and tokens.dtype == torch.int32 and lengths.shape == (N, K) and lengths.dtype == torch.int32
    assert scores.shape == (N, K) and scores.dtype == torch.float64
    wt, wl, ws = beam_spec.as_arrays(want, K, T)
    assert tokens.tolist() == wt and lengths.tolist() == wl and _same_scores(scores.tolist(), ws)
    if (T, C, K) == (5, 3, 32):
        assert (lengths == -1).any() and (scores[lengths == -1] == -math.inf).all()      # fewer labellings than K: padded rows


def test_host_loop_with_another_blank_and_with_minus_inf():
    from qea import beam as host
    lp = _log_probs(6, 4, 4, seed=5, blank=3)
    lp[:, :, 1] = -math.inf
    lp[2, 1, 0] = float("nan")
    want, _ = beam_spec.decode_batch(lp, 8, blank=3)
    tokens, lengths, scores = host.ctc_beam_decode(lp, 8, blank=3)
    wt, wl, ws = beam_spec.as_arrays(want, 8, 6)
    assert tokens.tolist() == wt and lengths.tolist() == wl and not torch.isnan(scores).any()
    assert _same_scores(scores.tolist(), ws)
    assert all(1 not in p and 3 not in p for b in want for p, _ in b)


def test_pred_to_string_interface_on_cpu_tensors():
    """beam=0 is today's greedy output on the decode fixture; beam / nbest / return_scores give the documented shapes."""
    from utils import pred_to_string
    fx = H.golden("helpers.npz")
    scores = torch.from_numpy(fx["dec|scores"])
    T, B, C = scores.shape
    want = [str(s) for s in fx["dec|strings"]]
    assert pred_to_string(scores, want, H.I2C) == want
    assert pred_to_string(scores, want, H.I2C, beam=0, nbest=1, return_scores=False) == want
    lp = F.log_softmax(scores.float(), dim=2)
    best = pred_to_string(lp, want, H.I2C, beam=4)
    assert len(best) == B and all(isinstance(s, str) for s in best)
    lists, logp = pred_to_string(lp, want, H.I2C, beam=4, nbest=3, return_scores=True)
    assert len(lists) == len(logp) == B
    for b in range(B):
        assert len(lists[b]) == len(logp[b]) == 3 and lists[b][0] == best[b] and len(set(lists[b])) == 3
        assert all(isinstance(v, float) for v in logp[b]) and logp[b][0] >= logp[b][1] >= logp[b][2]
    one, s1 = pred_to_string(lp, want, H.I2C, beam=4, return_scores=True)
    assert one == best and s1 == [l[0] for l in logp]
    spec, _ = beam_spec.decode_batch(lp, 4)
    assert best == ["".join(H.I2C[i] for i in b[0][0]) for b in spec]
    from qea._lib import QeaError
    with pytest.raises(QeaError):
        pred_to_string(lp, want, H.I2C, beam=4, nbest=5)
    with pytest.raises(QeaError):
        pred_to_string(lp, want, H.I2C, nbest=2)
    with pytest.raises(QeaError):
        pred_to_string(lp, want, H.I2C, beam=33)


def _one_hot_rows(classes, C=4, hot=-0.01):
    """T rows that put nearly all mass on the given classes."""
    rest = math.log((1 - math.exp(hot)) / (C - 1))
    lp = torch.full((len(classes), 1, C), rest)
    for t, c in enumerate(classes):
        lp[t, 0, c] = hot
    return lp


def test_hand_made_cases():
    from utils import pred_to_string
    i2c = {0: "-", 1: "a", 2: "b", 3: "c"}
    assert pred_to_string(_one_hot_rows([1, 1, 0, 1]), [""], i2c, beam=4) == ["aa"]
    assert pred_to_string(_one_hot_rows([1, 1, 1]), [""], i2c, beam=4) == ["a"]
    assert pred_to_string(_one_hot_rows([0, 0, 0]), [""], i2c, beam=4) == [""]
    # greedy reads the best path, the beam the best labelling: blank leads every step, yet "a" has more mass than ""
    lp = torch.log(torch.tensor([[[0.4, 0.3, 0.3, 0.0]], [[0.4, 0.3, 0.3, 0.0]]]))
    assert pred_to_string(lp, [""], i2c) == [""] and pred_to_string(lp, [""], i2c, beam=4) == ["a"]


def test_eval_crnn_has_the_beam_flag():
    from eval_crnn import build_parser as front_end
    from qea.cli_flags import build_parser
    ap = build_parser("e", "")
    act = {a.option_strings[0]: a for a in ap._actions if a.option_strings}["--beam"]
    assert act.help.startswith("[new]") and act.default == 0 and act.type is int
    assert ap.parse_args([]).beam == 0 and front_end().parse_args(["--beam", "8"]).beam == 8
    for tag in "cvpa":                                        # the other front ends, the trainers among them, keep greedy
        assert not hasattr(build_parser(tag, "").parse_args([]), "beam")


def test_eval_crnn_reports_the_beam_numbers(tmp_path):
    """EvalCRNN --beam on the oracle CRNN (CPU tensors: the host loop): three more keys, the same count; without the flag the dict
    has today's keys only."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_crnn import EvalCRNN, build_parser
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    from utils import pred_to_string
    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    model = OracleCRNN(95, False, seed=3).eval()
    torch.save(model, tmp_path / "crnn_ckpt")
    va = SyntheticTextAreas(4, seed=2)
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--dataset", "vgg", "--batch_size", "2", "--ocr", "stub"]
    plain = EvalCRNN(build_parser().parse_args(argv), backend=backend, dataset=va).eval()
    assert sorted(plain) == ["count", "crnn_accuracy", "crnn_cer", "crnn_correct"]
    res = EvalCRNN(build_parser().parse_args(argv + ["--beam", "4"]), backend=backend, dataset=va).eval()
    assert sorted(set(res) - set(plain)) == ["beam", "crnn_mean_log_score", "greedy_disagreements"]
    assert res["beam"] == 4 and res["count"] == plain["count"] == 4
    with torch.no_grad():                                     # the loader's batches of two
        lp = torch.cat([model(torch.stack([va[i][0] for i in (0, 1)])), model(torch.stack([va[i][0] for i in (2, 3)]))], dim=1)
    strings, logp = pred_to_string(lp, [""] * 4, H.I2C, beam=4, return_scores=True)
    greedy = pred_to_string(lp, [""] * 4, H.I2C)
    assert res["crnn_mean_log_score"] == pytest.approx(sum(logp) / 4, rel=1e-9)
    assert res["greedy_disagreements"] == sum(a != b for a, b in zip(strings, greedy))
