"""The device CTC prefix beam search (csrc/ctc_beam.hip, qea.ops.ctc_beam_decode) against the fp64 specification of
tests/beam_spec.py: the WHOLE beam must match, tokens, lengths and rank order exactly and scores within 1e-9 * max(1, |s|) (a few ulp
per step over at most 512 steps at |s| < 2500 is ~1e-10).

An exact comparison of a discrete result is only fair where no decision hangs on fp64 rounding: every case asserts that the smallest
non-zero gap between two scores whose order decided something (beam_spec.decode) is at least 1e-7 for its input.  The seeds below
were chosen on the CPU so that this holds; no case is skipped."""
import functools
import math

import pytest
import torch

import beam_checks
import beam_spec
import helpers as H

pytestmark = pytest.mark.gpu

MIN_GAP = beam_checks.MIN_GAP


@functools.lru_cache(maxsize=None)
def _case(T, N, C, K, seed, blank=0, variant=""):
    """(log-probs [T,N,C] fp32 on the CPU, the specification's beams, its smallest non-zero gap); computed once per case."""
    lp = beam_spec.log_probs(T, N, C, seed, blank=blank)
    if variant == "ties":                                   # classes 1 and 2 are indistinguishable
        lp[:, :, 2] = lp[:, :, 1]
    if variant == "inf":                                    # two classes impossible at every step, one entry NaN
        lp[:, :, 1] = -math.inf
        lp[:, :, 2] = -math.inf
        lp[2, 1, 3] = float("nan")
    beams, gap = beam_spec.decode_batch(lp, K, blank)
    return lp, beams, gap


def _check_against_spec(dev_scores, K, blank, beams, gap):
    from qea import ops
    return beam_checks.check_against_spec(ops.ctc_beam_decode(dev_scores, K, blank), beam_spec.as_arrays(beams, K, dev_scores.shape[0]), gap)


# (T, N, C, K, seed): one sample; more samples than CUs; K = 1; each candidate-register variant (1, 4, 12, 32 per thread); the longest
# T; fewer live prefixes than K in the early steps (the -1 / -inf padding).  The last two rows are the limits of C and of T.
SHAPES = [(1, 3, 2, 1, 1), (7, 300, 5, 4, 2), (31, 17, 95, 1, 3), (31, 17, 95, 8, 4), (31, 5, 95, 32, 5), (127, 2, 95, 16, 6),
          (5, 33, 3, 32, 7), (3, 2, 256, 32, 8), (512, 1, 4, 32, 9)]


@pytest.mark.parametrize("T,N,C,K,seed", SHAPES)
def test_beam_equals_the_spec(T, N, C, K, seed):
    lp, beams, gap = _case(T, N, C, K, seed)
    _, lengths, _ = _check_against_spec(lp.cuda(), K, 0, beams, gap)
    if (T, C, K) == (5, 3, 32):
        assert (lengths == -1).any()


def test_padded_strides():
    """A [T,N,C] view of a larger buffer: ld_t and ld_n both padded, the padding filled with values that would win every step."""
    T, N, C, K = 7, 9, 5, 4
    lp, beams, gap = _case(T, N, C, K, 12)
    big = torch.full((T, N + 3, C + 5), 50.0, device="cuda")
    view = big[:, 2:2 + N, :C]
    view.copy_(lp)
    assert view.stride() == ((N + 3) * (C + 5), C + 5, 1) and not view.is_contiguous()
    _check_against_spec(view, K, 0, beams, gap)
    # a [N,T,C] buffer read as [T,N,C]: ld_t < ld_n
    _check_against_spec(lp.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), K, 0, beams, gap)


def test_blank_is_the_last_class():
    T, N, C, K = 7, 9, 5, 4
    lp, beams, gap = _case(T, N, C, K, 13, blank=C - 1)
    _check_against_spec(lp.cuda(), K, C - 1, beams, gap)
    assert all(C - 1 not in p for b in beams for p, _ in b)


def test_exact_ties_keep_candidate_order():
    """Two classes with identical columns: their prefixes score exactly alike, on the device too, and the order is the candidate
    order (owner rank, then slot).  Gaps of exactly 0 are the point here; every other gap is still >= 1e-7."""
    lp, beams, gap = _case(6, 8, 6, 6, 14, variant="ties")
    _, _, scores = _check_against_spec(lp.cuda(), 6, 0, beams, gap)
    assert (scores[:, 1:] == scores[:, :-1]).any()


def test_minus_inf_and_nan():
    lp, beams, gap = _case(6, 4, 4, 8, 15, variant="inf")
    tokens, lengths, scores = _check_against_spec(lp.cuda(), 8, 0, beams, gap)
    assert ((lengths >= 0).sum(dim=1) < 8).all() and (lengths[:, 0] >= 0).all()
    assert not torch.isnan(scores).any() and ((tokens == 3) | (tokens == -1)).all()


def test_exhaustive_scores_are_the_ctc_likelihoods():
    """C = 3, T = 5, K = 32 holds every labelling: the device scores are the CTC log-likelihoods within 1e-9."""
    lp, beams, gap = _case(5, 16, 3, 32, 16)
    tokens, lengths, scores = _check_against_spec(lp.cuda(), 32, 0, beams, gap)
    for n in range(16):
        for k in range(32):
            L = lengths[n, k].item()
            if L < 0:
                continue
            want = beam_spec.ctc_log_likelihood(lp[:, n], tokens[n, k, :L].tolist())
            assert abs(scores[n, k].item() - want) <= 1e-9, (n, k, scores[n, k].item(), want)
        assert scores[n, 0] == scores[n].max()


def test_refusals():
    from qea import ops
    from qea._lib import QeaError
    ok = torch.zeros(4, 2, 5, device="cuda")
    for bad in (lambda: ops.ctc_beam_decode(ok, 0), lambda: ops.ctc_beam_decode(ok, 33), lambda: ops.ctc_beam_decode(ok[:, :, :1], 2),
                lambda: ops.ctc_beam_decode(torch.zeros(513, 1, 5, device="cuda"), 2), lambda: ops.ctc_beam_decode(ok, 2, blank=5),
                lambda: ops.ctc_beam_decode(ok, 2, blank=-1), lambda: ops.ctc_beam_decode(ok.cpu(), 2)):
        with pytest.raises(QeaError):
            bad()
    torch.cuda.synchronize()


def test_pred_to_string_and_batch_cers_with_a_beam(monkeypatch):
    """CUDA tensors decode on the device, CPU tensors through the host loop: the same strings, n-best lists and scores; batch_cers
    scores rank 0; QEA_BEAM=host sends the CUDA tensor through the host loop."""
    from utils import batch_cers, compare_labels, pred_to_string
    T, N, C, K = 31, 17, 95, 8
    lp, beams, gap = _case(T, N, C, K, 4)
    assert gap >= MIN_GAP
    labels = H.synth_labels(N, 21, 1, 10)
    want = ["".join(H.I2C[i] for i in b[0][0]) for b in beams]
    on_dev = pred_to_string(lp.cuda(), labels, H.I2C, beam=K)
    assert on_dev == pred_to_string(lp, labels, H.I2C, beam=K) == want
    ld, sd = pred_to_string(lp.cuda(), labels, H.I2C, beam=K, nbest=3, return_scores=True)
    lh, sh = pred_to_string(lp, labels, H.I2C, beam=K, nbest=3, return_scores=True)
    assert ld == lh and all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for ra, rb in zip(sd, sh) for a, b in zip(ra, rb))
    cers = batch_cers(lp.cuda(), labels, H.C2I, beam=K)
    assert cers == [compare_labels([p], [l])[1] for p, l in zip(on_dev, labels)]
    assert batch_cers(lp.cuda(), labels, H.C2I) == [compare_labels([p], [l])[1] for p, l in zip(pred_to_string(lp.cuda(), labels, H.I2C), labels)]
    monkeypatch.setenv("QEA_BEAM", "host")
    assert pred_to_string(lp.cuda(), labels, H.I2C, beam=K) == want


def test_eval_crnn_with_a_beam(tmp_path):
    """EvalCRNN --beam 4 on a freshly initialised CRNN, the document flow and the strip flow: the three new keys over the same
    count of strips, the mean of the best entries' log-probabilities; without the flag the dict has today's keys only."""
    from eval_crnn import EvalCRNN, build_parser
    from models.model_crnn import CRNN
    from utils import pred_to_string
    torch.manual_seed(5)
    torch.save(CRNN(95, False).cuda().eval(), tmp_path / "crnn_ckpt")
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--synthetic_size", "8", "--ocr", "stub"]
    for flow in (["--dataset", "pos"], ["--dataset", "vgg", "--batch_size", "4"]):
        plain = EvalCRNN(build_parser().parse_args(argv + flow)).eval()
        assert sorted(plain) == ["count", "crnn_accuracy", "crnn_cer", "crnn_correct"]
        ev = EvalCRNN(build_parser().parse_args(argv + flow + ["--beam", "4"]))
        seen = []
        scores_of = ev._scores
        ev._scores = lambda images: seen.append(scores_of(images)) or seen[-1]
        res = ev.eval()
        assert sorted(set(res) - set(plain)) == ["beam", "crnn_mean_log_score", "greedy_disagreements"]
        assert res["beam"] == 4 and res["count"] == plain["count"] == sum(s.shape[1] for s in seen)
        assert 0 <= res["greedy_disagreements"] <= res["count"]
        logp = [v for s in seen for v in pred_to_string(s, [""] * s.shape[1], H.I2C, beam=4, return_scores=True)[1]]
        assert math.isfinite(res["crnn_mean_log_score"]) and res["crnn_mean_log_score"] == pytest.approx(sum(logp) / len(logp), rel=1e-12)
