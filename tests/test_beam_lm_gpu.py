"""The device search with a character n-gram prior fused in (csrc/ctc_beam.hip, qea.ops.ctc_beam_decode_lm) against the fp64
specification of tests/beam_lm_spec.py, with the method of tests/test_beam_decode_gpu.py: the WHOLE beam must match, tokens, lengths
and rank order exactly, ctc and total within 1e-9 * max(1, |s|).

Every case asserts that the smallest non-zero gap between two ranking scores whose order decided something is at least 1e-7 for its
input; the seeds were checked on the CPU so that this holds, and no case is skipped.  Log-probs: beam_spec.log_probs(T, N, C, seed);
tables: randn(C ** m, C) - 1 in fp64 with generator seed 1000 + seed (beam_lm_spec.table)."""
import functools
import math

import pytest
import torch

import beam_checks
import beam_lm_spec
import beam_spec
import helpers as H

pytestmark = pytest.mark.gpu

MIN_GAP = beam_checks.MIN_GAP


@functools.lru_cache(maxsize=None)
def _case(T, N, C, K, m, seed, blank=0, variant=""):
    """(log-probs [T,N,C] fp32 and table [C**m, C] fp64 on the CPU, the specification's beams, its smallest non-zero gap)."""
    if variant == "forbidden":
        lp, W = beam_lm_spec.forbidden_case(T, N, C, K, seed)
    else:
        lp, W = beam_spec.log_probs(T, N, C, seed, blank=blank), beam_lm_spec.table(C, m, seed)
    beams, gap = beam_lm_spec.decode_batch(lp, K, W, m, blank)
    return lp, W, beams, gap


def _check_against_spec(dev_scores, K, W, m, blank, beams, gap):
    from qea import ops
    return beam_checks.check_against_spec(ops.ctc_beam_decode_lm(dev_scores, K, W.cuda(), m, blank), beam_lm_spec.as_arrays(beams, K, dev_scores.shape[0]),
                                          gap, (("ctc", torch.float64), ("total", torch.float64)))


# (T, N, C, K, m, seed): smallest everything; more samples than CUs and the trigram wrap of ctx; the workload's T and C (R = 4);
# R = 12 with a bigram and a unigram; long T; fewer live prefixes than K (the -1 / -inf padding); the table-size limit (R = 32); the
# limit of C; the limit of T.
SHAPES = [(1, 3, 2, 1, 1, 1), (7, 300, 5, 4, 2, 2), (31, 17, 95, 8, 2, 4), (31, 5, 95, 32, 1, 5), (31, 5, 95, 32, 0, 5), (127, 2, 95, 16, 2, 6),
          (5, 33, 3, 32, 2, 7), (3, 2, 128, 32, 2, 8), (3, 2, 256, 32, 1, 8), (512, 1, 4, 32, 2, 9)]


@pytest.mark.parametrize("T,N,C,K,m,seed", SHAPES)
def test_fused_beam_equals_the_spec(T, N, C, K, m, seed):
    lp, W, beams, gap = _case(T, N, C, K, m, seed)
    _, lengths, _, _ = _check_against_spec(lp.cuda(), K, W, m, 0, beams, gap)
    if (T, C, K) == (5, 3, 32):
        assert (lengths == -1).any()


@pytest.mark.parametrize("m", [0, 1, 2])
def test_zero_table_is_the_plain_kernel_bit_for_bit(m):
    from qea import ops
    T, N, C, K = 31, 17, 95, 8
    d = beam_spec.log_probs(T, N, C, 4).cuda()
    pt, pl, ps = ops.ctc_beam_decode(d, K)
    tokens, lengths, ctc, total = ops.ctc_beam_decode_lm(d, K, torch.zeros(C ** m, C, dtype=torch.float64, device="cuda"), m)
    assert torch.equal(tokens, pt) and torch.equal(lengths, pl)
    assert torch.equal(ctc.view(torch.int64), ps.view(torch.int64)) and torch.equal(total.view(torch.int64), ps.view(torch.int64))


def test_padded_strides():
    """A [T,N,C] view of a larger buffer: ld_t and ld_n both padded, the padding filled with values that would win every step."""
    T, N, C, K, m = 7, 9, 5, 4, 2
    lp, W, beams, gap = _case(T, N, C, K, m, 12)
    big = torch.full((T, N + 3, C + 5), 50.0, device="cuda")
    view = big[:, 2:2 + N, :C]
    view.copy_(lp)
    assert view.stride() == ((N + 3) * (C + 5), C + 5, 1) and not view.is_contiguous()
    _check_against_spec(view, K, W, m, 0, beams, gap)
    # a [N,T,C] buffer read as [T,N,C]: ld_t < ld_n
    _check_against_spec(lp.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), K, W, m, 0, beams, gap)


@pytest.mark.parametrize("m", [1, 2])
def test_blank_is_the_last_class(m):
    """BOS is the blank index: with blank = C - 1 the start context is not row 0 of the table."""
    T, N, C, K = 7, 9, 5, 4
    lp, W, beams, gap = _case(T, N, C, K, m, 13, blank=C - 1)
    assert beam_lm_spec.start_context(C, m, C - 1) == C ** m - 1
    _check_against_spec(lp.cuda(), K, W, m, C - 1, beams, gap)
    assert all(C - 1 not in p for b in beams for p, _, _ in b)


def test_hard_constraints():
    """A pair at -inf and a pair at NaN in a bigram table are absent from every returned prefix."""
    T, N, C, K = 7, 20, 5, 8
    lp, W, beams, gap = _case(T, N, C, K, 1, 21, variant="forbidden")
    tokens, lengths, _, _ = _check_against_spec(lp.cuda(), K, W, 1, 0, beams, gap)
    for n in range(N):
        for k in range(K):
            assert not beam_lm_spec.has_forbidden_pair(tokens[n, k, :max(lengths[n, k].item(), 0)].tolist())


def test_exhaustive_scores_are_the_likelihood_and_the_table_sum():
    """C = 3, T = 5, K = 32 holds every live labelling: the device's ctc is the CTC log-likelihood and total - ctc the table sum along
    the labelling, within 1e-9; total does not increase with rank."""
    T, N, C, K, m = 5, 16, 3, 32, 2
    lp, W, beams, gap = _case(T, N, C, K, m, 16)
    tokens, lengths, ctc, total = _check_against_spec(lp.cuda(), K, W, m, 0, beams, gap)
    for n in range(N):
        live = int((lengths[n] >= 0).sum())
        for k in range(live):
            label = tokens[n, k, :lengths[n, k].item()].tolist()
            assert abs(ctc[n, k].item() - beam_spec.ctc_log_likelihood(lp[:, n], label)) <= 1e-9, (n, k)
            assert abs((total[n, k] - ctc[n, k]).item() - beam_lm_spec.table_sum(W, label, C, m)) <= 1e-9, (n, k)
        assert (total[n, 1:live] <= total[n, :live - 1]).all()


def test_refusals():
    from qea import ops
    from qea._lib import QeaError
    ok = torch.zeros(4, 2, 5, device="cuda")
    tab = torch.zeros(25, 5, dtype=torch.float64, device="cuda")
    ops.ctc_beam_decode_lm(ok, 2, tab, 2)
    wide = torch.zeros(2, 1, 129, device="cuda")
    for bad in (lambda: ops.ctc_beam_decode_lm(ok, 2, torch.zeros(125, 5, dtype=torch.float64, device="cuda"), 3),
                lambda: ops.ctc_beam_decode_lm(ok, 2, tab, -1),
                lambda: ops.ctc_beam_decode_lm(wide, 2, torch.zeros(1, 129, dtype=torch.float64, device="cuda"), 2),   # 129^3 > 2^21
                lambda: ops.ctc_beam_decode_lm(ok, 2, tab.cpu(), 2), lambda: ops.ctc_beam_decode_lm(ok, 2, tab.float(), 2),
                lambda: ops.ctc_beam_decode_lm(ok, 2, tab, 1), lambda: ops.ctc_beam_decode_lm(ok, 2, tab.t(), 2),
                lambda: ops.ctc_beam_decode_lm(ok, 2, torch.zeros(50, 5, dtype=torch.float64, device="cuda")[::2], 2),
                lambda: ops.ctc_beam_decode_lm(ok, 0, tab, 2), lambda: ops.ctc_beam_decode_lm(ok, 33, tab, 2),
                lambda: ops.ctc_beam_decode_lm(ok, 2, tab, 2, blank=5), lambda: ops.ctc_beam_decode_lm(ok.cpu(), 2, tab, 2)):
        with pytest.raises(QeaError):
            bad()
    # the library's own checks, behind the binding's
    from qea import _lib
    L = _lib.lib()
    out = [torch.empty(2, 2, 4, dtype=torch.int32, device="cuda"), torch.empty(2, 2, dtype=torch.int32, device="cuda"),
           torch.empty(2, 2, dtype=torch.float64, device="cuda"), torch.empty(2, 2, dtype=torch.float64, device="cuda")]
    ptrs = [t.data_ptr() for t in out]
    assert L.qea_ctc_beam_decode_lm(ok.data_ptr(), 10, 5, 4, 2, 5, 0, 2, tab.data_ptr(), 3, *ptrs, None) < 0
    assert L.qea_ctc_beam_decode_lm(wide.data_ptr(), 129, 129, 2, 1, 129, 0, 2, tab.data_ptr(), 2, *ptrs, None) < 0
    assert L.qea_ctc_beam_decode_lm(ok.data_ptr(), 10, 5, 4, 2, 5, 0, 2, None, 2, *ptrs, None) < 0
    torch.cuda.synchronize()


def _char_lm():
    from qea.lm import CharLM
    return CharLM.from_labels(H.synth_labels(200, 7), H.C2I, order=3, add_k=0.1)


def test_pred_to_string_and_batch_cers_with_a_model(monkeypatch):
    """CUDA tensors decode on the device, CPU tensors through the host loop: the same strings, n-best lists and total scores;
    batch_cers scores rank 0 of the fused search; QEA_BEAM=host sends the CUDA tensor through the host loop."""
    from utils import batch_cers, compare_labels, pred_to_string
    T, N, C, K = 31, 17, 95, 8
    lp = beam_spec.log_probs(T, N, C, 4)
    lm = _char_lm()
    kw = dict(beam=K, lm=lm, lm_weight=0.6, lm_bonus=0.4)
    beams, gap = beam_lm_spec.decode_batch(lp, K, lm.fused(0.6, 0.4, "cpu"), 2)
    assert gap >= MIN_GAP, f"gap {gap:.3e}"
    labels = H.synth_labels(N, 21, 1, 10)
    want = ["".join(H.I2C[i] for i in b[0][0]) for b in beams]
    on_dev = pred_to_string(lp.cuda(), labels, H.I2C, **kw)
    assert on_dev == pred_to_string(lp, labels, H.I2C, **kw) == want
    assert want != pred_to_string(lp.cuda(), labels, H.I2C, beam=K)                  # the model changes some reading
    ld, sd = pred_to_string(lp.cuda(), labels, H.I2C, nbest=3, return_scores=True, **kw)
    lh, sh = pred_to_string(lp, labels, H.I2C, nbest=3, return_scores=True, **kw)
    assert ld == lh and all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for ra, rb in zip(sd, sh) for a, b in zip(ra, rb))
    assert all(abs(r[0] - b[0][2]) <= 1e-9 * max(1.0, abs(r[0])) for r, b in zip(sd, beams))      # the totals
    cers = batch_cers(lp.cuda(), labels, H.C2I, **kw)
    assert cers == [compare_labels([p], [l])[1] for p, l in zip(on_dev, labels)]
    monkeypatch.setenv("QEA_BEAM", "host")
    assert pred_to_string(lp.cuda(), labels, H.I2C, **kw) == want


def test_eval_crnn_with_a_model(tmp_path):
    """EvalCRNN --beam 4 --lm on a freshly initialised CRNN, the document flow and the strip flow: the five new keys over the same
    count of strips."""
    from eval_crnn import EvalCRNN, build_parser
    from models.model_crnn import CRNN
    torch.manual_seed(5)
    torch.save(CRNN(95, False).cuda().eval(), tmp_path / "crnn_ckpt")
    path = str(tmp_path / "chars.npz")
    _char_lm().save(path)
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--synthetic_size", "8", "--ocr", "stub", "--beam", "4"]
    for flow in (["--dataset", "pos"], ["--dataset", "vgg", "--batch_size", "4"]):
        beam = EvalCRNN(build_parser().parse_args(argv + flow)).eval()
        res = EvalCRNN(build_parser().parse_args(argv + flow + ["--lm", path, "--lm_weight", "0.5", "--lm_bonus", "0.25"])).eval()
        assert sorted(set(res) - set(beam)) == ["crnn_mean_total_score", "lm_bonus", "lm_disagreements", "lm_order", "lm_weight"]
        assert set(beam) <= set(res) and res["count"] == beam["count"] and res["beam"] == 4
        assert (res["lm_order"], res["lm_weight"], res["lm_bonus"]) == (3, 0.5, 0.25)
        assert 0 <= res["lm_disagreements"] <= res["count"]
        assert math.isfinite(res["crnn_mean_log_score"]) and math.isfinite(res["crnn_mean_total_score"])
