"""The device search inside a deterministic automaton (csrc/ctc_beam.hip, qea.ops.ctc_beam_decode_dfa) against the fp64 specification
of tests/beam_lexicon_spec.py, with the method of tests/test_beam_lm_gpu.py: the WHOLE beam must match, tokens, lengths, states and
rank order exactly, scores within 1e-9 * max(1, |s|).

Every case asserts that the smallest non-zero gap between two scores whose order decided something is at least 1e-7 for its input;
the seeds were checked on the CPU so that this holds, and no case is skipped.  Log-probs: beam_spec.log_probs(T, N, C, seed); tries:
beam_lexicon_spec.trie of beam_lexicon_spec.random_lexicon(C, blank, n_words, max_len, seed) unless a case says otherwise."""
import ctypes
import functools
import math

import pytest
import torch

import beam_checks
import beam_lexicon_spec as spec
import beam_spec
import helpers as H

pytestmark = pytest.mark.gpu

MIN_GAP = beam_checks.MIN_GAP


def _words(C, blank, n_words, max_len, seed, variant):
    if variant == "synth":                                             # 500 words over the workload's character set
        return [tuple(H.C2I[ch] for ch in w) for w in H.synth_labels(n_words, seed, 1, max_len)]
    words = spec.random_lexicon(C, blank, n_words, max_len, seed)
    if variant == "long":                                              # and one word as long as T: no class twice in a row
        classes = [c for c in range(C) if c != blank]
        words.append(tuple(classes[q % len(classes)] for q in range(max_len)))
    return words


@functools.lru_cache(maxsize=None)
def _case(T, N, C, K, seed, n_words, max_len, blank=0, variant=""):
    """(log-probs [T,N,C] fp32 on the CPU, the automaton as lists, the specification's beams, its smallest non-zero gap)."""
    lp = beam_spec.log_probs(T, N, C, seed, blank=blank)
    aut = spec.trie(_words(C, blank, n_words, max_len, seed, variant))
    if variant == "malformed":
        aut = spec.with_malformed_edges(aut, C)
    beams, gap = spec.decode_batch(lp, K, aut, blank)
    return lp, aut, beams, gap


def _lexicon(aut, C, blank=0):
    from qea.lexicon import Lexicon
    return Lexicon.from_automaton(*aut, vocabulary=[chr(0x100 + c) for c in range(C)], blank=blank)


def _compare(got, beams, K, T, gap):
    return beam_checks.check_against_spec(got, spec.as_arrays(beams, K, T), gap, (("score", torch.float64), ("state", torch.int32)))


def _check_against_spec(dev_scores, K, aut, blank, beams, gap):
    from qea import ops
    T, N, C = dev_scores.shape
    return _compare(ops.ctc_beam_decode_dfa(dev_scores, K, _lexicon(aut, C, blank).device("cuda"), blank), beams, K, T, gap)


# (T, N, C, K, seed, n_words, max_len, variant): smallest everything; more samples than CUs; the workload's T and C (R = 4) with 500
# words of helpers.synth_labels; R = 12; long T; fewer live prefixes
# than K (the -1 / -inf padding); the limit of C (R = 32, 255 edges out of the start state); the limit of T with a word as long
# as T; a trie with no edge out of state 0.
SHAPES = [(1, 3, 2, 1, 1, 2, 2, ""), (7, 300, 5, 4, 2, 20, 6, ""), (31, 17, 95, 8, 4, 500, 10, "synth"), (31, 5, 95, 32, 5, 2000, 8, ""),
          (127, 2, 95, 16, 6, 3000, 40, ""), (5, 33, 3, 32, 7, 6, 4, ""), (3, 2, 256, 32, 8, 5000, 3, ""), (512, 1, 4, 32, 9, 40, 512, "long"),
          (7, 9, 5, 4, 10, 0, 1, "")]


@pytest.mark.parametrize("T,N,C,K,seed,n_words,max_len,variant", SHAPES)
def test_constrained_beam_equals_the_spec(T, N, C, K, seed, n_words, max_len, variant):
    lp, aut, beams, gap = _case(T, N, C, K, seed, n_words, max_len, 0, variant)
    _, lengths, _, states = _check_against_spec(lp.cuda(), K, aut, 0, beams, gap)
    if (T, C, K) == (5, 3, 32):
        assert (lengths == -1).any()
    if variant == "long":
        assert max(aut[0][s + 1] - aut[0][s] for s in range(len(aut[3]))) <= 3 and len(aut[3]) > T
    if n_words == 0:
        assert aut[0] == [0, 0] and (lengths[:, 0] == 0).all() and (lengths[:, 1:] == -1).all() and (states[:, 0] == 0).all()
    elif K > 1:                                                        # K = 1, T = 1 keeps the empty prefix alone
        assert (states > 0).any()


@pytest.mark.parametrize("T,N,C,K,seed", [(31, 17, 95, 8, 4), (3, 2, 256, 32, 8)])
def test_accept_all_is_the_plain_kernel_bit_for_bit(T, N, C, K, seed):
    from qea import ops
    d = beam_spec.log_probs(T, N, C, seed).cuda()
    pt, pl, ps = ops.ctc_beam_decode(d, K)
    tokens, lengths, scores, states = ops.ctc_beam_decode_dfa(d, K, _lexicon(spec.accept_all(C), C).device("cuda"))
    assert torch.equal(tokens, pt) and torch.equal(lengths, pl)
    assert torch.equal(scores.view(torch.int64), ps.view(torch.int64))
    assert torch.equal(states, torch.where(pl >= 0, 0, -1).to(torch.int32))


def test_padded_strides():
    """A [T,N,C] view of a larger buffer: ld_t and ld_n both padded, the padding filled with values that would win every step."""
    T, N, C, K = 7, 9, 5, 4
    lp, aut, beams, gap = _case(T, N, C, K, 12, 20, 6)
    big = torch.full((T, N + 3, C + 5), 50.0, device="cuda")
    view = big[:, 2:2 + N, :C]
    view.copy_(lp)
    assert view.stride() == ((N + 3) * (C + 5), C + 5, 1) and not view.is_contiguous()
    _check_against_spec(view, K, aut, 0, beams, gap)
    # a [N,T,C] buffer read as [T,N,C]: ld_t < ld_n
    _check_against_spec(lp.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), K, aut, 0, beams, gap)


def test_blank_is_the_last_class():
    T, N, C, K = 7, 9, 5, 4
    lp, aut, beams, gap = _case(T, N, C, K, 13, 20, 6, blank=C - 1)
    assert 0 in aut[1] and C - 1 not in aut[1]
    _check_against_spec(lp.cuda(), K, aut, C - 1, beams, gap)
    assert all(C - 1 not in p for b in beams for p, _, _ in b) and any(0 in p for b in beams for p, _, _ in b)


def test_exhaustive_paths_likelihoods_and_the_best_word():
    """C = 3, T = 5, K = 32 holds every live path: every returned prefix is a path of the automaton, its score the CTC log-likelihood
    within 1e-9, and the best accepted rank is the arg-max of that likelihood over all words of the lexicon."""
    T, N, C, K = 5, 16, 3, 32
    lp, aut, beams, gap = _case(T, N, C, K, 16, 12, 4)
    words = sorted(set(spec.random_lexicon(C, 0, 12, 4, 16)))
    tokens, lengths, scores, states = _check_against_spec(lp.cuda(), K, aut, 0, beams, gap)
    for n in range(N):
        live = int((lengths[n] >= 0).sum())
        accepted = []
        for k in range(live):
            label = tuple(tokens[n, k, :lengths[n, k].item()].tolist())
            path, final = spec.accepts(aut, label, C)
            assert path and final == bool(aut[3][states[n, k].item()])
            assert abs(scores[n, k].item() - beam_spec.ctc_log_likelihood(lp[:, n], label)) <= 1e-9, (n, k)
            if final:
                accepted.append(label)
        like = {w: beam_spec.ctc_log_likelihood(lp[:, n], w) for w in words}
        assert accepted and accepted[0] == max(like, key=like.get)


def _dfa_by_pointers(d, K, first, label, child, S, E, out, blank=0):
    from qea import _lib
    T, N, C = d.shape
    ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
    return _lib.lib().qea_ctc_beam_decode_dfa(d.data_ptr(), d.stride(0), d.stride(1), T, N, C, blank, K, ptr(first), ptr(label), ptr(child), S, E,
                                              *[ptr(t) for t in out], None)


def _outputs(N, K, T):
    return [torch.empty(N, K, T, dtype=torch.int32, device="cuda"), torch.empty(N, K, dtype=torch.int32, device="cuda"),
            torch.empty(N, K, dtype=torch.float64, device="cuda"), torch.empty(N, K, dtype=torch.int32, device="cuda")]


def test_malformed_tables_through_ctypes():
    """Tables with an edge labelled with the blank, one with a label >= C and one with a child >= S, handed to the library directly
    (the binding would not take them): the result is the specification's on the automaton without those edges.  The arrays are
    views into larger allocations, so a read a missing guard would let through still lands in allocated memory."""
    T, N, C, K = 7, 20, 5, 8
    lp, bad, beams, gap = _case(T, N, C, K, 41, 10, 5, variant="malformed")
    clean = spec.drop_malformed(bad, C)
    assert len(clean[1]) == len(bad[1]) - 3
    want, want_gap = spec.decode_batch(lp, K, clean)
    assert beams == want and gap == want_gap
    assert want != spec.decode_batch(lp, K, spec.trie(spec.random_lexicon(C, 0, 10, 5, 41)))[0]       # the cut-off subtree is missed
    S, E = len(bad[3]), len(bad[1])
    views = []
    for t in spec.tensors(bad):
        big = torch.full((t.numel() + 128,), 3, dtype=torch.int32, device="cuda")
        big[64:64 + t.numel()].copy_(t)
        views.append(big[64:64 + t.numel()])
    out = _outputs(N, K, T)
    assert _dfa_by_pointers(lp.cuda(), K, *views, S, E, out) == 0
    _compare(out, beams, K, T, gap)


def test_refusals():
    from qea import ops
    from qea._lib import QeaError
    ok = torch.zeros(4, 2, 5, device="cuda")
    lex = _lexicon(spec.accept_all(5), 5)
    aut = lex.device("cuda")
    ops.ctc_beam_decode_dfa(ok, 2, aut)
    for bad in (lambda: ops.ctc_beam_decode_dfa(ok.cpu(), 2, aut), lambda: ops.ctc_beam_decode_dfa(ok, 2, lex.device("cpu")),
                lambda: ops.ctc_beam_decode_dfa(ok, 2, (aut.first, aut.label, aut.child)), lambda: ops.ctc_beam_decode_dfa(ok, 2, lex),
                lambda: ops.ctc_beam_decode_dfa(ok, 0, aut), lambda: ops.ctc_beam_decode_dfa(ok, 33, aut),
                lambda: ops.ctc_beam_decode_dfa(ok, 2, aut, blank=5), lambda: ops.ctc_beam_decode_dfa(ok, 2, aut, blank=1),
                lambda: ops.ctc_beam_decode_dfa(ok.double(), 2, aut), lambda: ops.ctc_beam_decode_dfa(ok[:, :, ::2], 2, aut),
                lambda: ops.ctc_beam_decode_dfa(torch.zeros(4, 2, 6, device="cuda"), 2, aut),
                lambda: ops.ctc_beam_decode_dfa(torch.zeros(513, 1, 5, device="cuda"), 2, aut)):
        with pytest.raises(QeaError):
            bad()
    # lm= together with lexicon=
    from utils import batch_cers, pred_to_string
    for bad in (lambda: pred_to_string(ok, ["", ""], {}, beam=2, lexicon=lex, lm=object()), lambda: pred_to_string(ok, ["", ""], {}, lexicon=lex),
                lambda: batch_cers(ok, ["", ""], {}, beam=2, lexicon=lex, lm=object())):
        with pytest.raises(QeaError):
            bad()
    # the library's own checks, behind the binding's
    out = _outputs(2, 2, 4)
    f, l, c = aut.first, aut.label, aut.child
    assert _dfa_by_pointers(ok, 2, f, l, c, 1, 4, out) == 0
    for args in ((None, l, c, 1, 4), (f, None, c, 1, 4), (f, l, None, 1, 4), (f, l, c, 0, 4), (f, l, c, -1, 4), (f, l, c, 1, -1), (f, l, c, 1, 1 << 26)):
        assert _dfa_by_pointers(ok, 2, *args, out) < 0, args
    for k in range(4):
        assert _dfa_by_pointers(ok, 2, f, l, c, 1, 4, out[:k] + [None] + out[k + 1:]) < 0
    assert _dfa_by_pointers(ok, 0, f, l, c, 1, 4, out) < 0 and _dfa_by_pointers(ok, 33, f, l, c, 1, 4, out) < 0
    assert _dfa_by_pointers(ok, 2, f, l, c, 1, 4, out, blank=5) < 0 and _dfa_by_pointers(ok, 2, f, l, c, 1, 4, out, blank=-1) < 0
    from qea import _lib
    L = _lib.lib()
    ptrs = [t.data_ptr() for t in out]
    tables = (f.data_ptr(), l.data_ptr(), c.data_ptr(), 1, 4)
    for T, C in ((0, 5), (513, 5), (4, 1), (4, 257)):
        assert L.qea_ctc_beam_decode_dfa(ok.data_ptr(), 10, 5, T, 2, C, 0, 2, *tables, *ptrs, None) < 0
    assert L.qea_ctc_beam_decode_dfa(None, 10, 5, 4, 2, 5, 0, 2, *tables, *ptrs, None) < 0
    assert L.qea_ctc_beam_decode_dfa(ok.data_ptr(), 10, 5, 4, 0, 5, 0, 2, *tables, *ptrs, None) < 0
    torch.cuda.synchronize()


def _word_lexicon():
    from qea.lexicon import Lexicon
    return Lexicon.from_words(H.synth_labels(3000, 7, 2, 4), H.C2I)                  # no word of one character


def test_pred_to_string_and_batch_cers_with_a_lexicon(monkeypatch):
    """CUDA tensors decode on the device, CPU tensors through the host loop: the same strings, n-best lists and scores; the lexicon
    changes some reading relative to the plain beam; a strip without an accepted entry reads as the plain rank 0; batch_cers scores
    what pred_to_string reads; QEA_BEAM=host sends the CUDA tensor through the host loop."""
    from utils import batch_cers, compare_labels, lexicon_best, pred_to_string
    T, N, C, K = 31, 17, 95, 8
    lp = beam_spec.log_probs(T, N, C, 4)
    for n in (0, 5, 16):                                               # three nearly blank strips: "" and single characters, no word
        lp[:, n, 0] += 12.0
        lp[:, n] = torch.log_softmax(lp[:, n], dim=1)
    lex = _word_lexicon()
    aut = (lex.first.tolist(), lex.label.tolist(), lex.child.tolist(), lex.final.tolist())
    beams, gap = spec.decode_batch(lp, K, aut)
    plain_beams, plain_gap = beam_spec.decode_batch(lp, K)
    assert gap >= MIN_GAP and plain_gap >= MIN_GAP, f"gaps {gap:.3e} {plain_gap:.3e}"
    labels = H.synth_labels(N, 21, 1, 10)
    text = lambda p: "".join(H.I2C[i] for i in p)                      # noqa: E731
    accepted = [[p for p, _, st in b if lex.final[st]] for b in beams]
    want = [text(a[0]) if a else text(pb[0][0]) for a, pb in zip(accepted, plain_beams)]
    misses = [not a for a in accepted]
    assert [n for n, m in enumerate(misses) if m] == [0, 5, 16]
    plain = pred_to_string(lp.cuda(), labels, H.I2C, beam=K)
    on_dev = pred_to_string(lp.cuda(), labels, H.I2C, beam=K, lexicon=lex)
    assert on_dev == pred_to_string(lp, labels, H.I2C, beam=K, lexicon=lex) == want
    assert on_dev != plain and all(a == b for a, b, m in zip(on_dev, plain, misses) if m)
    assert all(lex.accepts_string(a, H.C2I) for a, m in zip(on_dev, misses) if not m)
    assert lexicon_best(lp.cuda(), K, lex)[3].tolist() == misses
    ld, sd = pred_to_string(lp.cuda(), labels, H.I2C, beam=K, lexicon=lex, nbest=3, return_scores=True)
    lh, sh = pred_to_string(lp, labels, H.I2C, beam=K, lexicon=lex, nbest=3, return_scores=True)
    same = lambda a, b: a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b))     # noqa: E731
    assert ld == lh and all(same(a, b) for ra, rb in zip(sd, sh) for a, b in zip(ra, rb))
    assert [l[0] for l in ld] == want
    cers = batch_cers(lp.cuda(), labels, H.C2I, beam=K, lexicon=lex)
    assert cers == [compare_labels([p], [l])[1] for p, l in zip(on_dev, labels)]
    monkeypatch.setenv("QEA_BEAM", "host")
    assert pred_to_string(lp.cuda(), labels, H.I2C, beam=K, lexicon=lex) == want


def test_eval_crnn_with_a_lexicon(tmp_path):
    """EvalCRNN --beam 4 --lexicon on a freshly initialised CRNN, the document flow and the strip flow: the four new keys over the
    same count of strips."""
    from eval_crnn import EvalCRNN, build_parser
    from models.model_crnn import CRNN
    torch.manual_seed(5)
    torch.save(CRNN(95, False).cuda().eval(), tmp_path / "crnn_ckpt")
    path = str(tmp_path / "words.npz")
    lex = _word_lexicon()
    lex.save(path)
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--synthetic_size", "8", "--ocr", "stub", "--beam", "4"]
    for flow in (["--dataset", "pos"], ["--dataset", "vgg", "--batch_size", "4"]):
        beam = EvalCRNN(build_parser().parse_args(argv + flow)).eval()
        res = EvalCRNN(build_parser().parse_args(argv + flow + ["--lexicon", path])).eval()
        assert sorted(set(res) - set(beam)) == ["lexicon_disagreements", "lexicon_misses", "lexicon_oov_labels", "lexicon_words"]
        assert set(beam) <= set(res) and res["count"] == beam["count"] and res["beam"] == 4 and res["lexicon_words"] == lex.num_words
        assert 0 <= res["lexicon_misses"] <= res["count"] and 0 <= res["lexicon_disagreements"] <= res["count"]
        assert 0 <= res["lexicon_oov_labels"] <= res["count"] and math.isfinite(res["crnn_mean_log_score"])
