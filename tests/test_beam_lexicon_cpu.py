"""The automaton-constrained CTC prefix beam search without a GPU: the literal specification (tests/beam_lexicon_spec.py) against the
plain search and the CTC likelihood, the host loop (qea/beam.py) against the specification, qea.lexicon.Lexicon (build, validation,
save / load, vocabulary check, every refusal of from_automaton), the pred_to_string / batch_cers / eval_crnn / lexicon_cli interface
and the fallback on a strip without an accepted entry."""
import math

import numpy as np
import pytest
import torch

import beam_lexicon_spec as spec
import beam_spec
import helpers as H
from beam_checks import same_scores as _same_scores


def _host(lp, K, aut, blank=0):
    from qea import beam as host
    return host.ctc_beam_decode(lp, K, blank, automaton=aut)


def _vocab(C, blank=0):
    """class index -> a character: the blank is '-', class c the code point 0x100 + c."""
    return ["-" if c == blank else chr(0x100 + c) for c in range(C)]


def _lexicon(C, blank, words):
    from qea.lexicon import Lexicon
    v = _vocab(C, blank)
    return Lexicon.from_words(["".join(v[c] for c in w) for w in words], {ch: i for i, ch in enumerate(v)}, blank=blank)


# ---- the specification
@pytest.mark.parametrize("blank", [0, 4])
def test_accept_all_is_the_plain_search(blank):
    """The one-state automaton that loops on every class: the specification and the host loop return beam_spec.decode's beams, scores
    bit-equal, every state 0."""
    T, N, C, K = 7, 6, 5, 4
    lp = beam_spec.log_probs(T, N, C, seed=2, blank=blank)
    plain, _ = beam_spec.decode_batch(lp, K, blank)
    aut = spec.accept_all(C, blank)
    got, _ = spec.decode_batch(lp, K, aut, blank)
    assert [[(p, s) for p, s, _ in b] for b in got] == plain and all(st == 0 for b in got for _, _, st in b)
    from qea import beam as host
    tokens, lengths, scores, states = _host(lp, K, aut, blank)
    pt, pl, ps = host.ctc_beam_decode(lp, K, blank)
    assert torch.equal(tokens, pt) and torch.equal(lengths, pl) and torch.equal(scores, ps)
    assert torch.equal(states, torch.where(lengths >= 0, 0, -1).to(torch.int32))


def test_exhaustive_paths_scores_and_the_best_word():
    """C = 3, T = 5, K = 32 holds every live path of the trie: each returned prefix is a path, its score the CTC log-likelihood within
    1e-9, and the best accepted rank is the arg-max of that likelihood over all words of the lexicon."""
    T, N, C, K = 5, 8, 3, 32
    lp = beam_spec.log_probs(T, N, C, seed=16)
    words = sorted(set(spec.random_lexicon(C, 0, 12, 4, seed=3)))
    aut = spec.trie(words)
    for n in range(N):
        beam, _ = spec.decode(lp[:, n].tolist(), K, aut)
        assert len({p for p, _, _ in beam}) == len(beam)
        for p, s, st in beam:
            path, _ = spec.accepts(aut, p, C)
            assert path and abs(s - beam_spec.ctc_log_likelihood(lp[:, n], p)) <= 1e-9
        accepted = [(p, s) for p, s, st in beam if aut[3][st]]
        like = {w: beam_spec.ctc_log_likelihood(lp[:, n], w) for w in words if len(w) <= T}
        best = max(like, key=like.get)
        assert accepted and accepted[0][0] == best and abs(accepted[0][1] - like[best]) <= 1e-9


@pytest.mark.parametrize("T,C,K,blank,n_words,max_len", [(7, 5, 4, 0, 12, 5), (7, 5, 4, 4, 12, 5), (6, 4, 8, 3, 6, 3), (31, 95, 8, 0, 300, 10),
                                                         (5, 3, 32, 0, 5, 4), (9, 6, 6, 0, 1, 9), (4, 5, 3, 0, 0, 1)])
def test_host_loop_equals_the_spec(T, C, K, blank, n_words, max_len):
    """qea/beam.py with an automaton returns the specification's beams: same prefixes and states in the same order, scores within
    1e-12 * max(1, |s|); the automaton as a Lexicon and as a plain tuple."""
    N = 5
    lp = beam_spec.log_probs(T, N, C, seed=300 + T, blank=blank)
    words = spec.random_lexicon(C, blank, n_words, max_len, seed=T)
    aut = spec.trie(words)
    want, _ = spec.decode_batch(lp, K, aut, blank)
    wt, wl, ws, wst = spec.as_arrays(want, K, T)
    for automaton in (_lexicon(C, blank, words), aut):
        tokens, lengths, scores, states = _host(lp, K, automaton, blank)
        assert tokens.shape == (N, K, T) and tokens.dtype == torch.int32 and lengths.shape == states.shape == (N, K)
        assert lengths.dtype == states.dtype == torch.int32 and scores.shape == (N, K) and scores.dtype == torch.float64
        assert tokens.tolist() == wt and lengths.tolist() == wl and states.tolist() == wst
        assert _same_scores(scores.tolist(), ws)
    assert all(blank not in p for b in want for p, _, _ in b)
    if n_words == 0:                                                   # no edge out of state 0: only the empty prefix lives
        assert all([p for p, _, _ in b] == [()] for b in want)


def test_malformed_edges_are_absent():
    """An edge labelled with the blank, one with a label >= C and one with a child >= S: the host loop on the raw tables equals the
    specification on the automaton without them, and the specification itself skips them."""
    T, N, C, K = 7, 6, 5, 6
    lp = beam_spec.log_probs(T, N, C, seed=41)
    bad = spec.with_malformed_edges(spec.trie(spec.random_lexicon(C, 0, 10, 5, seed=41)), C)
    clean = spec.drop_malformed(bad, C)
    assert len(clean[1]) == len(bad[1]) - 3
    want, _ = spec.decode_batch(lp, K, clean)
    assert spec.decode_batch(lp, K, bad)[0] == want
    tokens, lengths, scores, states = _host(lp, K, bad)
    wt, wl, ws, wst = spec.as_arrays(want, K, T)
    assert tokens.tolist() == wt and lengths.tolist() == wl and states.tolist() == wst and _same_scores(scores.tolist(), ws)


# ---- qea.lexicon.Lexicon
_VOCAB = {"-": 0, "a": 1, "b": 2, "c": 3}


def test_lexicon_from_words():
    from qea._lib import QeaError
    from qea.lexicon import Lexicon
    lex = Lexicon.from_words(["cab", "ab", "", "abc", "ab", "b", ""], _VOCAB)
    # breadth first, children by ascending class: 0 -a-> 1, -b-> 2, -c-> 3; 1 -b-> 4; 3 -a-> 5; 4 -c-> 6; 5 -b-> 7
    assert lex.first.tolist() == [0, 3, 4, 4, 5, 6, 7, 7, 7] and lex.label.tolist() == [1, 2, 3, 2, 1, 3, 2] and lex.child.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert lex.final.tolist() == [0, 0, 1, 0, 1, 0, 1, 1] and lex.final.dtype == np.uint8 and lex.first.dtype == lex.label.dtype == lex.child.dtype == np.int32
    assert (lex.num_words, lex.num_empty, lex.num_states, lex.num_edges, lex.num_classes, lex.blank) == (4, 2, 8, 7, 4, 0)
    assert (lex.first.tolist(), lex.label.tolist(), lex.child.tolist(), lex.final.tolist()) == tuple(
        spec.trie([(3, 1, 2), (1, 2), (), (1, 2, 3), (1, 2), (2,)]))
    for word, ok in (("ab", True), ("abc", True), ("cab", True), ("b", True), ("a", False), ("ca", False), ("", False), ("abcc", False), ("bb", False)):
        assert lex.accepts([_VOCAB[ch] for ch in word]) is ok and lex.accepts_string(word, _VOCAB) is ok
    assert not lex.accepts_string("abz", _VOCAB) and not lex.accepts([0])
    none = Lexicon.from_words(["", ""], _VOCAB)                        # nothing but the start state
    assert (none.num_states, none.num_edges, none.num_words, none.num_empty) == (1, 0, 0, 2) and none.first.tolist() == [0, 0]
    last = Lexicon.from_words(["ab"], {"a": 0, "b": 1, "-": 2}, blank=2)
    assert last.label.tolist() == [0, 1] and last.blank == 2
    for bad in (lambda: Lexicon.from_words(["abd"], _VOCAB), lambda: Lexicon.from_words(["a-"], _VOCAB),
                lambda: Lexicon.from_words(["ab"], {"-": 0, "a": 1, "b": 1}), lambda: Lexicon.from_words(["ab"], _VOCAB, blank=4)):
        with pytest.raises(QeaError):
            bad()
    big = _lexicon(95, 0, spec.random_lexicon(95, 0, 500, 10, seed=1))
    want = spec.trie(spec.random_lexicon(95, 0, 500, 10, seed=1))
    assert (big.first.tolist(), big.label.tolist(), big.child.tolist(), big.final.tolist()) == tuple(want)


def test_every_refusal_of_from_automaton():
    """A digits-and-one-point pattern is accepted; each statement of the specification, broken alone, raises."""
    from qea._lib import QeaError
    from qea.lexicon import Lexicon
    vocab = ["-", "0", "1", "."]
    # state 0: digits loop, the point leads to state 1; state 1: digits loop.  Both accept.
    ok = dict(first=[0, 3, 5], label=[1, 2, 3, 1, 2], child=[0, 0, 1, 1, 1], final=[1, 1], vocabulary=vocab, blank=0)
    lex = Lexicon.from_automaton(**ok)
    assert lex.accepts([1, 2, 3, 1]) and lex.accepts([3]) and not lex.accepts([1, 3, 3]) and lex.num_words is None
    assert (lex.num_states, lex.num_edges) == (2, 5)
    Lexicon.from_automaton([0, 0], [], [], [0], vocab)                 # one state, no edge
    broken = dict(
        first_starts_at_0=dict(first=[1, 3, 5]), first_decreases=dict(first=[0, 5, 3, 5], final=[1, 1, 1]), first_ends_at_E=dict(first=[0, 3, 4]),
        first_too_short=dict(first=[0]), first_empty=dict(first=[]), first_two_dimensional=dict(first=[[0, 3, 5]]),
        first_of_floats=dict(first=[0.0, 3.0, 5.0]), label_is_the_blank=dict(label=[0, 2, 3, 1, 2]), label_above_C=dict(label=[1, 2, 4, 1, 2]),
        label_negative=dict(label=[-1, 2, 3, 1, 2]), labels_equal=dict(label=[1, 1, 3, 1, 2]), labels_descend=dict(label=[2, 1, 3, 1, 2]),
        child_above_S=dict(child=[0, 0, 2, 1, 1]), child_negative=dict(child=[0, -1, 1, 1, 1]), child_shorter=dict(child=[0, 0, 1, 1]),
        final_shorter=dict(final=[1]), final_not_a_mark=dict(final=[1, 2]), label_beyond_32_bits=dict(label=[1, 2, 2 ** 31, 1, 2]),
        blank_outside=dict(blank=4), one_class=dict(vocabulary=["-"], blank=0), too_many_classes=dict(vocabulary=[str(i) for i in range(257)]))
    for name, change in broken.items():
        with pytest.raises(QeaError):
            Lexicon.from_automaton(**{**ok, **change})
            pytest.fail(f"{name} was accepted")
    # ascending is asked within a state only: the first label of state 1 may be below the last of state 0
    Lexicon.from_automaton([0, 1, 2], [3, 1], [1, 0], [0, 1], vocab)


def test_save_load_and_device(tmp_path):
    from qea._lib import QeaError
    from qea.lexicon import DeviceAutomaton, Lexicon
    lex = Lexicon.from_words(["cab", "ab", "", "abc"], _VOCAB)
    path = str(tmp_path / "words.lex")
    lex.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["blank", "child", "final", "first", "label", "num_empty", "num_words", "vocabulary"]
    back = Lexicon.load(path, _VOCAB)
    assert all((getattr(back, k) == getattr(lex, k)).all() for k in ("first", "label", "child", "final"))
    assert (back.num_words, back.num_empty, back.blank, back.vocabulary) == (3, 1, 0, ["-", "a", "b", "c"])
    assert Lexicon.load(path).vocabulary == lex.vocabulary
    with pytest.raises(QeaError):
        Lexicon.load(path, {"-": 0, "a": 1, "c": 2, "b": 3})
    with pytest.raises(QeaError):
        Lexicon.load(path, {"-": 0, "a": 1, "b": 2})
    pattern = Lexicon.from_automaton([0, 1], [1], [0], [1], ["-", "a"])
    pattern.save(path)
    assert Lexicon.load(path).num_words is None
    dev = lex.device("cpu")
    assert isinstance(dev, DeviceAutomaton) and lex.device("cpu") is dev and lex.device(torch.device("cpu")) is dev
    assert dev.first.dtype == dev.label.dtype == dev.child.dtype == torch.int32 and dev.final.dtype == torch.uint8
    assert dev.first.tolist() == lex.first.tolist() and dev.label.tolist() == lex.label.tolist() and dev.final.tolist() == lex.final.tolist()
    assert (dev.num_states, dev.num_edges, dev.num_classes, dev.blank) == (lex.num_states, lex.num_edges, 4, 0)
    empty = Lexicon.from_words([], _VOCAB).device("cpu")              # no edge: one unused element, never a null pointer
    assert empty.num_edges == 0 and empty.label.numel() == 1 and empty.child.numel() == 1


# ---- interface
def test_a_hand_made_lexicon_and_the_fallback_on_a_miss():
    """T = 1, classes {blank, a, b} with probabilities (0.2, 0.41, 0.39): the plain beam reads "a"; the lexicon {b} reads "b"; the
    lexicon {ab} cannot be spelt in one step, so no entry is accepted and the strip reads as the plain beam's "a"."""
    from qea._lib import QeaError
    from qea.lexicon import Lexicon
    from utils import batch_cers, beam_decode_lexicon, lexicon_best, pred_to_string
    i2c, c2i = {0: "-", 1: "a", 2: "b"}, {"-": 0, "a": 1, "b": 2}
    lp = torch.log(torch.tensor([[[0.2, 0.41, 0.39]]]))
    only_b, only_ab = Lexicon.from_words(["b"], c2i), Lexicon.from_words(["ab"], c2i)
    assert pred_to_string(lp, [""], i2c, beam=4) == ["a"]
    strings, scores = pred_to_string(lp, [""], i2c, beam=4, lexicon=only_b, nbest=2, return_scores=True)
    assert strings == [["b", ""]] and scores[0][0] == pytest.approx(math.log(0.39), abs=1e-6) and scores[0][1] == -math.inf
    tokens, lengths, logp, accepted = beam_decode_lexicon(lp, 4, only_ab)
    assert lengths.tolist() == [[1, 0, -1, -1]] and tokens[0, 0, 0] == 1 and accepted.dtype == torch.bool and not accepted.any()
    assert lexicon_best(lp, 4, only_ab)[3].tolist() == [True] and lexicon_best(lp, 4, only_b)[3].tolist() == [False]
    strings, scores = pred_to_string(lp, [""], i2c, beam=4, lexicon=only_ab, nbest=3, return_scores=True)
    assert (strings, scores) == pred_to_string(lp, [""], i2c, beam=4, nbest=3, return_scores=True) and strings == [["a", "b", ""]]
    assert pred_to_string(lp, [""], i2c, beam=4, lexicon=only_ab) == ["a"]
    two = torch.cat([lp, lp], dim=1)
    assert pred_to_string(two, ["", ""], i2c, beam=4, lexicon=only_b) == ["b", "b"]
    for bad in (lambda: pred_to_string(lp, [""], i2c, lexicon=only_b), lambda: pred_to_string(lp, [""], i2c, beam=4, lexicon=only_b, lm=object()),
                lambda: batch_cers(lp, [""], c2i, lexicon=only_b), lambda: batch_cers(lp, [""], c2i, beam=4, lexicon=only_b, lm=object()),
                lambda: pred_to_string(lp, [""], i2c, beam=4, lexicon=Lexicon.from_words(["b"], {"-": 0, "a": 1, "b": 2, "c": 3})),
                lambda: beam_decode_lexicon(lp, 4, only_b, blank=1)):
        with pytest.raises(QeaError):
            bad()


def test_pred_to_string_reads_the_best_accepted_entry():
    """On the workload's C: the strings are the specification's best-ranked accepted entries (the plain rank 0 on a miss), the
    scores their CTC log-probabilities, and the n-best lists continue in rank order."""
    from utils import pred_to_string
    T, N, C, K = 12, 6, 95, 8
    lp = beam_spec.log_probs(T, N, C, seed=31)
    words = H.synth_labels(300, 5, 1, 4)
    from qea.lexicon import Lexicon
    lex = Lexicon.from_words(words, H.C2I)
    assert (lex.first.tolist(), lex.label.tolist(), lex.child.tolist(), lex.final.tolist()) == tuple(spec.trie([tuple(H.C2I[c] for c in w) for w in words]))
    beams, _ = spec.decode_batch(lp, K, (lex.first.tolist(), lex.label.tolist(), lex.child.tolist(), lex.final.tolist()))
    plain, _ = beam_spec.decode_batch(lp, K)
    want, want_scores, misses = [], [], 0
    for b, pb in zip(beams, plain):
        acc = [(p, s) for p, s, st in b if lex.final[st]]
        misses += not acc
        acc = (acc or pb)[:3]
        want.append(["".join(H.I2C[i] for i in p) for p, _ in acc] + [""] * (3 - len(acc)))
        want_scores.append([s for _, s in acc] + [-math.inf] * (3 - len(acc)))
    lists, scores = pred_to_string(lp, [""] * N, H.I2C, beam=K, lexicon=lex, nbest=3, return_scores=True)
    assert lists == want and _same_scores(scores, want_scores)
    assert pred_to_string(lp, [""] * N, H.I2C, beam=K, lexicon=lex) == [l[0] for l in want]
    assert all(lex.accepts_string(l[0], H.C2I) for l, b in zip(want, beams) if any(lex.final[st] for _, _, st in b))


def test_the_flag_is_on_eval_crnn_only():
    from qea.cli_flags import build_parser
    ap = build_parser("e", "")
    act = {a.option_strings[0]: a for a in ap._actions if a.option_strings}
    assert act["--lexicon"].help.startswith("[new]") and act["--lexicon"].default is None
    assert ap.parse_args(["--beam", "4", "--lexicon", "x.npz"]).lexicon == "x.npz"
    for tag in "cvpanr":
        ns = vars(build_parser(tag, "").parse_args(["--cers_tess_path", "x"] if tag == "r" else
                                                   ["--in_dir", "a", "--out_dir", "b"] if tag == "n" else []))
        assert "lexicon" not in ns


def test_lexicon_cli_and_eval_crnn(tmp_path, capsys):
    """lexicon_cli.py writes a loadable file from synthetic labels and from a word file; EvalCRNN --beam 4 --lexicon on the oracle CRNN
    (CPU tensors: the host loop) adds exactly four keys to --beam 4 alone over the same count; --lexicon without --beam or with --lm
    is refused."""
    import lexicon_cli
    from datasets.synthetic import SyntheticTextAreas
    from eval_crnn import EvalCRNN, build_parser
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.lexicon import Lexicon
    from qea.trainer_core import Backend
    from utils import lexicon_best, pred_to_string
    words = tmp_path / "words.txt"
    words.write_text("total\n\n  cash \ntotal\n12.50\n")
    path = str(tmp_path / "words.npz")
    built = lexicon_cli.main(["--words", str(words), "--out", path])
    out = capsys.readouterr().out
    assert (built.num_words, built.num_empty) == (3, 1) and f"3 words (1 empty skipped), {built.num_states} states, {built.num_edges} edges" in out
    assert Lexicon.load(path, H.C2I).accepts_string("cash", H.C2I) and not built.accepts_string("cas", H.C2I)
    built = lexicon_cli.main(["--dataset", "vgg", "--synthetic_size", "40", "--out", path])
    lex = Lexicon.load(path, H.C2I)
    labels = list(SyntheticTextAreas(40, seed=1).labels)
    assert lex.num_words == len(set(labels)) == built.num_words and all(lex.accepts_string(l, H.C2I) for l in labels)

    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    model = OracleCRNN(95, False, seed=3).eval()
    torch.save(model, tmp_path / "crnn_ckpt")
    va = SyntheticTextAreas(4, seed=2)
    argv = ["--crnn_path", str(tmp_path), "--crnn_model_name", "crnn_ckpt", "--dataset", "vgg", "--batch_size", "2", "--ocr", "stub"]
    beam = EvalCRNN(build_parser().parse_args(argv + ["--beam", "4"]), backend=backend, dataset=va).eval()
    res = EvalCRNN(build_parser().parse_args(argv + ["--beam", "4", "--lexicon", path]), backend=backend, dataset=va).eval()
    assert sorted(set(res) - set(beam)) == ["lexicon_disagreements", "lexicon_misses", "lexicon_oov_labels", "lexicon_words"]
    assert set(beam) <= set(res) and res["count"] == beam["count"] == 4 and res["beam"] == 4 and res["lexicon_words"] == lex.num_words
    with torch.no_grad():                                     # the loader's batches of two
        lp = torch.cat([model(torch.stack([va[i][0] for i in (0, 1)])), model(torch.stack([va[i][0] for i in (2, 3)]))], dim=1)
    gt = [va[i][1] for i in range(4)]
    strings, logp = pred_to_string(lp, gt, H.I2C, beam=4, lexicon=lex, return_scores=True)
    plain = pred_to_string(lp, gt, H.I2C, beam=4)
    assert res["lexicon_misses"] == int(lexicon_best(lp, 4, lex)[3].sum()) and 0 <= res["lexicon_misses"] <= 4
    assert res["lexicon_disagreements"] == sum(a != b for a, b in zip(strings, plain))
    assert res["lexicon_oov_labels"] == sum(not lex.accepts_string(l, H.C2I) for l in gt)
    assert res["crnn_mean_log_score"] == pytest.approx(sum(logp) / 4, rel=1e-9)
    assert res["crnn_correct"] == sum(a == b for a, b in zip(strings, gt))
    for bad in (["--lexicon", path], ["--beam", "4", "--lexicon", path, "--lm", path]):
        with pytest.raises(ValueError):
            EvalCRNN(build_parser().parse_args(argv + bad), backend=backend, dataset=va)


def test_refusals_of_the_host_loop():
    from qea import beam as host
    from qea._lib import QeaError
    lp = torch.zeros(4, 2, 5)
    aut = spec.accept_all(5)
    host.ctc_beam_decode(lp, 2, 0, automaton=aut)
    for bad in (lambda: host.ctc_beam_decode(lp, 2, 0, torch.zeros(1, 5, dtype=torch.float64), 0, automaton=aut),      # with a table
                lambda: host.ctc_beam_decode(lp, 33, 0, automaton=aut), lambda: host.ctc_beam_decode(lp, 2, 5, automaton=aut)):
        with pytest.raises(QeaError):
            bad()
