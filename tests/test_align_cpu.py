"""CTC forced alignment on the host: qea/align.py held to the statement (tests/align_spec.py) bit for bit, the statement held to a brute
force over every path, the properties that follow from it (the greedy string aligns to the arg-max path; the score is at most the CTC
log-likelihood), ties and feasibility edges by hand, char_boxes on hand-worked boxes, read_pages(chars=True) and clean_cli.py
--read_chars on the host backend with the oracle CRNN, the flag rules and the ABI."""
import ctypes as C
import functools
import itertools
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import align_spec as spec

torch.set_num_threads(4)

NEG = -math.inf


def host(lp, labels, blank=0, L_max=None):
    """qea.align.ctc_align on [T,N,C] -> numpy arrays in the order of spec.align_batch"""
    from qea import align
    targets, offsets = spec.flatten(labels)
    L_max = max([len(l) for l in labels], default=0) if L_max is None else L_max
    return tuple(v.numpy() for v in align.ctc_align(lp, targets, offsets, L_max, blank))


def assert_same(got, want):
    """(score, path, first, last, char_score): integers exactly, floats bit for bit"""
    for i in (1, 2, 3):
        assert got[i].dtype == np.int32 and np.array_equal(got[i], want[i]), i
    for i in (0, 4):
        assert got[i].dtype == np.float64 and np.array_equal(spec.bits(got[i]), spec.bits(want[i])), i


# ------------------------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("T,seed", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6)])
def test_brute_force_over_every_path(T, seed):
    """C = 3: all 3^T paths, every label of up to 3 characters.  The brute force adds in ascending t as the recursion does, and fp64
    addition is monotone, so the best score is the recursion's bit for bit; the seeds give a unique maximum everywhere."""
    Cn, blank = 3, 0
    labels = [list(l) for n in range(4) for l in itertools.product((1, 2), repeat=n)]
    lp = spec.log_probs(T, len(labels), Cn, seed)
    got = host(lp, labels, blank)
    want = spec.align_batch(lp, labels, blank)
    assert_same(got, want)
    feasible = 0
    for n, label in enumerate(labels):
        best, paths = spec.brute_force(lp[:, n].tolist(), label, blank)
        assert spec.bits([best])[0] == spec.bits(got[0][n:n + 1])[0], (n, label)
        if best == NEG:
            assert not paths and (got[1][n] == -2).all()
            continue
        feasible += 1
        assert len(paths) == 1, (n, label)                     # unique for these seeds
        classes = [blank if k < 0 else label[k] for k in got[1][n].tolist()]
        assert classes == list(paths[0]) and spec.collapse(classes, blank) == label
    assert feasible >= min(len(labels), 2 * T - 1)


def test_the_greedy_string_aligns_to_the_arg_max_path():
    """rows with a unique arg-max: no path beats the per-step maxima, and the arg-max path spells the greedy string"""
    T, N, Cn = 12, 40, 6
    lp = spec.log_probs(T, N, Cn, 21)
    top = lp.argmax(2)                                          # [T,N]
    assert (lp.sort(2, descending=True).values[:, :, 0] > lp.sort(2, descending=True).values[:, :, 1]).all()
    labels = [spec.collapse(top[:, n].tolist(), 0) for n in range(N)]
    score, path, first, last, _ = host(lp, labels)
    o = 0
    for n, label in enumerate(labels):
        classes = [0 if k < 0 else label[k] for k in path[n].tolist()]
        assert classes == top[:, n].tolist()
        acc = float(lp[0, n, top[0, n]])
        for t in range(1, T):
            acc = acc + float(lp[t, n, top[t, n]])
        assert score[n] == acc
        for k in range(len(label)):
            steps = [t for t in range(T) if path[n][t] == k]
            assert (first[o + k], last[o + k]) == (steps[0], steps[-1])
        o += len(label)
    assert any(len(l) >= 5 for l in labels) and any(a == b for l in labels for a, b in zip(l, l[1:]))


def test_the_score_is_at_most_the_ctc_log_likelihood():
    """one alignment against the sum over all of them; exactly the infeasible samples give -inf where torch gives +inf"""
    T, N, Cn = 9, 60, 5
    lp = spec.log_probs(T, N, Cn, 22)
    labels = spec.random_labels(N, Cn, 0, 7, 23, repeats=0.4)
    score = host(lp, labels)[0]
    targets, offsets = spec.flatten(labels)
    lens = offsets[1:] - offsets[:-1]
    nll = F.ctc_loss(lp.double(), targets.long(), torch.full((N,), T), lens, reduction="none").numpy()
    infeasible = 0
    for n in range(N):
        if score[n] == NEG:
            assert nll[n] == math.inf
            infeasible += 1
        else:
            assert math.isfinite(nll[n]) and score[n] <= -nll[n] + 1e-9 * max(1.0, abs(score[n])), n
    assert 0 < infeasible < N // 2


def test_ties_follow_the_candidate_order():
    """uniform rows, L = 2, T = 5: every alignment scores the same.  t = 1: state 2 can only step (1), state 3 only skip (2); t = 2: state 4
    steps from 3; everything else stays, because stay comes first.  The end is a tie and S - 1 = 4 wins.  Walking back from state 4:
    stay, stay, step to 3 at t = 1, skip to 1 at t = 0."""
    c = math.log(0.25)
    lp = torch.full((5, 1, 4), c)
    c = float(lp[0, 0, 0])
    for label in ([1, 2], [3, 1]):
        for got in (host(lp, [label]), spec.align_batch(lp, [label])):
            assert got[1].tolist() == [[0, 1, -1, -1, -1]] and got[2].tolist() == [0, 1] and got[3].tolist() == [0, 1]
            assert got[0][0] == c + c + c + c + c and got[4].tolist() == [c, c]
    # a repeated character cannot skip: state 3 waits for the blank between
    for got in (host(lp, [[2, 2]]), spec.align_batch(lp, [[2, 2]])):
        assert got[1].tolist() == [[0, -1, 1, -1, -1]]


def test_feasibility_edges():
    lp = spec.log_probs(3, 1, 4, 24)
    for T, label, ok in ((2, [1, 1], False), (3, [1, 1], True), (1, [], True), (1, [2], True), (1, [2, 3], False), (3, [], True),
                         (3, [1, 2, 3], True), (3, [1, 2, 2], False), (3, [0], False), (3, [1, 0, 2], False), (3, [4], False), (3, [-1], False)):
        x = lp[:T]
        got, want = host(x, [label]), spec.align_batch(x, [label])
        assert_same(got, want)
        assert (got[0][0] > NEG) == ok, (T, label)
        if not ok:
            assert (got[1] == -2).all() and (got[2] == -1).all() and (got[3] == -1).all() and (got[4] == NEG).all()
    assert host(lp, [[1, 1]])[1].tolist() == [[0, -1, 1]]
    got = host(lp, [[]])                                       # L = 0: the all-blank path, added up in ascending t
    assert got[1].tolist() == [[-1, -1, -1]] and got[0][0] == (float(lp[0, 0, 0]) + float(lp[1, 0, 0])) + float(lp[2, 0, 0])
    # a label over L_max is infeasible, its neighbour is not touched
    got = host(lp.expand(3, 2, 4), [[1, 2], [3]], L_max=1)
    assert got[0][0] == NEG and got[0][1] > NEG and got[2].tolist()[:2] == [-1, -1] and got[2][2] >= 0


def test_nan_and_infinities_count_as_minus_inf():
    T, N, Cn = 6, 5, 4
    lp = spec.log_probs(T, N, Cn, 25).clone()
    lp[:, 0, 1] = float("nan")                                 # class 1 impossible: a label with it is infeasible
    lp[:, 1, 2] = float("inf")                                 # +inf is no certainty: impossible as well
    lp[:, 2, 3] = -float("inf")
    lp[2, 3, 0] = float("nan")                                 # one step cannot be blank
    lp[0, 4, 1] = float("inf")
    labels = [[1, 2], [2], [1, 3], [1, 2], [1]]
    got, want = host(lp, labels), spec.align_batch(lp, labels)
    assert_same(got, want)
    assert got[0][:3].tolist() == [NEG] * 3 and got[0][3] > NEG and got[1][3][2] >= 0 and not np.isnan(got[0]).any()
    assert got[0][4] > NEG and got[2][7] >= 1                  # the last sample's character cannot sit on step 0
    other = [[2, 3], [1, 3], [1, 2], [3], [2]]
    assert_same(host(lp, other), spec.align_batch(lp, other))
    assert (host(lp, other)[0][:3] > NEG).all()


@pytest.mark.parametrize("T,N,Cn,lo,hi,seed,blank", [(7, 50, 5, 0, 3, 31, 0), (31, 17, 95, 1, 12, 32, 0), (40, 4, 7, 25, 33, 33, 6), (3, 2, 256, 1, 1, 34, 0)])
def test_the_host_path_is_the_statement(T, N, Cn, lo, hi, seed, blank):
    lp = spec.log_probs(T, N, Cn, seed)
    labels = spec.random_labels(N, Cn, lo, hi, seed + 100, blank=blank)
    assert_same(host(lp, labels, blank), spec.align_batch(lp, labels, blank))


def test_limits_and_char_spans():
    from qea import align
    from qea._lib import QeaError
    from utils import char_spans
    for kw in (dict(T=0), dict(T=513), dict(C=1), dict(C=257), dict(blank=-1), dict(blank=5), dict(L_max=-1), dict(L_max=128), dict(N=-1)):
        with pytest.raises(QeaError):
            align.check_limits(**{**dict(T=4, C=5, blank=0, L_max=3, N=1), **kw})
    align.check_limits(512, 256, 255, 127, 0)
    lp = spec.log_probs(8, 3, 6, 35)
    c2i = {c: i for i, c in enumerate("-abcde")}
    texts = ["abc", "", "ee"]
    spans = char_spans(lp, texts, c2i)
    want = spec.align_batch(lp, [[1, 2, 3], [], [5, 5]])
    assert [s[0] for s in spans] == want[0].tolist()
    assert np.array_equal(np.concatenate([s[1] for s in spans]), want[2]) and np.array_equal(np.concatenate([s[2] for s in spans]), want[3])
    assert np.array_equal(spec.bits(np.concatenate([s[3] for s in spans])), spec.bits(want[4]))
    assert isinstance(spans[0][0], float) and spans[1][1].shape == (0,)
    again = char_spans(lp, [[1, 2, 3], [], [5, 5]], c2i)       # class indices instead of strings
    assert [a[0] for a in again] == [s[0] for s in spans]
    assert char_spans(lp, [[1, 77], [], [0]], c2i)[0][0] == NEG  # a class that is none: infeasible, not refused
    with pytest.raises(ValueError, match="sample 2"):
        char_spans(lp, ["a", "b", "x"], c2i)
    with pytest.raises(ValueError, match="sample 1"):
        char_spans(lp, ["a", "a" * 128, "b"], c2i)
    with pytest.raises(ValueError):
        char_spans(lp, ["a"], c2i)
    assert char_spans(lp[:, :0], [], c2i) == []


def test_abi():
    """the symbol is in the header and in the built library; the library refuses bad arguments before any launch; N = 0 launches nothing"""
    from qea import _lib
    protos = {n: a for n, _, a in _lib.header_prototypes()}
    L = _lib.lib()
    assert len(protos["qea_ctc_align"]) == 16 and hasattr(L, "qea_ctc_align") and L.qea_version() == 9
    p = C.c_void_p(256)

    def call(scores=p, ld_t=10, ld_n=5, targets=p, offsets=p, T=4, N=2, Cn=5, blank=0, L_max=3, score=p, path=p, first=p, last=p, cs=p):
        return L.qea_ctc_align(scores, ld_t, ld_n, targets, offsets, T, N, Cn, blank, L_max, score, path, first, last, cs, None)
    for kw in (dict(T=0), dict(T=513), dict(Cn=1), dict(Cn=257), dict(blank=-1), dict(blank=5), dict(L_max=-1), dict(L_max=128), dict(N=-1),
               dict(ld_t=-1), dict(ld_n=-1), dict(scores=None), dict(targets=None), dict(offsets=None), dict(score=None),
               dict(path=None), dict(first=None), dict(last=None), dict(cs=None)):
        assert call(**kw) < 0, kw
        assert b"qea_ctc_align" in L.qea_last_error(), kw
    assert call(N=0) == 0 and call(N=0, scores=None, path=None) == 0


# ------------------------------------------------------------------------------------------------------------------ character boxes
def check_boxes(first, last, x0, cw, ch, sw, OW):
    from qea.reading import char_boxes
    got = char_boxes(first, last, x0, cw, ch, sw, OW)
    assert len(got) == len(first)
    for a, b in got:
        assert isinstance(a, int) and isinstance(b, int) and x0 <= a < b <= x0 + cw
    assert all(p[0] <= q[0] for p, q in zip(got, got[1:]))
    return got


def test_char_boxes_by_hand():
    # ch <= 32: 40 columns centred in 128 start at strip column 44.  Steps 11..12 own strip columns [46, 54): box columns [2, 10)
    assert check_boxes([11, 13], [12, 13], 100, 40, 20, 40, 128) == [(102, 110), (110, 114)]
    # ch = 80: sw = ceil(32 * 200 / 80) = 80 strip columns of 2.5 page columns, from strip column 24.  Steps 6..8 own [26, 38): scaled
    # columns [2, 14), page columns [floor(5), ceil(35)) = [5, 35)
    assert check_boxes([6], [8], 10, 200, 80, 80, 128) == [(15, 45)]
    # a cut strip: 150 columns in 128, left = -11: step 0 owns strip [2, 6) = box [13, 17); step 30 owns [122, 126) = [133, 137)
    assert (128 - 150) // 2 == -11
    assert check_boxes([0, 30], [0, 30], 0, 150, 30, 150, 128) == [(13, 17), (133, 137)]
    # characters the alignment put into the white padding: 20 columns from strip column 54; steps 0..1 and step 30 lie outside
    assert check_boxes([0, 30], [1, 30], 7, 20, 32, 20, 128) == [(7, 8), (26, 27)]
    # a shrunk box whose last scaled column is partly covered: cw = 33, ch = 64: sw = 17, left = 23; steps 5..9 own [22, 42) -> scaled [0, 17)
    assert check_boxes([5], [9], 3, 33, 64, 17, 64) == [(3, 36)]
    from qea.reading import char_boxes
    for empty in (dict(cw=0), dict(ch=0), dict(sw=0)):
        with pytest.raises(ValueError):
            char_boxes([0], [0], **{**dict(x0=0, cw=5, ch=5, sw=5, OW=64), **empty})


def test_char_boxes_on_random_spans():
    g = np.random.default_rng(41)
    for _ in range(300):
        OW = int(g.choice([64, 128, 256, 512]))
        ch = int(g.integers(1, 120))
        cw = int(g.integers(1, 700))
        sw = cw if ch <= 32 else (32 * cw + ch - 1) // ch
        T = OW // 4 - 1
        cuts = np.sort(g.choice(np.arange(T + 1), size=min(T + 1, 2 * int(g.integers(1, 8))), replace=False))
        first, last = cuts[0::2].tolist(), (cuts[1::2] - 1).tolist()
        first, last = zip(*[(f, max(f, l)) for f, l in zip(first, last)])
        check_boxes(first, last, int(g.integers(0, 50)), cw, ch, sw, OW)


# ------------------------------------------------------------------------------------------------------------------ the page pipeline
def test_read_pages_with_chars_on_the_host_backend():
    """a recording forward: the characters of every box are char_boxes of the statement's spans on exactly the recorded scores, and
    without chars the result is what it was"""
    import test_word_strips_cpu as W
    from qea.reading import _geometry, box_table, char_boxes, read_pages, strip_plan
    pages = W.tensors("u8")[:2]
    per_page = [torch.tensor([(0, 0, 199, 69), (10, 5, 49, 5), (3, 2, 89, 32), (0, 0, 199, 31), (7, 1, 149, 33)], dtype=torch.int32),
                torch.tensor([(0, 0, 66, 44), (5, 7, 59, 38)], dtype=torch.int32)]
    table = box_table(per_page)
    plan = strip_plan(table, [70, 45], [200, 67], (64, 128), strip_pixels=128)
    index_to_char = {i: chr(96 + i) for i in range(6)}
    seen = []

    class Model(torch.nn.Module):
        pass

    def forward(x):
        g = torch.Generator().manual_seed(len(seen) % len(plan.passes))
        s = torch.log_softmax(torch.randn(x.shape[3] // 4 - 1, x.shape[0], 6, generator=g) * 3, 2)
        seen.append(s)
        return s
    kw = dict(buckets=(64, 128), strip_pixels=128, forward=forward)
    texts, cut = read_pages(Model().eval(), pages, per_page, index_to_char, **kw)
    texts2, chars, cut2 = read_pages(Model().eval(), pages, per_page, index_to_char, chars=True, **kw)
    btexts, bscores, bchars, _ = read_pages(Model().eval(), pages, per_page, index_to_char, chars=True, beam=3, nbest=2, **kw)
    assert (texts2, cut2) == (texts, cut) and [len(c) for c in chars] == [5, 2] == [len(c) for c in bchars]
    assert read_pages(Model().eval(), pages, per_page, index_to_char, beam=3, nbest=2, **kw)[:2] == (btexts, bscores)
    x0, _, cw, ch, _ = _geometry(table, [70, 45], [200, 67])
    flat_t, flat_c = texts[0] + texts[1], chars[0] + chars[1]
    flat_b = [t[0] for t in btexts[0] + btexts[1]]
    for (OW, idx), s in zip(plan.passes, seen):
        for j, i in enumerate(idx.tolist()):
            for text, got in ((flat_t[i], flat_c[i]), (flat_b[i], (bchars[0] + bchars[1])[i])):
                label = [ord(c) - 96 for c in text]
                r = spec.align(s[:, j].tolist(), label)
                if not text:
                    assert got == []
                    continue
                assert r["score"] > NEG and "".join(c for c, _, _, _ in got) == text
                cols = char_boxes(r["first"], r["last"], x0[i], cw[i], ch[i], plan.sw[i], OW)
                assert [(a, b) for _, a, b, _ in got] == cols
                assert [v for _, _, _, v in got] == [cs / (l - f + 1) for cs, f, l in zip(r["char_score"], r["first"], r["last"])]
                for _, a, b, _ in got:                          # inside the row's own box
                    assert table[i, 1] <= a < b <= table[i, 3]
    assert sum(len(c) for c in flat_c) >= 10
    with pytest.raises(ValueError, match="one"):
        read_pages(Model().eval(), pages, per_page, {i: "a" for i in range(6)}, chars=True, **kw)


def test_clean_cli_read_chars_on_the_host_backend(tmp_path):
    import clean_cli
    import test_word_strips_cpu as W
    from datasets.patch_dataset import PatchDataset
    backend, OracleCRNN = W.host_backend()
    torch.save(OracleCRNN(95, seed=4).eval(), tmp_path / "crnn")
    W.word_scans(tmp_path / "in")
    read = ["--read", str(tmp_path / "crnn"), "--read_buckets", "64", "128"]
    plain = clean_cli.CleanPages(W.cli_args(tmp_path, "plain", *read), backend=backend).run()
    chars = clean_cli.CleanPages(W.cli_args(tmp_path, "chars", "--read_chars", *read), backend=backend).run()
    beam = clean_cli.CleanPages(W.cli_args(tmp_path, "beam", "--read_chars", "--read_beam", "3", *read), backend=backend).run()
    seen = 0
    for p, c, b in zip(plain, chars, beam):
        with open(p, "rb") as x, open(c, "rb") as y:
            assert x.read() == y.read()
        rows, with_chars, with_beam = (json.load(open(path[:-4] + ".json")) for path in (p, c, b))
        assert [{k: v for k, v in r.items() if k != "chars"} for r in with_chars] == rows
        for r in with_chars + with_beam:
            assert "".join(e["c"] for e in r["chars"]) == r["label"]
            for e in r["chars"]:
                assert sorted(e) == ["c", "conf", "x_max", "x_min"] and isinstance(e["x_min"], int) and isinstance(e["x_max"], int)
                assert r["x_min"] <= e["x_min"] < e["x_max"] <= r["x_max"] and e["conf"] <= 0.0
                seen += 1
            assert all(u["x_min"] <= v["x_min"] for u, v in zip(r["chars"], r["chars"][1:]))
        assert all("score" in r for r in with_beam)
    assert seen >= 4
    ds = PatchDataset(str(tmp_path / "chars"), pad=True)
    assert len(ds) == 3 and len(PatchDataset(str(tmp_path / "plain"), pad=True)) == 3
    ds[0]


def test_flag_rules(tmp_path):
    import clean_cli
    import test_word_strips_cpu as W
    from qea.cli_flags import build_parser
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"])
    assert a.read_chars is False
    assert clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--read", "x", "--read_chars"]).read_chars is True
    acts = {s: act for act in build_parser("n", "")._actions for s in act.option_strings}
    assert acts["--read_chars"].help.startswith("[new]")
    for tag in "pacerv":
        assert "--read_chars" not in {s for act in build_parser(tag, "")._actions for s in act.option_strings}
    backend, OracleCRNN = W.host_backend()
    torch.save(OracleCRNN(95).eval(), tmp_path / "crnn")
    (tmp_path / "in").mkdir()
    lead = ["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--method", "otsu"]
    with pytest.raises(ValueError, match="--read_chars"):
        clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--read_chars"]), backend=backend)
    ok = clean_cli.CleanPages(clean_cli.build_parser().parse_args(lead + ["--read_chars", "--read", str(tmp_path / "crnn")]), backend=backend)
    assert ok.read_chars and ok.boxes
