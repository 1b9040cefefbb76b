"""CTC forced alignment on the MI355X (csrc/ctc_align.hip, qea.ops.ctc_align) against the statement tests/align_spec.py: path, first and
last exactly, score and char_score BIT FOR BIT (compared as int64; every -inf is one pattern).  The recursion is fp64 adds and
comparisons in a fixed order, so there is no tolerance and no gap condition.  The kernel has one form (a second one for short labels
was measured and deleted: DESIGN.md "Forced alignment"), so every case runs once."""
import functools
import math

import numpy as np
import pytest
import torch

import align_spec as spec

pytestmark = pytest.mark.gpu

NEG = -math.inf


def device(lp_dev, labels, blank=0, L_max=None):
    from qea import ops
    targets, offsets = spec.flatten(labels)
    L_max = max([len(l) for l in labels], default=0) if L_max is None else L_max
    out = ops.ctc_align(lp_dev, targets.cuda(), offsets.cuda(), L_max, blank)
    assert [o.dtype for o in out] == [torch.float64, torch.int32, torch.int32, torch.int32, torch.float64] and all(o.is_cuda for o in out)
    return tuple(o.cpu().numpy() for o in out)


def assert_same(got, want, what=""):
    for i in (1, 2, 3):
        assert got[i].shape == want[i].shape and np.array_equal(got[i], want[i]), (what, i)
    for i in (0, 4):
        assert got[i].shape == want[i].shape and np.array_equal(spec.bits(got[i]), spec.bits(want[i])), (what, i)


def run(lp_dev, labels, want, blank=0, L_max=None):
    got = device(lp_dev, labels, blank, L_max)
    assert_same(got, want)
    return got


def mixed_labels(N, C, seed):
    """L 0..3 with many repeats; every seventh label holds the blank or a class that is none, and every eleventh is five equal
    characters, which need nine steps"""
    labels = spec.random_labels(N, C, 0, 3, seed, repeats=0.5)
    for n in range(0, N, 11):
        labels[n] = [1, 1, 1, 1, 1]
    for n in range(0, N, 7):
        labels[n] = [[1, 0, 2], [C], [2, -1]][n % 3]
    return labels


@functools.lru_cache(maxsize=None)
def case(name):
    """(log-probs [T,N,C] fp32 on the CPU, labels, blank, the statement's arrays); computed once"""
    blank = 0
    if name == "tiny":
        lp, labels = spec.log_probs(1, 3, 2, 1), [[], [1], []]
    elif name == "many":
        lp, labels = spec.log_probs(7, 300, 5, 2), mixed_labels(300, 5, 102)
    elif name == "words":
        lp, labels = spec.log_probs(31, 17, 95, 3), spec.random_labels(17, 95, 1, 12, 103)
    elif name in ("seam31", "seam32"):                          # S = 63 is the last size of a one-wave workgroup, S = 65 the first of two
        L = int(name[4:])
        g = np.random.default_rng(104)
        lp, labels = spec.log_probs(31, 6, 95, 4), [g.permutation(np.arange(1, 95))[:L].tolist() for _ in range(6)]      # no class twice
        labels[1][5] = labels[1][4]                             # one repeat: 31 characters no longer fit 31 steps
    elif name in ("long31", "long32"):                          # the same seam where both sides are feasible
        L = int(name[4:])
        lp, labels = spec.log_probs(127, 3, 95, 5), spec.random_labels(3, 95, L, L, 105)
    elif name == "two_waves":
        lp, labels = spec.log_probs(127, 2, 95, 6), [spec.random_labels(1, 95, 63, 63, 106, repeats=0.2)[0], spec.random_labels(1, 95, 40, 40, 107)[0]]
    elif name == "limits":                                      # T = 512, L = 127: S = 255
        lp, labels = spec.log_probs(512, 1, 4, 7), spec.random_labels(1, 4, 127, 127, 108)
    elif name == "wide":
        lp, labels = spec.log_probs(3, 2, 256, 8), [[255], [17]]
    elif name == "blank_last":
        blank = 4
        lp, labels = spec.log_probs(7, 9, 5, 9), spec.random_labels(9, 5, 0, 4, 109, blank=4)
    elif name == "ties":
        lp, labels = torch.full((5, 4, 4), math.log(0.25)), [[1, 2], [2, 2], [], [3, 1, 2]]
    elif name == "inf":
        lp = spec.log_probs(6, 5, 4, 10).clone()
        lp[:, 0, 1], lp[:, 1, 2], lp[:, 2, 3], lp[2, 3, 0], lp[0, 4, 1] = float("nan"), float("inf"), -float("inf"), float("nan"), float("inf")
        labels = [[1, 2], [1, 3], [1, 3], [1, 2], [1]]
    elif name == "bad_class":
        lp, labels = spec.log_probs(7, 6, 5, 11), [[1, 2], [3, 7, 1], [2], [1, -3], [4, 0, 1], [2 ** 30, 1]]
    else:
        raise KeyError(name)
    return lp, labels, blank, spec.align_batch(lp, labels, blank)


SHORT = ["tiny", "many", "words", "seam31", "long31", "wide", "blank_last", "ties", "inf", "bad_class"]


@pytest.mark.parametrize("name", SHORT)
def test_short_labels(name):
    lp, labels, blank, want = case(name)
    got = run(lp.cuda(), labels, want, blank)
    score = got[0]
    if name == "many":
        assert (score[::7] == NEG).all() and (score > NEG).sum() > 200 and any(a == b for l in labels for a, b in zip(l, l[1:]))
    if name == "seam31":
        assert max(len(l) for l in labels) == 31 and score[1] == NEG and (np.delete(score, 1) > NEG).all()
        assert got[1][0].tolist() == list(range(31))            # 31 different characters in 31 steps: one step each
    if name == "ties":                                          # the order of the candidates decides: tests/test_align_cpu.py works it out
        assert got[1].tolist() == [[0, 1, -1, -1, -1], [0, -1, 1, -1, -1], [-1] * 5, [0, 1, 2, -1, -1]]
    if name == "inf":
        assert score[0] == NEG and score[1] > NEG and score[2] == NEG and score[3] > NEG and not np.isnan(score).any()
        assert got[1][3][2] >= 0 and got[2][8] >= 1
    if name == "bad_class":                                     # the bad samples are infeasible, their neighbours are the statement's
        assert [s > NEG for s in score.tolist()] == [True, False, True, False, False, False]
        assert (got[1][[1, 3, 4, 5]] == -2).all() and got[1][2].max() == 0


@pytest.mark.parametrize("name", ["seam32", "long32", "two_waves", "limits"])
def test_long_labels(name):
    lp, labels, blank, want = case(name)
    got = device(lp.cuda(), labels, blank)
    assert_same(got, want)
    if name == "seam32":
        assert min(len(l) for l in labels) == 32 and (got[0] == NEG).all() and (got[1] == -2).all()
    else:
        assert (got[0] > NEG).all()
    if name == "limits":
        assert len(labels[0]) == 127 and got[1].shape == (1, 512) and got[1].max() == 126


def test_l_max_is_a_bound_not_a_length():
    """L_max above every label changes nothing; a label above L_max is infeasible and its neighbours are untouched"""
    lp, labels, blank, want = case("words")
    assert_same(device(lp.cuda(), labels, blank, L_max=127), want)
    short = spec.align_batch(lp, labels, blank, L_max=5)
    assert (short[0] == NEG).any() and (short[0] > NEG).any()
    run(lp.cuda(), labels, short, blank, L_max=5)


def test_padded_strides():
    """A [T,N,C] view of a larger buffer: ld_t and ld_n both padded, the padding filled with values that would win every step; and a
    [N,T,C] buffer read as [T,N,C]: ld_t < ld_n"""
    T, N, Cn = 7, 9, 5
    lp = spec.log_probs(T, N, Cn, 12)
    labels = spec.random_labels(N, Cn, 0, 3, 112)
    want = spec.align_batch(lp, labels)
    big = torch.full((T, N + 3, Cn + 5), 50.0, device="cuda")
    view = big[:, 2:2 + N, :Cn]
    view.copy_(lp)
    assert view.stride() == ((N + 3) * (Cn + 5), Cn + 5, 1) and not view.is_contiguous()
    run(view, labels, want)
    run(lp.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), labels, want)


def test_refusals_and_the_empty_batch():
    from qea import ops
    from qea._lib import QeaError
    ok = torch.zeros(4, 2, 5, device="cuda")
    tg, off = torch.tensor([1, 2, 3], dtype=torch.int32).cuda(), torch.tensor([0, 2, 3], dtype=torch.int64).cuda()
    for bad in (lambda: ops.ctc_align(torch.zeros(513, 2, 5, device="cuda"), tg, off, 2), lambda: ops.ctc_align(ok[:, :, :1], tg, off, 2),
                lambda: ops.ctc_align(torch.zeros(4, 2, 257, device="cuda"), tg, off, 2), lambda: ops.ctc_align(ok, tg, off, 2, blank=5),
                lambda: ops.ctc_align(ok, tg, off, 2, blank=-1), lambda: ops.ctc_align(ok, tg, off, 128), lambda: ops.ctc_align(ok, tg, off, -1),
                lambda: ops.ctc_align(ok.cpu(), tg, off, 2), lambda: ops.ctc_align(ok.double(), tg, off, 2), lambda: ops.ctc_align(ok, tg.long(), off, 2),
                lambda: ops.ctc_align(ok, tg, off.int(), 2), lambda: ops.ctc_align(ok, tg, off[:2], 2), lambda: ops.ctc_align(ok, tg.cpu(), off, 2),
                lambda: ops.ctc_align(ok.permute(0, 2, 1), tg, off[:2], 2), lambda: ops.ctc_align(torch.zeros(0, 2, 5, device="cuda"), tg, off, 2)):
        with pytest.raises(QeaError):
            bad()
    out = ops.ctc_align(ok[:, :0], tg[:0], off[:1], 0)         # N = 0: nothing is launched
    assert [tuple(o.shape) for o in out] == [(0,), (0, 4), (0,), (0,), (0,)]
    out = ops.ctc_align(ok, tg[:0], torch.zeros(3, dtype=torch.int64, device="cuda"), 0)      # a batch of empty labels
    torch.cuda.synchronize()
    assert out[0].tolist() == [0.0, 0.0] and (out[1] == -1).all() and out[2].numel() == 0


def test_char_spans_on_the_device_is_the_host_path(monkeypatch):
    from utils import char_spans
    lp, labels, blank, want = case("words")
    monkeypatch.delenv("QEA_ALIGN", raising=False)
    dev = char_spans(lp.cuda(), labels, {})
    monkeypatch.setenv("QEA_ALIGN", "host")
    host = char_spans(lp.cuda(), labels, {})
    cpu = char_spans(lp, labels, {})
    for d, h, c in zip(dev, host, cpu):
        assert spec.bits([d[0]])[0] == spec.bits([h[0]])[0] == spec.bits([c[0]])[0]
        assert np.array_equal(d[1], h[1]) and np.array_equal(d[2], h[2]) and np.array_equal(spec.bits(d[3]), spec.bits(h[3]))
        assert np.array_equal(d[1], c[1]) and np.array_equal(spec.bits(d[3]), spec.bits(c[3]))
    assert [d[0] for d in dev] == want[0].tolist()
    monkeypatch.delenv("QEA_ALIGN")
    half = char_spans(lp.cuda().half(), labels, {})            # any float dtype: converted as the decoders do
    assert all(math.isfinite(s[0]) for s in half)


def test_read_pages_with_chars_on_the_hip_crnn(monkeypatch, tmp_path):
    """two small pages through the HIP CRNN (its scores sharpened by seeded noise, so that the default-init weights read something): the
    characters with the spans from the kernel equal those with the spans from the host path on the very same scores"""
    import properties
    from qea.components import word_boxes
    from qea.reading import read_pages
    from test_word_strips_cpu import word_scans
    from test_word_strips_gpu import _crnn
    from utils import get_char_maps
    scans = word_scans(tmp_path / "in")
    pages = [torch.from_numpy(px).cuda() for px in list(scans.values())[:2]]
    boxes = word_boxes(pages, gap_x=2, min_area=16)
    index_to_char = get_char_maps(properties.char_set)[1]
    model, kept = _crnn(), []

    def forward(x):
        g = torch.Generator().manual_seed(len(kept))
        s = torch.log_softmax(model(x) + 4 * torch.randn(x.shape[3] // 4 - 1, x.shape[0], 95, generator=g).cuda(), 2)
        kept.append(s)
        return s
    monkeypatch.delenv("QEA_ALIGN", raising=False)
    texts, chars, cut = read_pages(model, pages, boxes, index_to_char, buckets=(64, 128), forward=forward, chars=True)
    plain = read_pages(model, pages, boxes, index_to_char, buckets=(64, 128), forward=lambda x, it=iter(list(kept)): next(it))
    assert plain == (texts, cut)
    monkeypatch.setenv("QEA_ALIGN", "host")
    again = read_pages(model, pages, boxes, index_to_char, buckets=(64, 128), forward=lambda x, it=iter(list(kept)): next(it), chars=True)
    assert again == (texts, chars, cut)
    flat = [(t, c) for tp, cp in zip(texts, chars) for t, c in zip(tp, cp)]
    assert sum(len(t) for t, _ in flat) >= 10
    for t, c in flat:
        assert "".join(e[0] for e in c) == t and all(e[1] < e[2] and e[3] <= 0 for e in c)
