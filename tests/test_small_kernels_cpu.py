"""The statements of tests/small_kernel_spec.py against independent ground: a brute force over all CTC paths, torch's CTC in double,
np.argmax / torch.argmax and the product's host decode, the published Random123 answers of Philox4x32-10, and the Adam of
oracle/path_oracle.py.  One test shows why the device CTC gates of tests/test_small_kernels_gpu.py exist: the same recursion run in
fp32 passes the gates the suite had before and misses the new ones."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernel_spec as S


# ----------------------------------------------------------------------------- CTC
@pytest.mark.parametrize("blank", S.TINY_BLANKS)
def test_ctc_spec_equals_brute_force(blank):
    lp = S.tiny_log_probs(6, len(S.TINY_LABELS) * len(S.TINY_TN), seed=100 + blank)
    seen_single, seen_infeasible, n = 0, 0, 0
    for lab in S.TINY_LABELS:
        need = len(lab) + S.repeats(lab)
        for tn in sorted(set(S.TINY_TN) | {max(need, 1), max(need - 1, 1)}):
            target = S.tiny_label(lab, blank)
            bf = S.ctc_bruteforce(lp[:, n % lp.shape[1]], target, tn, blank)
            nll, grad = S.ctc_spec(lp[:, n % lp.shape[1]], target, tn, blank)
            n += 1
            if tn < need:
                seen_infeasible += 1
                assert bf == math.inf and nll == np.inf, (lab, tn)
                assert np.isnan(grad[:tn]).all() and not grad[tn:].any()
                continue
            seen_single += tn == need
            assert abs(float(nll) - bf) <= 1e-12 * max(abs(bf), 1.0), (lab, tn, float(nll), bf)
            assert np.isfinite(grad).all() and not grad[tn:].any()
            if tn == need and lab:
                # exactly one alignment: its probability is the sum of its frames' log-probs
                path = []
                for i, c in enumerate(target):
                    if i and c == target[i - 1]:
                        path.append(blank)
                    path.append(c)
                assert abs(float(nll) + sum(float(lp[t, (n - 1) % lp.shape[1], c]) for t, c in enumerate(path))) <= 1e-12 * abs(bf)
    assert seen_single >= len(S.TINY_LABELS) - 1 and seen_infeasible >= len(S.TINY_LABELS) - 1
    nll, grad = S.ctc_spec(lp[:, 0], (1,), 0, blank)
    assert nll == np.inf and not grad.any()


@functools.lru_cache(maxsize=None)
def _batch_b(scale):
    """batch B with its fp64 statement and torch's double-precision answer (computed once, never modified)"""
    logits, lp, labels, in_len = S.batch_b(scale)
    nll, grad = S.ctc_batch_spec(lp, labels, in_len, 0)
    lpt = torch.from_numpy(lp).double().requires_grad_()
    tg = torch.tensor([c for lab in labels for c in lab], dtype=torch.long)
    tl = torch.tensor([len(lab) for lab in labels], dtype=torch.long)
    per = F.ctc_loss(lpt, tg, torch.from_numpy(np.minimum(in_len, S.B_T)).long(), tl, reduction="none")
    per.sum().backward()
    return lp, labels, in_len, nll, grad, per.detach().numpy(), lpt.grad.numpy()


@pytest.mark.parametrize("scale", (3.0, 30.0))
def test_ctc_spec_equals_torch_double(scale):
    lp, labels, in_len, nll, grad, nll_t, grad_t = _batch_b(scale)
    assert np.isinf(nll[69]) and np.isfinite(nll[:69]).all() and np.array_equal(np.isinf(nll), np.isinf(nll_t))
    worst_nll = np.abs(nll[:69] - nll_t[:69]).max() / np.abs(nll_t[:69]).max()
    assert np.array_equal(np.isnan(grad), np.isnan(grad_t))
    assert np.isnan(grad[:in_len[69], 69]).all() and not grad[in_len[69]:, 69].any()
    ok = ~np.isnan(grad_t)
    worst_g = np.abs(grad[ok] - grad_t[ok]).max() / np.abs(grad_t[ok]).max()
    print(f"ctc_spec vs torch double, logits x{scale:g}: nll {worst_nll:.2e}, grad {worst_g:.2e} of the largest magnitude")
    assert worst_nll <= 1e-12 and worst_g <= 1e-12


def test_new_ctc_gate_refuses_an_fp32_recursion_the_old_gates_admit():
    """The recursion of ctc_spec in float32 on batch B (logits x 3): it satisfies the two gates that were the suite's only direct
    checks of the CTC kernel (nll rtol 1e-5, gradient 1e-4 x max |ref|) and violates the derived gradient gate on most samples."""
    lp, labels, in_len, nll, grad, _, _ = _batch_b(3.0)
    nll32, grad32 = S.ctc_batch_spec(lp, labels, in_len, 0, dtype=np.float32)
    fin = np.isfinite(nll)
    assert np.array_equal(np.isfinite(nll32), fin) and np.array_equal(np.isnan(grad32), np.isnan(grad))
    ok = ~np.isnan(grad)
    err = np.abs(grad32.astype(np.float64) - grad)
    old_nll = (np.abs(nll32[fin].astype(np.float64) - nll[fin]) / np.abs(nll[fin])).max()
    old_grad = err[ok].max() / np.abs(grad[ok]).max()
    gate = S.ctc_grad_gate(grad)
    ratio = np.array([S.gate_ratio(grad32[:, n], grad[:, n], gate[:, n]) for n in range(S.B_N)])
    print(f"fp32 recursion on batch B: nll rel {old_nll:.2e} (old gate 1e-5), grad {old_grad:.2e} of max (old gate 1e-4); "
          f"new gate exceeded on {(ratio > 1).sum()} of {fin.sum()} samples, worst {ratio.max():.0f}x")
    assert old_nll <= 1e-5 and old_grad <= 1e-4
    assert (ratio > 1).any()
    # the fp64 statement rounded to fp32 once, what the kernel is asked to deliver, is inside the new gate
    assert S.gate_ratio(grad.astype(np.float32), grad, gate) <= 0.25 + 1e-9


# ----------------------------------------------------------------------------- decode
INDEX_TO_CHAR = {i: chr(0x100 + i) for i in range(max(S.DECODE_C))}


@pytest.mark.parametrize("C", S.DECODE_C)
def test_argmax_first_is_numpy_and_torch_argmax(C):
    import utils
    s = S.decode_rows(C)
    assert np.isnan(s).any() and np.isinf(s).any()
    mine = np.array([[S.argmax_first(s[t, n]) for n in range(s.shape[1])] for t in range(s.shape[0])])
    assert np.array_equal(mine, np.argmax(s, axis=2))
    assert np.array_equal(mine, torch.from_numpy(s).argmax(dim=2).numpy())
    want = ["".join(INDEX_TO_CHAR[k] for k in toks) for toks in S.greedy_spec(s, 0)]
    assert utils.pred_to_string(torch.from_numpy(s), None, INDEX_TO_CHAR) == want
    if C > 70:
        assert mine[1, 3] == 70 and mine[1, 4] == 1 and mine[1, 2] == 5 and mine[1, 0] == 9 and mine[1, 1] == 3


def test_argmax_first_plain_cases():
    nan, inf = float("nan"), float("inf")
    assert S.argmax_first([1.0, 3.0, 3.0]) == 1
    assert S.argmax_first([1.0, inf, nan, nan]) == 2
    assert S.argmax_first([-inf, -inf]) == 0
    assert S.argmax_first([nan]) == 0


# ----------------------------------------------------------------------------- Philox / jitter
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = S.philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in got) == want
    # vectorised: the same words at every position of an array of counters
    arr = S.philox4x32_10(tuple(np.full(3, c, dtype=np.uint64) for c in counter), key)
    assert all((a == g).all() for a, g in zip(arr, got))


def test_jitter_noise_spec_layout():
    K, R, HW = 3, 2, 20
    sigma = np.array([0.01 * (1 + im % 5) for im in range(R * K)], dtype=np.float32)
    z, r = S.jitter_noise_spec(K, R, HW, sigma, 2 ** 40 + 7, 2 ** 33 + 1)
    assert z.shape == r.shape == (R * K, HW) and np.isfinite(z).all() and (r > 0).all()
    # quad 7 = image 1, pixels 8..11, by hand
    w = [int(x) for x in S.philox4x32_10((7, 0, 1, 2), (7, 2 ** 8))]
    u = [float(np.float32(x >> 8) + np.float32(0.5)) / 2 ** 24 for x in w]      # the sum in fp32: it rounds above 2^23
    for e, (a, b, f) in enumerate(((0, 1, math.cos), (0, 1, math.sin), (2, 3, math.cos), (2, 3, math.sin))):
        want = math.sqrt(-2 * math.log(u[a])) * f(float(np.float32(2 * math.pi) * np.float32(u[b]))) * float(sigma[1])
        assert abs(z[1, 8 + e] - want) <= 1e-12
    assert np.array_equal(r[:, 0::4], r[:, 1::4]) and np.array_equal(r[:, 2::4], r[:, 3::4])
    # cos^2 + sin^2: elements 0 and 1 of a quad lie on the circle of radius r sigma
    assert np.allclose(z[:, 0::4] ** 2 + z[:, 1::4] ** 2, (r[:, 0::4] * sigma[:, None].astype(np.float64)) ** 2, rtol=1e-12)
    # another seed half, another offset half: another stream
    for seed, off in ((7, 2 ** 33 + 1), (2 ** 40 + 7, 1), (2 ** 40 + 7, 2 ** 33)):
        assert not np.array_equal(S.jitter_noise_spec(K, R, HW, sigma, seed, off)[1], r)


# ----------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("wd", (0.0, 5e-4))
def test_adam_spec_equals_path_oracle(wd):
    from oracle import path_oracle as po
    rng = np.random.RandomState(3)
    p, g, m = (rng.randn(1001).astype(np.float32) for _ in range(3))
    v = (rng.randn(1001) ** 2).astype(np.float32)
    for step in (1, 2, 7):
        a = S.adam_spec(p, g, m, v, step, 1e-4, weight_decay=wd)
        pr, mr, vr = po.adam_update(p, g, m, v, step, 1e-4, weight_decay=wd)
        for x, y in ((a.p, pr), (a.m, mr), (a.v, vr)):
            assert np.abs(x - y).max() <= 1e-15 * max(np.abs(y).max(), 1.0)
        assert np.allclose(a.p, p + a.update, rtol=0, atol=0)
    # the scale multiplies the gradient, not the weight-decay term
    a = S.adam_spec(p, g, m, v, 3, 1e-4, weight_decay=wd, grad_scale=0.25)
    b = S.adam_spec(p, (g.astype(np.float64) * 0.25), m, v, 3, 1e-4, weight_decay=wd)
    assert np.array_equal(a.p, b.p) and np.array_equal(a.g_eff, g * 0.25 + wd * p.astype(np.float64))
