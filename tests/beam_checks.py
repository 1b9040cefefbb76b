"""The comparisons the beam-search tests share (a plain module, imported like beam_spec): a device result against the arrays of one
of the three specifications, and host scores against a specification's."""
import math

import torch

MIN_GAP = 1e-7
SCORE = (("score", torch.float64),)


def same_scores(got, want):
    """Nested lists of scores, equal or within 1e-12 * max(1, |s|): the host loop against a specification."""
    return all(a == b or abs(a - b) <= 1e-12 * max(1.0, abs(b)) for r, w in zip(got, want) for a, b in zip(r, w))


def check_against_spec(got, want, gap, columns=SCORE):
    """got: what qea.ops.ctc_beam_decode / _lm / _dfa returned (tensors on the device); want: as_arrays(beams, K, T) of the matching
    specification; gap: its smallest decisive gap; columns: (name, dtype) of what follows tokens and lengths.  An exact comparison of
    a discrete result is only fair where no decision hangs on fp64 rounding, hence gap >= 1e-7.  Shapes, dtypes and no NaN; tokens,
    lengths and int32 columns exact, -1 in the rows beyond the live count; float64 columns -inf there and within 1e-9 * max(1, |s|)
    in the live rows.  Returns the result on the CPU."""
    assert gap >= MIN_GAP, f"input too close to a tie for an exact comparison: gap {gap:.3e}"
    N, K, T = len(want[0]), len(want[0][0]), len(want[0][0][0])
    assert len(got) == len(want) == 2 + len(columns) and all(v.is_cuda for v in got)
    tokens, lengths, *cols = (v.cpu() for v in got)
    assert tokens.shape == (N, K, T) and tokens.dtype == torch.int32 and lengths.shape == (N, K) and lengths.dtype == torch.int32
    for (name, dtype), col in zip(columns, cols):
        assert col.shape == (N, K) and col.dtype == dtype and not torch.isnan(col).any(), name
    assert lengths.tolist() == want[1]
    assert torch.equal(tokens, torch.tensor(want[0], dtype=torch.int32))
    dead = lengths < 0
    for (name, dtype), col, w in zip(columns, cols, want[2:]):
        w = torch.tensor(w, dtype=dtype)
        if dtype == torch.int32:
            assert torch.equal(col, w) and (col[dead] == -1).all(), name
            continue
        assert (col[dead] == -math.inf).all() and (w[dead] == -math.inf).all(), name
        err = (col[~dead] - w[~dead]).abs() / w[~dead].abs().clamp(min=1.0)
        print(f"max {name} error {err.max().item():.3e} (relative to max(1, |s|)), smallest gap {gap:.3e}")
        assert err.max().item() <= 1e-9, name
    return (tokens, lengths, *cols)
