"""The four qea_conv_igemm queries over a fixed grid of descriptors against the answers pinned before they were all made to read
one route() (tests/golden/conv_route_queries.json, written by tools/conv_route_queries.py).  No GPU: the queries read the
descriptor's fields and whether its pointers are null, nothing else."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_answers_equal_the_pinned_ones(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import conv_route_queries as Q
    finally:
        sys.path.pop(0)
    from qea import _lib
    pinned = json.load(open(os.path.join(golden_dir, "conv_route_queries.json")))
    assert pinned["axes"] == Q.AXES, "the grid changed: regenerate the golden file from the commit that pinned it"
    mode = _lib.lib().qea_set_mfma_mode(-1)
    got = Q.answers()
    assert _lib.lib().qea_set_mfma_mode(-1) == mode, "the generator must restore the MFMA mode"
    want = pinned["answers"]
    assert len(got) == len(want) == 13500
    bad = [(i, f, kw, m, want[i], got[i]) for i, (f, kw, m) in enumerate(Q.cases()) if want[i] != got[i]]
    assert not bad, f"{len(bad)} of {len(want)} answers moved (uses + 2 wants + 6 can_pool + 12 blocks); first: {bad[:3]}"
    # the grid reaches every answer worth pinning
    assert {v % 2 for v in want} == {0, 1} and {(v // 2) % 3 for v in want} == {0, 1, 2} and {(v // 6) % 2 for v in want} == {0, 1}
    assert sum(v >= 12 for v in want) > 100
