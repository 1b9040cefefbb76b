"""The engines' launch list against the one pinned in tests/golden/engine_schedule.json (tools/engine_schedule.py)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_engines_make_the_pinned_calls(golden_dir):
    """One forward + backward of every case of tools/engine_schedule.py (UNet: train with one and with two statistics groups, eval with
    and without a gradient, every switch off; CRNN: train, replica groups, backward_group, ragged groups, eval-mode BatchNorm, every
    switch off; each in split_f16 and split_bf16): every call into qea.ops, with its arguments (tensors by dtype, shape, stride,
    storage offset and parameter role), in order, equals the recording of the commit named in the golden file."""
    from qea import crnn_engine, ops, unet_engine
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import engine_schedule as E
    finally:
        sys.path.pop(0)
    pinned = json.load(open(os.path.join(golden_dir, "engine_schedule.json")))
    assert pinned["cases"] == json.loads(json.dumps(E.CASES)), "the cases changed: record the golden file again from the commit that pinned it"
    switches = [(m, n) for m in (unet_engine, crnn_engine) for n in vars(m) if n.startswith("FUSE_")]
    before = [getattr(m, n) for m, n in switches], ops.mfma_mode()
    try:
        got = E.record()
    finally:
        for (m, n), v in zip(switches, before[0]):
            setattr(m, n, v)
        ops.set_mfma_mode(before[1])
    assert sorted(got) == sorted(pinned["calls"]) and len(got) == 2 * len(E.CASES) == 22
    bad = []
    for case in sorted(got):
        want, have = pinned["calls"][case], got[case]
        for i, entry in enumerate(have):
            if i >= len(want) or want[i] != [entry[0], E.digest(entry)]:
                bad.append(f"{case}: call {i} is {entry[0]} {json.dumps(entry)}, pinned {want[i] if i < len(want) else 'nothing'}")
                break
        else:
            if len(want) > len(have):
                bad.append(f"{case}: {len(have)} calls, pinned {len(want)}; the first one missing is {want[len(have)]}")
    assert not bad, f"{len(bad)} of {len(got)} schedules moved (the first difference of each):\n" + "\n".join(bad)
