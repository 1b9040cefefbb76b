"""Wall time of the facility-location selection on the POS fixture (tests/golden/pruning/cers_pos.json, n = 3 676, k = 3 309):
backend "cpu" (numpy fp64, once) against backend "hip" (median of 5 after one warm-up, host clock around calls that end in the
read-back of the ranking), and the pair rate n^2 * k / t.  A larger synthetic n shows the kernel's own rate where the fixture is
launch-bound.  GPU box only.   python tools/bench_pruning.py [--skip_cpu] [--big N K]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
from pruning import methods  # noqa: E402

# fp64 vector rate of the device (256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz) over the five operations a pair costs at d = 1
EXPECTED_PAIRS_PER_S = 256 * 4 * 16 * 2.4e9 / 5


def time_hip(x, k, reps=5):
    methods.facility_select_hip(x, min(k, 64))            # warm-up: code object load, workspace
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = methods.facility_select_hip(x, k)           # returns host arrays: the device has finished
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def report(label, n, k, t):
    rate = float(n) * n * k / t
    print(f"{label}: n={n} k={k}  {t * 1e3:10.1f} ms  {rate:.3e} pairs/s  ({rate / EXPECTED_PAIRS_PER_S:.1%} of the fp64 vector rate / 5 ops)", flush=True)
    return dict(label=label, n=n, k=k, seconds=t, pairs_per_s=rate, share_of_expected=rate / EXPECTED_PAIRS_PER_S)


def main():
    assert torch.cuda.is_available(), "bench_pruning.py times the device kernel: it needs an MI355X"
    argv = sys.argv[1:]
    with open(os.path.join(ROOT, "tests", "golden", "pruning", "cers_pos.json")) as f:
        cers = json.load(f)
    x = methods.feature_rows(cers)
    n = x.shape[0]
    k = n - int(n * 0.10)
    rows = []
    t_hip, (r_hip, _) = time_hip(x, k)
    rows.append(report("hip  POS", n, k, t_hip))
    if "--skip_cpu" not in argv:
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        r_cpu, _ = methods.facility_select_cpu(x, k)
        t_cpu = time.perf_counter() - t0
        rows.append(report("cpu  POS", n, k, t_cpu))
        print(f"hip / cpu: {t_cpu / t_hip:.0f}x; positions of the two rankings that agree: {int((r_hip == r_cpu).sum())} of {k}")
    if "--big" in argv:
        i = argv.index("--big")
        nb, kb = int(argv[i + 1]), int(argv[i + 2])
        for d in (1, 8):
            xb = np.random.default_rng(0).random((nb, d))
            t_big, _ = time_hip(xb, kb, reps=3)
            rows.append(report(f"hip  synthetic d={d}", nb, kb, t_big))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
