"""Wall time of one `gen_weights` call of the label-history weight generators: the host loops (QEA_HISTORY_WEIGHTS=host, the code
before csrc/history.hip existed) against the device path (packing + one pinned copy + one launch), same process, same box.
Host clock around the call with the device synchronised at its end, median of 5 after one warm-up; both generators,
n in {32, 256, 1024, 2048}, W in {1, 3, 5}, random words of 3-12 characters.  Writes profiles/history_weights.json.
GPU box only.   python tools/bench_history_weights.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
import properties  # noqa: E402
from label_tracking.tracking_methods import weightgenerator_factory  # noqa: E402


def histories(n, W, seed):
    rng = np.random.RandomState(seed)
    chars = properties.char_set[1:]
    names = [f"s{i}" for i in range(n)]
    return {nm: ["".join(rng.choice(chars, rng.randint(3, 13))) for _ in range(W)] for nm in names}, names


def time_call(wg, hist, names, mode, reps=5):
    os.environ["QEA_HISTORY_WEIGHTS"] = mode
    ts = []
    for i in range(reps + 1):                                  # the first call is the warm-up (code object, pinned buffer, cache)
        if mode == "device":
            # what a training step does between two calls: one new label per strip
            for nm in names:
                hist[nm].append(hist[nm][0][::-1] + str(i))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = wg.gen_weights(hist, names)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:]) * 1e3, w


def main():
    assert torch.cuda.is_available(), "bench_history_weights.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "history_weights.json")
    c2i = {c: i for i, c in enumerate(properties.char_set)}
    dev = torch.device("cuda")
    rows = []
    for method in ("levenshtein", "self_attention"):
        for W in (1, 3, 5):
            wg = weightgenerator_factory(method)(types.SimpleNamespace(window_size=W), dev, c2i)
            for n in (32, 256, 1024, 2048):
                hist, names = histories(n, W, seed=n + W)
                host_ms, w_host = time_call(wg, hist, names, "host", reps=5 if n <= 256 else 3)
                dev_ms, _ = time_call(wg, hist, names, "device")
                os.environ["QEA_HISTORY_WEIGHTS"] = "device"
                same = (wg.gen_weights(hist, names) - wg._gen_weights_host(hist, names).to(dev)).abs().max().item()
                rows.append(dict(generator=method, n=n, window=W, host_ms=round(host_ms, 3), device_ms=round(dev_ms, 3),
                                 ratio=round(host_ms / dev_ms, 1), max_abs_diff=same))
                print(f"{method:15s} n={n:5d} W={W}  host {host_ms:9.2f} ms  device {dev_ms:7.3f} ms  x{host_ms / dev_ms:7.1f}  diff {same:.1e}", flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0), method="host clock, device synchronised at the end, median after a warm-up; "
                  "the device path appends one new label per strip before every call", rows=rows)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, rows=len(rows))))


if __name__ == "__main__":
    main()
