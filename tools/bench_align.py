"""Time of the CTC forced alignment (csrc/ctc_align.hip) beside the greedy decode kernel and qea_ctc_loss without gradient on the same
inputs, same process, same box, at C = 95 and (T, N, L) = (31, 2048, 4..12 random), an evaluation batch of ordinary words, and
(127, 256, 20..60 random), long strips.  The loss runs the same recursion with lse3 in place of the max, so it is the natural yardstick.
(While the kernel had a second form for short labels, this tool timed both: profiles/align_forms_ab.json.)  Inputs: log_softmax of
randn * 2 with the blank column raised by 2, seeded; labels without the blank, seeded.
  *_ms        device events around LAUNCHES back-to-back launches, per-launch time = the median of REPS such windows after a warm-up
              window, with the min and max of the windows
  *_graph_ms  the same launches captured into one graph and replayed: a call of qea.ops.ctc_align is shorter on the device than the
              host needs to issue it, so the first figure is the host's
Writes profiles/align.json.  GPU box only.   python tools/bench_align.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
from qea import align as host_align  # noqa: E402
from qea import ops  # noqa: E402

C = 95
SHAPES = ((31, 2048, 4, 12), (127, 256, 20, 60))
LAUNCHES, REPS, HOST_SAMPLES = 20, 9, 32


def event_ms(fn):
    """per-launch milliseconds: (median, min, max) over REPS windows of LAUNCHES launches, after one warm-up window"""
    ts = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / LAUNCHES)
    return tuple(round(v, 4) for v in (statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])))


def graph_ms(fn):
    """the same windows with the host taken out: LAUNCHES calls captured into one graph, one replay per window.  Where a call is shorter
    than the host needs to issue it, event_ms measures the host; this measures the device"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(LAUNCHES):
            fn()
    ts = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / LAUNCHES)
    return tuple(round(v, 4) for v in (statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])))


def time_shape(T, N, lo, hi, dev):
    g = torch.Generator().manual_seed(T * 1000 + N)
    x = torch.randn(T, N, C, generator=g) * 2
    x[:, :, 0] += 2
    lp = torch.log_softmax(x, dim=2)
    rng = np.random.default_rng(T + N)
    lengths = rng.integers(lo, hi + 1, N)
    targets = torch.from_numpy(rng.integers(1, C, int(lengths.sum())).astype(np.int32))
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int64))
    L_max = int(lengths.max())
    d, tg, off = lp.to(dev), targets.to(dev), offsets.to(dev)
    row = dict(T=T, N=N, C=C, L_min=lo, L_max=hi)
    got = [v.cpu() for v in ops.ctc_align(d, tg, off, L_max)]
    run_align = lambda: ops.ctc_align(d, tg, off, L_max)
    row["align_ms"], row["align_ms_min"], row["align_ms_max"] = event_ms(run_align)
    row["align_graph_ms"], row["align_graph_ms_min"], row["align_graph_ms_max"] = graph_ms(run_align)
    n = min(N, HOST_SAMPLES)
    host = host_align.ctc_align(lp[:, :n], targets[:int(offsets[n])], offsets[:n + 1], L_max)
    row["host_identical"] = bool(torch.equal(host[0].view(torch.int64), got[0][:n].view(torch.int64)) and torch.equal(host[1], got[1][:n]))
    row["feasible"] = int((got[0] > -float("inf")).sum())
    tokens = torch.empty(N, T, dtype=torch.int32, device=dev)
    glen = torch.empty(N, dtype=torch.int32, device=dev)
    row["greedy_ms"], _, _ = event_ms(lambda: ops.greedy_decode(d, d.stride(0), d.stride(1), T, N, C, 0, tokens, glen))
    row["greedy_graph_ms"], _, _ = graph_ms(lambda: ops.greedy_decode(d, d.stride(0), d.stride(1), T, N, C, 0, tokens, glen))
    in_len = torch.full((N,), T, dtype=torch.int32, device=dev)
    tg_len = torch.from_numpy(lengths.astype(np.int32)).to(dev)
    nll, loss = torch.empty(N, device=dev), torch.empty(1, device=dev)
    run_loss = lambda: ops.ctc_loss(d, d.stride(0), d.stride(1), tg, off, in_len, tg_len, T, N, C, 0, 2 * L_max + 1, 0, 1.0, nll, loss, None, 0, 0)
    row["ctc_loss_no_grad_ms"], row["ctc_loss_no_grad_ms_min"], row["ctc_loss_no_grad_ms_max"] = event_ms(run_loss)
    row["ctc_loss_no_grad_graph_ms"], _, _ = graph_ms(run_loss)
    return row


def main():
    assert torch.cuda.is_available(), "bench_align.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "align.json")
    dev = torch.device("cuda")
    rows = []
    for T, N, lo, hi in SHAPES:
        r = time_shape(T, N, lo, hi, dev)
        rows.append(r)
        print(" ".join(f"{k}={v}" for k, v in r.items()), flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method=f"device events around {LAUNCHES} back-to-back launches, per-launch median of {REPS} windows after a warm-up window "
                         f"(the five torch.empty of a call included for the alignment); min / max are over the same windows; *_graph_ms: "
                         f"the same {LAUNCHES} calls captured into one graph, one replay per window: device time where the host is the slower",
                  shapes=rows)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, shapes=len(rows))))


if __name__ == "__main__":
    main()
