"""Time of the CTC prefix beam search (csrc/ctc_beam.hip) beside the greedy decode kernel it complements and the host loop it replaces
for CUDA tensors (qea/beam.py, what QEA_BEAM=host runs), same process, same box, at
(T, N, C, K) = (31, 2048, 95, 8), (31, 2048, 95, 32), (127, 256, 95, 16): an evaluation batch at the two ends of the useful beam widths
and a long strip.  Inputs: log_softmax of randn * 2 with the blank column raised by 2, seeded.
  kernels    device events around LAUNCHES back-to-back launches, per-launch time = the median of REPS such windows after a warm-up
  host loop  host clock around the loop over the first HOST_SAMPLES samples (it is seconds per batch: the whole batch is not timed),
             reported per sample and scaled to N; its beams are compared with the kernel's on those samples
Writes profiles/beam_decode.json.  GPU box only.   python tools/bench_beam_decode.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
from qea import beam as host_beam  # noqa: E402
from qea import ops  # noqa: E402

SHAPES = ((31, 2048, 95, 8), (31, 2048, 95, 32), (127, 256, 95, 16))
LAUNCHES, REPS, HOST_SAMPLES = 20, 9, 32


def event_ms(fn):
    """per-launch milliseconds: median over REPS windows of LAUNCHES launches, after one warm-up window"""
    ts = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / LAUNCHES)
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])


def time_shape(T, N, C, K, dev):
    g = torch.Generator().manual_seed(T * 1000 + K)
    x = torch.randn(T, N, C, generator=g) * 2
    x[:, :, 0] += 2
    lp = torch.log_softmax(x, dim=2)
    d = lp.to(dev)
    tokens = torch.empty(N, T, dtype=torch.int32, device=dev)
    lengths = torch.empty(N, dtype=torch.int32, device=dev)
    beam_ms, beam_lo, beam_hi = event_ms(lambda: ops.ctc_beam_decode(d, K))
    greedy_ms, _, _ = event_ms(lambda: ops.greedy_decode(d, d.stride(0), d.stride(1), T, N, C, 0, tokens, lengths))
    n = min(N, HOST_SAMPLES)
    t0 = time.perf_counter()
    ht, hl, hs = host_beam.ctc_beam_decode(lp[:, :n], K)
    host_s = time.perf_counter() - t0
    dt, dl, ds = (v[:n].cpu() for v in ops.ctc_beam_decode(d, K))
    same = bool(torch.equal(ht, dt) and torch.equal(hl, dl))
    err = ((hs - ds).abs() / hs.abs().clamp(min=1.0)).max().item()
    gt, gl = tokens[:n].cpu(), lengths[:n].cpu().tolist()
    best_differs = sum(1 for i in range(n) if dl[i, 0].item() != gl[i] or dt[i, 0, :gl[i]].tolist() != gt[i, :gl[i]].tolist())
    return dict(T=T, N=N, C=C, K=K, beam_kernel_ms=round(beam_ms, 4), beam_kernel_ms_min=round(beam_lo, 4), beam_kernel_ms_max=round(beam_hi, 4),
                beam_us_per_sample=round(beam_ms * 1e3 / N, 3), greedy_kernel_ms=round(greedy_ms, 4),
                host_samples=n, host_ms_per_sample=round(host_s * 1e3 / n, 3), host_ms_scaled_to_N=round(host_s * 1e3 / n * N, 1),
                host_over_kernel=round(host_s * 1e3 / n * N / beam_ms, 1), host_beams_identical=same, host_max_score_err=err,
                best_differs_from_greedy=best_differs)


def main():
    assert torch.cuda.is_available(), "bench_beam_decode.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "beam_decode.json")
    dev = torch.device("cuda")
    rows = []
    for T, N, C, K in SHAPES:
        r = time_shape(T, N, C, K, dev)
        rows.append(r)
        print(f"T={T:3d} N={N:4d} C={C} K={K:2d}  beam {r['beam_kernel_ms']:8.4f} ms ({r['beam_us_per_sample']:.3f} us per sample)  greedy "
              f"{r['greedy_kernel_ms']:7.4f} ms  host loop {r['host_ms_per_sample']:8.3f} ms per sample (x{r['host_over_kernel']} at N)  "
              f"identical {r['host_beams_identical']}  best != greedy on {r['best_differs_from_greedy']}/{r['host_samples']}", flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method=f"kernels: device events around {LAUNCHES} back-to-back launches, per-launch median of {REPS} windows after a warm-up window "
                         f"(output allocation included for the beam: three torch.empty per call); host loop: host clock over the first "
                         f"{HOST_SAMPLES} samples, scaled to N",
                  shapes=rows)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, shapes=len(rows))))


if __name__ == "__main__":
    main()
