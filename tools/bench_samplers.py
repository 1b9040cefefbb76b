"""Wall time of the two estimate-driven samplers: the host code (QEA_SAMPLER=host: the reference's pick loop; the [T,B,C] copy and
per-strip loop of update_entropies) against the device path (csrc/sampling.hip: upload + one launch + read-back), same process, same
box.  Host clock around the call with the device synchronised at its end, median after one warm-up.
  picks      selection_utils._spread_pick at (n, k) = (2048, 1945), (512, 486), (64, 60), (20, 19): the area trainer's benchmark
             minibatch down to the patch flow's document; the routing threshold SPREAD_DEVICE_MIN_NK is checked against them
  forms      the kernel alone (device events) at n around the routing thresholds of include/qea_hip.h, k = 256
  entropies  selection_utils.update_entropies at (T, B, C) = (31, 2048, 95) and (31, 32, 95) on 96-column rows
Writes profiles/samplers.json.  GPU box only.   python tools/bench_samplers.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
import selection_utils as su  # noqa: E402
from qea import ops  # noqa: E402

PICKS = ((2048, 1945), (512, 486), (64, 60), (20, 19))
ENTROPIES = ((31, 2048, 95), (31, 32, 95))


def median_ms(fn, reps):
    ts = []
    for _ in range(reps + 1):                                  # the first call is the warm-up (code object, workspace)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:]) * 1e3, out


def time_pick(n, k, dev):
    g = torch.Generator().manual_seed(n)
    est = (torch.rand(n, generator=g) ** 2).tolist()
    rand = torch.rand(k, generator=g)
    os.environ["QEA_SAMPLER"] = "host"
    host_ms, want = median_ms(lambda: su._spread_pick(est, k, rand=rand, device=dev), reps=3 if n * k > 100000 else 9)
    os.environ["QEA_SAMPLER"] = "device"
    floor, su.SPREAD_DEVICE_MIN_NK = su.SPREAD_DEVICE_MIN_NK, 1     # time the device path at every size, routed or not
    try:
        before = ops.SAMPLER_LAUNCHES["spread"]
        dev_ms, got = median_ms(lambda: su._spread_pick(est, k, rand=rand, device=dev), reps=9)
        assert ops.SAMPLER_LAUNCHES["spread"] == before + 10
    finally:
        su.SPREAD_DEVICE_MIN_NK = floor
    return host_ms, dev_ms, bool(torch.equal(want, got))


def time_form(n, k, dev, reps=5):
    g = torch.Generator().manual_seed(n)
    est = (torch.rand(n, generator=g) ** 2).to(dev)
    pts = torch.rand(k, generator=g).to(dev)
    ops.spread_pick(est, pts)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.spread_pick(est, pts)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def time_entropy(T, B, C, dev):
    g = torch.Generator().manual_seed(B)
    wide = torch.zeros(T, B, 96)
    wide[:, :, :C] = torch.log_softmax(torch.randn(T, B, C, generator=g) * 2, dim=2)
    scores = wide.to(dev)[:, :, :C]
    names = [f"s{i}" for i in range(B)]

    def run(table):
        su.update_entropies(types.SimpleNamespace(sampler=su.UniformEntropySampler(table, {})), scores, names)
        return table

    def host(table):                                           # the code CUDA scores took before qea_seq_entropy: update_entropies on a host copy
        su.update_entropies(types.SimpleNamespace(sampler=su.UniformEntropySampler(table, {})), scores.cpu(), names)
        return table
    host_ms, th = median_ms(lambda: host({}), reps=3 if B > 256 else 9)
    dev_ms, td = median_ms(lambda: run({}), reps=9)
    return host_ms, dev_ms, max(abs(th[n] - td[n]) for n in names)


def main():
    assert torch.cuda.is_available(), "bench_samplers.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "samplers.json")
    dev = torch.device("cuda")
    picks, forms, ents = [], [], []
    for n, k in PICKS:
        host_ms, dev_ms, same = time_pick(n, k, dev)
        picks.append(dict(n=n, k=k, nk=n * k, host_ms=round(host_ms, 3), device_ms=round(dev_ms, 3), ratio=round(host_ms / dev_ms, 1), identical=same,
                          routed_to="device" if n * k >= su.SPREAD_DEVICE_MIN_NK else "host"))
        print(f"pick  n={n:5d} k={k:5d}  host {host_ms:9.3f} ms  device {dev_ms:7.3f} ms  x{host_ms / dev_ms:7.1f}  identical {same}", flush=True)
    for n in (512, 1024, 1536, 1537, 2048, 4096, 8192, 16384, 24576, 24577, 32768, 32769, 65536):
        ms = time_form(n, 256, dev)
        form = ("one wave" if n <= ops.SPREAD_WAVE_MAX_N else "four waves" if n <= ops.SPREAD_LDS4_MAX_N else
                "sixteen waves" if n <= ops.SPREAD_LDS_MAX_N else "sixteen waves, workspace")
        forms.append(dict(n=n, k=256, form=form, kernel_ms=round(ms, 4), us_per_pick=round(ms * 1e3 / 256, 3)))
        print(f"form  n={n:6d} k=256  {form:26s} {ms:8.4f} ms  {ms * 1e3 / 256:7.3f} us per pick", flush=True)
    for T, B, C in ENTROPIES:
        host_ms, dev_ms, diff = time_entropy(T, B, C, dev)
        ents.append(dict(T=T, B=B, C=C, host_ms=round(host_ms, 3), device_ms=round(dev_ms, 3), ratio=round(host_ms / dev_ms, 1), max_abs_diff=diff))
        print(f"entropy T={T} B={B:5d} C={C}  host {host_ms:9.3f} ms  device {dev_ms:7.3f} ms  x{host_ms / dev_ms:7.1f}  diff {diff:.1e}", flush=True)
    winners = [p["nk"] for p in picks if p["device_ms"] < p["host_ms"]]
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method="host clock, device synchronised at the end, median after a warm-up; forms: device events around the launch alone",
                  picks=picks, forms=forms, entropies=ents, routing=dict(SPREAD_DEVICE_MIN_NK=su.SPREAD_DEVICE_MIN_NK,
                                                                         smallest_measured_nk_where_device_wins=min(winners) if winners else None,
                                                                         SPREAD_WAVE_MAX_N=ops.SPREAD_WAVE_MAX_N, SPREAD_LDS4_MAX_N=ops.SPREAD_LDS4_MAX_N,
                                                                         SPREAD_LDS_MAX_N=ops.SPREAD_LDS_MAX_N))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, picks=len(picks), forms=len(forms), entropies=len(ents))))


if __name__ == "__main__":
    main()
