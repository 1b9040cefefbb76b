"""Time of the CTC prefix beam search with a character n-gram prior fused in (csrc/ctc_beam.hip, qea_ctc_beam_decode_lm) beside the
plain kernel of the same library, same process, same box, with the method of tools/bench_beam_decode.py, at its three shapes
(T, N, C, K) = (31, 2048, 95, 8), (31, 2048, 95, 32), (127, 256, 95, 16) and the same seeded inputs:
  plain      qea.ops.ctc_beam_decode
  fused      qea.ops.ctc_beam_decode_lm at context m = 0, 1, 2, tables randn(C ** m, C) - 1 in fp64
device events around LAUNCHES back-to-back launches, per-launch time = the median of REPS such windows after a warm-up; the window
spread (min, max) is reported with every figure, and the ratio fused / plain.
--plain-only times the plain kernel alone and prints one JSON line.  It binds qea_ctc_beam_decode by symbol, not through qea._lib
(which wants every entry point of the header), so QEA_HIP_LIB may name the PARENT commit's library: run it in processes of their own
for both libraries to see whether sharing the kernel body with the fused search changed the plain kernel; --parent-json PATH and
--current-json PATH merge those two runs' output into the result.
Writes profiles/beam_lm.json.  GPU box only.
    python tools/bench_beam_lm.py [--out PATH] [--parent-json PATH --current-json PATH] [--plain-only]"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
from qea import _lib, ops  # noqa: E402

SHAPES = ((31, 2048, 95, 8), (31, 2048, 95, 32), (127, 256, 95, 16))
LAUNCHES, REPS = 20, 9


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
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])


def scores(T, N, C, K, dev):
    g = torch.Generator().manual_seed(T * 1000 + K)
    x = torch.randn(T, N, C, generator=g) * 2
    x[:, :, 0] += 2
    return torch.log_softmax(x, dim=2).to(dev)


def figures(prefix, t):
    return {f"{prefix}_ms": round(t[0], 4), f"{prefix}_ms_min": round(t[1], 4), f"{prefix}_ms_max": round(t[2], 4)}


def plain_by_symbol():
    """ops.ctc_beam_decode's launch (three torch.empty per call included) on the library QEA_HIP_LIB names, bound by symbol"""
    fn = ctypes.CDLL(_lib.LIB_PATH).qea_ctc_beam_decode
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int32] * 7 + [ctypes.c_void_p] * 4

    def decode(d, K):
        T, N, C = d.shape
        tokens = torch.empty(N, K, T, dtype=torch.int32, device=d.device)
        lengths = torch.empty(N, K, dtype=torch.int32, device=d.device)
        out = torch.empty(N, K, dtype=torch.float64, device=d.device)
        rc = fn(d.data_ptr(), d.stride(0), d.stride(1), T, N, C, 0, K, tokens.data_ptr(), lengths.data_ptr(), out.data_ptr(),
                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return tokens, lengths, out
    return decode


def time_shape(T, N, C, K, dev, plain_only):
    d = scores(T, N, C, K, dev)
    decode = plain_by_symbol() if plain_only else ops.ctc_beam_decode
    plain = event_ms(lambda: decode(d, K))
    row = dict(T=T, N=N, C=C, K=K, **figures("plain", plain), plain_spread=round((plain[2] - plain[1]) / plain[0], 4))
    if plain_only:
        return row
    for m in (0, 1, 2):
        g = torch.Generator().manual_seed(1000 + m)
        W = (torch.randn(C ** m, C, generator=g, dtype=torch.float64) - 1.0).to(dev)
        fused = event_ms(lambda: ops.ctc_beam_decode_lm(d, K, W, m))
        row.update(figures(f"fused_m{m}", fused))
        row[f"fused_m{m}_spread"] = round((fused[2] - fused[1]) / fused[0], 4)
        row[f"fused_m{m}_over_plain"] = round(fused[0] / plain[0], 4)
    return row


def main():
    assert torch.cuda.is_available(), "bench_beam_lm.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    plain_only = "--plain-only" in argv
    dev = torch.device("cuda")
    rows = [time_shape(T, N, C, K, dev, plain_only) for T, N, C, K in SHAPES]
    if plain_only:
        print(json.dumps(dict(library=os.path.basename(os.environ.get("QEA_HIP_LIB", "")) or "in-tree", shapes=rows)))
        return
    for r in rows:
        print(f"T={r['T']:3d} N={r['N']:4d} C={r['C']} K={r['K']:2d}  plain {r['plain_ms']:8.4f} ms (spread {r['plain_spread']:.4f})  fused m=0 "
              f"{r['fused_m0_ms']:8.4f}  m=1 {r['fused_m1_ms']:8.4f}  m=2 {r['fused_m2_ms']:8.4f} ms  ratios {r['fused_m0_over_plain']:.4f} "
              f"{r['fused_m1_over_plain']:.4f} {r['fused_m2_over_plain']:.4f}", flush=True)
    if "--parent-json" in argv:
        def plain_only_run(flag):
            with open(argv[argv.index(flag) + 1]) as f:
                return json.loads(f.read().strip().splitlines()[-1])["shapes"]
        for r, p, c in zip(rows, plain_only_run("--parent-json"), plain_only_run("--current-json")):
            assert (r["T"], r["N"], r["K"]) == (p["T"], p["N"], p["K"]) == (c["T"], c["N"], c["K"])
            r.update({f"by_symbol_parent_{k}": v for k, v in p.items() if k.startswith("plain_")})
            r.update({f"by_symbol_current_{k}": v for k, v in c.items() if k.startswith("plain_")})
            r["by_symbol_current_over_parent"] = round(c["plain_ms"] / p["plain_ms"], 4)
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "beam_lm.json")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method=f"device events around {LAUNCHES} back-to-back launches, per-launch median of {REPS} windows after a warm-up window "
                         f"(output allocation included: three torch.empty per plain call, four per fused call); spread = (max - min) / median "
                         f"of the windows; by_symbol_parent_* / by_symbol_current_*: the plain kernel of the parent commit's library and of this one, "
                         f"--plain-only runs in processes of their own on the same box",
                  shapes=rows)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, shapes=len(rows))))


if __name__ == "__main__":
    main()
