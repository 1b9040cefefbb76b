"""What the binarisation baselines (csrc/binarize.hip; qea/binarize.py) cost on the device, 8-bit pages in and 8-bit pages out:
  workloads   docs64: 64 documents of 400 x 512 (the training canvas);  a4x8: 8 pages of 2480 x 3508
  methods     otsu (both launches), sauvola at windows 15, 25, 51 and 127 (k = 0.2, R = 128)
  device_ms   device events around the launches alone (store, page table and output on the device before), median of 20 after 3 warm-ups
  copy_ms     the yardstick: a plain device copy_ of the same store, timed the same way — a binariser moves 1 B in and 1 B out per pixel,
              exactly what the copy moves
  host_ms     the product's host path (binarize_pages on CPU tensors: numpy integral images) on the same pages, host clock, one run
  identical   whether the device result equals the host path's, bit for bit
Each workload runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/binarize.json.  GPU box only.   python tools/bench_binarize.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
WORKLOADS = {"docs64": [(400, 512)] * 64, "a4x8": [(2480, 3508)] * 8}
WINDOWS = [15, 25, 51, 127]
STEP_TIMEOUT = 420


def arg(name, default):
    argv = sys.argv[1:]
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def _timed(torch, fn, warmups=3, reps=20):
    ms = []
    for k in range(warmups + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmups:
            ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def step(name):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    from qea import ops
    from qea.binarize import binarize_pages
    from qea.pages import pack_pages, unpack_pages
    assert torch.cuda.is_available(), "bench_binarize.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    # text-like pages: dark strokes on a noisy light ground, so that both classes occur in every window size
    pages = []
    for h, w in WORKLOADS[name]:
        page = torch.randint(170, 256, (h, w), generator=g, dtype=torch.uint8)
        ink = torch.rand(h // 8 + 1, w // 4 + 1, generator=g) < 0.2
        mask = ink.repeat_interleave(8, 0).repeat_interleave(4, 1)[:h, :w]
        page[mask] = torch.randint(0, 90, (int(mask.sum()),), generator=g, dtype=torch.uint8)
        pages.append(page)
    pk = pack_pages(pages)
    store = pk.store.to(dev)
    table = ops.page_table(pk.offset, pk.h, pk.w, dev)
    out, copy = torch.empty_like(store), torch.empty_like(store)
    res = dict(workload=name, pages=len(pages), page_size=list(WORKLOADS[name][0]), pixels=int(store.numel()))
    res["copy_ms"] = _timed(torch, lambda: copy.copy_(store))
    res["copy_gb_per_s"] = round(2 * store.numel() / res["copy_ms"] / 1e6, 1)
    rows = []
    for method, win in [("otsu", None)] + [("sauvola", w) for w in WINDOWS]:
        if method == "otsu":
            fn = lambda: ops.binarize_otsu(store, table, ops.otsu_histogram(store, table), out_u8=out)
        else:
            fn = lambda: ops.binarize_sauvola(store, table, win, 0.2, 128.0, out_u8=out)
        row = dict(method=method, window=win, device_ms=_timed(torch, fn))
        t0 = time.perf_counter()
        want = binarize_pages(pages, method, window=win or 25, out="u8")
        row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["identical"] = all(torch.equal(a.cpu(), b) for a, b in zip(unpack_pages(out, pk), want))
        row["ink_share"] = round(float(sum(int((b == 0).sum()) for b in want)) / store.numel(), 4)
        row["ratio_to_copy"] = round(row["device_ms"] / res["copy_ms"], 2)
        row["gpixel_per_s"] = round(store.numel() / row["device_ms"] / 1e6, 2)
        row["host_over_device"] = round(row["host_ms"] / row["device_ms"], 1)
        rows.append(row)
    res["rows"] = rows
    return res


def main():
    if "--step" in sys.argv:                                                  # a child: one workload, one JSON line
        print("RESULT " + json.dumps(step(arg("--step", ""))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "binarize.json"))
    results = []
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                                    # nothing more is started after a failure
            sys.exit(f"workload {name} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        results.append(json.loads(lines[-1][7:]))
        print(name, lines[-1][7:], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        commit_source = "git HEAD of the measured tree" + (", which had uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
        commit_source = "QEA_COMMIT (the measured tree was no git checkout): the commit the tree was based on"
    result = dict(
        commit=commit, commit_source=commit_source,
        method="device events around the launches alone (store, page table and output on the device before), median of 20 after 3 warm-ups; "
               "copy_: a device copy_ of the same uint8 store timed the same way; host_ms: host clock of binarize_pages on CPU tensors, one "
               "run; every workload in a process of its own",
        workloads=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(row["identical"] for r in results for row in r["rows"]), "the device and the host path differ"


if __name__ == "__main__":
    main()
