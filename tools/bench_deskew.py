"""What skew estimation and deskew (csrc/deskew.hip; qea/deskew.py) cost on the device, 8-bit grey pages in:
  workloads   docs64: 64 documents of 400 x 512 (the training canvas);  a4x8: 8 pages of 2480 x 3508: text-like blocks on a light noisy
              ground, every page sheared per column by its own slope k / 1024, k spread over -80..80
  sequences   estimate      strip sums + scores + pick at A = 90, ink = 127: three launches, nothing synchronises
              strip_sums    its first launch alone, the one pass over the pixels
              rotate        the one rotation launch, bilinear, 8-bit out, from the slopes the estimate left on the device
              deskew_pages  the whole product call on device pages (packing, the page table upload, Otsu's two launches for the ink,
                            the four launches, unpacking)
  device_ms   device events around the sequence (store and page table on the device before), median of 20 after 3 warm-ups
  copy_ms     the yardstick of the HBM-bound passes: a plain device copy_ of the same uint8 store, timed the same way
  host_ms     this module's host path (numpy) on the same pages, host clock, one run
  identical   whether the device result equals the host path's, bit for bit
Each workload runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/deskew.json.  GPU box only.   python tools/bench_deskew.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
WORKLOADS = {"docs64": [(400, 512)] * 64, "a4x8": [(2480, 3508)] * 8}
STEP_TIMEOUT = 420
A = 90


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


def _pages(torch, name):
    """-> (8-bit pages on the host, the slopes they were sheared by)"""
    import numpy as np
    g = torch.Generator().manual_seed(5)
    sizes = WORKLOADS[name]
    ks = [round(-80 + 160 * i / max(1, len(sizes) - 1)) for i in range(len(sizes))]
    pages = []
    for (h, w), k in zip(sizes, ks):
        page = torch.randint(170, 256, (h, w), generator=g, dtype=torch.uint8)
        ink = torch.rand(h // 24 + 1, w // 4 + 1, generator=g) < 0.4                # lines of 10 rows every 24, blocks of 4 columns
        mask = ink.repeat_interleave(24, 0).repeat_interleave(4, 1)[:h, :w] & ((torch.arange(h) % 24) < 10)[:, None]
        page[mask] = torch.randint(0, 90, (int(mask.sum()),), generator=g, dtype=torch.uint8)
        d = (k * (np.arange(w) - w // 2) + 512) // 1024                              # column x moves down by d[x]
        rows = np.arange(h)[:, None] - d[None, :]
        px = np.where((rows >= 0) & (rows < h), page.numpy()[np.clip(rows, 0, h - 1), np.arange(w)[None, :]], 255).astype(np.uint8)
        pages.append(torch.from_numpy(px))
    return pages, ks


def step(name):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    from qea import deskew, ops
    from qea.pages import pack_pages, unpack_pages
    assert torch.cuda.is_available(), "bench_deskew.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda")
    pages, ks = _pages(torch, name)
    pk = pack_pages(pages)
    store = pk.store.to(dev)
    table = ops.page_table(pk.offset, pk.h, pk.w, dev)
    dev_pages = unpack_pages(store, pk)
    copy = torch.empty_like(store)
    res = dict(workload=name, pages=len(pages), page_size=list(WORKLOADS[name][0]), pixels=int(store.numel()), max_slope=A, sheared_by=ks)
    res["copy_ms"] = _timed(torch, lambda: copy.copy_(store))
    res["copy_gb_per_s"] = round(2 * store.numel() / res["copy_ms"] / 1e6, 1)
    C = torch.empty(store.numel(), dtype=torch.uint8, device=dev)
    scores = torch.empty(len(pages), 2 * A + 1, dtype=torch.int64, device=dev)
    slopes = torch.empty(len(pages), dtype=torch.int32, device=dev)
    out = torch.empty_like(store)
    rot = torch.from_numpy(deskew.rotation_table(A)).to(dev)
    got = {}

    def estimate():
        ops.skew_strip_sums(store, table, 127, C=C)
        ops.skew_scores(C, table, A, scores=scores)
        ops.skew_pick(scores, 0, slopes=slopes)

    def whole():
        got["pages"], got["slopes"] = deskew.deskew_pages(dev_pages, A)
    t0 = time.perf_counter()
    want_slopes, want_scores = deskew.estimate_skew(pages, A, 127)
    host_estimate = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_rot, _ = deskew.deskew_pages(pages, A, slopes=want_slopes)
    host_rotate = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_pages, want_otsu_slopes = deskew.deskew_pages(pages, A)
    host_whole = (time.perf_counter() - t0) * 1e3
    res["slopes"] = want_slopes.tolist()
    rows = []
    for seq, fn, host_ms in (("estimate", estimate, host_estimate), ("strip_sums", lambda: ops.skew_strip_sums(store, table, 127, C=C), None),
                             ("rotate", lambda: ops.deskew_rotate(store, table, slopes, rot, "bilinear", 255, out_u8=out), host_rotate),
                             ("deskew_pages", whole, host_whole)):
        before = dict(ops.DESKEW_LAUNCHES)
        fn()
        row = dict(sequence=seq, launches=sum(ops.DESKEW_LAUNCHES.values()) - sum(before.values()), device_ms=_timed(torch, fn))
        if seq == "estimate":
            same = torch.equal(slopes.cpu(), want_slopes) and torch.equal(scores.cpu(), want_scores)
        elif seq == "rotate":
            same = all(torch.equal(a.cpu(), b) for a, b in zip(unpack_pages(out, pk), want_rot))
        elif seq == "deskew_pages":
            same = torch.equal(got["slopes"].cpu(), want_otsu_slopes) and all(torch.equal(a.cpu(), b) for a, b in zip(got["pages"], want_pages))
        else:
            same = None
        if same is not None:
            row["identical"] = bool(same)
        if host_ms is not None:
            row["host_ms"] = round(host_ms, 1)
            row["host_over_device"] = round(host_ms / row["device_ms"], 1)
        row["ratio_to_copy"] = round(row["device_ms"] / res["copy_ms"], 2)
        row["gpixel_per_s"] = round(store.numel() / row["device_ms"] / 1e6, 2)
        rows.append(row)
    res["rows"] = rows
    return res


def main():
    if "--step" in sys.argv:                                                  # a child: one workload, one JSON line
        print("RESULT " + json.dumps(step(arg("--step", ""))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "deskew.json"))
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
        method="device events around each sequence (store and page table on the device before), median of 20 after 3 warm-ups; deskew_pages "
               "is the whole product call on device pages, Otsu's two launches for the ink included; copy_: a device copy_ of the same uint8 "
               "store timed the same way; host_ms: host clock of this module's host path on CPU tensors, one run; every workload in a "
               "process of its own",
        workloads=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(row.get("identical", True) for r in results for row in r["rows"]), "the device and the host path differ"


if __name__ == "__main__":
    main()
