"""What connected-component labelling (csrc/components.hip; qea/components.py) costs on the device, 8-bit binarised pages in:
  workloads   docs64: 64 documents of 400 x 512 (the training canvas);  a4x8: 8 pages of 2480 x 3508, both the synthetic text of
              tools/bench_binarize.py binarised by Sauvola (window 25) on the device;  serpentine: ONE adversarial page of 1051 x 2057, every
              even row ink, the odd rows joined alternately at the last and first column: one component whose path crosses every tile border
  sequences   despeckle   label (3 launches) + stats + apply at min_area 4, connectivity 8, 8-bit out: nothing synchronises
              label       its first three launches alone
              word_boxes  smear (gap 8 along rows) + label of the mask + stats + the one read of the per-page counts + boxes
  device_ms   device events around the sequence (store and page table on the device before), median of 20 after 3 warm-ups; word_boxes
              contains its host read, so its figure is the call, not kernels alone
  copy_ms     the yardstick of the HBM-bound passes: a plain device copy_ of the same uint8 store, timed the same way
  host_ms     this module's host path (numpy runs and pointer jumping) on the same pages, host clock, one run
  identical   whether the device result equals the host path's, bit for bit
Each workload runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/components.json.  GPU box only.   python tools/bench_components.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
WORKLOADS = {"docs64": [(400, 512)] * 64, "a4x8": [(2480, 3508)] * 8, "serpentine": [(1051, 2057)]}
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


def _pages(torch, name):
    """8-bit binarised pages on the host"""
    if name == "serpentine":
        h, w = WORKLOADS[name][0]
        page = torch.full((h, w), 255, dtype=torch.uint8)
        page[0::2] = 0
        page[1::4, w - 1] = 0
        page[3::4, 0] = 0
        return [page]
    from qea.binarize import binarize_pages
    g = torch.Generator().manual_seed(5)
    pages = []
    for h, w in WORKLOADS[name]:                                # the text-like pages of tools/bench_binarize.py
        page = torch.randint(170, 256, (h, w), generator=g, dtype=torch.uint8)
        ink = torch.rand(h // 8 + 1, w // 4 + 1, generator=g) < 0.2
        mask = ink.repeat_interleave(8, 0).repeat_interleave(4, 1)[:h, :w]
        page[mask] = torch.randint(0, 90, (int(mask.sum()),), generator=g, dtype=torch.uint8)
        pages.append(page)
    return [p.cpu() for p in binarize_pages(pages, "sauvola", window=25, out="u8", device="cuda")]


def step(name):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    from qea import components, ops
    from qea.pages import pack_pages, unpack_pages
    assert torch.cuda.is_available(), "bench_components.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda")
    pages = _pages(torch, name)
    pk = pack_pages(pages)
    store = pk.store.to(dev)
    table = ops.page_table(pk.offset, pk.h, pk.w, dev)
    dev_pages = unpack_pages(store, pk)
    copy = torch.empty_like(store)
    res = dict(workload=name, pages=len(pages), page_size=list(WORKLOADS[name][0]), pixels=int(store.numel()),
               ink_share=round(float((store == 0).sum()) / store.numel(), 4))
    res["copy_ms"] = _timed(torch, lambda: copy.copy_(store))
    res["copy_gb_per_s"] = round(2 * store.numel() / res["copy_ms"] / 1e6, 1)
    labels = torch.empty(store.numel(), dtype=torch.int32, device=dev)
    got = {}

    def despeckle():
        got["despeckle"] = components.despeckle_store(store, table, 4, 8, out="u8")

    def word_boxes():
        got["boxes"] = components.word_boxes(dev_pages, gap_x=8, gap_y=0, min_area=16)
    rows = []
    for seq, fn in (("label", lambda: ops.cc_label(store, table, 8, 127, labels=labels)), ("despeckle", despeckle), ("word_boxes", word_boxes)):
        before = dict(ops.COMPONENT_LAUNCHES)
        fn()
        launches = sum(ops.COMPONENT_LAUNCHES.values()) - sum(before.values())
        row = dict(sequence=seq, launches=launches, device_ms=_timed(torch, fn))
        t0 = time.perf_counter()
        if seq == "label":
            want = components.label_pages(pages, 8)
            same = all(torch.equal(a.cpu(), b) for a, b in zip(unpack_pages(labels, pk), want))
            row["components"] = int(sum(int((b.reshape(-1) == torch.arange(b.numel(), dtype=torch.int32)).sum()) for b in want))
        elif seq == "despeckle":
            want = components.despeckle_pages(pages, 4, 8, out="u8")
            same = all(torch.equal(a.cpu(), b) for a, b in zip(unpack_pages(got["despeckle"], pk), want))
            row["ink_removed"] = int(sum(int(((b != 0) & (p == 0)).sum()) for b, p in zip(want, pages)))
        else:
            want = components.word_boxes(pages, gap_x=8, gap_y=0, min_area=16)
            same = all(torch.equal(a.cpu(), b) for a, b in zip(got["boxes"], want))
            row["boxes"] = int(sum(len(b) for b in want))
        row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["identical"] = bool(same)
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
    out = arg("--out", os.path.join(ROOT, "profiles", "components.json"))
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
    text = {r["workload"]: {row["sequence"]: row["device_ms"] for row in r["rows"]} for r in results}
    slow = {s: round(text["serpentine"][s] / results[2]["pixels"] / (text["a4x8"][s] / results[1]["pixels"]), 1) for s in text["a4x8"]}
    result = dict(
        commit=commit, commit_source=commit_source,
        method="device events around each sequence (store and page table on the device before), median of 20 after 3 warm-ups; word_boxes "
               "contains its one host read of the per-page counts; copy_: a device copy_ of the same uint8 store timed the same way; host_ms: "
               "host clock of this module's host path on CPU tensors, one run; every workload in a process of its own",
        serpentine_time_per_pixel_over_a4_text=slow, workloads=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(row["identical"] for r in results for row in r["rows"]), "the device and the host path differ"


if __name__ == "__main__":
    main()
