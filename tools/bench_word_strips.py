"""What cutting word boxes into CRNN strips (csrc/word_strips.hip; qea/reading.py) and reading them cost on the device.
  workloads   docs64: 64 documents of 400 x 512 with text 7..10 rows high (every box is copied 1:1);  a4x8: 8 pages of 2480 x 3508 with
              text 40..100 rows high (every box is shrunk).  Synthetic words (dark bars with light holes on a light noisy ground),
              binarised by Sauvola on the device, boxes from components.word_boxes: what clean_cli.py --method sauvola --boxes hands on
  per bucket  strips_ms  the ONE word_strips launch of the bucket's boxes, device events, median of 20 after 3 warm-ups
              copy_ms    the yardstick: a device copy_ of the same output bytes, timed the same way
              host_ms    this module's numpy host path on the same boxes, host clock, one run;  identical: device == host, bit for bit
  crop        the boxes of at most 32 rows, all at width 128: word_strips against the existing crop kernel (ops.crop_pad_gather, one launch
              per page, the boxes uploaded before), which writes identical strips there
  read        read_pages whole (strips, CRNN passes with default-init weights, decode, the strings back on the host), greedy and beam = 8:
              host clock around the call, median of 3 after 1 warm-up;  crnn_ms: device events around the CRNN passes alone on strips cut
              before;  strips_ms_total: the sum of the buckets' launches
Each workload runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/word_strips.json.  GPU box only.   python tools/bench_word_strips.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
WORKLOADS = {"docs64": dict(sizes=[(400, 512)] * 64, bar=(7, 11), pitch=24, word=(12, 90), gap=(10, 22)),
             "a4x8": dict(sizes=[(3508, 2480)] * 8, bar=(40, 101), pitch=150, word=(90, 520), gap=(45, 90))}
STEP_TIMEOUT = 540


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


def _wall(torch, fn, warmups=1, reps=3):
    ms = []
    for k in range(warmups + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmups:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 2)


def _pages(np, name):
    """8-bit pages: a light noisy ground, lines of words; a word is a dark bar with light holes"""
    w_ = WORKLOADS[name]
    rng = np.random.default_rng(9)
    pages = []
    for h, w in w_["sizes"]:
        page = rng.integers(190, 256, (h, w), dtype=np.uint8)
        y = w_["pitch"] // 3
        while y + w_["bar"][1] < h - 4:
            x = int(rng.integers(8, 40))
            while x + w_["word"][0] < w - 8:
                n, bar = int(rng.integers(*w_["word"])), int(rng.integers(*w_["bar"]))
                x1 = min(x + n, w - 8)
                word = rng.integers(0, 70, (bar, x1 - x), dtype=np.uint8)
                word[rng.random(word.shape) < 0.08] = 230
                page[y:y + bar, x:x1] = word
                x = x1 + int(rng.integers(*w_["gap"]))
            y += w_["pitch"]
        pages.append(page)
    return pages


def step(name):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import properties
    from models.model_crnn import CRNN
    from oracle import model_oracle as mo
    from qea import ops, reading
    from qea.binarize import binarize_pages
    from qea.components import word_boxes
    from qea.pages import norm_table, pack_pages
    from utils import get_char_maps
    assert torch.cuda.is_available(), "bench_word_strips.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda")
    pages = binarize_pages([torch.from_numpy(p) for p in _pages(np, name)], "sauvola", out="u8", device=dev)
    per_page = word_boxes(pages, gap_x=8 if name == "docs64" else 40, min_area=16)
    table = reading.box_table(per_page)
    host_pages = [p.cpu() for p in pages]
    pk = pack_pages(pages)
    store, ptable, norm = pk.store, ops.page_table(pk.offset, pk.h, pk.w, dev), norm_table().to(dev)
    plan = reading.strip_plan(table, pk.h, pk.w)
    heights = np.minimum(table[:, 4], pk.h[table[:, 0]]) - np.maximum(table[:, 2], 0)
    res = dict(workload=name, pages=len(pages), page_size=list(WORKLOADS[name]["sizes"][0]), boxes=len(table), cut=int(plan.cut.sum()),
               box_rows=dict(min=int(heights.min()), median=int(np.median(heights)), max=int(heights.max())), buckets=[])
    total = 0.0
    for OW in reading.default_buckets():
        rows = np.ascontiguousarray(table[plan.bucket == OW])
        if not len(rows):
            continue
        boxes = torch.from_numpy(rows).to(dev)
        out = torch.empty(len(rows), 1, 32, OW, device=dev)
        copy = torch.empty_like(out)
        row = dict(width=OW, strips=len(rows), shrunk=int((heights[plan.bucket == OW] > 32).sum()), out_mb=round(out.numel() * 4 / 1e6, 2))
        row["strips_ms"] = _timed(torch, lambda: ops.word_strips(store, ptable, boxes, OW, norm, out=out))
        row["copy_ms"] = _timed(torch, lambda: copy.copy_(out))
        row["ratio_to_copy"] = round(row["strips_ms"] / row["copy_ms"], 2)
        t0 = time.perf_counter()
        want = reading.word_strips(host_pages, rows, OW)
        row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["identical"] = bool(torch.equal(out.cpu(), want))
        total += row["strips_ms"]
        res["buckets"].append(row)
    res["strips_ms_total"] = round(total, 4)
    # the existing crop kernel where both write the same strips: ch <= 32, width 128, one launch per page for it
    small = np.ascontiguousarray(table[heights <= 32])
    if len(small):
        images = [norm[p.long()][None].contiguous() for p in pages]
        per = [torch.from_numpy(np.ascontiguousarray(small[small[:, 0] == p, 1:])).to(dev) for p in range(len(pages))]
        first = np.searchsorted(small[:, 0], np.arange(len(pages) + 1))
        boxes, out, crop = torch.from_numpy(small).to(dev), torch.empty(len(small), 1, 32, 128, device=dev), torch.empty(len(small), 1, 32, 128, device=dev)

        def crops():
            for p, (img, b) in enumerate(zip(images, per)):
                if len(b):
                    ops.crop_pad_gather(img, img.shape[1], img.shape[2], b, len(b), 32, 128, crop[first[p]:first[p + 1]])
        res["crop"] = dict(strips=len(small), width=128, word_strips_ms=_timed(torch, lambda: ops.word_strips(store, ptable, boxes, 128, norm, out=out)),
                           crop_kernel_ms=_timed(torch, crops), crop_kernel_launches=int(sum(len(b) > 0 for b in per)))
        res["crop"]["identical"] = bool(torch.equal(out, crop))
    # the whole reading
    model = CRNN(95, False)
    model.load_state_dict(mo.default_init_state(mo.crnn_state_shapes(), 6))
    model = model.to(dev).eval()
    index_to_char = get_char_maps(properties.char_set)[1]
    cutter = reading._Cutter(pages, dev)
    cut = {OW: cutter.strips(table[plan.bucket == OW], OW) for OW in {OW for OW, _ in plan.passes}}
    done = {}
    feeds = []
    for OW, idx in plan.passes:
        feeds.append(cut[OW][done.get(OW, 0):done.get(OW, 0) + len(idx)])
        done[OW] = done.get(OW, 0) + len(idx)

    def passes():
        with torch.no_grad():
            for x in feeds:
                model(x)
    res["read"] = dict(passes=len(feeds), crnn_ms=_timed(torch, passes, 2, 5),
                       greedy_ms=_wall(torch, lambda: reading.read_pages(model, pages, per_page, index_to_char)),
                       beam8_ms=_wall(torch, lambda: reading.read_pages(model, pages, per_page, index_to_char, beam=8)))
    res["read"]["strips_share_of_crnn"] = round(total / res["read"]["crnn_ms"], 4)
    return res


def main():
    if "--step" in sys.argv:                                                  # a child: one workload, one JSON line
        print("RESULT " + json.dumps(step(arg("--step", ""))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "word_strips.json"))
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
        method="device events around each launch (store, page table and boxes on the device before), median of 20 after 3 warm-ups; copy_: a "
               "device copy_ of the same output bytes timed the same way; host_ms: host clock of the numpy host path on CPU tensors, one run; "
               "crop: the existing crop kernel on the boxes of at most 32 rows, one launch per page; read: host clock around read_pages "
               "(default-init CRNN weights), median of 3 after 1 warm-up, crnn_ms: device events around the CRNN passes alone; every "
               "workload in a process of its own",
        workloads=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(row["identical"] for r in results for row in r["buckets"] + ([r["crop"]] if "crop" in r else [])), "the device paths differ"


if __name__ == "__main__":
    main()
