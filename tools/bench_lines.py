"""What grouping word boxes into text lines (csrc/lines.hip; qea/lines.py) costs on the device, beside the word_boxes call that feeds it:
  workloads   docs64 and a4x8: the two standing workloads of tools/bench_components.py (its synthetic text, Sauvola-binarised on the
              device), boxes by word_boxes(gap_x=8, min_area=16) on the device.  The synthetic A4 pages are block noise, not words: each
              holds far more than the 4096 boxes a page may have, so a4x8 groups the FIRST 4096 boxes of every page (boxes_found and
              boxes_used say how many were cut); docs64 is used whole.
              text4096: ONE page of 4096 word-like boxes in lines 40 rows apart, shuffled.
              chain4096: ONE adversarial page, 4096 boxes each overlapping the next by exactly the threshold: one line, the longest chain
              of links there is.
  kernel_ms   device events around qea_line_group alone, called through the C ABI into buffers allocated before
  call_ms     device events around the whole group_lines call on the device tables: one torch.cat, the upload of box_first, the launch,
              and the one read of the line counts, which synchronises
  word_boxes_ms  the same around components.word_boxes on the same pages (docs64, a4x8), which also ends in its one read
  copy_ms     a plain device copy_ of the int32 box table, the smallest thing one can do to it
  host_ms     the numpy host path of qea/lines.py on the same tables, host clock, one run
  identical   whether the device result equals the host path's, bit for bit
Device figures are medians of 20 after 3 warm-ups.  Each workload runs in a child process of its own under `timeout`; the first failure
stops the script.  Writes profiles/lines.json.  GPU box only.   python tools/bench_lines.py [--out PATH]"""
import json
import os
import subprocess
import sys
import time

from bench_components import PKG, ROOT, STEP_TIMEOUT, _pages, _timed, arg

WORKLOADS = ["docs64", "a4x8", "text4096", "chain4096"]


def _made_page(name):
    """the two pages that are built, not found: int32 [4096, 4] on the host"""
    import numpy as np
    if name == "chain4096":
        i = np.arange(4096)
        return np.stack([30 * i, 10 * i, 30 * i + 24, 10 * i + 19], 1).astype(np.int32)
    g = np.random.default_rng(9)
    rows, x, y = [], 0, 20
    while len(rows) < 4096:
        ww = int(g.integers(12, 140))
        rows.append((x, y - int(g.integers(0, 8)), x + ww - 1, y + 19 + int(g.integers(0, 7))))
        x += ww + int(g.integers(6, 25))
        if x > 3000:
            x, y = int(g.integers(0, 60)), y + 40
    return g.permutation(np.asarray(rows, np.int32))


def step(name):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    from qea import _lib, components, lines, ops
    assert torch.cuda.is_available(), "bench_lines.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = dict(workload=name)
    if name in ("docs64", "a4x8"):
        dev_pages = [p.cuda() for p in _pages(torch, name)]
        found = components.word_boxes(dev_pages, gap_x=8, gap_y=0, min_area=16)
        res["word_boxes_ms"] = _timed(torch, lambda: components.word_boxes(dev_pages, gap_x=8, gap_y=0, min_area=16))
        res["boxes_found"] = [len(b) for b in found]
        tables = [b[:lines.MAX_BOXES].contiguous() for b in found]
    else:
        tables = [torch.from_numpy(_made_page(name)).cuda()]
    counts = [len(t) for t in tables]
    res.update(pages=len(tables), boxes_used=sum(counts), largest_page=max(counts))
    table = torch.cat(tables)
    first = torch.tensor([0] + [sum(counts[:k + 1]) for k in range(len(counts))], dtype=torch.int32).cuda()
    copy = torch.empty_like(table)
    res["copy_ms"] = _timed(torch, lambda: copy.copy_(table))
    out = ops.line_group(table, first, max(counts))             # the buffers of the bare launch, and the first result
    L = _lib.lib()

    def launch():
        _lib.check(L.qea_line_group(table.data_ptr(), first.data_ptr(), len(counts), len(table), max(counts), 50, 3, 0,
                                    *(t.data_ptr() for t in out), torch.cuda.current_stream().cuda_stream), "qea_line_group")
    res["kernel_ms"] = _timed(torch, launch)
    got = {}

    def call():
        got["lines"] = lines.group_lines(tables)
    res["call_ms"] = _timed(torch, call)
    on_host = [t.cpu() for t in tables]
    t0 = time.perf_counter()
    want = lines.group_lines(on_host)
    res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["identical"] = all(torch.equal(a.cpu(), b) for g, w in zip(got["lines"], want) for a, b in zip(g, w))
    res["lines"] = int(sum(len(lb) for _, _, lb in want))
    res["host_over_call"] = round(res["host_ms"] / res["call_ms"], 1)
    if "word_boxes_ms" in res:
        res["kernel_over_word_boxes"] = round(res["kernel_ms"] / res["word_boxes_ms"], 3)
        res["call_over_word_boxes"] = round(res["call_ms"] / res["word_boxes_ms"], 3)
    return res


def main():
    if "--step" in sys.argv:                                                  # a child: one workload, one JSON line
        print("RESULT " + json.dumps(step(arg("--step", ""))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "lines.json"))
    results = []
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        found = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not found:                                    # nothing more is started after a failure
            sys.exit(f"workload {name} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        results.append(json.loads(found[-1][7:]))
        print(name, found[-1][7:], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        commit_source = "git HEAD of the measured tree" + (", which had uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
        commit_source = "QEA_COMMIT (the measured tree was no git checkout): the commit the tree was based on"
    import socket
    import torch
    result = dict(
        commit=commit, commit_source=commit_source, box=socket.gethostname(), device=torch.cuda.get_device_name(0),
        method="device events around each item (tables on the device before), median of 20 after 3 warm-ups; kernel_ms: qea_line_group alone "
               "through the C ABI into buffers allocated before; call_ms: the whole group_lines call with its one host read; word_boxes_ms: "
               "components.word_boxes on the same pages, which also ends in a host read; copy_ms: a device copy_ of the box table; host_ms: "
               "host clock of the numpy host path on CPU tables, one run; every workload in a process of its own",
        workloads=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(r["identical"] for r in results), "the device and the host path differ"


if __name__ == "__main__":
    main()
