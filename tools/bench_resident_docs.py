"""Time per step of building a batch of documents and cutting its text strips, (a) through the sample loader patch_cli.py uses without
--resident (PatchDataset -> DataLoader(collate_fn=PatchDataset.collate), no workers -> .to(device) -> utils.get_text_stack per
document -> torch.cat) and (b) from the device-resident store (datasets/resident.py: ResidentDocLoader -> utils.get_text_stacks: one
launch for the batch, one for all strips), at --docs_per_step 1 and 8; and, separately, the device time of N x (qea_crop_pad_gather,
memset + qea_crop_pad_scatter) against the two launches of csrc/doc_crops.hip on the same documents and gradients.

The data: 64 generated grey PNG documents in a temporary directory, 200-400 rows by 200-512 columns, 20-60 word boxes each (seeded).
The strips are cut from the loaded images themselves (the cleaner between the two is the same on both paths and is left out).
  loader steps   host clock from `next(iterator)` to a synchronise after the cut, files warm in the page cache, median over the steps
                 of two epochs after a warm-up epoch; both paths draw the same index batches (same seed) and are compared bit for bit
  crops steps    device events around the forward and backward launches, boxes and tables uploaded before, median of 20 after 5 warm-ups
Every step that touches the device runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/resident_docs.json.  GPU box only.   python tools/bench_resident_docs.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
N_DOCS, OUT = 64, (32, 128)
STEP_TIMEOUT = 240


def arg(name, default):
    argv = sys.argv[1:]
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def write_documents(root, seed=7):
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    letters = list("abcdefghijkmnopqrstuvwxyz23456789")
    for i in range(N_DOCS):
        h, w = int(rng.randint(200, 401)), int(rng.randint(200, 513))
        Image.fromarray(rng.randint(0, 256, size=(h, w)).astype(np.uint8), mode="L").save(os.path.join(root, f"doc_{i:03d}.png"))
        boxes = []
        for _ in range(int(rng.randint(20, 61))):
            bw, bh = int(rng.randint(10, 128)), int(rng.randint(6, 32))
            x, y = int(rng.randint(0, w - bw)), int(rng.randint(0, h - bh))
            boxes.append({"label": "".join(rng.choice(letters, rng.randint(2, 9))), "x_min": x, "y_min": y, "x_max": x + bw, "y_max": y + bh})
        with open(os.path.join(root, f"doc_{i:03d}.json"), "w") as f:
            json.dump(boxes, f)


def _setup(root):
    sys.path.insert(0, PKG)
    import torch
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    assert torch.cuda.is_available(), "bench_resident_docs.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ds = PatchDataset(root, pad=True, include_name=True)
    assert len(ds) == N_DOCS
    return torch, ds, ResidentDocuments(ds, device="cuda")                    # reads every file: the page cache is warm from here on


def step_loader(root, n):
    """ms per step of batch + strips, sample loader against resident loader, at n documents per step."""
    torch, ds, store = _setup(root)
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocLoader
    from utils import get_text_stack, get_text_stacks
    dev = torch.device("cuda")

    def sample_step(it):
        images, box_lists, _ = next(it)
        images = images.to(dev)
        return torch.cat([get_text_stack(images[i], box_lists[i], OUT)[0] for i in range(len(box_lists))])

    def resident_step(it):
        images, box_lists, _ = next(it)
        return get_text_stacks(images, box_lists, OUT)[0]

    def run(loader, step):
        torch.manual_seed(3)
        ms, crops = [], []
        for epoch in range(3):
            it = iter(loader)
            for _ in range(len(loader)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = step(it)
                torch.cuda.synchronize()
                if epoch:
                    ms.append((time.perf_counter() - t0) * 1e3)
                else:
                    crops.append(c.cpu())
        return ms, crops

    kw = dict(batch_size=n, drop_last=True, shuffle=True)
    a_ms, a_crops = run(torch.utils.data.DataLoader(ds, collate_fn=PatchDataset.collate, **kw), sample_step)
    b_ms, b_crops = run(ResidentDocLoader(ds, store, **kw), resident_step)
    identical = len(a_crops) == len(b_crops) and all(torch.equal(x, y) for x, y in zip(a_crops, b_crops))
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    return dict(docs_per_step=n, steps_timed=len(a_ms), strips_per_step=round(sum(len(c) for c in a_crops) / len(a_crops), 1),
                sample_loader_ms=round(a, 3), sample_loader_ms_min_max=[round(min(a_ms), 3), round(max(a_ms), 3)],
                resident_ms=round(b, 4), resident_ms_min_max=[round(min(b_ms), 4), round(max(b_ms), 4)],
                ratio_sample_over_resident=round(a / b, 1), strips_identical=identical, pack_bytes=store.nbytes,
                pack_build_s=round(store.build_seconds, 3))


def step_crops(root, n):
    """device ms of n x (gather, memset + atomic scatter) against the two launches of csrc/doc_crops.hip, forward and backward."""
    torch, ds, store = _setup(root)
    from qea import ops
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(5)
    rows = torch.randperm(N_DOCS, generator=gen)[:n].tolist()
    x = store.batch(rows)
    H, W = store.H, store.W
    doc, first = store.strip_tables(rows)
    S = int(first[-1])
    d_doc, d_first = torch.from_numpy(doc).to(dev), torch.from_numpy(first).to(dev)
    lo = store._host_box_first
    boxes = [store.box[int(lo[r]): int(lo[r + 1])].contiguous() for r in rows]
    dout = torch.randint(-8, 9, (S, 1) + OUT, generator=gen).float().to(dev)  # integers: both backward forms give the same bits
    douts = [dout[int(first[i]): int(first[i + 1])].contiguous() for i in range(n)]
    out_new, dimg_new = torch.empty(S, 1, *OUT, device=dev), torch.empty(n, 1, H, W, device=dev)
    outs_old = [torch.empty(len(b), 1, *OUT, device=dev) for b in boxes]
    dimg_old = torch.empty(n, 1, H, W, device=dev)

    def old_fwd():
        for i in range(n):
            ops.crop_pad_gather(x[i], H, W, boxes[i], len(boxes[i]), OUT[0], OUT[1], outs_old[i])

    def old_bwd():
        for i in range(n):
            dimg_old[i].zero_()
            ops.crop_pad_scatter(douts[i], boxes[i], len(boxes[i]), OUT[0], OUT[1], dimg_old[i], H, W)

    def new_fwd():
        ops.doc_crops_gather(x, store.box, store.box_first, d_doc, d_first, out_new)

    def new_bwd():
        ops.doc_crops_scatter(dout, store.box, store.box_first, d_doc, d_first, dimg_new)

    def timed(fn, warmups=5, reps=20):
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

    res = dict(docs=n, strips=S, old_gather_ms=timed(old_fwd), new_gather_ms=timed(new_fwd), old_memset_scatter_ms=timed(old_bwd),
               new_scatter_ms=timed(new_bwd))
    res["identical"] = bool(torch.equal(torch.cat(outs_old), out_new) and torch.equal(dimg_old, dimg_new))
    res["ratio_old_over_new_forward"] = round(res["old_gather_ms"] / res["new_gather_ms"], 2)
    res["ratio_old_over_new_backward"] = round(res["old_memset_scatter_ms"] / res["new_scatter_ms"], 2)
    return res


def main():
    if "--step" in sys.argv:                                                  # a child: one device step, one JSON line
        fn = {"loader": step_loader, "crops": step_crops}[arg("--step", "")]
        print("RESULT " + json.dumps(fn(arg("--root", ""), arg("--n", 1))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "resident_docs.json"))
    results = {"loader": [], "crops": []}
    with tempfile.TemporaryDirectory() as root:
        write_documents(root)
        for step in ("loader", "crops"):
            for n in (1, 8):
                cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", step, "--root", root,
                       "--n", str(n)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not lines:                            # nothing more is started after a failure
                    sys.exit(f"step {step} n={n} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
                results[step].append(json.loads(lines[-1][7:]))
                print(step, n, lines[-1][7:], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        commit_source = "git HEAD of the measured tree" + (", which had uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
        commit_source = "QEA_COMMIT (the measured tree was no git checkout): the commit the tree was based on"
    result = dict(
        commit=commit, commit_source=commit_source, documents=N_DOCS, strip_size=list(OUT),
        method="loader: host clock from next(iterator) to a synchronise after the strips are cut, files warm, median over the steps of two "
               "epochs after a warm-up epoch, no cleaner in between, the same index batches on both paths; crops: device events around "
               "the launches alone (boxes, tables and gradients on the device before), median of 20 after 5 warm-ups; every step in a "
               "process of its own",
        loader=results["loader"], crops=results["crops"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(r["strips_identical"] for r in results["loader"]) and all(r["identical"] for r in results["crops"]), "the two paths differ"


if __name__ == "__main__":
    main()
