"""Time of one B = 2048 minibatch of text strips, (a) through the sample loader the trainers use without --resident (ImgDataset ->
PadWhite((32, 128)) -> float32 / 255 -> DataLoader(batch_size=2048), no workers, then the host-to-device copy) and (b) from the
device-resident store (datasets/resident.py: one launch of qea_strip_batch per batch).

The data: 4096 synthetic grey PNG strips in a temporary directory, heights 8-40 and widths 20-300 from a seeded generator (so about
a third take PadWhite's thumbnail branch).  (a) is a host clock around `next(iter(loader))` plus `.to(device)` and a synchronise,
with the files warm in the page cache (the whole set is read once before), median of --loader_reps batches.  (b) is the time between
two device events around `store.batch(idx)` (host index check, pinned staging, index copy and the kernel), 20 timed calls after 5
warm-ups, each call on fresh indices; the host clock around the same call with a synchronise at its end is reported next to it.  The
two batches are compared bit for bit on the same indices before anything is timed.
Writes profiles/resident_loader.json.  GPU box only.   python tools/bench_resident_loader.py [--out PATH] [--n N] [--batch B]"""
import json
import os
import platform
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
import properties  # noqa: E402
from datasets._io import to_tensor  # noqa: E402
from datasets.img_dataset import ImgDataset  # noqa: E402
from datasets.resident import ResidentStrips  # noqa: E402
from transform_helper import PadWhite  # noqa: E402


def arg(name, default):
    argv = sys.argv[1:]
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def write_strips(root, n, seed=7):
    from PIL import Image
    rng = np.random.RandomState(seed)
    for i in range(n):
        h, w = int(rng.randint(8, 41)), int(rng.randint(20, 301))
        a = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
        Image.fromarray(a, mode="L").save(os.path.join(root, f"{i}_w{i % 97}_s.png"))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    assert torch.cuda.is_available(), "bench_resident_loader.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = arg("--out", os.path.join(ROOT, "profiles", "resident_loader.json"))
    n, B, loader_reps = arg("--n", 4096), arg("--batch", 2048), arg("--loader_reps", 3)
    warmups, reps = 5, 20
    dev = torch.device("cuda")
    size = properties.input_size
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_strips(root, n)
        write_s = time.perf_counter() - t0
        pad = PadWhite(size)
        ds = ImgDataset(root, transform=lambda img: to_tensor(pad(img)), include_name=True, include_index=True)
        assert len(ds) == n
        store = ResidentStrips(ds, size, device=dev)                          # reads every file: the page cache is warm from here on
        torch.cuda.synchronize()
        gen = torch.Generator().manual_seed(1)
        # same indices through both paths, before any timing
        loader = torch.utils.data.DataLoader(ds, batch_size=B, drop_last=True, shuffle=True, generator=gen)
        images, labels, names, indices = next(iter(loader))
        got = store.batch(indices)
        identical = bool(torch.equal(got.cpu(), images)) and [store.names[i] for i in indices.tolist()] == list(names)
        # (a) the sample loader
        loader_ms = []
        for _ in range(loader_reps):
            it = iter(loader)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images = next(it)[0].to(dev)
            torch.cuda.synchronize()
            loader_ms.append((time.perf_counter() - t0) * 1e3)
        # (b) the resident store
        idxs = [torch.randint(0, n, (B,), generator=gen) for _ in range(warmups + reps)]
        ev_ms, host_ms = [], []
        for k, idx in enumerate(idxs):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            store.batch(idx)
            b.record()
            torch.cuda.synchronize()
            if k >= warmups:
                host_ms.append((time.perf_counter() - t0) * 1e3)
                ev_ms.append(a.elapsed_time(b))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        commit_source = "git HEAD of the measured tree" + (", which had uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
        commit_source = "QEA_COMMIT (the measured tree was no git checkout): the commit the tree was based on"
    a_ms, b_ms = statistics.median(loader_ms), statistics.median(ev_ms)
    out_bytes = B * size[0] * size[1] * 4
    result = dict(
        commit=commit, commit_source=commit_source, device=torch.cuda.get_device_name(0), host_cpu=cpu_model(), host_threads=torch.get_num_threads(),
        method="(a) host clock around next(iter(DataLoader)) + .to(device) + synchronise, files warm, median; (b) device events around "
               "one store.batch(idx) (index check, pinned staging, index copy, one kernel), median of the timed calls after the "
               "warm-ups; host_ms: host clock around the same call with a synchronise at its end; resident_end_to_end_gbps: the batch's "
               "bytes over (b), an end-to-end rate, not the kernel's bandwidth (the kernel alone was not timed)",
        strips=n, batch=B, size=list(size), batches_identical=identical,
        pack_bytes=store.nbytes, pack_build_s=round(store.build_seconds, 3), strips_write_s=round(write_s, 3),
        loader_ms=round(a_ms, 2), loader_ms_all=[round(v, 2) for v in loader_ms], loader_ms_per_image=round(a_ms / B, 4),
        resident_event_ms=round(b_ms, 4), resident_event_ms_min_max=[round(min(ev_ms), 4), round(max(ev_ms), 4)],
        resident_host_ms=round(statistics.median(host_ms), 4), warmups=warmups, timed_calls=reps,
        batch_bytes_written=out_bytes, resident_end_to_end_gbps=round(out_bytes / (b_ms * 1e-3) / 1e9, 1),
        ratio_loader_over_resident=round(a_ms / b_ms, 1), bound_ms=0.9, within_bound=bool(b_ms <= 0.9))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert identical, "the resident batch differs from the sample loader's"


if __name__ == "__main__":
    main()
