"""What the tiled whole-page pass (qea/pages.py: clean_pages) spends where, on one A4-class page (3508 rows x 2480 columns, 8-bit,
synthetic) and on a batch of eight 900 x 1200 pages, with the default 1024 x 1024 tile and the default pixels per pass:
  cut + paste, kernels   device ms of one qea_page_tiles_gather + one qea_page_tiles_scatter per chunk (csrc/page_tiles.hip), the cut tiles
                         pasted straight back (the cleaner between the two is timed on its own)
  cut + paste, torch     the same cut and paste as torch slicing, stack and copy_ per tile on the device (tiles_gather_spec /
                         tiles_scatter_spec of qea/pages.py, the specification path), and whether both give the same bits
  unet                   device ms of the eval-mode no-grad UNet passes over the same chunks (f = 32, seeded weights)
  clean_pages            host clock of the whole call, upload, planning and tables included, synchronised
device events, median of 10 after 3 warm-ups.  A third step measures the deviations of tests/test_pages_gpu.py's whole-path test: the
whole-page device pass and the tiled pass (T = 320) over a 437 x 531 page, each against the fp64 oracle's pass over the padded page.
Every step runs in a child process of its own under `timeout`; the first failure stops the script.
Writes profiles/page_tiles.json.  GPU box only.   python tools/bench_page_tiles.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd")
CASES = {"a4": [(3508, 2480)], "batch8": [(900, 1200)] * 8}
TILE = (1024, 1024)
STEP_TIMEOUT = 300


def arg(name, default):
    argv = sys.argv[1:]
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def _setup(seed):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    from models.model_unet import UNet
    from oracle import model_oracle as mo
    assert torch.cuda.is_available(), "bench_page_tiles.py times the device path: it needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = UNet()
    model.load_state_dict(mo.seeded_state(mo.unet_state_shapes(), seed))
    return torch, mo, model.cuda().eval()


def _timed(torch, fn, warmups=3, reps=10):
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


def step_case(name):
    torch, _, model = _setup(1)
    from qea import ops, pages as pg
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    pages = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in CASES[name]]
    pk = pg.pack_pages(pages)
    store, table = pk.store.to(dev), pg.norm_table().to(dev)
    offset, h, w = (torch.from_numpy(a).to(dev) for a in (pk.offset, pk.h, pk.w))
    chunks = []                                           # (TH, TW, host rows, device rows [n][7], device rows [n][3], tiles)
    for (TH, TW), rows in pg.plan_groups(pk.h, pk.w, TILE).items():
        step = max(1, pg.MAX_TILE_PIXELS // (TH * TW))
        for i in range(0, len(rows), step):
            r7 = torch.from_numpy(rows[i:i + step]).to(dev)
            chunks.append((TH, TW, rows[i:i + step], r7, r7[:, :3].contiguous(), torch.empty(len(r7), 1, TH, TW, device=dev)))
    res_k, res_t = torch.empty(store.numel(), device=dev), torch.empty(store.numel(), device=dev)

    def kernels():
        for TH, TW, _, r7, r3, x in chunks:
            ops.page_tiles_gather(store, offset, h, w, r3, x, table)
            ops.page_tiles_scatter(x, r7, offset, h, w, out_f32=res_k)

    def torch_ops():
        for TH, TW, rows, _, _, _ in chunks:
            x = pg.tiles_gather_spec(store, pk.offset, pk.h, pk.w, rows, TH, TW, table)
            pg.tiles_scatter_spec(x, rows, pk.offset, pk.h, pk.w, out_f=res_t)

    def unet():
        with torch.no_grad():
            for _, _, _, _, _, x in chunks:
                model(x)

    res = dict(case=name, pages=[list(s) for s in CASES[name]], tile=list(TILE), tiles=sum(len(c[2]) for c in chunks),
               tile_shapes=sorted({f"{c[0]}x{c[1]}" for c in chunks}), passes=len(chunks), page_pixels=int(store.numel()),
               tile_pixels=int(sum(c[5].numel() for c in chunks)))
    res["cut_paste_kernels_ms"] = _timed(torch, kernels)
    res["cut_paste_torch_ms"] = _timed(torch, torch_ops)
    res["identical"] = bool(torch.equal(res_k, res_t))
    res["unet_ms"] = _timed(torch, unet, warmups=2, reps=5)
    wall = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pg.clean_pages(model, pages, tile=TILE, out="u8")
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["clean_pages_host_ms"] = round(statistics.median(wall[1:]), 3)
    res["ratio_torch_over_kernels"] = round(res["cut_paste_torch_ms"] / res["cut_paste_kernels_ms"], 1)
    res["kernels_share_of_unet_percent"] = round(100 * res["cut_paste_kernels_ms"] / res["unet_ms"], 2)
    return res


def step_deviation(_):
    torch, mo, model = _setup(1)
    from qea.pages import clean_pages
    hh, ww = 437, 531
    page = torch.rand(hh, ww, generator=torch.Generator().manual_seed(7))           # the page of the test
    padded = torch.ones(1, 1, 448, 544)
    padded[0, 0, :hh, :ww] = page
    P, Bf = mo.split_state({k: v.double() if v.is_floating_point() else v for k, v in mo.seeded_state(mo.unet_state_shapes(), 1).items()},
                           requires_grad=False)
    with torch.no_grad():
        want = mo.unet_forward(P, Bf, padded.double(), training=False)[0, 0]
        whole = (model(padded.cuda())[0, 0].double().cpu() - want).abs().max().item()
    tiled = (clean_pages(model, [page], tile=(320, 320))[0].double().cpu() - want[:hh, :ww]).abs().max().item()
    return dict(page=[hh, ww], tile=[320, 320], tiles=6, whole_page_device_pass_vs_fp64_oracle=whole, tiled_pass_vs_fp64_oracle=tiled,
                bound_of_the_test=2 * whole + 1e-6)


def main():
    if "--step" in sys.argv:                                                  # a child: one device step, one JSON line
        fn = {"case": step_case, "deviation": step_deviation}[arg("--step", "")]
        print("RESULT " + json.dumps(fn(arg("--name", ""))))
        return
    out = arg("--out", os.path.join(ROOT, "profiles", "page_tiles.json"))
    results = []
    for step, name in (("deviation", "-"), ("case", "a4"), ("case", "batch8")):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", step, "--name", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                                    # nothing more is started after a failure
            sys.exit(f"step {step} {name} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        results.append(json.loads(lines[-1][7:]))
        print(step, name, lines[-1][7:], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        commit_source = "git HEAD of the measured tree" + (", which had uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
        commit_source = "QEA_COMMIT (the measured tree was no git checkout): the commit the tree was based on"
    result = dict(
        commit=commit, commit_source=commit_source,
        method="device events around the launches alone (pages, tables and tiles on the device before), median of 10 after 3 warm-ups (the "
               "UNet passes: 5 after 2); clean_pages: host clock of the whole call, synchronised, median of 3 after one warm-up; every step "
               "in a process of its own",
        deviation=results[0], cases=results[1:])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert all(r["identical"] for r in results[1:]), "the kernels and the torch path differ"


if __name__ == "__main__":
    main()
