"""Time of one label-history weighted CTC loss plus backward (tracking_utils.weighted_ctc_loss) at the area trainer's Phase-A size:
n = 1946 strips (0.95 x 2048), T = 31, the CRNN's class count, W = 5, ragged depths, labels of 3-12 characters.  The fused call
(csrc/ctc_history.hip) against the loop over the depths (QEA_HISTORY_CTC=steps, the code before the fused call existed), same
process, same inputs, the two alternating in blocks of calls.  Each call (packing, copies, forward, backward) sits between two
device events; the host clock around the same call with a synchronise at its end is reported next to it.  Medians after a warm-up of
both paths.  Also: launches per fused call, and the largest difference of loss and gradient between the two paths.
Writes profiles/history_ctc.json.  GPU box only.   python tools/bench_history_ctc.py [--out PATH] [--n N] [--rounds R] [--reps K]"""
import json
import os
import statistics
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
import properties  # noqa: E402
import tracking_utils as tu  # noqa: E402
from qea import ops  # noqa: E402
from qea.loss import CTCLoss  # noqa: E402


def arg(name, default):
    argv = sys.argv[1:]
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def setup(n, W, form, seed=5):
    rng = np.random.RandomState(seed)
    chars = properties.char_set[1:]
    names = [f"s{i}" for i in range(n)]
    hist = {nm: ["".join(rng.choice(chars, rng.randint(3, 13))) for _ in range(1 + (i * 7 + i // 5) % W)] for i, nm in enumerate(names)}
    c2i = {c: i for i, c in enumerate(properties.char_set)}
    self = types.SimpleNamespace(char_to_index=c2i, window_size=W, tracked_labels=hist, weightgen_method=form, device=torch.device("cuda"),
                                 primary_loss_fn=CTCLoss(), primary_loss_fn_sample_wise=CTCLoss(reduction="none"))
    if form == "decaying":
        w = torch.tensor([0.7 ** i for i in range(W)]).cuda()
    else:
        w = torch.rand(n, W + 1, generator=torch.Generator().manual_seed(seed)).cuda()
    return self, names, w


def one_call(self, scores, pred, batches, w):
    scores.grad = None
    loss = tu.weighted_ctc_loss(self, scores, pred, batches, w)
    loss.backward()
    return loss


def timed(self, scores, pred, batches, w, mode, reps):
    os.environ["QEA_HISTORY_CTC"] = mode
    ev_ms, host_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        one_call(self, scores, pred, batches, w)
        b.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(a.elapsed_time(b))
    return ev_ms, host_ms


def main():
    assert torch.cuda.is_available(), "bench_history_ctc.py times the device path: it needs an MI355X"
    out = arg("--out", os.path.join(ROOT, "profiles", "history_ctc.json"))
    n, W, T, C = arg("--n", 1946), 5, 31, len(properties.char_set)
    rounds, reps = arg("--rounds", 5), arg("--reps", 20)
    rows = []
    for form in ("levenshtein", "decaying"):
        self, names, w = setup(n, W, form)
        batches = tu.generate_ctc_target_batches(self, names)
        pred = torch.full((n,), T, dtype=torch.int)
        scores = torch.randn(T, n, C, generator=torch.Generator().manual_seed(1)).log_softmax(2).cuda().requires_grad_(True)
        res = {}
        for mode in ("fused", "steps"):                          # warm-up of both paths, and their results on the same input
            os.environ["QEA_HISTORY_CTC"] = mode
            before = ops.HISTORY_CTC_LAUNCHES["ctc"]
            for _ in range(3):
                loss = one_call(self, scores, pred, batches, w)
            res[mode] = (loss.item(), scores.grad.clone(), (ops.HISTORY_CTC_LAUNCHES["ctc"] - before) // 3)
        ev = {"fused": [], "steps": []}
        host = {"fused": [], "steps": []}
        for _ in range(rounds):
            for mode in ("fused", "steps"):
                e, h = timed(self, scores, pred, batches, w, mode, reps)
                ev[mode] += e
                host[mode] += h
        g_f, g_s = res["fused"][1].double(), res["steps"][1].double()
        row = dict(weights="sample-wise table" if form != "decaying" else "decaying vector", n=n, T=T, C=C, window=W,
                   depth_n=[len(b[2]) for b in batches], calls_per_path=rounds * reps,
                   fused_event_ms=round(statistics.median(ev["fused"]), 4), steps_event_ms=round(statistics.median(ev["steps"]), 4),
                   fused_event_ms_min_max=[round(min(ev["fused"]), 4), round(max(ev["fused"]), 4)],
                   steps_event_ms_min_max=[round(min(ev["steps"]), 4), round(max(ev["steps"]), 4)],
                   fused_host_ms=round(statistics.median(host["fused"]), 4), steps_host_ms=round(statistics.median(host["steps"]), 4),
                   fused_launches_per_call=res["fused"][2], steps_fused_launches_per_call=res["steps"][2],
                   loss_fused=res["fused"][0], loss_steps=res["steps"][0],
                   grad_rel_diff=((g_f - g_s).norm() / g_s.norm()).item())
        row["ratio_steps_over_fused"] = round(row["steps_event_ms"] / row["fused_event_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.environ.pop("QEA_HISTORY_CTC", None)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method="device events around one weighted_ctc_loss + backward (host packing and copies included), median over "
                         "rounds x reps calls after a warm-up, the two paths alternating per round; host_ms: host clock around the "
                         "same call with a synchronise at its end", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, rows=len(rows))))


if __name__ == "__main__":
    main()
