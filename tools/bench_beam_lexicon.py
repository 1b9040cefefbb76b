"""Time of the automaton-constrained CTC prefix beam search (csrc/ctc_beam.hip, qea_ctc_beam_decode_dfa) beside the plain kernel of the
same library, same process, same box, with the method and the seeded inputs of tools/bench_beam_decode.py, at
(T, N, C, K) = (31, 2048, 95, 8) and (31, 2048, 95, 32):
  plain      qea.ops.ctc_beam_decode
  dfa        qea.ops.ctc_beam_decode_dfa with the trie of 1 000 synthetic words, the trie of about 90 000 (lower-case words of 3..12
             letters, seeded; duplicates merge) and the one-state automaton that accepts everything
  fused      qea.ops.ctc_beam_decode_lm at context m = 0, 1, 2 (the tables of tools/bench_beam_lm.py), only to see whether it moved
device events around LAUNCHES back-to-back launches; a round times one such window of every variant in turn, so the variants alternate;
per-launch time = the median of REPS rounds after a warm-up round, the window spread (min, max) is reported with every figure, and
the ratio dfa / plain.  The plain and fused figures are also set against profiles/beam_decode.json and profiles/beam_lm.json (ratios
this run / that file) where those files are present.
Writes profiles/beam_lexicon.json.  GPU box only.   python tools/bench_beam_lexicon.py [--out PATH]"""
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))
import properties  # noqa: E402
from qea import ops  # noqa: E402
from qea.lexicon import Lexicon  # noqa: E402
from utils import get_char_maps  # noqa: E402

SHAPES = ((31, 2048, 95, 8), (31, 2048, 95, 32))
LAUNCHES, REPS = 20, 9


def alternating_ms(fns):
    """{name: (median, min, max)} per-launch milliseconds over REPS rounds, each round one window of LAUNCHES launches per variant in turn,
    after one warm-up round"""
    ts = {name: [] for name in fns}
    for _ in range(REPS + 1):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) / LAUNCHES)
    return {name: (statistics.median(t[1:]), min(t[1:]), max(t[1:])) for name, t in ts.items()}


def synthetic_words(n, seed):
    rng = np.random.RandomState(seed)
    letters = "abcdefghijklmnopqrstuvwxyz"
    return ["".join(letters[i] for i in rng.randint(0, 26, rng.randint(3, 13))) for _ in range(n)]


def lexicons(char_to_index, C):
    classes = np.arange(1, C)
    vocabulary = [None] * C
    for ch, i in char_to_index.items():
        vocabulary[i] = ch
    return {"trie_1000": Lexicon.from_words(synthetic_words(1000, 1), char_to_index), "trie_90000": Lexicon.from_words(synthetic_words(90000, 2), char_to_index),
            "accept_all": Lexicon.from_automaton([0, C - 1], classes, np.zeros(C - 1, dtype=np.int64), [1], vocabulary)}


def figures(prefix, t):
    return {f"{prefix}_ms": round(t[0], 4), f"{prefix}_ms_min": round(t[1], 4), f"{prefix}_ms_max": round(t[2], 4),
            f"{prefix}_spread": round((t[2] - t[1]) / t[0], 4)}


def time_shape(T, N, C, K, dev, lex):
    g = torch.Generator().manual_seed(T * 1000 + K)
    x = torch.randn(T, N, C, generator=g) * 2
    x[:, :, 0] += 2
    d = torch.log_softmax(x, dim=2).to(dev)
    fns = {"plain": lambda: ops.ctc_beam_decode(d, K)}
    for name, lexicon in lex.items():
        fns[f"dfa_{name}"] = (lambda a: lambda: ops.ctc_beam_decode_dfa(d, K, a))(lexicon.device(dev))
    for m in (0, 1, 2):
        gm = torch.Generator().manual_seed(1000 + m)
        W = (torch.randn(C ** m, C, generator=gm, dtype=torch.float64) - 1.0).to(dev)
        fns[f"fused_m{m}"] = (lambda W, m: lambda: ops.ctc_beam_decode_lm(d, K, W, m))(W, m)
    t = alternating_ms(fns)
    row = dict(T=T, N=N, C=C, K=K)
    for name, v in t.items():
        row.update(figures(name, v))
        if name.startswith("dfa_"):
            row[f"{name}_over_plain"] = round(v[0] / t["plain"][0], 4)
    # the accept-all automaton returns the plain beams; the tries accept some entry on so many strips
    pt, pl, ps = ops.ctc_beam_decode(d, K)
    at, al, asc, _ = ops.ctc_beam_decode_dfa(d, K, lex["accept_all"].device(dev))
    row["accept_all_equals_plain"] = bool(torch.equal(pt, at) and torch.equal(pl, al) and torch.equal(ps.view(torch.int64), asc.view(torch.int64)))
    for name in ("trie_1000", "trie_90000"):
        a = lex[name].device(dev)
        states = ops.ctc_beam_decode_dfa(d, K, a)[3]
        accepted = (states >= 0) & (a.final[states.clamp(min=0).long()] != 0)
        row[f"dfa_{name}_strips_with_a_word"] = int(accepted.any(dim=1).sum())
    return row


def stored(name, key):
    """{(T, N, K): value} of a profile written earlier, {} where the file is missing"""
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return {(r["T"], r["N"], r["K"]): r[key] for r in json.load(f)["shapes"] if key in r}
    except (OSError, ValueError, KeyError):
        return {}


def main():
    assert torch.cuda.is_available(), "bench_beam_lexicon.py times the device path: it needs an MI355X"
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "beam_lexicon.json")
    dev = torch.device("cuda")
    char_to_index, _, C = get_char_maps(properties.char_set)
    lex = lexicons(char_to_index, C)
    automata = {name: dict(words=l.num_words, states=l.num_states, edges=l.num_edges) for name, l in lex.items()}
    print(json.dumps(automata), flush=True)
    before = {"plain": stored("beam_decode.json", "beam_kernel_ms"), **{f"fused_m{m}": stored("beam_lm.json", f"fused_m{m}_ms") for m in (0, 1, 2)}}
    rows = []
    for T, N, C_, K in SHAPES:
        assert C_ == C
        r = time_shape(T, N, C, K, dev, lex)
        for name, table in before.items():
            if (T, N, K) in table:
                r[f"{name}_over_stored_profile"] = round(r[f"{name}_ms"] / table[(T, N, K)], 4)
        rows.append(r)
        print(f"T={T} N={N} C={C} K={K:2d}  plain {r['plain_ms']:.4f} ms (spread {r['plain_spread']:.4f})  dfa 1000 words {r['dfa_trie_1000_ms']:.4f} "
              f"(x{r['dfa_trie_1000_over_plain']:.4f})  90000 words {r['dfa_trie_90000_ms']:.4f} (x{r['dfa_trie_90000_over_plain']:.4f})  accept-all "
              f"{r['dfa_accept_all_ms']:.4f} (x{r['dfa_accept_all_over_plain']:.4f})  fused m=0,1,2 {r['fused_m0_ms']:.4f} {r['fused_m1_ms']:.4f} "
              f"{r['fused_m2_ms']:.4f}", flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("QEA_COMMIT", "unknown")
    result = dict(commit=commit, device=torch.cuda.get_device_name(0),
                  method=f"device events around {LAUNCHES} back-to-back launches; a round times one window of every variant in turn (the variants "
                         f"alternate); per-launch median of {REPS} rounds after a warm-up round (output allocation included: three torch.empty per "
                         f"plain call, four per dfa or fused call); spread = (max - min) / median of the windows; *_over_stored_profile: this run's "
                         f"figure over the one in profiles/beam_decode.json (plain) or profiles/beam_lm.json (fused) at the same shape",
                  automata=automata, shapes=rows)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(wrote=out, shapes=len(rows))))


if __name__ == "__main__":
    main()
