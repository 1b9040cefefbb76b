"""Per-kernel summary of one translation unit's device assembly: the gate of a change that claims "same code".

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S conv_wgrad.hip -o conv_wgrad.s     (flags as build.sh)
    python3 isa_report.py conv_wgrad.s > head.json          one JSON row per kernel
    python3 isa_report.py --diff parent.json head.json      the kernels whose rows differ, field by field; exit 1 if any does

A row: name (demangled, anonymous namespace and argument list dropped), VGPRs, SGPRs, scratch bytes per lane, the number of
instructions whose mnemonic starts with each prefix of CLASSES, the instruction total, and the SHA-256 of the instruction text
with the labels renumbered in order of appearance (a kernel that moved inside the file, or whose neighbours changed, keeps its
hash).  Instruction classes are named by prefix only.  Not wired into build.sh."""
import hashlib
import json
import re
import subprocess
import sys

CLASSES = ("v_mfma", "ds_read", "ds_write", "global_load", "global_store", "scratch_", "s_barrier", "s_waitcnt")
CXXFILT = ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt")      # the first that runs


def demangle(names):
    for tool in CXXFILT:
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    else:
        return names
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", l)).rsplit("(", 1)[0] for l in out]


def kernel_bodies(text):
    """{mangled name: instruction lines} of every .amdhsa_kernel of the file: from the name's label to its s_endpgm-terminated end"""
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    lines = text.splitlines()
    start = {l[:-1].split(":")[0]: i for i, l in enumerate(lines) if l and not l[0].isspace() and not l.startswith(".") and ":" in l}
    bodies = {}
    for k in kernels:
        body = []
        for l in lines[start[k] + 1:]:
            s = l.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if s and not (s.startswith(".") and not s.endswith(":")):   # instructions and labels; no directives
                body.append(" ".join(s.split()))
        bodies[k] = body
    return bodies


def report(path):
    text = open(path, errors="replace").read()
    meta = {}
    for blk in re.split(r"^\s+- \.agpr_count:", text, flags=re.M)[1:]:   # the amdhsa.kernels metadata, one block per kernel
        f = dict(re.findall(r"^\s+\.(name|sgpr_count|vgpr_count|private_segment_fixed_size):\s+(\S+)", blk, re.M))
        meta[f["name"]] = f
    bodies = kernel_bodies(text)
    rows = []
    for (k, body), name in zip(bodies.items(), demangle(list(bodies))):
        labels = {}
        norm = []
        for l in body:
            l = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), l)
            norm.append(l)
        ins = [l.split()[0] for l in norm if not l.endswith(":")]
        row = {"name": name, "vgpr": int(meta[k]["vgpr_count"]), "sgpr": int(meta[k]["sgpr_count"]),
               "scratch": int(meta[k]["private_segment_fixed_size"])}
        for c in CLASSES:
            row[c] = sum(i.startswith(c) for i in ins)
        row["total"] = len(ins)
        row["hash"] = hashlib.sha256("\n".join(norm).encode()).hexdigest()[:16]
        rows.append(row)
    return rows


def diff(path_a, path_b):
    """-> [{name, field: [a, b], ...}] of the kernels whose rows differ.  A kernel present on one side only is paired with the one
    unpaired kernel of the other side that has the same name in front of its template arguments, if there is exactly one."""
    a, b = ({r["name"]: r for r in map(json.loads, open(p))} for p in (path_a, path_b))
    pairs = [(n, n) for n in a if n in b]
    only_a, only_b = [n for n in a if n not in b], [n for n in b if n not in a]
    for n in list(only_a):
        same = [m for m in only_b if m.split("<")[0] == n.split("<")[0]]
        if len(same) == 1 and sum(m.split("<")[0] == n.split("<")[0] for m in only_a) == 1:
            pairs.append((n, same[0]))
            only_a.remove(n)
            only_b.remove(same[0])
    out = [{"name": n, "only_in": path_a} for n in only_a] + [{"name": n, "only_in": path_b} for n in only_b]
    for na, nb in pairs:
        d = {k: [a[na][k], b[nb][k]] for k in a[na] if k != "name" and a[na][k] != b[nb].get(k)}
        if d:
            out.append({"name": na if na == nb else f"{na} -> {nb}", **d})
    return out, len(pairs)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        rows, n = diff(sys.argv[2], sys.argv[3])
        for r in rows:
            print(json.dumps(r))
        print(f"[isa_report] {n} kernels paired, {len(rows)} differ", file=sys.stderr)
        sys.exit(1 if rows else 0)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    for r in report(sys.argv[1]):
        print(json.dumps(r))
