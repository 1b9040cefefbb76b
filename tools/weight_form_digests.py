"""SHA-256 of every derived weight form (flip-transposed filter, 3x3 fragment planes in the 32-row and 16-row fp16 orders and the
bf16 order, 1x1 fragment planes) over a fixed list of shapes, through the single entry points and through qea_weight_forms_multi.
Needs a GPU.

    python tools/weight_form_digests.py > tests/golden/weight_form_digests.json     # pin the bytes of the build in the tree

tests/test_kernels_gpu.py::test_weight_forms_multi_equals_the_single_launches re-runs the cases and requires every digest to equal
the pinned one: the layouts are the contract between the packers and conv3x3_halo_bf3_kernel, conv3x3_halo_m16_kernel and
gemm1x1_f16_kernel, and once the single and the multi launches share their bodies, comparing one with the other proves nothing.

Inputs: numpy.random.RandomState(seed).standard_normal(shape).astype(float32) * scale (the frozen legacy stream: the file does not
depend on the torch version), seed = SEED0[kind] + index, scale = 0.1 + index (another power-of-two scale per case).  The abs-max is
ops.absmax over the whole tensor.  Outputs are zero-filled first (the planes end in 12 unspecified bytes).
The multi entry runs all jobs of a kind in one call, once in the listed order and once reversed (every job in another table slot);
the bf16 planes have a single entry only.  Per kind the smallest shapes that reach every branch of the index map, and one that
exceeds the multi kernel's 512 x 256 grid so that its stride loop runs."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))

CASES = {
    "flip": [[64, 32, 3, 3], [32, 64, 3, 3], [8, 12, 1, 3], [64, 32, 2, 2], [512, 512, 3, 3]],      # Co, Ci, KH, KW
    "f16_rows32": [[32, 32], [64, 32], [256, 32]],                                                  # N, Cin
    "f16_rows16": [[32, 64], [128, 64], [256, 128], [512, 512]],                                    # N, Cin
    "bf16": [[32, 32], [256, 32], [128, 64], [256, 128]],                                           # N, Cin
    "1x1": [[128, 64], [256, 128], [512, 2048]],                                                    # N, K
}
SEED0 = {"flip": 100, "f16_rows32": 200, "f16_rows16": 300, "bf16": 400, "1x1": 500}
MULTI_KIND = {"flip": 0, "f16_rows32": 1, "f16_rows16": 1, "1x1": 2}        # kind of qea_wform_job; the two 3x3 orders share a call


def _input(kind, i, dims):
    import numpy as np
    import torch
    shape = (dims[0], dims[2], dims[3], dims[1]) if kind == "flip" else (dims[0], dims[1]) if kind == "1x1" else (dims[0], 3, 3, dims[1])
    return torch.from_numpy(np.random.RandomState(SEED0[kind] + i).standard_normal(shape).astype(np.float32) * np.float32(0.1 + i)).cuda()


def _out(L, kind, dims):
    import torch
    if kind == "flip":
        return torch.zeros(dims[1], dims[2], dims[3], dims[0], device="cuda")
    nbytes = {"bf16": L.qea_pack_frag_planes_bytes, "1x1": L.qea_pack_frag_planes_f16_1x1_bytes}.get(kind, L.qea_pack_frag_planes_f16_bytes)(*dims)
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digests():
    """{"<kind>/<dims>/<single | multi | multi_reversed>": sha256 of the output's bytes}"""
    import torch
    from qea import _lib, ops
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    work = {}                                                   # multi kind -> [(name, dims, w, amax)]
    for kind, shapes in CASES.items():
        for i, dims in enumerate(shapes):
            name = f"{kind}/{'x'.join(map(str, dims))}"
            w = _input(kind, i, dims)
            am = None if kind in ("flip", "bf16") else ops.absmax(w, w.numel(), 1, w.numel())
            o = _out(L, kind, dims)
            if kind == "flip":
                ops.filter_flip_transpose(w, o, *dims)
            elif kind == "bf16":
                _lib.check(L.qea_pack_frag_planes(w.data_ptr(), dims[0], dims[1], o.data_ptr(), st), "qea_pack_frag_planes")
            elif kind == "1x1":
                _lib.check(L.qea_pack_frag_planes_f16_1x1(w.data_ptr(), dims[0], dims[1], am.data_ptr(), o.data_ptr(), st), "qea_pack_frag_planes_f16_1x1")
            else:
                _lib.check(L.qea_pack_frag_planes_f16(w.data_ptr(), dims[0], dims[1], am.data_ptr(), o.data_ptr(), st), "qea_pack_frag_planes_f16")
            out[name + "/single"] = _sha(o)
            if kind in MULTI_KIND:
                work.setdefault(MULTI_KIND[kind], []).append((name, kind, dims, w, am))
    for mk, items in work.items():
        for tag, order in (("multi", items), ("multi_reversed", items[::-1])):
            jobs = (_lib.WformJob * len(order))()
            outs = [_out(L, kind, dims) for _n, kind, dims, _w, _a in order]
            for j, ((_n, _k, dims, w, am), o) in enumerate(zip(order, outs)):
                jobs[j].src, jobs[j].dst, jobs[j].amax, jobs[j].kind = w.data_ptr(), o.data_ptr(), (am.data_ptr() if am is not None else None), mk
                jobs[j].a, jobs[j].b, jobs[j].c, jobs[j].d = (list(dims) + [0, 0])[:4]
            _lib.check(L.qea_weight_forms_multi(jobs, len(order), st), "qea_weight_forms_multi")
            for (name, *_r), o in zip(order, outs):
                out[f"{name}/{tag}"] = _sha(o)
    return out


def disagreements(d):
    """names whose multi digests differ from the single one"""
    return sorted(k for k in d if not k.endswith("/single") and d[k] != d[k.rsplit("/", 1)[0] + "/single"])


if __name__ == "__main__":
    d = digests()
    bad = disagreements(d)
    if bad:
        sys.exit(f"single and multi launches disagree: {bad}")
    json.dump({"cases": CASES, "sha256": d}, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
