"""Answers of the four qea_conv_igemm queries (uses_split_bf16, wants_frag_planes, can_pool, stats_blocks) over a fixed grid of
descriptors, in both modes of qea_set_mfma_mode.  The queries dereference no pointer, so this runs without a GPU.

    python tools/conv_route_queries.py > tests/golden/conv_route_queries.json     # pin the answers of the build in the tree

tests/test_conv_route_cpu.py re-runs the grid and requires every answer to equal the pinned one.

The grid is the full product of (Cin, N, image, filter, forced tile, mode); the remaining axes (B, which operand pointers are
given, the epilogue flags, the pool width) are drawn per case from a fixed multiplicative hash of the case index, so every value of
every axis meets many values of the others without the product of all ten.
One answer per case: uses + 2 * wants + 6 * can_pool + 12 * stats_blocks."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))

AXES = {
    "Cin": [32, 64, 128, 256, 512],
    "N": [32, 40, 64, 128, 256, 512],
    "HW": [[2, 8], [4, 16], [8, 32], [32, 128], [7, 9]],
    "filter": ["3x3p1", "1x1", "2x2s2", "1x1convt", "1x1tbc"],
    "tile": [0, -1, 4, 20, 21, 24, 25, 26, 99],
    "mode": [0, 1],
    # drawn per case:
    "B": [1, 5, 64, 2048],
    "pointers": ["x_planes", "w_planes", "w_frag_planes", "x_absmax"],          # bit k of the draw: pointer k is non-null
    "flags": [[], [], [], [], ["scale"], ["bias"], ["relu"], ["mask"], ["accumulate"], ["stats"], ["scale", "bias", "relu"], ["stats", "mask"]],
    "pool_kw": [1, 2, 3],
}
DUMMY = 0x1000          # non-null, never dereferenced


def cases():
    """(descriptor fields, pool width, mode) in grid order"""
    prod = itertools.product(AXES["Cin"], AXES["N"], AXES["HW"], AXES["filter"], AXES["tile"], AXES["mode"])
    for i, (cin, n, (h, w), filt, tile, mode) in enumerate(prod):
        k = ((i >> 1) * 2654435761) & 0xffffffff     # the two modes of one descriptor share the draw
        f = dict(B=AXES["B"][(k >> 28) & 3], H=h, W=w, Cin=cin, N=n, tile=tile, KH=1, KW=1, pad_h=0, pad_w=0, stride_h=1, stride_w=1, out_mode=0)
        if filt == "3x3p1":
            f.update(KH=3, KW=3, pad_h=1, pad_w=1)
        elif filt == "2x2s2":
            f.update(KH=2, KW=2, stride_h=2, stride_w=2)
        elif filt == "1x1convt":
            f.update(out_mode=2)
        elif filt == "1x1tbc":
            f.update(out_mode=1, H=1)
        f["OH"] = (f["H"] + 2 * f["pad_h"] - f["KH"]) // f["stride_h"] + 1
        f["OW"] = (f["W"] + 2 * f["pad_w"] - f["KW"]) // f["stride_w"] + 1
        f["ldx"], f["ldy"], f["ldmask"] = cin, n, n
        for b, name in enumerate(AXES["pointers"]):
            if (k >> (20 + b)) & 1:
                f[name] = DUMMY
        for name in AXES["flags"][((k >> 12) & 0xff) % len(AXES["flags"])]:
            f[name] = 1 if name in ("relu", "accumulate") else DUMMY
        yield f, AXES["pool_kw"][((k >> 4) & 0xff) % 3], mode


def answers():
    from qea import _lib
    L = _lib.lib()
    prev = L.qea_set_mfma_mode(-1)
    out = []
    try:
        for f, kw, mode in cases():
            L.qea_set_mfma_mode(mode)
            d = _lib.ConvDesc(**f)
            p = C.byref(d)
            out.append(L.qea_conv_igemm_uses_split_bf16(p) + 2 * L.qea_conv_igemm_wants_frag_planes(p) + 6 * L.qea_conv_igemm_can_pool(p, kw) +
                       12 * L.qea_conv_igemm_stats_blocks(p))
    finally:
        L.qea_set_mfma_mode(prev)
    return out


if __name__ == "__main__":
    json.dump({"axes": AXES, "encoding": "uses + 2 * wants + 6 * can_pool + 12 * stats_blocks, grid order of tools/conv_route_queries.py",
               "answers": answers()}, sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")
