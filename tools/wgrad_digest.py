"""SHA-256 of what ops.conv_wgrad writes for a fixed list of nine-tap descriptors: bit-equality of two builds.  Needs a GPU.

    python tools/wgrad_digest.py > head.jsonl
    QEA_HIP_LIB=/path/to/other/libqea_hip.so python tools/wgrad_digest.py > parent.jsonl
    cmp parent.jsonl head.jsonl

Every nine-tap form is bit-reproducible (order-fixed slab reduction, no float atomics), so a change that reorders no floating-point
operation must leave every line as it was.  One JSON line per case: the case's name, the digest of dW and, where the launch takes
dbias, of dbias.  No timing.

Cases: the shapes below (3x3, pad 1; those of tests/test_conv_wgrad_gpu.py that reach each form: one workgroup crossing ring strips,
two column tiles, the 16-wide producer / consumer policy, the 32-wide channel blocks at both tile widths) x tile {0, 23, 29} x
splits {0, 1, 3}, accumulate on for splits = 3, dbias on and off where qea_conv_wgrad_fuses_bias says 1; all of it in "split_f16"
mode (two fp16 planes) and again in "split_bf16" mode (the three-plane instances).
Inputs: numpy.random.RandomState(seed).standard_normal(shape).astype(float32) on the CPU (the frozen legacy stream), seed = 1000 +
the shape's index for dY, 2000 + for X; dW and dbias start from 0.25 where they accumulate, from NaN where they must be overwritten."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-efficient-approx-to-improve-ocr_amd"))

SHAPES = [(2, 8, 32, 128, 128), (3, 8, 32, 256, 128), (2, 16, 64, 64, 128), (1, 4, 32, 512, 512), (9, 4, 16, 256, 256), (5, 4, 16, 128, 256),
          (3, 8, 16, 96, 32), (2, 8, 32, 32, 96), (3, 32, 128, 32, 32), (2, 32, 128, 64, 32)]          # B, H, W, Cin, Cout
TILES = (0, 23, 29)
SPLITS = (0, 1, 3)
MODES = ("split_f16", "split_bf16")


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    import numpy as np
    import torch
    from qea import _lib, ops
    L = _lib.lib()
    for mode in MODES:
        ops.set_mfma_mode(mode)
        for i, (B, H, W, Cin, Cout) in enumerate(SHAPES):
            dy = torch.from_numpy(np.random.RandomState(1000 + i).standard_normal((B, H, W, Cout)).astype(np.float32)).cuda()
            x = torch.from_numpy(np.random.RandomState(2000 + i).standard_normal((B, H, W, Cin)).astype(np.float32)).cuda()
            amax = dict(p_amax=ops.absmax(dy, Cout, B * H * W, Cout), q_amax=ops.absmax(x, Cin, B * H * W, Cin)) if mode == "split_f16" else {}
            for tile in TILES:
                for splits in SPLITS:
                    acc = splits == 3
                    kw = dict(B=B, PH=H, PW=W, QH=H, QW=W, R=Cout, Cc=Cin, KH=3, KW=3, pad=(1, 1), ldp=Cout, ldq=Cin, accumulate=acc, splits=splits, tile=tile)
                    d = _lib.WgradDesc(B=B, PH=H, PW=W, QH=H, QW=W, R=Cout, C=Cin, KH=3, KW=3, pad_h=1, pad_w=1, stride_h=1, stride_w=1, ldp=Cout,
                                       ldq=Cin, accumulate=int(acc), splits=splits, tile=tile)
                    if amax:
                        d.p_absmax, d.q_absmax = amax["p_amax"].data_ptr(), amax["q_amax"].data_ptr()
                    for bias in ((False, True) if L.qea_conv_wgrad_fuses_bias(C.byref(d)) else (False,)):
                        fill = 0.25 if acc else float("nan")
                        dw = torch.full((Cout, 3, 3, Cin), fill, device="cuda")
                        db = torch.full((Cout,), fill, device="cuda") if bias else None
                        ops.conv_wgrad(dy, x, dw, dbias=db, **amax, **kw)
                        torch.cuda.synchronize()
                        row = {"case": f"{mode}/{B}x{H}x{W}x{Cin}x{Cout}/tile{tile}/splits{splits}/{'dbias' if bias else 'plain'}", "dw": _sha(dw)}
                        if bias:
                            row["dbias"] = _sha(db)
                        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
