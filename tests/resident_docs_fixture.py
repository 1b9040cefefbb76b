"""The document folders of the resident-document tests (tests/test_resident_docs_cpu.py, tests/test_resident_docs_gpu.py), written
with PIL as PNG and JPG with `.json` box files in both formats (quads and x_min...), and the patch-trainer run the GPU test compares
with and without --resident.

write_documents: eight documents, one per corner of the canvas arithmetic (DOCS), listed in the order of their names:
  0  1x1        only a too-wide box: the dataset leaves the blank placeholder                                   (1 box)
  1  399x511    300 small boxes on a 20 x 15 grid whose neighbours overlap, across and down: more than one
                LDS chunk of the scatter, overlaps inside a chunk and across the chunk border                  (300 boxes)
  2  400x512    boxes at the four canvas corners, odd sizes, one of 127x31, one too wide and one with an
                over-long label (both dropped)                                                                  (37 boxes)
  3  57x300     six boxes stacked over one another                                                              (6 boxes)
  4  400x100    one box                                                                                         (1 box)
  5  120x512    a box with a negative coordinate (NEGATIVE: python slicing and the device clip differ on it, so
                it is held against the device kernel only) and two plain ones                                   (3 boxes)
  6  10x600     wider than the canvas only: the central 512 columns are kept; boxes inside them                 (2 boxes)
  7  450x200    taller than the canvas only: the central 400 rows are kept; boxes inside them                   (2 boxes)
write_trainer_documents: four documents with a few non-overlapping, in-canvas boxes and labels of the CRNN's alphabet."""
import json
import os

import numpy as np
from PIL import Image

from resident_fixture import Log, _pixels, flat

CANVAS = (400, 512)
DOCS = [(1, 1, "png"), (399, 511, "jpg"), (400, 512, "png"), (57, 300, "jpg"), (400, 100, "png"), (120, 512, "jpg"), (10, 600, "png"),
        (450, 200, "jpg")]
N_BOXES = [1, 300, 37, 6, 1, 3, 2, 2]
PLACEHOLDER, MANY, CORNERS, OVERLAP, ONE, NEGATIVE, WIDE, TALL = range(8)
IN_CANVAS = [i for i in range(8) if i != NEGATIVE]                 # the documents whose boxes take one branch on every path
LETTERS = "abcdefghijkmnopqrstuvwxyz23456789"


def _label(rng):
    return "".join(rng.choice(list(LETTERS), rng.randint(2, 7)))


def _as_json(boxes, quad):
    """[(x0, y0, x1, y1, label)] in one of the two formats of the .json files."""
    if quad:
        return [{"label": l, "x1": x0, "y1": y0, "x2": x1, "y2": y0, "x3": x1, "y3": y1, "x4": x0, "y4": y1} for x0, y0, x1, y1, l in boxes]
    return [{"label": l, "x_min": x0, "y_min": y0, "x_max": x1, "y_max": y1} for x0, y0, x1, y1, l in boxes]


def _boxes(k, rng):
    import properties
    L = lambda: _label(rng)
    if k == PLACEHOLDER:
        return [(0, 0, 128, 1, L())]                    # 128 wide: dropped, the placeholder remains
    if k == MANY:                                                                 # widths 9..30 at pitch 25, heights 5..31 at pitch 26
        return [(3 + 25 * c, 2 + 26 * r, 3 + 25 * c + int(rng.randint(9, 31)), 2 + 26 * r + int(rng.randint(5, 32)), L())
                for r in range(15) for c in range(20)]
    if k == CORNERS:
        b = [(0, 0, 20, 10, L()), (492, 390, 512, 400, L()), (0, 380, 31, 400, L()), (499, 0, 512, 13, L()), (100, 100, 227, 131, L()),
             (30, 40, 30 + 128, 60, L()),                                         # too wide: dropped
             (40, 200, 90, 220, "x" * (properties.max_char_len + 1)),             # over-long label: dropped
             (13, 17, 50, 28, L()), (301, 77, 304, 78, L())]
        for i in range(30):                                                       # 30 more of odd sizes on a 6 x 5 grid, apart from one another
            x, y = 5 + 83 * (i % 6), 140 + 45 * (i // 6)
            b.append((x, y, x + 2 * int(rng.randint(1, 38)) + 1, y + 2 * int(rng.randint(0, 15)) + 1, L()))
        return b
    if k == OVERLAP:
        return [(10, 5, 110, 30, L()), (40, 10, 160, 41, L()), (40, 10, 160, 41, L()), (100, 0, 227, 31, L()), (105, 20, 120, 50, L()),
                (0, 0, 127, 31, L())]
    if k == ONE:
        return [(7, 180, 93, 211, L())]
    if k == NEGATIVE:
        return [(-5, 10, 60, 30, L()), (200, 3, 300, 20, L()), (400, 90, 511, 120, L())]
    if k == WIDE:                                                                 # source columns 44..555 survive
        return [(50, 1, 120, 9, L()), (500, 0, 555, 10, L())]
    if k == TALL:                                                                 # source rows 25..424 survive
        return [(10, 30, 100, 55, L()), (150, 400, 199, 424, L())]
    raise ValueError(k)


def write_documents(root, seed=5):
    """Writes the eight documents and returns the directory."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    for k, (h, w, ext) in enumerate(DOCS):
        Image.fromarray(_pixels(rng, h, w), mode="L").save(os.path.join(root, f"d{k}_{h}x{w}.{ext}"))
        with open(os.path.join(root, f"d{k}_{h}x{w}.json"), "w") as f:
            json.dump(_as_json(_boxes(k, rng), quad=k % 2 == 1), f)
    return root


TRAINER_DOCS = [(400, 512, "png"), (120, 300, "jpg"), (399, 511, "png"), (57, 200, "jpg")]


def write_trainer_documents(root, seed=9):
    """Four documents for the trainer runs: 3-5 boxes each, apart from one another and inside the canvas after the shift."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    for k, (h, w, ext) in enumerate(TRAINER_DOCS):
        Image.fromarray(_pixels(rng, h, w), mode="L").save(os.path.join(root, f"t{k}.{ext}"))
        boxes = []
        for i in range(3 + k % 3):                                                # one column of boxes per document, 11 rows apart at least
            bh, bw = int(rng.randint(6, 11)), int(rng.randint(20, min(120, w - 10)))
            boxes.append((5 + 3 * i, 2 + 11 * i, 5 + 3 * i + bw, 2 + 11 * i + bh, _label(rng)))
        with open(os.path.join(root, f"t{k}.json"), "w") as f:
            json.dump(_as_json(boxes, quad=k % 2 == 0), f)
    return root


def patch_run(tmp, doc_dir, resident, docs_per_step, epochs=2):
    """patch_cli's trainer on the four trainer documents (training and validation set alike): topKCER at 0.5 with a CER file, the stub
    OCR, --inner_limit 2 -> (logged rows, black-box calls, UNet parameters, CRNN parameters, trainer)."""
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocLoader
    from qea.cli_flags import build_parser
    from train_nn_patch import TrainNNPrep
    tr = PatchDataset(doc_dir, pad=True, include_name=True)
    va = PatchDataset(doc_dir, pad=True)
    cers, k = {}, 0
    for i in range(len(tr)):
        _, boxes, name = tr[i]
        for s in TrainNNPrep._strip_names([b["label"] for b in boxes], name):
            cers[s] = (k % 5) / 4
            k += 1
    cers_path = str(tmp / "cers.json")
    json.dump(cers, open(cers_path, "w"))
    argv = ["--exp_base_path", str(tmp / f"exp_{int(resident)}_{docs_per_step}"), "--ocr", "stub", "--epoch", str(epochs), "--inner_limit", "2",
            "--minibatch_subset", "topKCER", "--minibatch_subset_prop", "0.5", "--cers_ocr_path", cers_path, "--docs_per_step", str(docs_per_step)]
    argv += ["--resident"] if resident else []
    t = TrainNNPrep(build_parser("p", "").parse_args(argv), train_set=tr, val_set=va)
    assert (type(t.loader_train) is ResidentDocLoader) == resident and len(t.loader_train) == 4 // docs_per_step
    t.log = Log()
    t.train()
    assert len(t.log.rows) == epochs
    rows = [{k: v for k, v in r.items()} for r in t.log.rows]
    assert all(v == v for r in rows for v in r.values())
    return rows, rows[-1]["Total Black-Box Calls"], flat(t.prep_model), flat(t.crnn_model), t

