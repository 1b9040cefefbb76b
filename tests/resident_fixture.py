"""The strip directory of the resident-store tests (tests/test_resident_cpu.py, tests/test_resident_gpu.py): 24 strips written with
PIL as PNG and JPG, `<idx>_<label>_<tag>.<ext>`, plus two files the dataset's listing rules drop; and the area-trainer run the GPU
tests compare with and without --resident (also from tests/resident_children.py, in an interpreter of its own)."""
import json
import os

import numpy as np
import torch
from PIL import Image

SIZE = (32, 128)
# (h, w): the corners of the pad arithmetic (1x1, odd margins, one short of full, exactly full, narrow, low and full width) and three
# oversize strips that take PadWhite's thumbnail branch (both too large; one row too tall; too wide only)
SIZES = [(1, 1), (5, 3), (31, 127), (32, 128), (32, 20), (7, 128), (40, 300), (33, 64), (16, 200)]
EXTRA = [(9, 77), (30, 2), (2, 126), (17, 65), (64, 64), (12, 129)]            # 9 PNG + 9 JPG + 6 = 24 strips
BROKEN = "61_✓_145.png"                                                         # one of datasets.img_dataset._BROKEN_NAMES
N_STRIPS = 24


def _pixels(rng, h, w):
    """Grey noise over a ramp, never white on the border rows and columns: a pad off by one pixel changes the batch."""
    a = rng.randint(0, 200, size=(h, w)) + (np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) % 56
    return a.astype(np.uint8)


def write_strips(root, seed=11):
    """Writes the directory and returns the number of strips an ImgDataset lists from it."""
    import properties
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    letters = "abcdefghijkmnopqrstuvwxyzABCDEFGHJKLMNPQRSTUVWXYZ23456789"
    k = 0
    for ext, sizes in (("png", SIZES), ("jpg", SIZES), ("png", EXTRA)):
        for h, w in sizes:
            label = "".join(rng.choice(list(letters), rng.randint(3, 8)))
            Image.fromarray(_pixels(rng, h, w), mode="L").save(os.path.join(root, f"{k}_{label}_{h}x{w}.{ext}"))
            k += 1
    Image.fromarray(_pixels(rng, 10, 40), mode="L").save(os.path.join(root, BROKEN))
    long_label = "x" * (properties.max_char_len + 1)
    Image.fromarray(_pixels(rng, 10, 40), mode="L").save(os.path.join(root, f"{k}_{long_label}_long.png"))
    assert k == N_STRIPS
    return k


def pad_transform(size=SIZE):
    """The trainers' transform: PadWhite(size), then float32 / 255."""
    from datasets._io import to_tensor
    from transform_helper import PadWhite
    pad = PadWhite(size)
    return lambda img: to_tensor(pad(img))


class Log:
    def __init__(self):
        self.rows = []

    def log(self, d):
        self.rows.append(dict(d))

    def save(self, *_a):
        pass

    def summary_update(self, *_a):
        pass


def flat(m):
    return torch.cat([p.detach().flatten().clone() for p in m.parameters()])


def area_run(tmp, strip_dir, resident, graph, epochs):
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentLoader
    from qea.cli_flags import build_parser
    from train_nn_area import TrainNNPrep
    tf = pad_transform()
    tr = ImgDataset(strip_dir, transform=tf, include_name=True, include_index=True)
    va = ImgDataset(strip_dir, transform=tf, include_name=True)
    cers = str(tmp / "cers.json")
    json.dump({os.path.basename(f): (i % 5) / 4 for i, f in enumerate(tr.files)}, open(cers, "w"))
    argv = ["--exp_base_path", str(tmp / f"exp_{int(resident)}_{int(graph)}"), "--ocr", "stub", "--epoch", str(epochs), "--batch_size", "8",
            "--inner_limit", "2", "--minibatch_subset", "topKCER", "--minibatch_subset_prop", "0.5", "--cers_ocr_path", cers,
            "--train_subset_size", "8", "--val_subset_size", "8"] + (["--resident"] if resident else []) + (["--graph"] if graph else [])
    t = TrainNNPrep(build_parser("a", "").parse_args(argv), train_set=tr, val_set=va)
    assert (type(t.loader_train) is ResidentLoader) == resident and (type(t.loader_validation) is ResidentLoader) == resident
    assert len(t.loader_train) == 1
    t.log = Log()
    t.train()
    losses = [(r["train_loss"], r["CRNN_loss"], r["val_loss"]) for r in t.log.rows]
    assert len(losses) == epochs and all(v == v for row in losses for v in row)
    return losses, flat(t.prep_model), flat(t.crnn_model), t
