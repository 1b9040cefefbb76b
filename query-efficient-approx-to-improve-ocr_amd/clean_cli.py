"""[new] Clean a folder of scans with a trained preprocessor (flags: qea/cli_flags.py tag "n").

    python clean_cli.py --prep_path PREP --in_dir scans --out_dir cleaned [--tile H W] [--batch_pages N]
    python clean_cli.py --method {otsu,sauvola} [--window W --k K] --in_dir scans --out_dir binarised [--batch_pages N]

Every png / jpg / jpeg of --in_dir, in name order, is decoded to 8-bit grey, sent through the tiled eval-mode pass of qea/pages.py
(clean_pages: pages of any size, --batch_pages of them per call so that tiles of different pages share UNet passes) and written to
--out_dir as an 8-bit grey PNG of the same size and stem.  PIL does the file I/O only: the p / 255 normalisation, the tiling and the
(uint8)(clamp(x, 0, 1) * 255) quantisation run on the device.  `backend` is the injection seam of the other drivers (the default is
the HIP path; the oracle backend runs the same plan on the host).

--method otsu / sauvola writes the classic baseline instead (qea/binarize.py: binarize_pages, one call per --batch_pages group): no
checkpoint is loaded and --tile is ignored; same output names, sizes and 8-bit PNG format, ink 0 and background 255.

[new] --despeckle N (with --method otsu / sauvola) also turns connected components of fewer than N ink pixels into background
(binarize_pages(despeckle=N)); with the UNet, whose output is grey, it is a ValueError at construction.
[new] --boxes [--boxes_gap G --boxes_min_area A], with any method: the word boxes of every WRITTEN page (8-bit, ink = 127 or darker;
qea/components.py: word_boxes, one call per --batch_pages group) go into <stem>.json beside the PNG as a list of {"label": "", "x_min",
"y_min", "x_max", "y_max"}, the form datasets/patch_dataset.py reads.  x_max / y_max are EXCLUSIVE, one past the component's last column
and row, because the crops (utils.get_text_stack, the crop kernel) cut image[y_min:y_max, x_min:x_max]: the crop of a box holds every
pixel of its component.
[new] --deskew [--deskew_max_slope A --deskew_min_gain G --deskew_interp {bilinear,nearest}], with any method: the decoded 8-bit pages of a
--batch_pages group first go through ONE call of qea/deskew.py: deskew_pages (skew estimate from each page's Otsu ink, rotation about the
page centre, white fill), so that the UNet or the binariser, and with them --boxes, see and describe the deskewed page that is written;
a line "<stem>: slope a/1024" is printed per page.  Without the flag nothing changes.
[new] --read CRNN_CHECKPOINT [--read_beam K [--read_lm PATH --read_lm_weight a --read_lm_bonus b | --read_lexicon PATH]] [--read_buckets
W ...], with any method; implies --boxes: the word boxes of the WRITTEN pages of a --batch_pages group go through ONE call of
qea/reading.py: read_pages (every box cut into a 32-row strip on the device, taller boxes shrunk by the exact area average; the strips
through the eval-mode CRNN bucket by bucket; greedy, beam, n-gram-fused or lexicon-constrained decoding as in eval_crnn.py, with its
exclusion rules) and "label" holds what the CRNN reads; with a beam "score" (the log-score the search ranked by) is added.  A line
"<stem>: N words read, M cut" is printed per page (cut: wider than the last bucket).  Without the flag nothing changes: the same JSON
bytes.
[new] --read_chars (with --read): every label is also aligned to the scores it was decoded from (CTC forced alignment, utils.char_spans:
one more launch per CRNN pass) and each row gains "chars": [{"c", "x_min", "x_max", "conf"}], one entry per character of the label: its
columns on the page (x_max exclusive; y_min / y_max are the row's own) and the mean of its log-probabilities over the steps it
occupies.  An empty label has an empty list.  The folder still loads as a PatchDataset, which ignores the key.
[new] --lines [--lines_overlap P --lines_tall T --lines_gap G], with any method; implies --boxes: the word boxes of a --batch_pages group
go through ONE call of qea/lines.py: group_lines (one launch: neighbours along x that overlap vertically form a line), after the reading,
which keeps the order read_pages was given.  The rows of <stem>.json are then written in READING order, lines top to bottom and each line
left to right, and each gains "line"; a line "<stem>: L lines" is printed per page.  The grouping is local and meant for level or
--deskew'ed pages.  Without the flag nothing changes: the same JSON bytes.
[new] --text (needs --read, implies --lines): <stem>.txt holds what the CRNN read, the words of a line joined by a space and the lines by
a newline (lines.page_text; an empty label is skipped).

    python clean_cli.py --deskew --method sauvola --boxes --read out/crnn/model_1_0.00 --in_dir scans --out_dir read

is a complete OCR run, and the written folder loads as a labelled PatchDataset; with --text it also writes the pages' text.
"""
import json
import os

import numpy as np
import torch

from qea import components, deskew, lines, reading
from qea.binarize import binarize_pages, check_params
from qea.pages import clean_pages
from qea.trainer_core import hip_backend

EXTENSIONS = (".png", ".jpg", ".jpeg")


class CleanPages:
    def __init__(self, args, backend=None):
        self.in_dir, self.out_dir = args.in_dir, args.out_dir
        self.tile = tuple(args.tile)
        self.batch_pages = max(1, int(args.batch_pages))
        self.device = (backend or hip_backend()).device
        self.method = getattr(args, "method", "unet")
        self.despeckle = int(getattr(args, "despeckle", 0) or 0)
        self.boxes = bool(getattr(args, "boxes", False))
        self.boxes_gap, self.boxes_min_area = getattr(args, "boxes_gap", 8), getattr(args, "boxes_min_area", 16)
        self.deskew = bool(getattr(args, "deskew", False))
        self.deskew_max_slope, self.deskew_min_gain = getattr(args, "deskew_max_slope", 90), getattr(args, "deskew_min_gain", 0)
        self.deskew_interp = getattr(args, "deskew_interp", "bilinear")
        if self.deskew:
            deskew.check_params(self.deskew_max_slope, min_gain=self.deskew_min_gain, interp=self.deskew_interp)
        self.read_path = getattr(args, "read", None)
        self.read_beam = int(getattr(args, "read_beam", 0) or 0)
        self.read_lm_path, self.read_lexicon_path = getattr(args, "read_lm", None), getattr(args, "read_lexicon", None)
        self.read_lm_weight, self.read_lm_bonus = float(getattr(args, "read_lm_weight", 1.0)), float(getattr(args, "read_lm_bonus", 0.0))
        self.read_buckets = tuple(getattr(args, "read_buckets", None) or reading.default_buckets())
        self.read_lm = self.read_lexicon = self.read_model = None
        self.read_chars = bool(getattr(args, "read_chars", False))
        if self.read_chars and not self.read_path:
            raise ValueError("--read_chars needs --read CRNN_CHECKPOINT")
        if self.read_path:
            self.boxes = True
            reading.check_params(self.read_buckets, beam=self.read_beam)
            if self.read_lm_path and not self.read_beam:
                raise ValueError("--read_lm needs --read_beam K: the model is fused into the prefix beam search")
            if self.read_lexicon_path and (not self.read_beam or self.read_lm_path):
                raise ValueError("--read_lexicon needs --read_beam K and cannot be combined with --read_lm")
        elif self.read_beam or self.read_lm_path or self.read_lexicon_path or getattr(args, "read_buckets", None):
            raise ValueError("--read_beam, --read_lm, --read_lexicon and --read_buckets need --read CRNN_CHECKPOINT")
        self.text = bool(getattr(args, "text", False))
        if self.text and not self.read_path:
            raise ValueError("--text needs --read CRNN_CHECKPOINT: it writes what the CRNN read")
        self.lines = bool(getattr(args, "lines", False)) or self.text
        given = [getattr(args, name, None) for name in ("lines_overlap", "lines_tall", "lines_gap")]
        if self.lines:
            self.boxes = True
            self.lines_params = tuple(d if v is None else v for v, d in zip(given, (50, 3, 0)))
            lines.check_params(*self.lines_params)
        elif any(v is not None for v in given):
            raise ValueError("--lines_overlap, --lines_tall and --lines_gap need --lines")
        if self.despeckle:
            if self.method == "unet":
                raise ValueError("--despeckle needs --method otsu or sauvola: the UNet's output is grey, and despeckling would binarise it")
            components.check_params(min_area=self.despeckle)
        if self.boxes:
            components.check_params(min_area=self.boxes_min_area, gap_x=self.boxes_gap)
        if self.method == "unet":
            self.prep_model = torch.load(args.prep_path, map_location=self.device, weights_only=False).to(self.device).eval()
        else:
            self.window, self.k = args.window, args.k
            check_params(self.method, self.window, self.k)
        if self.read_path:
            import properties
            from utils import get_char_maps
            self.read_model = torch.load(self.read_path, map_location=self.device, weights_only=False).to(self.device).eval()
            char_to_index, self.index_to_char, _ = get_char_maps(properties.char_set)
            if self.read_lm_path:
                from qea.lm import CharLM
                self.read_lm = CharLM.load(self.read_lm_path, char_to_index)
            if self.read_lexicon_path:
                from qea.lexicon import Lexicon
                self.read_lexicon = Lexicon.load(self.read_lexicon_path, char_to_index)
        self.names = sorted(n for n in os.listdir(self.in_dir) if n.lower().endswith(EXTENSIONS))
        stems = [os.path.splitext(n)[0] for n in self.names]
        twice = sorted({s for s in stems if stems.count(s) > 1})
        if twice:
            raise ValueError(f"{self.in_dir}: several files share the stems {twice}; their outputs would overwrite each other")

    def run(self):
        """-> the paths written, in input order"""
        from PIL import Image
        os.makedirs(self.out_dir, exist_ok=True)
        written = []
        for i in range(0, len(self.names), self.batch_pages):
            names = self.names[i:i + self.batch_pages]
            pages = []
            for n in names:
                with Image.open(os.path.join(self.in_dir, n)) as img:
                    pages.append(torch.from_numpy(np.array(img.convert("L"), dtype=np.uint8)))
            if self.deskew:
                pages, slopes = deskew.deskew_pages(pages, self.deskew_max_slope, min_gain=self.deskew_min_gain, interp=self.deskew_interp,
                                                    out="u8", device=self.device)
                for n, a in zip(names, slopes.cpu().tolist()):
                    print(f"{os.path.splitext(n)[0]}: slope {a}/1024")
            if self.method == "unet":
                cleaned = clean_pages(self.prep_model, pages, tile=self.tile, out="u8")
            else:
                cleaned = binarize_pages(pages, self.method, window=self.window, k=self.k, out="u8", device=self.device,
                                         despeckle=self.despeckle)
            boxes = components.word_boxes(cleaned, gap_x=self.boxes_gap, min_area=self.boxes_min_area, device=self.device) if self.boxes else None
            texts = scores = chars = None
            if self.read_model is not None:
                texts, *scores, _ = reading.read_pages(self.read_model, cleaned, boxes, self.index_to_char, buckets=self.read_buckets,
                                                       beam=self.read_beam, lm=self.read_lm, lm_weight=self.read_lm_weight,
                                                       lm_bonus=self.read_lm_bonus, lexicon=self.read_lexicon, chars=self.read_chars)
                if self.read_chars:
                    chars = scores.pop()
                table = reading.box_table(boxes)
                plan = reading.strip_plan(table, [p.shape[-2] for p in cleaned], [p.shape[-1] for p in cleaned], self.read_buckets)
                for n, t, m in zip(names, texts, np.bincount(table[plan.cut, 0], minlength=len(names)).tolist()):
                    print(f"{os.path.splitext(n)[0]}: {len(t)} words read, {m} cut")
            grouped = None
            if self.lines:                                     # after the reading, which keeps the order read_pages was given
                grouped = [(o.cpu().tolist(), l.cpu().tolist(), len(lb))
                           for o, l, lb in lines.group_lines(boxes, *self.lines_params, device=self.device)]
                for n, (_, _, L) in zip(names, grouped):
                    print(f"{os.path.splitext(n)[0]}: {L} lines")
            for i, (n, page) in enumerate(zip(names, cleaned)):
                path = os.path.join(self.out_dir, os.path.splitext(n)[0] + ".png")
                Image.fromarray(page.cpu().numpy()).save(path)
                written.append(path)
                if boxes is not None:                          # x_max / y_max one past the last pixel: the crops' slicing convention
                    rows = [dict(label="", x_min=a, y_min=b, x_max=c + 1, y_max=d + 1) for a, b, c, d in boxes[i].cpu().tolist()]
                    if texts is not None:
                        for row, t in zip(rows, texts[i]):
                            row["label"] = t
                        for row, s in zip(rows, scores[0][i] if scores else []):
                            row["score"] = s
                        for row, cs in zip(rows, chars[i] if chars else []):   # y_min / y_max of a character are its row's own
                            row["chars"] = [dict(c=c, x_min=a, x_max=b, conf=v) for c, a, b, v in cs]
                    if grouped is not None:
                        order, line, _ = grouped[i]
                        for row, l in zip(rows, line):
                            row["line"] = l
                        rows = [rows[k] for k in order]
                        if self.text:
                            with open(os.path.splitext(path)[0] + ".txt", "w") as f:
                                f.write(lines.page_text(texts[i], order, line))
                    with open(os.path.splitext(path)[0] + ".json", "w") as f:
                        json.dump(rows, f)
        print(f"{len(written)} pages cleaned into {self.out_dir}")
        return written


def build_parser():
    from qea.cli_flags import build_parser as _build
    return _build("n", "Cleans every scan of a folder with a trained preprocessor")


if __name__ == "__main__":
    args = build_parser().parse_args()
    print(args)
    CleanPages(args).run()
