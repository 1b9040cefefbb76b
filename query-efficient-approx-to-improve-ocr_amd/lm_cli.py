"""[new] Build the character n-gram model that eval_crnn.py --beam K --lm PATH fuses into the prefix beam search (qea/lm.py: CharLM).

    python lm_cli.py --dataset {pos,vgg} [--data_base_path DIR | --synthetic_size N] --order n --add_k k --out PATH

The labels are those of the training split train_crnn.py reads for the same --dataset (the strip folders of properties.py, the label
in the file name), or of N synthetic strips; no image is decoded and nothing runs on the device.  Counts are add-k smoothed over the
94 printable classes of properties.char_set; there is no end-of-word term (eval_crnn.py --lm_bonus is the length control).
"""
import argparse
import os

import properties
from qea.lm import CharLM
from utils import get_char_maps


def training_labels(args):
    if args.synthetic_size:
        from datasets.synthetic import SyntheticTextAreas
        return list(SyntheticTextAreas(args.synthetic_size, seed=1).labels)
    from datasets._io import ascii_label
    from datasets.img_dataset import ImgDataset, _label_of
    folder = properties.pos_text_dataset_train if args.dataset == "pos" else properties.vgg_text_dataset_train
    files = ImgDataset(os.path.join(args.data_base_path, folder)).files
    labels = [ascii_label(_label_of(f)) for f in files]
    return [l for l in labels if len(l) <= properties.max_char_len]


def build_parser():
    ap = argparse.ArgumentParser(description="Builds a character n-gram model from a training split's labels")
    ap.add_argument("--dataset", choices=["pos", "vgg"], default="pos", help="whose training labels to count")
    ap.add_argument("--data_base_path", default=".", help="Base path training, validation and test data")
    ap.add_argument("--synthetic_size", type=int, help="count the labels of N synthetic strips instead of reading --data_base_path")
    ap.add_argument("--order", type=int, default=2, help="n of the n-gram: 1, 2 or 3")
    ap.add_argument("--add_k", type=float, default=0.1, help="add-k smoothing constant (> 0)")
    ap.add_argument("--out", required=True, help="the .npz file to write")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    char_to_index, _, _ = get_char_maps(properties.char_set)
    labels = training_labels(args)
    lm = CharLM.from_labels(labels, char_to_index, order=args.order, add_k=args.add_k, blank=0)
    lm.save(args.out)
    print(f"{args.order}-gram over {len(labels)} labels ({int(lm.count.sum())} characters, add_k {args.add_k:g}) -> {args.out}")
    return lm


if __name__ == "__main__":
    main()
