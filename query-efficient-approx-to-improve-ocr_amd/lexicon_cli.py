"""[new] Build the word-list trie that eval_crnn.py --beam K --lexicon PATH keeps the prefix beam search inside (qea/lexicon.py: Lexicon).

    python lexicon_cli.py --dataset {pos,vgg} [--data_base_path DIR | --synthetic_size N | --words FILE] --out PATH

The words are the labels of the training split train_crnn.py reads for the same --dataset (the strip folders of properties.py, the
label in the file name), those of N synthetic strips, or the lines of FILE (one word per line, surrounding white space dropped); no
image is decoded and nothing runs on the device.  Duplicates are merged and empty lines skipped; a word with a character outside the
94 printable classes of properties.char_set is refused.
"""
import argparse

import properties
from lm_cli import training_labels
from qea.lexicon import Lexicon
from utils import get_char_maps


def words_of(args):
    if args.words:
        with open(args.words, encoding="utf-8") as f:
            return [line.strip() for line in f]
    return training_labels(args)


def build_parser():
    ap = argparse.ArgumentParser(description="Builds a lexicon (a word-list trie) from a training split's labels or a word file")
    ap.add_argument("--dataset", choices=["pos", "vgg"], default="pos", help="whose training labels to take")
    ap.add_argument("--data_base_path", default=".", help="Base path training, validation and test data")
    ap.add_argument("--synthetic_size", type=int, help="take the labels of N synthetic strips instead of reading --data_base_path")
    ap.add_argument("--words", help="take the lines of this file, one word per line, instead of a dataset's labels")
    ap.add_argument("--out", required=True, help="the .npz file to write")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    char_to_index, _, _ = get_char_maps(properties.char_set)
    lexicon = Lexicon.from_words(words_of(args), char_to_index, blank=0)
    lexicon.save(args.out)
    print(f"{lexicon.num_words} words ({lexicon.num_empty} empty skipped), {lexicon.num_states} states, {lexicon.num_edges} edges -> {args.out}")
    return lexicon


if __name__ == "__main__":
    main()
