"""The reference's command-line surface, as data.  Names, defaults, types, choices and the
`store_false` quirk of --random_std are those of patch_cli.py:11-155 and area_cli.py:11-124
(SURVEY.md §5.6), and of train_crnn.py:217-275, eval_crnn.py and eval_prep.py (tags "c", "e", "v") and pruning/prune_dataset.py:88-106 (tag "r"); the MI355X
build only ADDS flags (marked new), and one front end the reference does not have: clean_cli.py (tag "n")."""
import properties as _properties

SUBSETS = ["random", "uniformCER", "uniformCERglobal", "randomglobal", "rangeCER", "uniformEntropy", "topKCER"]
WEIGHTGEN = ["levenshtein", "self_attention", "decaying"]

# (flag, kwargs, which CLIs carry it: "p" = patch_cli, "a" = area_cli)
FLAGS = [
    ("--batch_size", dict(type=int, default=32, help="input batch size"), "a"),
    ("--lr_crnn", dict(type=float, default=0.0001, help="CRNN learning rate, not used by adadealta"), "pa"),
    ("--scalar", dict(type=float, default=1, help="scalar in which the secondary loss is multiplied"), "pa"),
    ("--lr_prep", dict(type=float, default=0.00005, help="prep model learning rate, not used by adadealta"), "pa"),
    ("--epoch", dict(type=int, default={"p": 25, "a": 50}, help="number of epochs"), "pa"),
    ("--random_seed", dict(type=int, default=42, help="Random seed for experiment"), "pa"),
    ("--warmup_epochs", dict(type=int, default=0, help="number of warmup epochs"), "pa"),
    ("--std", dict(type=int, default=5, help="standard deviation of Gaussian noice added to images (this value devided by 100)"), "pa"),
    ("--inner_limit", dict(type=int, default=2, help="number of inner loop iterations in Alogorithm 1"), "pa"),
    ("--inner_limit_skip", dict(action="store_true", help="In the first inner limit loop, do NOT add noise to the image"), "pa"),
    ("--crnn_model", dict(help="specify non-default CRNN model location. By default, a new CRNN model will be used"), "pa"),
    ("--prep_model", dict(help="specify non-default Prep model location. By default, a new Prep model will be used"), "pa"),
    ("--exp_base_path", dict(default=".", help="Base path for experiment. Defaults to current directory"), "pa"),
    ("--ocr", dict(default="Tesseract", help="performs training labels from given OCR [Tesseract,EasyOCR,gvision,stub]"), "pa"),
    ("--random_std", dict(action="store_false", help="randomly selected integers from 0 upto given std value (devided by 100) will be used"), "pa"),
    ("--minibatch_subset", dict(choices=SUBSETS, help="Specify method to pick subset from minibatch."), "pa"),
    ("--minibatch_subset_prop", dict(default=0.5, type=float, help="If --minibatch_subset is provided, specify percentage of samples per mini-batch."), "pa"),
    ("--start_epoch", dict(type=int, default=0, help="Starting epoch. If loading from a ckpt, pass the ckpt epoch here."), "pa"),
    ("--data_base_path", dict(default=".", help="Base path training, validation and test data"), "pa"),
    ("--exp_name", dict(default={"p": "test_patch", "a": "test_area"}, help="Specify name of experiment (JVP Jitter, Sample Dropping Etc.)"), "pa"),
    ("--exp_id", dict(help="Specify unique experiment ID"), "pa"),
    ("--train_subset_size", dict(type=int, help="Subset of training size to use"), "pa"),
    ("--val_subset_size", dict(type=int, help="Subset of val size to use"), "pa"),
    ("--weight_decay", dict(type=float, default=5e-4, help="Weight Decay for the optimizer"), "p"),
    ("--cers_ocr_path", dict(help="Cer information json"), "pa"),
    ("--image_prop", dict(type=float, help="Proportion of images per epoch"), "p"),
    ("--discount_factor", dict(type=float, default=1, help="Discount factor for CER values"), "p"),
    ("--update_CRNN", dict(action="store_true", help="Update CRNN along with the preprocessor"), "p"),
    ("--window_size", dict(type=int, default=1, help="Window size if tracking is enabled"), "pa"),
    ("--query_dim", dict(type=int, default=32, help="Dimension of the query/key projection (attention weight generator)"), "p"),
    ("--emb_dim", dict(type=int, default=256, help="Character embedding dimension (attention weight generator)"), "p"),
    ("--attn_activation", dict(default="sigmoid", help="Activation of the attention weight generator"), "p"),
    ("--weightgen_method", dict(choices=WEIGHTGEN, default="decaying", help="Method for generating loss weights for tracking"), "pa"),
    ("--decay_factor", dict(type=float, default=0.7, help="Decay factor for decaying loss weight generation"), "pa"),
    ("--optim_crnn_path", dict(help="CRNN optimizer state to resume from"), "p"),
    ("--optim_prep_path", dict(help="Preprocessor optimizer state to resume from"), "p"),
    ("--pruning_artifact", dict(help="Name of the pruning artifact (subset of the training set)"), "p"),
    ("--lr_scheduler", dict(choices=["cosine"], help="Learning-rate scheduler for the CRNN"), "a"),
    # ---- new (additive) ----
    ("--synthetic_size", dict(type=int, help="[new] train on N synthetic samples instead of reading --data_base_path"), "pa"),
    ("--entropies_path", dict(help="[new] --minibatch_subset uniformEntropy: start from this name -> entropy table (the cers/entropies.json "
                                   "an earlier run wrote) instead of an empty one, where every strip counts as entropy 1.0"), "pa"),
    ("--select_before_clean", dict(action="store_true", help="[new] Phase A: pick the TopKCER / rangeCER / uniformEntropy / random subset FIRST and run the cleaner only on "
                                                             "the picked images (the pick depends on names and CERs alone; eval-mode BatchNorm "
                                                             "makes every image's output independent of the rest of the minibatch)"), "a"),
    ("--per_shard_topk", dict(action="store_true", help="[new] data-parallel runs only: pick the TopKCER subset per GPU shard instead of "
                                                        "over the whole minibatch (not the reference's selection; saves one 32 KB all-gather)"), "a"),
    ("--docs_per_step", dict(type=int, default=1, help="[new] documents per optimiser step (the reference hard-codes one, train_nn_patch.py:37). "
                                                      "The N documents go through the cleaner as ONE batch with per-document BatchNorm statistics "
                                                      "and through the CRNN of Phase B as one batch; forward values equal N sequential passes, the "
                                                      "gradients of the N documents accumulate into one Adam step"), "p"),
    ("--graph", dict(action="store_true", help="[new] replay Phase B (cleaner -> CRNN -> CTC + MSE -> backward -> Adam) and the CRNN side of Phase A as ONE hipGraph each per "
                                               "(batch size, width): at the reference's batch sizes (tens of strips) a step is bound by the host "
                                               "time of ~600 launches, which the replay removes; the first two steps of a shape run eagerly, "
                                               "single-process runs only"), "a"),
    ("--no_rebalance_topk", dict(action="store_true", help="[new] data-parallel runs only: process every global TopKCER winner on the rank "
                                                           "that owns it instead of dealing the winners out in equal slices (one all-reduce of "
                                                           "k x 16 KB images); always so with --inner_limit_skip (label histories stay with the owner)"), "a"),
    ("--resident", dict(action="store_true", help="[new] decode every strip of the training and validation ImgDatasets once, keep the 8-bit pixels on "
                                                  "the device and build each minibatch by one launch (datasets/resident.py) instead of the "
                                                  "per-image PIL / numpy / host-to-device path; same batches, same order, same values.  The store reproduces PadWhite(input_size) + "
                                                  "float32 / 255 only: a dataset with another transform is refused"), "a"),
    ("--resident_pack", dict(help="[new] --resident: keep the decoded strips in this .npz pack file (the validation set's in PATH with "
                                  "'.val' before the extension) and reuse it while the files' names, sizes and mtimes are unchanged"), "a"),
    ("--resident_max_gb", dict(type=float, default=8, help="[new] --resident: refuse a pack larger than this many GB"), "a"),
    ("--resident", dict(action="store_true", help="[new] decode every document of the training and validation PatchDatasets once, keep the 8-bit pixels "
                                                  "and the word boxes on the device, build each batch of documents by one launch and cut all strips of a "
                                                  "step by one launch (datasets/resident.py) instead of the per-document PIL / json / host-to-device "
                                                  "path; same batches, same order, same values.  The store reproduces PatchDataset's white 400x512 "
                                                  "canvas + float32 / 255 only: any other training set is refused"), "p"),
    ("--resident_pack", dict(help="[new] --resident: keep the decoded documents in this .npz pack file (the validation set's in PATH with "
                                  "'.val' before the extension) and reuse it while the files' names, sizes and mtimes are unchanged"), "p"),
    ("--resident_max_gb", dict(type=float, default=8, help="[new] --resident: refuse a pack larger than this many GB"), "p"),
]

# the warm-up and evaluation drivers: "c" = train_crnn.py (:217-275), "e" = eval_crnn.py, "v" = eval_prep.py (their __main__ blocks).
# Kept apart from the trainers' entries above, whose defaults and help differ for several shared names (--ocr, --batch_size, ...).
FLAGS += [
    ("--batch_size", dict(type=int, default=32, help="input batch size"), "c"),
    ("--batch_size", dict(type=int, default=64, help="Inference batch size"), "ev"),
    ("--lr", dict(type=float, default=0.0001, help="learning rate, not used by adadealta"), "c"),
    ("--epoch", dict(type=int, default=50, help="number of epochs"), "c"),
    ("--std", dict(type=int, default=5, help="standard deviation of Gussian noice added to images (this value devided by 100)"), "c"),
    ("--random_seed", dict(type=int, default=42, help="random seed for shuffles"), "c"),
    ("--ocr", dict(help="performs training lebels from given OCR [Tesseract,EasyOCR,stub]"), "c"),
    ("--ocr", dict(default="Tesseract", help="performs training lebels from given OCR [Tesseract,EasyOCR,stub]"), "ev"),
    ("--train_subset", dict(type=int, help="Specify subset of training samples"), "c"),
    ("--val_subset", dict(type=int, help="Specify subset of validation samples"), "c"),
    ("--dataset", dict(default="pos", help="performs training with given dataset [pos, vgg]"), "c"),
    ("--dataset", dict(default="pos", help="evaluates on the given dataset [pos, vgg, pos_textarea]"), "e"),
    ("--dataset", dict(default="patch_dataset", help="evaluates on the given dataset [patch_dataset, vgg, wildreceipt]"), "v"),
    ("--random_std", dict(action="store_false", default=True,
                          help="randomly selected integers from 0 upto given std value (devided by 100) will be used"), "c"),
    ("--crnn_model_path", dict(default=_properties.crnn_model_path, help="CRNN model save path. Default picked from properties"), "c"),
    ("--data_base_path", dict(default=".", help="Base path training, validation and test data"), "cev"),
    ("--ckpt_path", dict(help="Path to CRNN checkpoint"), "c"),
    ("--start_epoch", dict(type=int, default=-1, help="Starting epoch. If loading from a ckpt, pass the ckpt epoch here."), "c"),
    ("--show_txt", dict(action="store_true", help="prints predictions and groud truth"), "ev"),
    ("--show_img", dict(action="store_true", help="shows each batch of images"), "ev"),
    ("--crnn_path", dict(default=_properties.crnn_model_path, help="specify non-default CRNN model location"), "e"),
    ("--crnn_model_name", dict(default="prep_tesseract_pos", help="CRNN model name"), "e"),
    ("--prep_path", dict(default=_properties.prep_model_path, help="specify non-default prep model location"), "v"),
    ("--show_orig", dict(action="store_true", help="Show original flow evaluation"), "ev"),
    # ---- new (additive) ----
    ("--synthetic_size", dict(type=int, help="[new] use N synthetic samples (datasets/synthetic.py) instead of reading --data_base_path"), "cev"),
    ("--beam", dict(type=int, default=0, help="[new] decode with a CTC prefix beam search of K entries (1..32) instead of the greedy best path: the most "
                                              "probable labelling, its log-probability, and how many strips it reads differently from greedy; "
                                              "0 = greedy"), "e"),
    ("--lm", dict(help="[new] --beam K: fuse the character n-gram model of this file (written by lm_cli.py) into the prefix beam search: a "
                       "candidate is ranked by its CTC log-probability plus lm_weight * log P(c | context) + lm_bonus per character"), "e"),
    ("--lm_weight", dict(type=float, default=1.0, help="[new] --lm: weight of the model's log-probabilities"), "e"),
    ("--lm_bonus", dict(type=float, default=0.0, help="[new] --lm: bonus per character (the model has no end-of-word term: this is the "
                                                      "length control)"), "e"),
    ("--lexicon", dict(help="[new] --beam K: keep the prefix beam search inside the word list of this file (written by lexicon_cli.py) and read "
                            "each strip as its best-ranked entry that is a word of the list; a strip with none among its K reads as the plain "
                            "beam's best.  Not together with --lm"), "e"),
    ("--graph", dict(action="store_true", help="[new] replay the warm-up step (CRNN -> CTC -> backward -> Adam) as ONE hipGraph per (batch size, "
                                               "width, target-length cap, lr); the first two steps of a shape run eagerly, single-process runs only"),
     "c"),
    ("--resident", dict(action="store_true", help="[new] decode every strip of the training and validation ImgDatasets once, keep the 8-bit pixels on "
                                                  "the device and build each minibatch by one launch (datasets/resident.py) instead of the "
                                                  "per-image PIL / numpy / host-to-device path; same batches, same order, same values.  The store reproduces PadWhite(input_size) + "
                                                  "float32 / 255 only: a dataset with another transform is refused"), "c"),
    ("--resident_pack", dict(help="[new] --resident: keep the decoded strips in this .npz pack file (the validation set's in PATH with "
                                  "'.val' before the extension) and reuse it while the files' names, sizes and mtimes are unchanged"), "c"),
    ("--resident_max_gb", dict(type=float, default=8, help="[new] --resident: refuse a pack larger than this many GB"), "c"),
]

# the dataset pruner: "r" = pruning/prune_dataset.py (its __main__ block, :88-106)
FLAGS += [
    ("--prune_method", dict(choices=["topk", "FL"], default="topk", help="Pruning method"), "r"),
    ("--prune_prop", dict(type=int, default=10, help="Proportion of samples to be pruned"), "r"),
    ("--dataset", dict(choices=["vgg", "pos"], help="Name of dataset to be pruned"), "r"),
    ("--cers_tess_path", dict(required=True, help="Path to text strip cers information with respect to Tesseract"), "r"),
    # ---- new (additive) ----
    ("--backend", dict(choices=["hip", "cpu"], help="[new] where the FL selection runs: hip = the device kernel (qea_facility_select), cpu = the "
                                                    "same definition in numpy fp64 (forms the n x n matrix); default: hip when a device is present"), "r"),
    ("--features", dict(choices=["mean", "history"], default="mean",
                        help="[new] FL feature of a document: mean = its mean CER (the reference); history = the means of its strips' CERs over "
                             "the last --history_len epochs of a trainer's all_cers.json (name -> list of per-epoch CERs)"), "r"),
    ("--history_len", dict(type=int, default=8, help="[new] --features history: epochs per feature row (1..32)"), "r"),
]


# [new] whole pages through the cleaner, tile by tile (qea/pages.py): "n" = clean_cli.py; --tile also on "v" = eval_prep.py
FLAGS += [
    ("--prep_path", dict(default=_properties.prep_model_path, help="[new] the trained preprocessor (a whole-module checkpoint)"), "n"),
    ("--in_dir", dict(required=True, help="[new] folder of scans: every png / jpg / jpeg in it is cleaned"), "n"),
    ("--out_dir", dict(required=True, help="[new] folder for the cleaned pages: 8-bit grey PNGs of the same sizes and stems"), "n"),
    ("--tile", dict(type=int, nargs=2, metavar=("H", "W"), default=[1024, 1024],
                    help="[new] largest tile of the tiled eval-mode pass: multiples of 16, at least 208 each"), "n"),
    ("--tile", dict(type=int, nargs=2, metavar=("H", "W"),
                    help="[new] send the images through the tiled whole-page pass (qea/pages.py: clean_pages) with tiles of at most H x W "
                         "(multiples of 16, at least 208): documents of any size evaluate instead of raising"), "v"),
    ("--batch_pages", dict(type=int, default=8, help="[new] pages decoded, cleaned and written per call of clean_pages"), "n"),
]

# [new] the classic binarisers as baselines (qea/binarize.py): an extra column of eval_prep.py, another method of clean_cli.py
FLAGS += [
    ("--baseline", dict(choices=["otsu", "sauvola"], help="[new] also send the same images through this classic binariser (qea/binarize.py: "
                                                         "binarize_pages) and the OCR engine, and print its correct count and CER beside the cleaner's"), "v"),
    ("--baseline_window", dict(type=int, default=25, help="[new] --baseline sauvola: window side, odd, 3..127"), "v"),
    ("--baseline_k", dict(type=float, default=0.2, help="[new] --baseline sauvola: k, strictly between 0 and 1"), "v"),
    ("--method", dict(choices=["unet", "otsu", "sauvola"], default="unet",
                      help="[new] unet: the trained preprocessor of --prep_path; otsu / sauvola: a classic binariser instead (no checkpoint is "
                           "loaded, --tile is ignored)"), "n"),
    ("--window", dict(type=int, default=25, help="[new] --method sauvola: window side, odd, 3..127"), "n"),
    ("--k", dict(type=float, default=0.2, help="[new] --method sauvola: k, strictly between 0 and 1"), "n"),
]

# [new] connected components (qea/components.py): the area filter every classic pipeline puts behind its binariser, and word boxes
FLAGS += [
    ("--baseline_despeckle", dict(type=int, default=0, help="[new] --baseline: also turn connected components (connectivity 8) of fewer than N ink "
                                                            "pixels of the binarised image into background; 0 = off"), "v"),
    ("--despeckle", dict(type=int, default=0, help="[new] --method otsu / sauvola: also turn connected components (connectivity 8) of fewer than N "
                                                   "ink pixels into background; 0 = off.  Refused with --method unet, whose output is grey"), "n"),
    ("--boxes", dict(action="store_true", help="[new] also write <stem>.json beside every PNG: the word boxes of the written page (ink = 127 "
                                               "or darker) by run-length smearing and connected components, in the x_min / y_min / x_max / y_max "
                                               "form datasets/patch_dataset.py reads, labels empty"), "n"),
    ("--boxes_gap", dict(type=int, default=8, help="[new] --boxes: horizontal gaps of at most G background pixels join into one word, 0..127"), "n"),
    ("--boxes_min_area", dict(type=int, default=16, help="[new] --boxes: drop words of fewer than A smeared pixels"), "n"),
]

# [new] page skew estimation and deskew (qea/deskew.py): the first stage of clean_cli.py's page pipeline
FLAGS += [
    ("--deskew", dict(action="store_true", help="[new] first estimate every page's skew (projection profiles of its Otsu ink over the slopes "
                                                "a / 1024) and rotate it about its centre, so that the cleaner or the binariser and --boxes see "
                                                "horizontal lines; prints '<stem>: slope a/1024' per page"), "n"),
    ("--deskew_max_slope", dict(type=int, default=90, help="[new] --deskew: the candidates are a = -A..A in 1024ths, 0..256 (90 = +-5.0 degrees)"), "n"),
    ("--deskew_min_gain", dict(type=int, default=0, help="[new] --deskew: rotate only if the best score exceeds the unrotated page's by G per "
                                                         "cent, 0..10000"), "n"),
    ("--deskew_interp", dict(choices=["bilinear", "nearest"], default="bilinear", help="[new] --deskew: how the rotation resamples"), "n"),
]

# [new] reading the word boxes with the CRNN (qea/reading.py): the last stage of clean_cli.py's page pipeline
FLAGS += [
    ("--read", dict(metavar="CRNN_CHECKPOINT", help="[new] implies --boxes: cut every word box of the written page into a 32-row strip (taller "
                                                    "boxes shrunk by the exact area average), read the strips with this CRNN (a whole-module "
                                                    "checkpoint) and write what it reads as the boxes' labels; prints '<stem>: N words read, M "
                                                    "cut' per page"), "n"),
    ("--read_beam", dict(type=int, default=0, help="[new] --read: decode with a CTC prefix beam search of K entries (1..32) and also write each "
                                                   "label's log-score; 0 = greedy"), "n"),
    ("--read_lm", dict(help="[new] --read --read_beam K: fuse the character n-gram model of this file (written by lm_cli.py) into the search"), "n"),
    ("--read_lm_weight", dict(type=float, default=1.0, help="[new] --read_lm: weight of the model's log-probabilities"), "n"),
    ("--read_lm_bonus", dict(type=float, default=0.0, help="[new] --read_lm: bonus per character"), "n"),
    ("--read_lexicon", dict(help="[new] --read --read_beam K: keep the search inside the word list of this file (written by lexicon_cli.py).  Not "
                                 "together with --read_lm"), "n"),
    ("--read_buckets", dict(type=int, nargs="+", metavar="W", help="[new] --read: the strip widths, ascending multiples of 16 in 64..512 "
                                                                   "(default 128 256 384 512); a word wider than the last loses its sides"), "n"),
    ("--read_chars", dict(action="store_true", help="[new] --read: align every label to the scores it was decoded from (CTC forced alignment) and "
                                                    "add 'chars': [{c, x_min, x_max, conf}] to each row: the character's columns on the page "
                                                    "(x_max exclusive) and the mean of its log-probabilities"), "n"),
]

# [new] word boxes grouped into text lines and the page's plain text (qea/lines.py): what makes the rows of <stem>.json readable in order
FLAGS += [
    ("--lines", dict(action="store_true", help="[new] implies --boxes: group the word boxes of every page into text lines (neighbours along x "
                                               "that overlap vertically), write the rows of <stem>.json in reading order, each with its "
                                               "'line', and print '<stem>: L lines' per page.  Meant for level or --deskew'ed pages"), "n"),
    ("--lines_overlap", dict(type=int, help="[new] --lines: per cent of the smaller height two boxes must share vertically to be "
                                                        "neighbours, 1..100 (default 50)"), "n"),
    ("--lines_tall", dict(type=int, help="[new] --lines: a box taller than this many median heights (a rule, a picture, a drop cap) "
                                                    "is a line of its own, 1..64 (default 3)"), "n"),
    ("--lines_gap", dict(type=int, help="[new] --lines: the largest horizontal gap between neighbours of one line, in median "
                                                   "heights, 1..1024; 0 = no limit (default)"), "n"),
    ("--text", dict(action="store_true", help="[new] needs --read, implies --lines: also write <stem>.txt, the words the CRNN read, line by "
                                              "line in reading order"), "n"),
]


def build_parser(which, description):
    import argparse
    ap = argparse.ArgumentParser(description=description)
    for flag, kw, where in FLAGS:
        if which not in where:
            continue
        kw = dict(kw)
        if isinstance(kw.get("default"), dict):
            kw["default"] = kw["default"][which]
        ap.add_argument(flag, **kw)
    return ap
