"""CRNN evaluation — MI355X-native drop-in for the reference's eval_crnn.py.

`EvalCRNN(args).eval()` with the reference's flags (qea/cli_flags.py tag "e"):
  * --dataset vgg / pos_textarea: batches of the test strips (ImgDataset) -> eval-mode CRNN -> greedy decode on the device
    (utils.pred_to_string) -> exact-match count and CER against the ground truth;
  * --dataset pos: PatchDataset(pad=True) documents, each cut into its word strips on the device (utils.get_text_stack) -> the
    same, one CRNN batch per document (its strip count varies from document to document);
  * --show_orig also runs the OCR engine on the same strips.
The printed lines are the reference's.  Differences, all deliberate:
  * [new] eval() also RETURNS the numbers as a dict: count, crnn_correct, crnn_accuracy, crnn_cer (CER averaged over the strips),
    and with --show_orig ocr_correct, ocr_accuracy, ocr_cer.
  * The pos flow's CER: the reference replaces its running sum by round(sum / strips of this document, 2) after every document, so
    the printed average is neither a mean nor a sum; here the sum runs over all strips and is divided once, as in the area flow.
  * --show_txt without --show_orig prints the predictions (the reference reads an unassigned variable there).
  * [new] --synthetic_size N evaluates on N synthetic strips / documents (datasets/synthetic.py).
  * [new] --beam K decodes all three flows with a CTC prefix beam search of K entries (utils.pred_to_string(beam=K): the device kernel
    of csrc/ctc_beam.hip for CUDA scores) instead of the greedy best path: the strings are the most probable LABELLINGS.  The dict then
    also has beam, crnn_mean_log_score (the mean log-probability of those labellings) and greedy_disagreements (the strips whose
    greedy string differs), and one more line is printed.  Without the flag nothing changes.
  * [new] --lm PATH (with --beam K) fuses the character n-gram model of that file (qea/lm.py, written by lm_cli.py) into the search,
    weight --lm_weight, per-character bonus --lm_bonus: the strings are the fused search's.  The dict then also has lm_order,
    lm_weight, lm_bonus, crnn_mean_total_score (the mean of the scores the search ranked by) and lm_disagreements (the strips the plain
    beam of the same K reads differently); crnn_mean_log_score stays the mean CTC log-probability of the chosen readings.
  * [new] --lexicon PATH (with --beam K, not with --lm) keeps the search inside the word list of that file (qea/lexicon.py, written by
    lexicon_cli.py; utils.pred_to_string(beam=K, lexicon=)): a strip reads as its best-ranked entry that is a word of the list, and
    as the plain beam's best where none of its K is.  The dict then also has lexicon_words, lexicon_misses (the strips with no word
    among their K), lexicon_disagreements (the strips the plain beam of the same K reads differently) and lexicon_oov_labels (the
    ground-truth labels that are not in the list: they bound the accuracy).
  * The loaders run in the main process (the reference asks for properties.num_workers workers).
`backend` / `dataset` / `ocr` are injection seams for tests, as in the trainers; the default backend is the HIP path.
"""
import os

import torch

import properties
from qea.trainer_core import hip_backend
from utils import beam_decode_lm, compare_labels, lexicon_best, get_char_maps, get_ocr_helper, get_text_stack, pred_to_string, show_img


class EvalCRNN:
    def __init__(self, args, backend=None, dataset=None, ocr=None):
        self.batch_size = args.batch_size
        self.show_txt = args.show_txt
        self.show_img = args.show_img
        self.crnn_model_name = args.crnn_model_name
        self.crnn_model_path = args.crnn_path
        self.ocr_name = args.ocr
        self.dataset_name = args.dataset
        self.show_orig = args.show_orig
        self.beam = int(getattr(args, "beam", 0) or 0)               # [new] --beam K: prefix beam search instead of greedy
        self.beam_log_score, self.greedy_disagreements = 0.0, 0
        self.lm_path = getattr(args, "lm", None)                     # [new] --lm PATH: a character n-gram model fused into the search
        self.lm_weight, self.lm_bonus = float(getattr(args, "lm_weight", 1.0)), float(getattr(args, "lm_bonus", 0.0))
        self.lm, self.beam_total_score, self.lm_disagreements = None, 0.0, 0
        if self.lm_path and not self.beam:
            raise ValueError("--lm needs --beam K: the model is fused into the prefix beam search")
        self.lexicon_path = getattr(args, "lexicon", None)           # [new] --lexicon PATH: the search stays inside a word list
        self.lexicon, self.lexicon_misses, self.lexicon_disagreements, self.lexicon_oov_labels = None, 0, 0, 0
        if self.lexicon_path and (not self.beam or self.lm_path):
            raise ValueError("--lexicon needs --beam K and cannot be combined with --lm")
        self.input_size = properties.input_size
        if self.dataset_name == "vgg":
            self.test_set = os.path.join(args.data_base_path, properties.vgg_text_dataset_test)
        elif self.dataset_name == "pos":
            self.test_set = os.path.join(args.data_base_path, properties.patch_dataset_test)
        elif self.dataset_name == "pos_textarea":
            self.test_set = os.path.join(args.data_base_path, properties.pos_text_dataset_test)
        else:
            raise ValueError(f"--dataset {self.dataset_name!r}: one of pos, vgg, pos_textarea")

        self.device = (backend or hip_backend()).device
        self.crnn_model = torch.load(os.path.join(self.crnn_model_path, self.crnn_model_name), weights_only=False).to(self.device)
        print(f"OCR name - {self.ocr_name}")
        self.ocr = ocr if ocr is not None else get_ocr_helper(self.ocr_name, is_eval=True)
        print(self.ocr)
        self.char_to_index, self.index_to_char, self.vocab_size = get_char_maps(properties.char_set)
        if self.lm_path:
            from qea.lm import CharLM
            self.lm = CharLM.load(self.lm_path, self.char_to_index)
        if self.lexicon_path:
            from qea.lexicon import Lexicon
            self.lexicon = Lexicon.load(self.lexicon_path, self.char_to_index)

        n = getattr(args, "synthetic_size", None)
        if self.dataset_name == "pos":
            if dataset is None and n:
                from datasets.synthetic import SyntheticPatches
                dataset = SyntheticPatches(n, seed=3, include_name=False)
            elif dataset is None:
                from datasets.patch_dataset import PatchDataset
                dataset = PatchDataset(self.test_set, pad=True)
            self.dataset = dataset
        else:
            if dataset is None and n:
                from datasets.synthetic import SyntheticTextAreas
                dataset = SyntheticTextAreas(n, seed=3, include_name=True)
            elif dataset is None:
                from datasets._io import to_tensor
                from datasets.img_dataset import ImgDataset
                from transform_helper import PadWhite
                dataset = ImgDataset(self.test_set, transform=lambda img: to_tensor(PadWhite(self.input_size)(img)), include_name=True)
            self.dataset = dataset
            self.loader_eval = torch.utils.data.DataLoader(self.dataset, batch_size=self.batch_size)

    def _scores(self, images):
        return self.crnn_model(images.to(self.device))

    def _decode(self, scores, labels):
        """The strings the CRNN reads: greedy, or with --beam K the best entry of the prefix beam search; that flow also adds up the
        entries' log-probabilities and counts the strips that greedy reads differently."""
        if not self.beam:
            return pred_to_string(scores, labels, self.index_to_char)
        greedy = pred_to_string(scores, labels, self.index_to_char)
        if self.lm is not None:                                       # rank 0 of the fused search, its CTC score and its total
            tokens, lengths, ctc, total = (v[:, 0].cpu().tolist() for v in beam_decode_lm(scores, self.beam, self.lm, self.lm_weight, self.lm_bonus))
            preds = ["".join(self.index_to_char[i] for i in tk[:max(n, 0)]) for tk, n in zip(tokens, lengths)]
            plain = pred_to_string(scores, labels, self.index_to_char, beam=self.beam)
            self.beam_log_score += sum(ctc)
            self.beam_total_score += sum(total)
            self.lm_disagreements += sum(int(p != q) for p, q in zip(preds, plain))
            self.greedy_disagreements += sum(int(p != q) for p, q in zip(preds, greedy))
            return preds
        if self.lexicon is not None:                                  # the best-ranked word of the list, the plain beam's best on a miss
            tokens, lengths, logp, miss = (v.cpu().tolist() for v in lexicon_best(scores, self.beam, self.lexicon))
            preds = ["".join(self.index_to_char[i] for i in tk[0][:max(n[0], 0)]) for tk, n in zip(tokens, lengths)]
            plain = pred_to_string(scores, labels, self.index_to_char, beam=self.beam)
            self.beam_log_score += sum(lp[0] for lp in logp)
            self.lexicon_misses += sum(int(m) for m in miss)
            self.lexicon_disagreements += sum(int(p != q) for p, q in zip(preds, plain))
            self.lexicon_oov_labels += sum(int(not self.lexicon.accepts_string(l, self.char_to_index)) for l in labels)
            self.greedy_disagreements += sum(int(p != q) for p, q in zip(preds, greedy))
            return preds
        preds, logp = pred_to_string(scores, labels, self.index_to_char, beam=self.beam, return_scores=True)
        self.beam_log_score += sum(logp)
        self.greedy_disagreements += sum(int(p != q) for p, q in zip(preds, greedy))
        return preds

    def _print_labels(self, labels, pred, ori):
        print()
        print("{:<25}{:<25}{:<25}".format("GT Label", "Label for pred", "Label for original"))
        for i in range(len(labels)):
            print("{:<25}{:<25}{:<25}".format(labels[i], pred[i] if i < len(pred) else "*******", ori[i] if i < len(ori) else ""))

    def _result(self, count, crnn_correct, crnn_cer, ori_correct, ori_cer):
        res = {"count": count, "crnn_correct": crnn_correct, "crnn_accuracy": crnn_correct / max(1, count),
               "crnn_cer": crnn_cer / max(1, count)}
        if self.show_orig:
            res.update(ocr_correct=ori_correct, ocr_accuracy=ori_correct / max(1, count), ocr_cer=ori_cer / max(1, count))
        if self.beam:
            res.update(beam=self.beam, crnn_mean_log_score=self.beam_log_score / max(1, count), greedy_disagreements=self.greedy_disagreements)
            print("Beam {:d}: mean log-probability of the best labelling {:.5f}, differs from greedy on {:d}/{:d} strips".format(
                self.beam, res["crnn_mean_log_score"], self.greedy_disagreements, count))
        if self.lm is not None:
            res.update(lm_order=self.lm.order, lm_weight=self.lm_weight, lm_bonus=self.lm_bonus,
                       crnn_mean_total_score=self.beam_total_score / max(1, count), lm_disagreements=self.lm_disagreements)
            print("Character {:d}-gram fused (weight {:g}, bonus {:g}): mean total score {:.5f}, differs from the plain beam on {:d}/{:d} strips".format(
                self.lm.order, self.lm_weight, self.lm_bonus, res["crnn_mean_total_score"], self.lm_disagreements, count))
        if self.lexicon is not None:
            res.update(lexicon_words=self.lexicon.num_words, lexicon_misses=self.lexicon_misses,
                       lexicon_disagreements=self.lexicon_disagreements, lexicon_oov_labels=self.lexicon_oov_labels)
            print("Lexicon of {} words: no word among the {:d} entries of {:d}/{:d} strips, differs from the plain beam on {:d}, {:d} labels "
                  "are not in the lexicon".format(self.lexicon.num_words, self.beam, self.lexicon_misses, count, self.lexicon_disagreements,
                                                  self.lexicon_oov_labels))
        return res

    def eval_area(self):
        print("Eval with ", self.ocr_name)
        self.crnn_model.eval()
        self.beam_log_score, self.greedy_disagreements, self.beam_total_score, self.lm_disagreements = 0.0, 0, 0.0, 0
        self.lexicon_misses, self.lexicon_disagreements, self.lexicon_oov_labels = 0, 0, 0
        crnn_correct_count, ori_correct_count, ori_cer, crnn_cer = 0, 0, 0.0, 0.0
        with torch.no_grad():
            for batch in self.loader_eval:
                images, labels = batch[0], list(batch[1])
                scores = self._scores(images)
                ocr_lbl_crnn = self._decode(scores, labels)
                ocr_lbl_ori = []
                if self.show_orig:
                    ocr_lbl_ori = self.ocr.get_labels(images.cpu())
                    c, e = compare_labels(ocr_lbl_ori, labels)
                    ori_correct_count += c
                    ori_cer += e
                if self.show_txt:
                    self._print_labels(labels, ocr_lbl_crnn, ocr_lbl_ori)
                c, e = compare_labels(ocr_lbl_crnn, labels)
                crnn_correct_count += c
                crnn_cer += e
        n = len(self.dataset)
        print()
        print("Correct count from CRNN: {:d}/{:d} ({:.5f})".format(crnn_correct_count, n, crnn_correct_count / n))
        if self.show_orig:
            print("Correct count from Tesseract: {:d}/{:d} ({:.5f})".format(ori_correct_count, n, ori_correct_count / n))
            print("Average CER using Tesseract: {:.5f}".format(ori_cer / n))
        print("Average CER using CRNN: {:.5f}".format(crnn_cer / n))
        return self._result(n, crnn_correct_count, crnn_cer, ori_correct_count, ori_cer)

    def eval_patch(self):
        print("Eval with ", self.ocr_name)
        self.crnn_model.eval()
        self.beam_log_score, self.greedy_disagreements, self.beam_total_score, self.lm_disagreements = 0.0, 0, 0.0, 0
        self.lexicon_misses, self.lexicon_disagreements, self.lexicon_oov_labels = 0, 0, 0
        ori_lbl_crt_count, ori_lbl_cer, lbl_count, crnn_correct_count, crnn_cer = 0, 0.0, 0, 0, 0.0
        with torch.no_grad():
            for i in range(len(self.dataset)):
                image, labels_dict = self.dataset[i][:2]
                text_crops, labels = get_text_stack(image.detach().to(self.device), labels_dict, self.input_size)
                lbl_count += len(labels)
                if self.show_orig:
                    ocr_labels = self.ocr.get_labels(text_crops.cpu())
                    c, e = compare_labels(ocr_labels, labels)
                    ori_lbl_crt_count += c
                    ori_lbl_cer += e
                scores = self._scores(text_crops)
                ocr_lbl_crnn = self._decode(scores, labels)
                c, e = compare_labels(ocr_lbl_crnn, labels)
                crnn_correct_count += c
                crnn_cer += e
                if self.show_img:
                    show_img(image.cpu())
        print()
        print("Correct count from predicted images: {:d}/{:d} ({:.5f})".format(crnn_correct_count, lbl_count, crnn_correct_count / lbl_count))
        if self.show_orig:
            print("Correct count from original images: {:d}/{:d} ({:.5f})".format(ori_lbl_crt_count, lbl_count, ori_lbl_crt_count / lbl_count))
            print("Average CER from original images: ({:.5f})".format(ori_lbl_cer / lbl_count))
        print("Average CER from predicted images: ({:.5f})".format(crnn_cer / lbl_count))
        return self._result(lbl_count, crnn_correct_count, crnn_cer, ori_lbl_crt_count, ori_lbl_cer)

    def eval(self):
        if self.dataset_name == "pos":
            return self.eval_patch()
        return self.eval_area()


def build_parser():
    from qea.cli_flags import build_parser as _build
    return _build("e", "Evaluates a CRNN model")


if __name__ == "__main__":
    args = build_parser().parse_args()
    print(args)
    evaluator = EvalCRNN(args)
    evaluator.eval()
