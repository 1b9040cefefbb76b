"""Preprocessor evaluation — MI355X-native drop-in for the reference's eval_prep.py.

`EvalPrep(args).eval()` with the reference's flags (qea/cli_flags.py tag "v"):
  * --dataset vgg: batches of test strips -> eval-mode UNet (BatchNorm folded into the conv epilogue) -> the OCR engine on the
    cleaned strips -> exact-match count and CER against the ground truth;
  * --dataset patch_dataset / wildreceipt: each document [1,1,400,512] -> eval-mode UNet -> word strips cut on the device
    (utils.get_text_stack) -> the OCR engine (documents are padded, never resized: PatchDataset(pad=True, resize_images=False));
    for wildreceipt the spaces are stripped from the OCR's labels;
  * --show_orig also runs the OCR on the uncleaned strips.
Returns (accuracy, cer) of the cleaned strips, as the reference's patch flow does.  Differences, all deliberate:
  * [new] the area flow returns the same pair (the reference returns None).
  * The area flow's --show_orig: the reference adds to `ori_lbl_cer` before assigning it and divides the original strips' CER
    twice (by the batch, then by the set); here it is summed over the strips and divided once by the set size.
  * A document whose size is not a multiple of 16 raises the UNet's ValueError with the file's name added (the reference fails
    on it too); it is not padded silently.
  * [new] --tile H W sends the images of both flows through the tiled whole-page pass (qea/pages.py: clean_pages) instead: a document
    of ANY size evaluates, as the eval-mode pass over the page padded with white to the next multiple of 16 and cropped back.  Without
    the flag nothing changes, the ValueError included.
  * [new] --baseline {otsu,sauvola} [--baseline_window W --baseline_k K] also sends the same images through a classic binariser
    (qea/binarize.py: binarize_pages) and the OCR engine, prints "Correct count from <method> images" / "Average CER from <method>
    images" and sets self.baseline_result = (accuracy, cer).  Area flow: every strip of the batch is its own page.  Patch flow: the
    document the model sees is binarised as a whole, then cut by get_text_stack, so window statistics come from the page, not from
    the crop.  Return values and the other prints stay as they are.
  * [new] --baseline_despeckle N (only with --baseline) puts the area filter of every classic pipeline behind the binariser: connected
    components of fewer than N ink pixels become background (binarize_pages(despeckle=N)); the printed method name becomes e.g.
    "sauvola+despeckle4".
  * [new] --synthetic_size N evaluates on N synthetic strips / documents (datasets/synthetic.py).
  * The loaders run in the main process (the reference asks for properties.num_workers workers).
`backend` / `dataset` / `ocr` are injection seams for tests, as in the trainers; the default backend is the HIP path.
"""
import os

import torch

import properties
from qea._lib import QeaError
from qea.binarize import binarize_pages, check_params
from qea.components import check_params as components_check
from qea.pages import clean_pages
from qea.trainer_core import hip_backend
from utils import compare_labels, get_ocr_helper, get_text_stack, show_img


class EvalPrep:
    def __init__(self, args, backend=None, dataset=None, ocr=None):
        self.batch_size = args.batch_size
        self.show_txt = args.show_txt
        self.show_img = args.show_img
        self.prep_model_path = args.prep_path
        self.ocr_name = args.ocr
        self.dataset_name = args.dataset
        self.show_orig = args.show_orig
        self.tile = tuple(args.tile) if getattr(args, "tile", None) else None
        self.input_size = properties.input_size
        self.baseline = getattr(args, "baseline", None)
        self.baseline_args = dict(window=getattr(args, "baseline_window", 25), k=getattr(args, "baseline_k", 0.2))
        self.baseline_result = None
        self.baseline_despeckle = int(getattr(args, "baseline_despeckle", 0) or 0)
        if self.baseline_despeckle and not self.baseline:
            raise ValueError("--baseline_despeckle needs --baseline otsu or sauvola")
        if self.baseline:
            check_params(self.baseline, **self.baseline_args)
        if self.baseline_despeckle:
            components_check(min_area=self.baseline_despeckle)
        self.baseline_name = (self.baseline or "") + (f"+despeckle{self.baseline_despeckle}" if self.baseline_despeckle else "")
        if self.dataset_name == "vgg":
            self.test_set = os.path.join(args.data_base_path, properties.vgg_text_dataset_test)
        elif self.dataset_name == "patch_dataset":
            self.test_set = os.path.join(args.data_base_path, properties.patch_dataset_test)
        elif self.dataset_name == "wildreceipt":
            self.test_set = os.path.join(args.data_base_path, properties.wr_dataset_test)
        else:
            raise ValueError(f"--dataset {self.dataset_name!r}: one of patch_dataset, vgg, wildreceipt")

        self.device = (backend or hip_backend()).device
        self.prep_model = torch.load(self.prep_model_path, map_location=self.device, weights_only=False).to(self.device)
        self.ocr = ocr if ocr is not None else get_ocr_helper(self.ocr_name, is_eval=True)

        n = getattr(args, "synthetic_size", None)
        if dataset is None and n:
            from datasets.synthetic import SyntheticPatches, SyntheticTextAreas
            dataset = SyntheticTextAreas(n, seed=3, include_name=True) if self.dataset_name == "vgg" else SyntheticPatches(n, seed=3)
        elif dataset is None and self.dataset_name in ("patch_dataset", "wildreceipt"):
            from datasets.patch_dataset import PatchDataset
            dataset = PatchDataset(self.test_set, pad=True, include_name=True, resize_images=False)
        elif dataset is None:
            from datasets._io import to_tensor
            from datasets.img_dataset import ImgDataset
            from transform_helper import PadWhite
            dataset = ImgDataset(self.test_set, transform=lambda img: to_tensor(PadWhite(self.input_size)(img)), include_name=True)
        self.dataset = dataset
        if self.dataset_name == "vgg":
            self.loader_eval = torch.utils.data.DataLoader(self.dataset, batch_size=self.batch_size)

    def _print_labels(self, labels, pred, ori):
        print()
        print("{:<25}{:<25}{:<25}".format("GT Label", "Label for pred", "Label for original"))
        for i in range(len(labels)):
            print("{:<25}{:<25}{:<25}".format(labels[i], pred[i] if i < len(pred) else "*******", ori[i] if i < len(ori) else ""))

    def _ocr(self, crops):
        labels = self.ocr.get_labels(crops.cpu())
        if self.dataset_name == "wildreceipt":
            labels = [lbl.replace(" ", "") for lbl in labels]
        return labels

    def _binarize(self, pages):
        """the --baseline binariser over a list of [1, h, w] images -> the same list binarised (fp32 0 / 1), on the backend's device"""
        return binarize_pages(pages, self.baseline, out="float", device=self.device, despeckle=self.baseline_despeckle, **self.baseline_args)

    def _print_baseline(self, correct, cer, n, brackets):
        print("Correct count from {} images: {:d}/{:d} ({:.5f})".format(self.baseline_name, correct, n, correct / n))
        print(("Average CER from {} images: ({:.5f})" if brackets else "Average CER from {} images: {:.5f}").format(self.baseline_name, cer / n))
        self.baseline_result = (correct / n, cer / n)

    def eval_area(self):
        print("Eval with ", self.ocr_name)
        self.prep_model.eval()
        pred_correct_count, ori_correct_count, ori_cer, pred_cer = 0, 0, 0.0, 0.0
        base_correct_count, base_cer = 0, 0.0
        with torch.no_grad():
            for batch in self.loader_eval:
                images, labels = batch[0], list(batch[1])
                if self.tile:
                    img_preds = torch.stack(clean_pages(self.prep_model, list(images), tile=self.tile))
                else:
                    img_preds = self.prep_model(images.to(self.device))
                ocr_lbl_pred = self.ocr.get_labels(img_preds.cpu())
                ocr_lbl_ori = []
                if self.show_orig:
                    ocr_lbl_ori = self.ocr.get_labels(images.cpu())
                    c, e = compare_labels(ocr_lbl_ori, labels)
                    ori_correct_count += c
                    ori_cer += e
                if self.baseline:
                    c, e = compare_labels(self.ocr.get_labels(torch.stack(self._binarize(list(images))).cpu()), labels)
                    base_correct_count += c
                    base_cer += e
                c, e = compare_labels(ocr_lbl_pred, labels)
                pred_correct_count += c
                pred_cer += e
                if self.show_img:
                    show_img(img_preds.detach().cpu(), "Processed images")
                if self.show_txt:
                    self._print_labels(labels, ocr_lbl_pred, ocr_lbl_ori)
        n = len(self.dataset)
        print()
        print("Correct count from predicted images: {:d}/{:d} ({:.5f})".format(pred_correct_count, n, pred_correct_count / n))
        if self.show_orig:
            print("Correct count from original images: {:d}/{:d} ({:.5f})".format(ori_correct_count, n, ori_correct_count / n))
            print("Average CER from original images: {:.5f}".format(ori_cer / n))
        print("Average CER from predicted images: {:.5f}".format(pred_cer / n))
        if self.baseline:
            self._print_baseline(base_correct_count, base_cer, n, brackets=False)
        self.orig_result = (ori_correct_count / n, ori_cer / n) if self.show_orig else None
        return pred_correct_count / n, pred_cer / n

    def eval_patch(self):
        print("Eval with ", self.ocr_name)
        self.prep_model.eval()
        ori_lbl_crt_count, ori_lbl_cer, prd_lbl_crt_count, prd_lbl_cer, lbl_count = 0, 0.0, 0, 0.0, 0
        base_crt_count, base_cer = 0, 0.0
        with torch.no_grad():
            for i in range(len(self.dataset)):
                item = self.dataset[i]
                image, labels_dict = item[0], item[1]
                name = item[2] if len(item) > 2 else f"document {i}"
                image = image.detach().to(self.device)
                ocr_labels = []
                if self.show_orig:
                    text_crops, labels = get_text_stack(image, labels_dict, self.input_size)
                    ocr_labels = self._ocr(text_crops)
                    c, e = compare_labels(ocr_labels, labels)
                    ori_lbl_crt_count += c
                    ori_lbl_cer += e
                try:
                    pred = clean_pages(self.prep_model, [image], tile=self.tile)[0] if self.tile else self.prep_model(image.unsqueeze(0))[0]
                except ValueError as err:
                    raise ValueError(f"{name}: {err}") from err
                try:
                    pred_crops, labels = get_text_stack(pred, labels_dict, self.input_size)
                except QeaError as err:
                    raise ValueError(f"{name} ({pred.shape[-2]}x{pred.shape[-1]}): the device crops refuse this page: {err}") from err
                lbl_count += len(labels)
                if self.baseline:
                    base_crops, _ = get_text_stack(self._binarize([image])[0], labels_dict, self.input_size)
                    c, e = compare_labels(self._ocr(base_crops), labels)
                    base_crt_count += c
                    base_cer += e
                pred_labels = self._ocr(pred_crops)
                c, e = compare_labels(pred_labels, labels)
                prd_lbl_crt_count += c
                prd_lbl_cer += e
                if self.show_img:
                    show_img(image.cpu())
                if self.show_txt:
                    self._print_labels(labels, pred_labels, ocr_labels)
                if not i % 100:
                    print(f"{i} samples completed")
        print()
        print("Correct count from predicted images: {:d}/{:d} ({:.5f})".format(prd_lbl_crt_count, lbl_count, prd_lbl_crt_count / lbl_count))
        if self.show_orig:
            print("Correct count from original images: {:d}/{:d} ({:.5f})".format(ori_lbl_crt_count, lbl_count, ori_lbl_crt_count / lbl_count))
            print("Average CER from original images: ({:.5f})".format(ori_lbl_cer / lbl_count))
        print("Average CER from predicted images: ({:.5f})".format(prd_lbl_cer / lbl_count))
        if self.baseline:
            self._print_baseline(base_crt_count, base_cer, lbl_count, brackets=True)
        self.orig_result = (ori_lbl_crt_count / lbl_count, ori_lbl_cer / lbl_count) if self.show_orig else None
        return prd_lbl_crt_count / lbl_count, prd_lbl_cer / lbl_count

    def eval(self):
        if self.dataset_name in ("patch_dataset", "wildreceipt"):
            return self.eval_patch()
        return self.eval_area()


def build_parser():
    from qea.cli_flags import build_parser as _build
    return _build("v", "Evaluates a trained preprocessor")


if __name__ == "__main__":
    args = build_parser().parse_args()
    print(args)
    evaluator = EvalPrep(args)
    evaluator.eval()
