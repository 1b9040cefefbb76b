"""Text strips labelled by the black-box OCR — same files and sample tuple as the reference's datasets/ocr_dataset.py:14-45:
files `<idx>_<label>_<anything>.png|jpg` (labels over max_char_len dropped at listing time), `num_samples` keeps the first N
files, sample = (image, OCR label[, file_name]) where the OCR label is `ocr_helper.get_labels` of the transformed image.

`OCRRelabelled` (new) gives any dataset with the (image, label, ...) tuple the same treatment (synthetic strips)."""
import os

from torch.utils.data import Dataset

from datasets.img_dataset import ImgDataset


def _ocr_label(ocr_helper, image):
    return ocr_helper.get_labels(image[None] if image.dim() == 3 else image)[0]


class OCRDataset(Dataset):
    def __init__(self, data_dir, ocr_helper, transform=None, include_name=False, num_samples=None):
        self.include_name, self.ocr_helper = include_name, ocr_helper
        self.images = ImgDataset(data_dir, transform=transform, include_name=True)
        if num_samples:
            self.images.files = self.images.files[:num_samples]
        self.files = self.images.files

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        image, _label, file_name = self.images[idx]
        ocr_label = _ocr_label(self.ocr_helper, image)
        return (image, ocr_label, os.path.basename(file_name)) if self.include_name else (image, ocr_label)


class OCRRelabelled(Dataset):
    """[new] dataset[i] = (image, label, *rest) -> (image, OCR label of image, *rest)."""

    def __init__(self, dataset, ocr_helper):
        self.dataset, self.ocr_helper = dataset, ocr_helper

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        item = tuple(self.dataset[idx])
        return (item[0], _ocr_label(self.ocr_helper, item[0])) + item[2:]
