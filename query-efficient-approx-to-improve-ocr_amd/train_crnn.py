"""CRNN warm-up trainer — MI355X-native drop-in for the reference's train_crnn.py.

`TrainCRNN(args).train()` keeps the reference's constructor contract (an argparse Namespace with the flags of
train_crnn.py:217-275, qea/cli_flags.py tag "c"), its loop (:146-214: zero_grad -> CRNN(train BN) -> CTC(mean) -> backward ->
Adam, validation in eval mode, StepLR(10, 0.8) stepped once per epoch after validation) and its whole-module checkpoints
`{crnn_model_path}_{epoch}_{acc*100:.2f}`, and returns (best_val_acc, best_val_epoch).  The checkpoints load through
`--crnn_model` of area_cli.py / patch_cli.py and, having the reference's class paths and state_dict keys, in the reference.

Differences from the reference, all deliberate:
  * Training noise.  The reference jitters each image in the CPU loader (AddGaussianNoice in `noisy_transform`); here the clean
    batch is jittered on the device by ONE Philox launch (AddGaussianNoice.batch) with the per-image sigma drawn on the host by the
    reference's rule.  The normal deviates therefore come from Philox instead of torch.normal: same distribution, other draws
    (as in the preprocessor trainers).  With --ocr the OCR engine labels that noisy batch, as OCRDataset labels
    its noisy items in the reference.  An injected CPU backend keeps the reference's per-image torch.normal draws, in its order.
  * Without --ocr the reference crashes: it passes `num_subset=` to ImgDataset, which has no such argument.  Here
    --train_subset / --val_subset keep the first N samples through a torch.utils.data.Subset.
  * The epoch-summary line divides the summed losses by max(1, set size // batch size) (the reference divides by zero when the
    validation set is smaller than one batch).
  * [new] --synthetic_size N: synthetic strips (datasets/synthetic.py) instead of --data_base_path.
  * [new] --graph: the training step as one hipGraph replay per (batch, width, target-length cap, lr) — qea.graph.PhaseAGraphs with
    one replica group; Adam is built capturable, a StepLR change of the lr records a new graph.  Single process only.
  * [new] --resident: the strips of the ImgDataset training set (and of the validation set, without --ocr) are decoded once and kept
    on the device; every minibatch is one launch (datasets/resident.py).  Same batches, order, RNG draws and values.

As in the preprocessor trainers, `backend` / `train_set` / `val_set` / `ocr` are injection seams for tests: the default backend is
the HIP path (there is no CPU implementation); datasets are (image [1,32,W], ground-truth label, ...) samples.
"""
import os
import random

import numpy as np
import torch

import properties
from qea.trainer_core import hip_backend
from transform_helper import AddGaussianNoice
from utils import compare_labels, get_char_maps, get_ocr_helper, pred_to_string


class TrainCRNN:
    def __init__(self, args, backend=None, train_set=None, val_set=None, ocr=None):
        print("Experiment Arguments")
        print(args)
        self.batch_size = args.batch_size
        self.random_seed = args.random_seed
        self.lr = args.lr
        self.max_epochs = args.epoch
        self.ocr_name = args.ocr
        self.std = args.std
        self.is_random_std = args.random_std
        self.dataset_name = args.dataset
        self.crnn_model_path = args.crnn_model_path
        self.crnn_ckpt_path = args.ckpt_path
        self.start_epoch = args.start_epoch
        self.train_batch_size = self.batch_size

        self.decay = 0.8
        self.decay_step = 10
        torch.manual_seed(self.random_seed)
        np.random.seed(torch.initial_seed())
        random.seed(torch.initial_seed())

        if self.dataset_name == "pos":
            self.train_set = os.path.join(args.data_base_path, properties.pos_text_dataset_train)
            self.validation_set = os.path.join(args.data_base_path, properties.pos_text_dataset_dev)
        elif self.dataset_name == "vgg":
            self.train_set = os.path.join(args.data_base_path, properties.vgg_text_dataset_train)
            self.validation_set = os.path.join(args.data_base_path, properties.vgg_text_dataset_dev)
        self.input_size = properties.input_size
        self.char_to_index, self.index_to_char, self.vocab_size = get_char_maps(properties.char_set)

        self.backend = backend or hip_backend()
        self.device = self.backend.device
        if self.crnn_ckpt_path is None:
            self.model = self.backend.CRNN(self.vocab_size, False).to(self.device)
        else:
            self.model = torch.load(self.crnn_ckpt_path, weights_only=False).to(self.device)
        self.model.register_backward_hook(self.model.backward_hook)          # the fused NaN scrub of infeasible CTC targets

        self.ocr = ocr if ocr is not None else get_ocr_helper(self.ocr_name)
        dataset, validation_set = self._datasets(args, train_set, val_set)
        print(f"Train Dataset - {dataset}")
        print(f"Validation Dataset - {validation_set}")
        self.loader_train = self._loader(args, dataset, "training set", batch_size=self.batch_size, drop_last=True, shuffle=True)
        # with --ocr the validation samples are relabelled by the OCR item by item: that set keeps the sample loader
        self.loader_validation = self._loader(args if self.ocr is None else None, validation_set, "validation set", batch_size=self.batch_size)
        self.train_set_size = len(self.loader_train.dataset)
        self.val_set_size = len(self.loader_validation.dataset)
        print(f"Train Set size - {self.train_set_size}, Val Set Size - {self.val_set_size}")
        self.noiser = AddGaussianNoice(std=self.std, is_stochastic=self.is_random_std, return_noise=False)

        B = self.backend
        self.loss_function = B.CTCLoss().to(self.device)
        self.loss_func_samplewise = B.CTCLoss(reduction="none").to(self.device)
        self.graphs = None
        adam_kw = {}
        if getattr(args, "graph", False) and self.device.type == "cuda" and B.gpu_jitter:
            adam_kw = {"capturable": True}                                   # the step count lives on the device
        self.optimizer = B.Adam(self.model.parameters(), lr=self.lr, **adam_kw)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=self.decay_step, gamma=self.decay)
        if adam_kw:
            from qea.graph import PhaseAGraphs
            # PhaseAGraphs drives a trainer through these names (qea/trainer_core.py); one replica group = the warm-up step
            self.crnn_model, self.optimizer_crnn, self.primary_loss_fn = self.model, self.optimizer, self.loss_function
            self._step_crnn = self.optimizer.step
            self.graphs = PhaseAGraphs(self)

    def _loader(self, args, dataset, what, **kw):
        if not getattr(args, "resident", False):
            return torch.utils.data.DataLoader(dataset, **kw)
        # [new] --resident: the strips decoded once and kept on the device, the same index batches
        if getattr(args, "synthetic_size", None):
            from qea._lib import QeaError
            raise QeaError("--resident keeps ImgDataset strips on the device: it does not go with --synthetic_size")
        from datasets.resident import resident_args, resident_loader
        return resident_loader(dataset, self.input_size, self.device, what=what, **resident_args(args, what), **kw)

    def _datasets(self, args, train_set, val_set):
        """(training set of clean strips, validation set).  Training labels are the datasets' (ground truth) unless --ocr is given,
        in which case the loop replaces them by the OCR's labels of the noisy batch; validation labels are then the OCR's labels
        of the clean strips (reference: OCRDataset with the noise-free transform)."""
        if train_set is None or val_set is None:
            n = getattr(args, "synthetic_size", None)
            if n:
                from datasets.synthetic import SyntheticTextAreas
                train_set = SyntheticTextAreas(n, seed=1, include_name=True)
                val_set = SyntheticTextAreas(max(self.batch_size, n // 4), seed=2, include_name=True)
            else:
                from datasets._io import to_tensor
                from datasets.img_dataset import ImgDataset
                from transform_helper import PadWhite
                tf = lambda img: to_tensor(PadWhite(self.input_size)(img))
                train_set = ImgDataset(self.train_set, transform=tf, include_name=True)
                if self.ocr is not None:
                    from datasets.ocr_dataset import OCRDataset
                    return train_set, OCRDataset(self.validation_set, transform=tf, ocr_helper=self.ocr)
                val_set = ImgDataset(self.validation_set, transform=tf)
        if self.ocr is not None:
            from datasets.ocr_dataset import OCRRelabelled
            return train_set, OCRRelabelled(val_set, self.ocr)
        # the reference's num_subset= (a TypeError there): the first N samples
        if args.train_subset:
            train_set = torch.utils.data.Subset(train_set, range(min(args.train_subset, len(train_set))))
        if args.val_subset:
            val_set = torch.utils.data.Subset(val_set, range(min(args.val_subset, len(val_set))))
        return train_set, val_set

    def _jitter(self, images):
        """The training noise of the reference's noisy_transform.  HIP: one Philox launch for the batch; injected CPU backend: the
        reference's per-image draws (sigma, then torch.normal), in the order its loader makes them."""
        if self.backend.gpu_jitter and images.is_cuda:
            return self.noiser.batch(images)[0]
        return torch.stack([self.noiser(img) for img in images])

    def _call_model(self, images, labels):
        X_var = images.to(self.device)
        scores = self.model(X_var)
        out_size = torch.tensor([scores.shape[0]] * images.shape[0], dtype=torch.int)
        y_size = torch.tensor([len(l) for l in labels], dtype=torch.int)
        y = torch.tensor([self.char_to_index[c] for c in "".join(labels)], dtype=torch.int)
        return scores, y, out_size, y_size

    def train_step(self, images, labels):
        """One optimiser step on a clean batch (reference :155-162, with the loader's noise applied here).  Returns the loss (a tensor
        with .item())."""
        X_var = self._jitter(images.to(self.device))
        if self.ocr is not None:
            labels = self.ocr.get_labels(X_var.cpu())
        if self.graphs is not None:
            loss = self.graphs.step(X_var, labels, 1)            # [new] --graph: forward, CTC, backward and Adam as one replay
            if loss is not None:
                return loss
        self.model.zero_grad()
        scores, y, pred_size, y_size = self._call_model(X_var, labels)
        loss = self.loss_function(scores, y, pred_size, y_size)
        loss.backward()
        self.optimizer.step()
        return loss

    def validate(self):
        """(validation loss sum, correct count, CER sum) over the whole validation set in eval mode (reference :171-189); the last
        batch is whatever remains (no drop_last)."""
        self.model.eval()
        validation_loss, pred_correct_count, pred_CER = 0.0, 0, 0.0
        with torch.no_grad():
            for batch in self.loader_validation:
                images, labels = batch[0], list(batch[1])
                scores, y, pred_size, y_size = self._call_model(images, labels)
                loss = self.loss_function(scores, y, pred_size, y_size)
                preds = pred_to_string(scores, labels, self.index_to_char)
                crt, cer = compare_labels(preds, labels)
                pred_correct_count += crt
                pred_CER += cer
                validation_loss += loss.item()
        return validation_loss, pred_correct_count, pred_CER

    def _save(self, epoch, accuracy):
        path = f"{self.crnn_model_path}_{epoch}_{accuracy * 100:.2f}"
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        torch.save(self.model, path)
        return path

    def train(self):
        best_val_acc = 0
        best_val_epoch = 0
        print(f"Batch size is {self.batch_size}")
        print(f"Train batch size is {self.train_batch_size}")
        for epoch in range(self.start_epoch + 1, self.max_epochs):
            self.model.train()
            step = 0
            training_loss = 0
            for batch in self.loader_train:
                loss = self.train_step(batch[0], list(batch[1]))
                training_loss += loss.item()
                if step % 100 == 0:
                    print(f"Epoch: {epoch}, Iteration: {step} => {loss.item()}")
                step += 1

            validation_loss, pred_correct_count, pred_CER = self.validate()
            CRNN_accuracy = pred_correct_count / self.val_set_size
            if CRNN_accuracy > best_val_acc:
                best_val_acc = CRNN_accuracy
                best_val_epoch = epoch
                self._save(epoch, CRNN_accuracy)
            print("Epoch: %d/%d => Training loss: %f | Validation loss: %f"
                  % ((epoch + 1), self.max_epochs, training_loss / max(1, self.train_set_size // self.train_batch_size),
                     validation_loss / max(1, self.val_set_size // self.batch_size)))
            print(f"Validation Accuracy - {CRNN_accuracy*100}, {pred_correct_count} / {self.val_set_size}")
            self.last_val_accuracy, self.last_val_cer = CRNN_accuracy, pred_CER / self.val_set_size
            self.last_train_loss = training_loss / max(1, step)

            self.scheduler.step()
            if (epoch + 1) == self.max_epochs:                   # save the last model specifically
                self._save(epoch, CRNN_accuracy)
        return best_val_acc, best_val_epoch


def build_parser():
    from qea.cli_flags import build_parser as _build
    return _build("c", "Trains the CRNN model")


if __name__ == "__main__":
    args = build_parser().parse_args()
    trainer = TrainCRNN(args)
    trainer.train()
