"""Label-history ("label tracking") helpers of the `--inner_limit_skip` branch — same functions and
argument meaning as the reference's root tracking_utils.py (:5-81); the CRNN forward and every CTC
evaluation run on the HIP path."""
import torch


def call_crnn(self, images):
    scores = self.crnn_model(images.to(self.device))
    out_size = torch.tensor([scores.shape[0]] * images.shape[0], dtype=torch.int)
    return scores, out_size


def str_to_tensor(self, words):
    """history words -> [window_size, max_char_len] index tensor, padded with the out-of-vocabulary index
    len(char_set) (characters inside a word, and whole missing words) — reference tracking_utils.py:13-31."""
    import properties
    pad = len(properties.char_set)
    rows = [[self.char_to_index[c] for c in w] + [pad] * max(0, properties.max_char_len - len(w)) for w in words]
    rows += [[pad] * properties.max_char_len] * max(0, self.window_size - len(words))
    return torch.tensor(rows).to(self.device)


def generate_ctc_label(self, labels):
    y_size = torch.tensor([len(l) for l in labels], dtype=torch.int)
    y = torch.tensor([self.char_to_index[c] for c in "".join(labels)], dtype=torch.int)
    return y, y_size


def generate_ctc_target_batches(self, img_names):
    """For history depth i = 0..window-1: the i-th most recent OCR label of every strip that has one."""
    batches = []
    for depth in range(self.window_size):
        picked = [(j, self.tracked_labels[n][-(depth + 1)]) for j, n in enumerate(img_names) if depth < len(self.tracked_labels[n])]
        if picked:
            target, target_size = generate_ctc_label(self, [l for _, l in picked])
            batches.append([target, target_size, [j for j, _ in picked]])
    return batches


def weighted_ctc_loss(self, scores, pred_size, target_batches, loss_weights):
    """[new] On the GPU with this project's CTCLoss the W depths are evaluated by ONE call of csrc/ctc_history.hip (three launches,
    one pinned host-to-device copy); everything else — CPU tensors, torch's own CTCLoss, weights that carry a graph, a window above 8,
    a label above 127 characters, QEA_HISTORY_CTC=steps — runs the reference's loop below."""
    fused = _fused_weighted_ctc_loss(self, scores, pred_size, target_batches, loss_weights)
    if fused is not None:
        return fused
    losses = []
    for i in range(min(len(target_batches), self.window_size)):
        target, target_size, idx = target_batches[i]
        sub = scores[:, idx, :]
        if self.weightgen_method == "decaying":
            losses.append(loss_weights[i] * self.primary_loss_fn(sub, target, pred_size[idx], target_size))
        else:
            per = self.primary_loss_fn_sample_wise(sub, target, pred_size[idx], target_size)
            losses.append(torch.mean(loss_weights[idx, i] * per))
    return sum(losses)


def _fused_weighted_ctc_loss(self, scores, pred_size, target_batches, loss_weights):
    """the loss of weighted_ctc_loss from qea.autograd.HistoryCTCFn, or None when the call has to take the loop"""
    from qea import history
    W = min(len(target_batches), self.window_size)
    decaying = self.weightgen_method == "decaying"
    loss_fn = getattr(self, "primary_loss_fn" if decaying else "primary_loss_fn_sample_wise", None)
    if W < 1 or history.ctc_route(scores, loss_weights, self.window_size, 0, loss_fn) != "fused":
        return None
    if loss_fn.reduction != ("mean" if decaying else "none") or loss_fn.max_target_length is not None:
        return None
    n = scores.shape[1]
    if loss_weights.dim() != (1 if decaying else 2) or loss_weights.shape[-1] < W or (not decaying and loss_weights.shape[0] != n):
        return None
    if any(torch.is_tensor(t) and t.is_cuda for b in target_batches[:W] for t in b[:2]):
        return None
    from qea.autograd import HistoryCTCFn
    packer = getattr(self, "_ctc_packer", None)
    if packer is None:
        packer = self._ctc_packer = history.TargetBatchPacker()
    on_host = not (torch.is_tensor(pred_size) and pred_size.is_cuda)
    packed = packer.pack(target_batches[:W], n, pred_size if on_host else None)
    if packed is None or history.ctc_route(scores, loss_weights, self.window_size, packed[4], loss_fn) != "fused":
        return None
    host, _, W, total, longest = packed
    dev = packer.to_device(packed[:2], scores.device)
    depth_n, lens, offs, chars, in_len = packer.unpack(dev, n, W, total)
    if not on_host:
        in_len = pred_size.to(torch.int32).contiguous()
    strides = (0, loss_weights.stride(0)) if decaying else (loss_weights.stride(0), loss_weights.stride(1))
    return HistoryCTCFn.apply(scores, in_len, lens, offs, chars, depth_n, loss_weights, strides[0], strides[1], int(decaying),
                              2 * max(longest, 1) + 1, loss_fn.blank)


def add_labels_to_history(self, image_keys, ocr_labels):
    for i, name in enumerate(image_keys):
        self.tracked_labels.setdefault(name, []).append(ocr_labels[i])
