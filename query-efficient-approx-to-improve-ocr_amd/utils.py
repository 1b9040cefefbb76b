"""Helpers of the training loop — drop-in for the hot subset of the reference's utils.py
(get_char_maps :22-40, show_img :49-54, pred_to_string :74-92, compare_labels :95-110, set_bn_eval :113-115,
padder / get_text_stack :118-141, get_ocr_helper :180-188, create_dirs :191-206, save_json /
save_all_jsons :209-231, handle_optuna_trial :233-237, set_random_seeds :240-243).

GPU-side work goes through the HIP library: greedy CTC decode (one wave per sample instead of a
Python loop with an .item() per (b,t)), crop + pad gather with a scatter-add backward.  [new] beam_decode and the
beam= / nbest= / return_scores= arguments of pred_to_string and batch_cers add a CTC prefix beam search (csrc/ctc_beam.hip for CUDA
scores, qea/beam.py on the host), and beam_decode_lm / lm= / lm_weight= / lm_bonus= fuse a character n-gram prior (qea/lm.py) into
that search; beam_decode_lexicon / lexicon= keep it inside a word list (qea/lexicon.py); the reference has no beam and the defaults
are its greedy decode.  [new] char_spans aligns given strings to the scores (CTC forced alignment: csrc/ctc_align.hip, qea/align.py) and
returns where each character sits and how confident the CRNN is of it.  The optional
third-party pieces of the reference file (wandb, optuna, unidecode, Levenshtein, torchvision) are
imported lazily and only where the corresponding feature is used."""
import json
import os
import random as python_random

import numpy as np
import torch

import properties


def get_char_maps(vocabulary=None):
    if vocabulary is None:
        import string
        vocabulary = ["-"] + list(string.ascii_lowercase) + list(string.ascii_uppercase) + list(string.digits)
    char_to_index = {c: i for i, c in enumerate(vocabulary)}
    index_to_char = {i: c for i, c in enumerate(vocabulary)}
    return char_to_index, index_to_char, len(vocabulary)


# ----------------------------------------------------------------------------- decode / CER
def _beam_search(who, scores, beam, blank, model, on_device, on_host):
    """The one path of beam_decode / beam_decode_lm / beam_decode_lexicon.  model: None, or the CharLM / Lexicon whose class count
    and blank must be the scores'.  CUDA scores (and not QEA_BEAM=host): on_device(ops, float32 scores with a unit class stride),
    results stay on the device; otherwise on_host(qea.beam, scores), moved to the scores' device."""
    from qea import beam as host_beam
    s = scores.detach()
    if model is not None and (model.num_classes != s.shape[2] or model.blank != blank):
        from qea._lib import QeaError
        raise QeaError(f"{who}: the {type(model).__name__} has {model.num_classes} classes and blank {model.blank}, the scores "
                       f"{s.shape[2]} and {blank}")
    if s.is_cuda and not host_beam.use_host():
        from qea import ops
        if s.dtype != torch.float32:
            s = s.float()
        if s.stride(2) != 1:
            s = s.contiguous()
        return on_device(ops, s)
    return tuple(v.to(s.device) for v in on_host(host_beam, s))


def beam_decode(scores, beam, blank=0):
    """[new] CTC prefix beam search of scores [T,B,C] with `beam` entries per sample -> (tokens int32 [B,K,T], lengths int32 [B,K],
    log-probabilities float64 [B,K]), best first.  CUDA tensors: one launch (qea.ops.ctc_beam_decode), results stay on the device;
    CPU tensors, or QEA_BEAM=host: the same specification as a host loop (qea/beam.py)."""
    return _beam_search("beam_decode", scores, beam, blank, None, lambda ops, s: ops.ctc_beam_decode(s, beam, blank),
                        lambda host, s: host.ctc_beam_decode(s, beam, blank))


def beam_decode_lm(scores, beam, lm, alpha=1.0, beta=0.0, blank=0):
    """[new] beam_decode with the character n-gram model `lm` (qea.lm.CharLM) fused into the search: a candidate is ranked by its CTC
    log-probability plus alpha * log P(c | context) + beta per character -> (tokens int32 [B,K,T], lengths int32 [B,K],
    ctc float64 [B,K], total float64 [B,K]), best first by total.  CUDA tensors: one launch (qea.ops.ctc_beam_decode_lm); CPU
    tensors, or QEA_BEAM=host: the same specification as a host loop (qea/beam.py)."""
    return _beam_search("beam_decode_lm", scores, beam, blank, lm,
                        lambda ops, s: ops.ctc_beam_decode_lm(s, beam, lm.fused(alpha, beta, s.device), lm.context, blank),
                        lambda host, s: host.ctc_beam_decode(s, beam, blank, lm.fused(alpha, beta, "cpu"), lm.context))


def beam_decode_lexicon(scores, beam, lexicon, blank=0):
    """[new] beam_decode restricted to the paths of `lexicon` (qea.lexicon.Lexicon: a word-list trie or any deterministic automaton
    over the non-blank classes): an extension that leaves the automaton does not exist -> (tokens int32 [B,K,T], lengths int32
    [B,K], log-probabilities float64 [B,K], accepted bool [B,K]), the whole last beam, best first; accepted marks the ranks that end
    in an accepting state (whole words).  The scores are CTC log-likelihoods, as in beam_decode.  CUDA tensors: one launch
    (qea.ops.ctc_beam_decode_dfa) on tables uploaded once, no synchronisation; CPU tensors, or QEA_BEAM=host: the host loop."""
    tokens, lengths, logp, states = _beam_search(
        "beam_decode_lexicon", scores, beam, blank, lexicon,
        lambda ops, s: ops.ctc_beam_decode_dfa(s, beam, lexicon.device(s.device), blank),
        lambda host, s: host.ctc_beam_decode(s, beam, blank, automaton=lexicon))
    final = lexicon.device(states.device).final
    accepted = (states >= 0) & (final[states.clamp(min=0).long()] != 0)
    return tokens, lengths, logp, accepted


def lexicon_best(scores, beam, lexicon, blank=0, nbest=1):
    """[new] The nbest best-ranked ACCEPTED entries of beam_decode_lexicon per strip -> (tokens int32 [B,n,T], lengths int32 [B,n],
    log-probabilities float64 [B,n], miss bool [B]); ranks beyond a strip's accepted count have length -1 and score -inf.  A strip
    with no accepted entry among its K (miss) reads as the plain search of the same K: one extra beam_decode over those strips only."""
    if not 1 <= nbest <= beam:
        from qea._lib import QeaError
        raise QeaError(f"lexicon_best: nbest={nbest} outside 1..beam={beam}")
    tokens, lengths, logp, accepted = beam_decode_lexicon(scores, beam, lexicon, blank)
    B, K, T = tokens.shape
    order = torch.sort((~accepted).to(torch.int32), dim=1, stable=True).indices[:, :nbest]       # accepted ranks first, in rank order
    count = accepted.sum(dim=1)
    tokens = tokens.gather(1, order[:, :, None].expand(B, nbest, T))
    lengths, logp = lengths.gather(1, order), logp.gather(1, order)
    behind = torch.arange(nbest, device=tokens.device)[None, :] >= count[:, None]
    tokens[behind], lengths[behind], logp[behind] = -1, -1, -float("inf")
    miss = count == 0
    strips = miss.nonzero().flatten()
    if strips.numel():
        pt, pl, ps = beam_decode(scores.detach()[:, strips], beam, blank)
        tokens[strips], lengths[strips], logp[strips] = pt[:, :nbest], pl[:, :nbest], ps[:, :nbest]
    return tokens, lengths, logp, miss


def _check_beam_arguments(who, beam, lm, lexicon):
    """The rules of the beam= / lm= / lexicon= arguments of pred_to_string and batch_cers."""
    from qea._lib import QeaError
    if lm is not None and not beam:
        raise QeaError(f"{who}: lm needs beam=K > 0 (the greedy decode has no search to fuse a prior into)")
    if lexicon is not None and (lm is not None or not beam):
        raise QeaError(f"{who}: lexicon needs beam=K > 0 and cannot be combined with lm")


def _beam_readings(scores, beam, blank, nbest, lm, lm_weight, lm_bonus, lexicon):
    """(tokens, lengths, log-scores) of the readings of the search that (lm, lexicon) choose; at least nbest ranks per strip."""
    if lexicon is not None:
        return lexicon_best(scores, beam, lexicon, blank, nbest)[:3]
    if lm is None:
        return beam_decode(scores, beam, blank)
    tokens, lengths, _, total = beam_decode_lm(scores, beam, lm, lm_weight, lm_bonus, blank)
    return tokens, lengths, total                                      # the totals: what decided the order


def _beam_to_string(scores, labels, index_to_char, show_text, beam, nbest, return_scores, lm=None, lm_weight=1.0, lm_bonus=0.0, lexicon=None):
    if not 1 <= nbest <= beam:
        from qea._lib import QeaError
        raise QeaError(f"pred_to_string: nbest={nbest} outside 1..beam={beam}")
    tokens, lengths, logp = _beam_readings(scores, beam, 0, nbest, lm, lm_weight, lm_bonus, lexicon)
    tk, ln, lp = tokens.cpu().tolist(), lengths.cpu().tolist(), logp.cpu().tolist()
    B = len(tk)
    # a rank beyond the live count (length -1, score -inf: fewer than `beam` labellings have a non-zero probability) reads ""
    lists = [["".join(index_to_char[i] for i in tk[b][k][:max(ln[b][k], 0)]) for k in range(nbest)] for b in range(B)]
    preds = [l[0] for l in lists]
    if show_text:
        for l, p in zip(labels, preds):
            print(l, " -> ", p)
    out = preds if nbest == 1 else lists
    if return_scores:
        return out, ([lp[b][0] for b in range(B)] if nbest == 1 else [lp[b][:nbest] for b in range(B)])
    return out


def pred_to_string(scores, labels, index_to_char, show_text=False, beam=0, nbest=1, return_scores=False, lm=None, lm_weight=1.0,
                   lm_bonus=0.0, lexicon=None):
    """Greedy CTC decode of scores [T,B,C]: per-step argmax, collapse repeats, drop index 0.
    [new] beam=K > 0: CTC prefix beam search with K entries instead (beam_decode) -> the most probable labelling per sample;
    nbest=n <= K: a list of the n best strings per sample instead of one string; return_scores=True: (strings, log-probabilities
    as Python floats of the same nesting).  beam=0 is the greedy path; it has no scores and no second-best reading.
    [new] lm=CharLM (with beam=K): the search with that character n-gram model fused in (beam_decode_lm), weight lm_weight and
    per-character bonus lm_bonus; the strings are the fused search's and return_scores gives its TOTAL scores.
    [new] lexicon=Lexicon (with beam=K, not with lm): the search stays inside that word list (beam_decode_lexicon) and the strings are
    its best-ranked entries that are whole words, with their CTC log-probabilities; a strip with no word among its K reads as the
    plain search of the same K (lexicon_best)."""
    _check_beam_arguments("pred_to_string", beam, lm, lexicon)
    if beam:
        return _beam_to_string(scores, labels, index_to_char, show_text, int(beam), int(nbest), return_scores, lm, lm_weight, lm_bonus, lexicon)
    if nbest != 1 or return_scores:
        from qea._lib import QeaError
        raise QeaError("pred_to_string: nbest and return_scores need beam=K > 0 (the greedy decode has neither)")
    T, B, C = scores.shape
    if scores.is_cuda:
        from qea import ops
        s = scores.detach()
        if s.stride(2) != 1:
            s = s.contiguous()
        tokens = torch.empty(B, T, dtype=torch.int32, device=s.device)
        lengths = torch.empty(B, dtype=torch.int32, device=s.device)
        ops.greedy_decode(s, s.stride(0), s.stride(1), T, B, C, 0, tokens, lengths)
        tk, ln = tokens.cpu().tolist(), lengths.cpu().tolist()
        preds = ["".join(index_to_char[i] for i in tk[b][:ln[b]]) for b in range(B)]
    else:
        idx = scores.detach().argmax(dim=2).t().tolist()
        preds = []
        for row in idx:
            out, prev = "", None
            for k in row:
                if k != 0 and (len(out) == 0 or k != prev):
                    out += index_to_char[k]
                prev = k
            preds.append(out)
    if show_text:
        for l, p in zip(labels, preds):
            print(l, " -> ", p)
    return preds


def char_spans(scores, texts, char_to_index, blank=0):
    """[new] CTC forced alignment of scores [T,N,C] to N given readings: texts is N strings (mapped through char_to_index) or N lists of
    class indices -> per sample (score, first, last, char_score): the log-score of the best single alignment as a Python float, and per
    character the first and last step it occupies (int32 numpy) and the sum of its log-probs over those steps (float64 numpy; divided by
    last - first + 1 it is the character's mean log-prob).  An infeasible sample (more characters, counting a blank between repeats, than
    steps; a class outside the scores; the blank inside the label) gives (-inf, all -1, all -1, all -inf).  CUDA scores: one launch
    (qea.ops.ctc_align); CPU scores, or QEA_ALIGN=host: the same statement as a host loop (qea/align.py), bit for bit.  ValueError, naming
    the sample, for a character outside the vocabulary and for a label of more than 127 characters."""
    from qea import align
    s = scores.detach()
    if s.dim() != 3 or len(texts) != s.shape[1]:
        raise ValueError(f"char_spans: {len(texts)} texts for scores of shape {tuple(s.shape)} ([T, N, C] with N texts wanted)")
    labels = []
    for n, text in enumerate(texts):
        if isinstance(text, str):
            missing = sorted({c for c in text if c not in char_to_index})
            if missing:
                raise ValueError(f"char_spans: sample {n}: {missing} not in the vocabulary")
            text = [char_to_index[c] for c in text]
        if len(text) > align.MAX_L:
            raise ValueError(f"char_spans: sample {n}: a label of {len(text)} characters, more than {align.MAX_L}")
        labels.append([int(c) for c in text])
    lengths = [len(l) for l in labels]
    offsets = np.concatenate(([0], np.cumsum(lengths, dtype=np.int64))).astype(np.int64)
    flat = np.asarray([c for l in labels for c in l], dtype=np.int64)
    flat = np.where((flat < -1) | (flat >= 2 ** 31), -1, flat).astype(np.int32)      # any class that is none stays one in 32 bits
    L_max = max(lengths, default=0)
    if s.is_cuda and not align.use_host():
        from qea import ops
        if s.dtype != torch.float32:
            s = s.float()
        if s.stride(2) != 1:
            s = s.contiguous()
        out = ops.ctc_align(s, torch.from_numpy(flat).to(s.device), torch.from_numpy(offsets).to(s.device), L_max, blank)
    else:
        out = align.ctc_align(s, flat, offsets, L_max, blank)
    score, _, first, last, char_score = (v.cpu().numpy() for v in out)
    return [(float(score[n]), first[a:b], last[a:b], char_score[a:b]) for n, (a, b) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist()))]


def levenshtein(a, b):
    """Unit-cost edit distance (what python-Levenshtein's `distance` returns)."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def compare_labels(preds, labels):
    if not isinstance(labels, (list, tuple)):
        labels = [labels]
    correct, total_cer = 0, 0
    for p, l in zip(preds, labels):
        correct += int(p == l)
        total_cer += levenshtein(l, p) / max(1, len(l))
    return correct, total_cer


def batch_cers(scores, labels, char_to_index, blank=0, beam=0, lm=None, lm_weight=1.0, lm_bonus=0.0, lexicon=None):
    """Per-sample CER of the greedy decode of `scores` [T,B,C] against `labels`, entirely on the GPU up to
    the final division: decode kernel -> edit-distance kernel -> one [B] int32 copy to the host.  Equals
    [compare_labels([pred_i], [label_i])[1] for i] of the reference loop (train_nn_patch.py:336-342).
    [new] beam=K > 0: the CER of the best entry of the prefix beam search instead (rank 0 of beam_decode); with lm=CharLM, of the
    search with that model fused in (rank 0 of beam_decode_lm); with lexicon=Lexicon (not with lm), of the best-ranked whole word of
    the search inside that word list, and of the plain search's rank 0 where a strip has none (lexicon_best)."""
    from qea import ops
    _check_beam_arguments("batch_cers", beam, lm, lexicon)
    T, B, C = scores.shape
    s = scores.detach()
    dev = s.device
    if beam:
        btok, blen, _ = _beam_readings(s, int(beam), blank, 1, lm, lm_weight, lm_bonus, lexicon)
        # the edit-distance kernel takes rows of at most 128 tokens: rank 0 as a [B][T] slice of its own, not a K * T stride
        # (length -1 = no labelling with a non-zero probability at all: scored as the empty string)
        tokens, plen = btok[:, 0, :].contiguous(), blen[:, 0].clamp(min=0).contiguous()
    else:
        if s.stride(2) != 1:
            s = s.contiguous()
        tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
        plen = torch.empty(B, dtype=torch.int32, device=dev)
        ops.greedy_decode(s, s.stride(0), s.stride(1), T, B, C, blank, tokens, plen)
    glen = torch.tensor([len(l) for l in labels], dtype=torch.int32)
    goff = torch.zeros(B, dtype=torch.int64)
    if B > 1:
        goff[1:] = torch.cumsum(glen.to(torch.int64), 0)[:-1]
    flat = [char_to_index[c] for c in "".join(labels)] or [0]
    gt = torch.tensor(flat, dtype=torch.int32)
    dist = torch.empty(B, dtype=torch.int32, device=dev)
    ops.edit_distance(tokens, T, plen, gt.to(dev), goff.to(dev), glen.to(dev), B, dist)
    d = dist.cpu().tolist()
    return [d[i] / max(1, len(labels[i])) for i in range(B)]


def set_bn_eval(module):
    if isinstance(module, torch.nn.modules.batchnorm._BatchNorm):
        module.eval()


# ----------------------------------------------------------------------------- crop + pad
class _CropPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, boxes_dev, n, oh, ow):
        from qea import ops
        _, H, W = image.shape
        out = torch.empty(n, 1, oh, ow, device=image.device)
        ops.crop_pad_gather(image.contiguous(), H, W, boxes_dev, n, oh, ow, out)
        ctx.save_for_backward(boxes_dev)
        ctx.dims = (H, W, n, oh, ow)
        return out

    @staticmethod
    def backward(ctx, dout):
        from qea import ops
        (boxes_dev,) = ctx.saved_tensors
        H, W, n, oh, ow = ctx.dims
        dimg = torch.zeros(1, H, W, device=dout.device)
        ops.crop_pad_scatter(dout.contiguous(), boxes_dev, n, oh, ow, dimg, H, W)
        return dimg, None, None, None, None


class _DocCrops(torch.autograd.Function):
    """[new] All strips of a step out of a device-resident document store (datasets.resident.ResidentDocuments.crops): one launch
    forward, one order-fixed launch without atomics backward (csrc/doc_crops.hip)."""

    @staticmethod
    def forward(ctx, images, store, doc, strip_first, S, oh, ow):
        from qea import ops
        out = torch.empty(S, 1, oh, ow, dtype=torch.float32, device=images.device)
        ops.doc_crops_gather(images.contiguous(), store.box, store.box_first, doc, strip_first, out)
        ctx.save_for_backward(doc, strip_first)
        ctx.store, ctx.shape = store, tuple(images.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        from qea import ops
        doc, strip_first = ctx.saved_tensors
        dimg = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)      # written whole by the launch: no fill
        ops.doc_crops_scatter(dout.contiguous(), ctx.store.box, ctx.store.box_first, doc, strip_first, dimg)
        return dimg, None, None, None, None, None, None


def padder(crop, h, w):
    _, c_h, c_w = crop.shape
    left, top = (w - c_w) // 2, (h - c_h) // 2
    return torch.nn.functional.pad(crop, (left, w - left - c_w, top, h - top - c_h), value=1.0)


def get_text_stack(image, labels, input_size):
    """image [1,H,W]; labels: list of dicts with label,x_min,y_min,x_max,y_max -> ([N,1,h,w], [label])."""
    names = [l["label"] for l in labels]
    if image.is_cuda and image.shape[0] == 1 and labels:
        _, H, W = image.shape
        # python slicing clips to the image; the kernel takes pre-clipped boxes
        boxes = torch.tensor([[max(0, l["x_min"]), max(0, l["y_min"]), min(W, l["x_max"]), min(H, l["y_max"])] for l in labels],
                             dtype=torch.int32)
        return _CropPad.apply(image, boxes.to(image.device), len(labels), input_size[0], input_size[1]), names
    crops = [padder(image[:, l["y_min"]:l["y_max"], l["x_min"]:l["x_max"]], *input_size) for l in labels]
    return torch.stack(crops), names


def get_text_stacks(images, box_lists, input_size):
    """[new] images [N,1,H,W], box_lists: one list of box dicts per document -> (crops [S,1,h,w] of all documents, document after
    document, [labels per document]).  Box lists that come from a device-resident document store (datasets.resident.DocBoxes) and CUDA
    images: ONE launch for all strips, and one order-fixed launch for their gradient.  Anything else: get_text_stack per document."""
    store = getattr(box_lists, "store", None)
    if images.dim() == 3:
        images = images[:, None]
    if store is not None and store.device.type == "cuda" and images.is_cuda:
        return store.crops(images, box_lists.rows, input_size[0], input_size[1]), store.labels(box_lists.rows)
    stacks = [get_text_stack(images[i], box_lists[i], input_size) for i in range(len(box_lists))]
    return torch.cat([c for c, _ in stacks]), [names for _, names in stacks]


# ----------------------------------------------------------------------------- OCR / dirs / json / seeds
def get_ununicode(text):
    for a, b in (("_", "-"), ("`", "'"), ("©", "c"), ("°", "'"), ("£", "E"), ("§", "S")):
        text = text.replace(a, b)
    from unidecode import unidecode          # only needed by the real OCR engines
    has_eur = "€" in text
    text = unidecode(text.replace("€", "<eur>"))
    return text.replace("<eur>", "€") if has_eur else text


def get_ocr_helper(ocr, is_eval=False):
    """Same names as the reference (:180-188).  The real engines are optional third-party black boxes;
    'stub' is the deterministic stand-in with the identical get_labels contract."""
    if ocr == "stub":
        from ocr_helper.stub_helper import StubHelper
        return StubHelper(is_eval=is_eval)
    if ocr in ("Tesseract", "EasyOCR", "gvision"):
        mod = {"Tesseract": "tess_helper", "EasyOCR": "eocr_helper", "gvision": "gcloud_helper"}[ocr]
        cls = {"Tesseract": "TessHelper", "EasyOCR": "EocrHelper", "gvision": "GcloudHelper"}[ocr]
        try:
            m = __import__(f"ocr_helper.{mod}", fromlist=[cls])
        except ImportError as e:
            raise ImportError(f"OCR engine {ocr!r} needs its third-party package and an ocr_helper/{mod}.py adapter "
                              f"(black box, out of scope here); use --ocr stub for plumbing runs") from e
        return getattr(m, cls)(is_eval=is_eval)
    return None


def create_dirs(self, args):
    self.crnn_model_path = args.crnn_model
    self.prep_model_path = args.prep_model
    self.data_base_path = args.data_base_path
    self.exp_base_path = args.exp_base_path
    sub = lambda s: os.path.join(self.exp_base_path, s)
    self.ckpt_base_path = sub(properties.prep_crnn_ckpts)
    self.cers_base_path = sub("cers")
    self.tracked_labels_path = sub("tracked_labels")
    self.selectedsamples_path = sub("selected_samples")
    self.img_out_path = sub(properties.img_out)
    for d in (self.exp_base_path, self.ckpt_base_path, self.img_out_path, self.cers_base_path, self.tracked_labels_path,
              self.selectedsamples_path):
        os.makedirs(d, exist_ok=True)


def _wandb():
    try:
        import wandb
        return wandb if wandb.run is not None else None
    except ImportError:
        return None


def save_json(metrics, json_path, wandb_save=True):
    with open(json_path, "w") as f:
        json.dump(metrics, f)
    wb = _wandb()
    if wandb_save and wb is not None:
        wb.save(json_path)


def save_all_jsons(self, epoch):
    save_json(self.tracked_labels, os.path.join(self.tracked_labels_path, f"tracked_labels_{epoch}.json"), wandb_save=False)
    save_json(self.tracked_labels, os.path.join(self.tracked_labels_path, "tracked_labels_current.json"))
    save_json(self.selected_samples, os.path.join(self.selectedsamples_path, "selected_samples_current.json"))
    save_json(self.sampler.all_cers, os.path.join(self.cers_base_path, "all_cers.json"))
    if hasattr(self.sampler, "entropies"):               # [new] uniformEntropy: the sampler's current table, readable back through --entropies_path
        save_json(self.sampler.entropies, os.path.join(self.cers_base_path, "entropies.json"))


def save_img(images, name, dir, nrow=8):
    """Grid PNG of [N,1,H,W] images in [0,1] (reference :43-46 via torchvision.make_grid, 2-px padding)."""
    from PIL import Image
    imgs = images.detach().cpu().float().clamp(0, 1)
    n, _, h, w = imgs.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    pad = 2
    grid = torch.zeros(rows * (h + pad) + pad, cols * (w + pad) + pad)
    for i in range(n):
        r, c = divmod(i, cols)
        grid[pad + r * (h + pad): pad + r * (h + pad) + h, pad + c * (w + pad): pad + c * (w + pad) + w] = imgs[i, 0]
    Image.fromarray((grid.numpy() * 255).round().astype(np.uint8)).save(os.path.join(dir, name + ".png"), "PNG")


def show_img(images, title="Figure", nrow=8):
    """Shows a grid of [N,1,H,W] images (reference :49-54; the eval drivers' --show_img).  matplotlib is imported only here."""
    import matplotlib.pyplot as plt
    imgs = images.detach().cpu().float().clamp(0, 1)
    if imgs.dim() == 3:
        imgs = imgs[None]
    n, _, h, w = imgs.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    grid = torch.zeros(rows * (h + 2) + 2, cols * (w + 2) + 2)
    for i in range(n):
        r, c = divmod(i, cols)
        grid[2 + r * (h + 2): 2 + r * (h + 2) + h, 2 + c * (w + 2): 2 + c * (w + 2) + w] = imgs[i, 0]
    plt.figure(num=title)
    plt.imshow(grid.numpy(), cmap="gray")
    plt.show()


def handle_optuna_trial(trial, accuracy, epoch):
    if trial is not None:
        trial.report(accuracy, epoch)
        if trial.should_prune():
            import optuna
            raise optuna.TrialPruned()


def get_pruning_sampler(dataset, artifact_name):
    """SubsetRandomSampler over the documents an artifact of pruning/prune_dataset.py names (reference :246-263): keys are
    `<folder>_<file stem>` of the dataset's names.  The artifact is read from pruning/<cer_artifacts>/<name>.json below the working
    directory, or fetched through wandb when a wandb run is active and enabled."""
    from qea._lib import QeaError
    wb = _wandb()
    if wb is not None and not getattr(wb.run, "disabled", False) and "Disabled" not in type(getattr(wb.run, "mode", None)).__name__:
        data = wb.run.use_artifact(f"{artifact_name}:latest")
        cers_path = os.path.join(data.download(), f"{artifact_name}.json")
    else:
        cers_path = os.path.join("pruning", properties.cer_artifacts_path, f"{artifact_name}.json")
    if not os.path.exists(cers_path):
        raise QeaError(f"pruning artifact {cers_path} not found (write it with pruning/prune_dataset.py)")
    with open(cers_path, "r") as f:
        pruned_data_info = json.load(f)
    names = getattr(dataset, "names", None) or getattr(dataset, "files", None)   # a dataset that lists its names spares loading every image
    if names is None:
        names = (dataset[i][-1] for i in range(len(dataset)))
    indices = list()
    for i, name in enumerate(names):
        folder_name, file_name = name.split("/")[-2:]
        file_name = file_name.split(".")[0]
        if f"{folder_name}_{file_name}" in pruned_data_info:
            indices.append(i)
    if not indices:
        raise QeaError(f"pruning artifact {cers_path} names none of the {len(dataset)} training documents "
                       f"(keys look like {next(iter(pruned_data_info), None)!r})")
    return torch.utils.data.SubsetRandomSampler(torch.tensor(indices))


def set_random_seeds(random_seed):
    torch.manual_seed(random_seed)
    python_random.seed(random_seed)
    np.random.seed(random_seed)
