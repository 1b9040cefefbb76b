"""Loss-weight generators for the label-history CTC — same classes, constructor and `gen_weights(tracked_labels,
img_names)` protocol as the reference's label_tracking/tracking_methods.py:

  * decaying       (:105-115)  weights decay^i per history depth                      -> 1-D tensor [window]
  * levenshtein    (:63-101)   agreement of each remembered label with the others     -> [len(names), window+1]
  * self_attention (:26-59)    HistoryAttention scores of the remembered labels       -> [len(names), window+1]

On a CUDA device the two tables are built by one launch each of csrc/history.hip (qea.ops.history_lev_weights /
history_attn_weights) from histories packed by qea.history: one pinned host-to-device copy and one launch per call, whatever the
number of strips.  The per-strip host loops below are the CPU path, the QEA_HISTORY_WEIGHTS=host path, and the fall-back for what
the kernels do not take (a window above 8, a word above 128 characters, anything the host path itself answers with an exception).
The CTC evaluations the weights multiply run on the HIP path (tracking_utils.weighted_ctc_loss)."""
import torch

import properties


class LossWeightGenerator:
    def __init__(self, tracking_args, device, char_to_index=None):
        self.window_size = tracking_args.window_size
        self.device = device
        self.char_to_index = char_to_index

    def print_debug_statements(self):
        pass

    def _recent(self, tracked_labels, name):
        """labels of `name` inside the window, most recent first"""
        return tracked_labels[name][-self.window_size:][::-1] if name in tracked_labels else []

    def _table(self, n):
        w = torch.zeros(n, self.window_size + 1)
        w[:, 0] = 1                                              # the label of the current epoch always counts fully
        return w


class DecayingWeightGenerator(LossWeightGenerator):
    def __init__(self, tracking_args, device, char_to_index=None):
        super().__init__(tracking_args, device, char_to_index)
        self.decay_factor = tracking_args.decay_factor

    def gen_weights(self, training_obj, img_names):
        return torch.tensor([self.decay_factor ** i for i in range(self.window_size)]).to(self.device)


class LevenshteinWeightGenerator(LossWeightGenerator):
    HIST_MULTIPLIER = 0.5

    def select_path(self, tracked_labels, img_names):
        """('device', packed call) or ('host', None); callable without a GPU"""
        from qea import history
        if history.route(self.device, self.window_size) == "host" or len(img_names) == 0:
            return "host", None
        if getattr(self, "_packer", None) is None or self._packer.window != self.window_size:
            self._packer = history.LevenshteinPacker(self.window_size)
        packed = self._packer.pack(tracked_labels, img_names)
        return history.route(self.device, self.window_size, packed=packed is not None), packed

    def gen_weights(self, tracked_labels, img_names):
        path, packed = self.select_path(tracked_labels, img_names)
        if path == "device":
            from qea import ops
            n, W = len(img_names), self.window_size
            dev = self._packer.to_device(packed, self.device)
            o_count, o_lens, o_rows, _ = self._packer.sizes(n)
            w = torch.empty(n, W + 1, device=self.device)
            ops.history_lev_weights(dev[o_rows:], dev[o_lens:o_rows], dev[o_count:o_lens], n, W, w)
            return w
        return self._gen_weights_host(tracked_labels, img_names)

    def _gen_weights_host(self, tracked_labels, img_names):
        from utils import levenshtein
        w = self._table(len(img_names))
        for row, name in enumerate(img_names):
            hist = self._recent(tracked_labels, name)
            others = max(len(hist) - 1, 1)
            for i, word in enumerate(hist):
                mean_dist = sum(levenshtein(word, o) for j, o in enumerate(hist) if j != i) / others
                n_chars = max(1, len(word))
                w[row, i + 1] = self.HIST_MULTIPLIER * (1 - min(mean_dist, n_chars) / n_chars)
        return w.to(self.device)


class AttentionWeightGenerator(LossWeightGenerator):
    def __init__(self, tracking_args, device, char_to_index):
        super().__init__(tracking_args, device, char_to_index)
        from models.model_attention import HistoryAttention
        # area_cli.py has no --query_dim / --emb_dim / --attn_activation (the reference's area trainer raises
        # AttributeError here); fall back to patch_cli's defaults
        self.query_dim, self.emb_dim = getattr(tracking_args, "query_dim", 32), getattr(tracking_args, "emb_dim", 256)
        self.attn_activation = getattr(tracking_args, "attn_activation", "sigmoid")
        self.attention_model = HistoryAttention(len(properties.char_set), self.emb_dim, self.query_dim, self.window_size,
                                                self.attn_activation).to(self.device)

    def _params(self):
        """the scorer's parameters as the kernel reads them (contiguous fp32; no copy for a module in its default state)"""
        m = self.attention_model
        ts = (m.embedding, m.Wq.weight, m.Wq.bias, m.loss_coef_layer.weight, m.loss_coef_layer.bias, m.positional_encodings)
        return [t.detach().float().contiguous() for t in ts]

    def select_path(self, tracked_labels, img_names):
        """('device', packed call) or ('host', None); callable without a GPU"""
        from qea import history, ops
        m = self.attention_model
        table = (m.embedding.shape[0] + self.window_size) * m.Wq.weight.shape[0]
        on_dev = all(t.device.type == "cuda" for t in (m.embedding, m.Wq.weight, m.loss_coef_layer.weight, m.positional_encodings))
        ok = (m.embedding.shape[1] % 4 == 0 and m.activation in ops.HISTORY_ACTIVATIONS and m.loss_coef_layer.weight.shape[1] == self.window_size
              and m.embedding.shape[0] == len(properties.char_set) + 1)
        if history.route(self.device, self.window_size, table_floats=table, params_on_device=on_dev and ok) == "host" or len(img_names) == 0:
            return "host", None
        if getattr(self, "_packer", None) is None or self._packer.window != self.window_size or self._packer.char_to_index is not self.char_to_index:
            self._packer = history.AttentionPacker(self.window_size, self.char_to_index)
        packed = self._packer.pack(tracked_labels, img_names)
        return history.route(self.device, self.window_size, packed=packed is not None), packed

    def gen_weights(self, tracked_labels, img_names):
        path, packed = self.select_path(tracked_labels, img_names)
        if path == "device":
            from qea import ops
            n, W = len(img_names), self.window_size
            dev = self._packer.to_device(packed, self.device)
            o_count, o_lens, o_rows, _ = self._packer.sizes(n)
            w = torch.empty(n, W + 1, device=self.device)
            ops.history_attn_weights(dev[o_rows:], dev[o_count:o_lens], n, W, self._packer.row_len, *self._params(),
                                     self.attention_model.activation, w)
            return w
        return self._gen_weights_host(tracked_labels, img_names)

    def _gen_weights_host(self, tracked_labels, img_names):
        from tracking_utils import str_to_tensor
        w = self._table(len(img_names)).to(self.device)
        for row, name in enumerate(img_names):
            hist = self._recent(tracked_labels, name)
            if hist:
                with torch.no_grad():
                    scores = self.attention_model(str_to_tensor(self, hist))
                w[row, 1:len(hist) + 1] = scores[:len(hist)]
        return w


_GENERATORS = {"self_attention": AttentionWeightGenerator, "levenshtein": LevenshteinWeightGenerator, "decaying": DecayingWeightGenerator}


def weightgenerator_factory(method):
    return _GENERATORS[method]
