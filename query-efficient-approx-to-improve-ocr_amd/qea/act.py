"""One activation of the UNet / CRNN schedules as the kernels take it, stated once: the tensor, the channels used, the pixel stride and the
abs-max slot its producer fills.  An Act is [pixels][channels] rows (any leading dimensions, e.g. [T][B][C], are rows too: nrows) with unit
channel stride; a layer reads and writes channel slices of wider rows, so t, C and ld are stored, never re-derived: the up half of a
concat buffer is the whole [M][2c] tensor with C = c, ld = 2c.  amax: the 4-byte slot (ops.AmaxPool) the two-way fp16 split scales the
tensor from, or None (no producer carries it: the consumer makes its own pass where it needs one).  The bound of a whole tensor bounds
every slice of it, so every view shares its parent's slot.  What a record does not define itself it answers as its tensor (shape,
detach(), indexing), so the saved contexts read as they did when they held tensors."""
import torch


class Act:
    __slots__ = ("t", "C", "ld", "amax", "nrows")

    def __init__(self, t, C=None, ld=None, amax=None):
        width, stride = t.shape[-1], t.stride()
        self.t, self.C, self.ld, self.amax, self.nrows = t, width if C is None else C, stride[-2] if ld is None else ld, amax, t.numel() // width
        if stride[-1] != 1 or self.ld < self.C or self.C > width:
            raise ValueError(f"no [rows][{self.C}] operand with pixel stride {self.ld} in a tensor of shape {tuple(t.shape)}, strides {stride}")

    @classmethod
    def empty(cls, rows, C, device, slot=None):
        """a fresh dense [rows][C] (rows: a count or the leading dimensions) and, from the pool `slot`, its abs-max slot with it"""
        a = object.__new__(cls)                                # (dense by construction: nothing to check)
        a.t = torch.empty((rows, C) if isinstance(rows, int) else (*rows, C), device=device)
        a.C, a.ld, a.amax, a.nrows = C, C, slot() if slot is not None else None, a.t.numel() // C
        return a

    def rows(self, r0, n):
        """n entries of the leading dimension from r0 on (as a view)"""
        return Act(self.t[r0:r0 + n], self.C, self.ld, self.amax)

    def cols(self, c0, C):
        """channels c0 .. c0 + C (as a view)"""
        return Act(self.t[..., c0:c0 + C], C, self.ld, self.amax)

    def __getattr__(self, name):
        return getattr(self.t, name)                           # whoever only reads the saved activations (trace tools, tests) reads the tensor

    def __getitem__(self, index):
        return self.t[index]
