"""Tensors a GPU test lays out itself (TEST INFRASTRUCTURE, see oracle/__init__.py): shared by tests/test_gpu_upsample.py and
tests/test_gpu_norm.py.  Needs torch and, to construct a Laid, the device."""
import ctypes

import numpy as np
import torch

DEV = "cuda:0"
SENT = 12288.0                    # the sentinel around every tensor: a value fp16 and bf16 hold exactly
PAD = 64                          # sentinel elements before and after (keeps the 16-byte alignment of the first element)
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ST = {"f32": 0, "f16": 1, "bf16": 2}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


class Laid:
    """A logical channels-last [N, D, H, W, C] tensor as channels [lo, lo + C) of a Wd-channel buffer the test owns, PAD
    sentinels before and after.  The other channels hold `other` (NaN for an input, the sentinel for an output); the
    elements hold `data` (float32 values the storage type holds exactly) or NaN (an output: an element never written shows)."""

    def __init__(self, shape, dtype, data=None, Wd=None, lo=0, other=float("nan")):
        N, D, H, W, C = shape
        Wd = Wd or C
        self.shape, self.Wd, self.lo, self.other, self.C = tuple(shape), Wd, lo, other, C
        self.vox = N * D * H * W
        self.buf = torch.full((2 * PAD + self.vox * Wd,), SENT, dtype=dtype, device=DEV)
        last = PAD + lo + (self.vox - 1) * Wd + C - 1
        assert 0 <= lo and lo + C <= Wd and last < PAD + self.vox * Wd == self.buf.numel() - PAD, "the tensor leaves its buffer"
        if Wd != C:
            self._body().fill_(other)
        if data is None:
            self.view.fill_(float("nan"))
        else:
            assert tuple(data.shape) == self.shape and data.dtype == np.float32
            src = torch.from_numpy(data).to(DEV)
            self.view.copy_(src)
            assert torch.equal(self.view.float(), src), "the storage type holds the inputs exactly"

    def _body(self):
        return self.buf[PAD:PAD + self.vox * self.Wd].view(self.vox, self.Wd)

    @property
    def view(self):
        N, D, H, W, C = self.shape
        Wd = self.Wd
        return torch.as_strided(self.buf, self.shape, (D * H * W * Wd, H * W * Wd, W * Wd, Wd, 1), PAD + self.lo)

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def host(self):
        return self.view.to(torch.float64).cpu().numpy()

    def bits(self):
        return self.view.contiguous().view(BITS[self.buf.dtype]).clone()

    def intact(self):
        """the sentinels before and after, and the channels that are not the tensor's, hold what they held"""
        ok = bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[-PAD:] == SENT).all())
        if self.Wd != self.C:
            b = self._body()
            rest = torch.cat([b[:, :self.lo], b[:, self.lo + self.C:]], dim=1)
            ok = ok and bool(torch.isnan(rest).all() if self.other != self.other else (rest == self.other).all())
        return ok
