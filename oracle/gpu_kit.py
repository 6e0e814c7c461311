"""The apparatus of a GPU op-by-op suite (TEST INFRASTRUCTURE, see oracle/__init__.py): what two or more of
tests/test_gpu_{dice,norm,upsample,maxpool,conv_valu,spoco_ops,defect}.py use.  Needs torch and pytest and, to construct a
Laid or a Flat, the device.

  lib / ops / stream      the library module, torch_em_amd.ops, the current stream as a C pointer
  option_fixture          factory of the fixture "set library options for one test, restore them afterwards"
  Laid, Flat, lay         tensors the test lays out itself, between sentinels;  holds_values / holds_bits: still an input
  Ledger                  the worst figure and the case count per (key, quantity); `<PREFIX>_SUMMARY` rows at teardown
  judge                   the three-way assertion (exact / fp32 units / 16-bit interval) with a reference module's bound judge
"""
import ctypes

import numpy as np
import pytest
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


class Flat:
    """a float32 array between sentinels: an output the library writes (NaN until written) or a small input (weights, bias,
    coefficients); off: elements the first one is moved off its 16-byte boundary"""

    def __init__(self, n, fill=float("nan"), data=None, off=0):
        n = int(np.asarray(data).size) if data is not None else int(n)
        self.buf = torch.full((2 * PAD + n + off,), SENT, dtype=torch.float32, device=DEV)
        self.body = self.buf[PAD + off:PAD + off + n]
        self.off = off
        if data is not None:
            self.data = torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1)).to(DEV)
            self.body.copy_(self.data)
        else:
            self.data = None
            self.body.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.body.data_ptr())

    def intact(self):
        """the sentinels, and for an input the values"""
        ok = bool((self.buf[:PAD + self.off] == SENT).all()) and bool((self.buf[PAD + self.off + self.body.numel():] == SENT).all())
        return ok and (self.data is None or torch.equal(self.body.view(torch.int32), self.data.view(torch.int32)))

    def bits(self):
        return self.body.view(torch.int32).clone()

    def host(self):
        return self.body.double().cpu().numpy()

    def unwritten(self):
        return bool(torch.isnan(self.body).all())


def lay(shape, dt, spec, data=None, output=False):
    """a Laid of storage type dt ("f32" | "f16" | "bf16"); spec: None, or (Wd, lo): channels [lo, lo + C) of a Wd-channel
    buffer whose other channels hold NaN (an input) or the sentinel (an output)"""
    Wd, lo = spec if spec else (None, 0)
    return Laid(shape, TORCH[dt], data, Wd, lo, other=SENT if output else float("nan"))


def holds_values(L, data):
    """the tensor still holds `data` as values (NaN matches NaN)"""
    want = torch.from_numpy(data).to(DEV)
    got = L.view.float()
    return L.intact() and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


def holds_bits(L, data):
    """the tensor still holds `data`, bit for bit (-0.0 included)"""
    want = torch.from_numpy(data).to(DEV).to(L.buf.dtype)
    return L.intact() and torch.equal(L.bits(), want.contiguous().view(L.bits().dtype))


# ------------------------------------------------------------------------------------------ the library
def lib():
    from torch_em_amd import _lib
    return _lib


def ops():
    from torch_em_amd import ops
    return ops


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def option_fixture(name=None):
    """-> a fixture, to be assigned to the module-level name the tests request: it yields set_option(name, value), or with
    `name` set_option(value) of that one option; the values found at the first change are restored after the test"""
    @pytest.fixture
    def option():
        L, old = lib(), {}

        def set_option(key, value):
            old.setdefault(key, L.get_option(key))
            L.set_option(key, value)
        yield set_option if name is None else lambda value: set_option(name, value)
        for key, value in old.items():
            L.set_option(key, value)
    return option


# ------------------------------------------------------------------------------------------ worst figures, for the record
class Ledger:
    """per (key, quantity): the case with the worst ratio = kernel units / max(e32, 1), as (kernel, f32, ratio), and the
    number of cases noted.  prefix: the suite's print prefix ("UPSAMPLE_ERR"); the per-case lines start with it, the rows at
    teardown with `<prefix>_SUMMARY`."""

    def __init__(self, prefix):
        self.prefix, self.worst = prefix, {}
        self.exact = {"elements": 0, "mismatches": 0, "cases": 0}        # totals over the exact judgements of judge()

    def note(self, key, quantity, ek, e32, ratio=None):
        """ratio: given by a suite whose figure is not units over max(e32, 1) (a band quantity: ek = e32 = None)"""
        if ratio is None:
            ratio = ek / max(e32, 1.0)
        cur = self.worst.get((key, quantity))
        n = 1 + (cur[3] if cur else 0)
        self.worst[(key, quantity)] = (ek, e32, ratio, n) if cur is None or ratio > cur[2] else cur[:3] + (n,)
        return ratio

    def print_summary(self, legend="", left_out=None, footnote=""):
        """left_out(quantity): rows that are printed but are not part of the worst ratio"""
        p = self.prefix + "_SUMMARY"
        print(f"\n{p} key / quantity: kernel, f32, ratio, cases{legend}")
        for (key, q), (ek, e32, ratio, n) in sorted(self.worst.items()):
            cols = "      -       -" if ek is None else f"{ek:7.2f} {e32:7.2f}"
            print(f"{p} {key:<36} {q:<22} {cols} {ratio:6.2f} {n:4d}")
        judged = [v[2] for (_, q), v in self.worst.items() if left_out is None or not left_out(q)]
        if judged:
            print(f"{p} worst ratio {max(judged):.2f}{footnote}")

    def summary_fixture(self, after=None, **how):
        """-> the module-scoped autouse fixture that prints the summary at teardown, to be assigned to a module-level name;
        how: print_summary's arguments; after(): the suite's own rows, printed behind the shared ones"""
        @pytest.fixture(scope="module", autouse=True)
        def print_worst():
            yield
            self.print_summary(**how)
            if after is not None:
                after()
        return print_worst


def judge(ledger, R, tag, label, quantity, dt, got, ref, scale=None, e32=0.0, exact=False, finite=True, suffix=False):
    """One judged quantity: printed, noted in the ledger, asserted.  R: the reference module, for ITS bound units / within /
    outside16 / excess16 / mismatches (its allowance, its NaN rule).
      exact     every element equals `ref`, the exact value as the storage type holds it (R.mismatches)
      fp32      every element within MARGIN * max(e32, 1) units of 2^-23 x scale
      16-bit    every stored element inside the rounded band's closed interval
    finite: a non-finite element (never written) fails first; off for exact quantities that hold NaN or inf.
    suffix: the ledger keys of 16-bit and exact judgements carry " 16" and " (exact)"."""
    p = ledger.prefix
    if finite:
        assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} elements of {quantity} were never written or are not finite"
    key = label + (" 16" if suffix and dt != "f32" else "")
    if exact:
        bad = R.mismatches(got, ref)
        ledger.exact["elements"] += ref.size
        ledger.exact["mismatches"] += bad
        ledger.exact["cases"] += 1
        print(f"{p} {tag} -> {label} {quantity}: {bad} of {ref.size} elements differ from the exact value")
        ledger.note(key, quantity + (" (exact)" if suffix else ""), 0.0 if bad == 0 else float("inf"), 0.0)
        assert bad == 0, (f"{tag}: {bad} elements of {quantity} are not the exact value (first at "
                          f"{np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:3].tolist()})")
    elif dt == "f32":
        ek = R.units(got, ref, scale)
        print(f"{p} {tag} -> {label} {quantity}: kernel {ek:.2f} f32 {e32:.2f}")
        ledger.note(key, quantity, ek, e32)
        assert R.within(ek, e32), f"{tag}: {quantity} is {ek:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"
    else:
        ek = R.excess16(got, ref, scale, dt)
        bad = R.outside16(got, ref, scale, e32, dt)
        print(f"{p} {tag} -> {label} {quantity}: {bad} of {got.size} stored elements outside their interval; beyond the "
              f"ideal rounding: kernel {ek:.2f} f32 {e32:.2f}")
        ledger.note(key, quantity, ek, e32)
        assert bad == 0, f"{tag}: {bad} stored elements of {quantity} outside [round16(ref - band), round16(ref + band)]"
