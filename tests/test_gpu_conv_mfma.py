"""GPU: every kernel of the matrix-core forward / data-gradient convolution family (use_mfma 1 .. 7: csrc/conv_zr.hip,
conv_pp.hip, conv_bf16x3.hip, conv_mfma.hip, conv1x1_stream.hip and the split-K epilogues) on every dispatch path, op by op
through tem_conv3d_fwd_ex, against the float64 references of oracle/conv_mfma_ref.py (which tests/test_conv_mfma_cpu.py pins to
torch float64 conv3d / conv_transpose-free data gradients and whose judge it tests on planted errors).  Cases:
oracle/conv_mfma_cases.py.

Rules, none of them measured.
  lattice inputs     integers, quarters and powers of two: every lo plane of every split is zero and, with sum |terms| / step
                     < 2^24 (asserted on the CPU), every partial sum in any order is a float32 number, so EVERY arithmetic mode
                     returns the float64 value in EVERY element -- fp32 as it is, 16-bit as round16 of it.  No tolerance.
  split inputs       a lattice whose lo planes are not zero (modes 2 and 4): every product the mode keeps is exact, the dropped
                     lo lo is dropped in the model: equality with float32(the modelled sum) -- mode 4 joins its two accumulators
                     with one fma, which rounds once.
  random inputs and every sigmoid output    errors in units of 2^-23 x (sum |modelled terms| + |bias|) against
                     MARGIN x max(e32, 1), e32 the numpy float32 restatement on the modelled terms (a reference, not the code
                     under test), MARGIN of oracle/judge.py: 4; a stored 16-bit element in [round16(ref - band), round16(ref + band)].
  statistics rows    every row written; the units rule per (row group, channel, quantity) against the float64 sums of the tensor
                     AS STORED (just judged): per tile for the team kernels (the sum of a tile's 4 / WM wave rows: z-reuse tiles
                     4 x 16 x 8, ping-pong 4 x 8 x 8), per patch for the patch kernel, per block of consecutive voxels for the
                     split-K epilogue, and per (sample, channel) in total.
  bwd_sums rows      TEM_BP_NORM_SUMS of a split-K data gradient: (sum gy, sum gy xn) per block of the epilogue, the units rule
                     against the float64 sums of the gradient as stored; `delivered` carries the bit.
  chunk strides      16-bit x and y as dense 32-channel planes (x_cs / y_cs), laid out by the test between sentinels.
  out_amax           fp32: the word is the bit pattern of max |y| as stored; 16-bit: round16(word) == max |y stored|; a word
                     preloaded with 2^127 keeps it.

Every case asserts and prints the kernel and the instantiation the library's own dispatch query (tem_conv3d_fwd_mfma_path)
names for exactly the pointers, leading dimensions, operands and options of the launch.

No test provokes a device fault: the test lays every tensor out itself (oracle/gpu_kit.py: extent asserted against its buffer,
NaN in the unused channels of wide inputs, sentinel fill in those of wide outputs, outputs start as NaN, sentinels before and
after), every launch is one the library accepts or refuses with an error code, and every accepted launch is repeated into
outputs reset to NaN and must return the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_mfma_cases as K
from oracle import conv_mfma_ref as M
from oracle import conv_ref as R
from oracle import gpu_kit as kit
from oracle.gpu_kit import Flat, holds_bits as _holds, lay as _lay, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu
BIG = 0x7F000000                  # the bit pattern of 2^127: more than any |y| here
NAN = float("nan")
LEDGER = kit.Ledger("CONV_MFMA_ERR")
option = kit.option_fixture()


def _totals():
    e = LEDGER.exact
    print(f"CONV_MFMA_ERR_SUMMARY lattice and split: {e['mismatches']} of {e['elements']} elements differ from float64 "
          f"in {e['cases']} judged quantities")


_print_worst = LEDGER.summary_fixture(after=_totals)


def _optr(t):
    return t.ptr() if t is not None else None


_SUMS = {}                        # the accumulated sums of a layer, shared by the cases that differ in their epilogue (K.reference)


def _reference(c):
    d = K.inputs(c)
    return d, K.reference(c, d, _SUMS)


class Chunked:
    """A logical [N, D, H, W, C] 16-bit tensor in the chunk-stride layout (tem_conv3d_fwd_ex: x_cs / y_cs): C / 32 dense planes
    [NV][32], plane k at k * NV * 32 elements, leading dimension 32, PAD sentinels before and after.  The interface of
    gpu_kit.Laid as far as the test uses it; `view` is [N, D, H, W, C / 32, 32]."""

    def __init__(self, shape, dtype, data=None):
        N, D, H, W, C = shape
        assert C % 32 == 0
        self.shape, self.vox, self.nk, self.Wd = tuple(shape), N * D * H * W, C // 32, 32
        self.cs = self.vox * 32
        self.buf = torch.full((2 * kit.PAD + self.nk * self.cs,), kit.SENT, dtype=dtype, device=kit.DEV)
        assert kit.PAD + (self.nk - 1) * self.cs + (self.vox - 1) * 32 + 31 < self.buf.numel() - kit.PAD, "the tensor leaves its buffer"
        if data is None:
            self.view.fill_(NAN)
        else:
            src = torch.from_numpy(data).to(kit.DEV).reshape(N, D, H, W, self.nk, 32)
            self.view.copy_(src)
            assert torch.equal(self.view.float(), src), "the storage type holds the inputs exactly"

    @property
    def view(self):
        N, D, H, W, _ = self.shape
        return torch.as_strided(self.buf, (N, D, H, W, self.nk, 32), (D * H * W * 32, H * W * 32, W * 32, 32, self.cs, 1), kit.PAD)

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def host(self):
        return self.view.to(torch.float64).cpu().numpy().reshape(self.shape)

    def bits(self):
        return self.view.contiguous().view(kit.BITS[self.buf.dtype]).clone()

    def intact(self):
        return bool((self.buf[:kit.PAD] == kit.SENT).all()) and bool((self.buf[-kit.PAD:] == kit.SENT).all())

    def holds(self, data):
        want = torch.from_numpy(data).to(kit.DEV).to(self.buf.dtype).reshape(self.view.shape)
        return self.intact() and torch.equal(self.bits(), want.contiguous().view(kit.BITS[self.buf.dtype]))


def _holds_any(L, data):
    return L.holds(data) if isinstance(L, Chunked) else _holds(L, data)


class Call:
    """the tensors of one launch, laid out by the test"""

    def __init__(self, c, d, ncu):
        self.c, self.d = c, d
        lib = _lib().load()
        sh = c.shape
        xlay = (c.cin + 8, 8) if c.wide else None
        ylay = (c.cout + 8, 8) if c.wide or c.ybuf else None
        if c.cs:
            self.X, self.Y = Chunked(sh + (c.cin,), kit.TORCH[c.st], d["x"]), Chunked(sh + (c.cout,), kit.TORCH[c.st])
            assert (self.X.cs, self.Y.cs) == c.strides()
        else:
            self.X = _lay(sh + (c.cin,), c.st, xlay, d["x"])
            self.Y = _lay(sh + (c.cout,), c.st, ylay, None, output=True)
        self.REF = _lay(sh + (c.cout,), c.st, (c.cout + 8, 8) if c.wide else None, d["ref"]) if c.ref else None
        # the packed weights: the library's own pack of the layer's state_dict weights (transpose: the data-gradient operator)
        co, ci = (c.cin, c.cout) if c.dgrad else (c.cout, c.cin)
        self.Wsd = Flat(0, data=d["w_sd"])
        self.W = Flat(int(lib.tem_conv_packed_size(co, ci, *c.k)))
        assert lib.tem_conv_pack_weights(self.Wsd.ptr(), self.W.ptr(), co, ci, *c.k, int(c.dgrad), c.mode, _stream()) == 0, lib.tem_last_error()
        torch.cuda.synchronize()
        self.W.data = self.W.body.clone()                                   # from here on an input: must stay as packed
        self.B = Flat(0, data=d["bias"]) if c.bias else None
        self.S = Flat(0, data=d["scale"]) if c.norm else None
        self.T = Flat(0, data=d["shift"]) if c.norm else None
        self.CO = Flat(0, data=d["coef"]) if c.refnorm else None
        self.AI = Flat(0, data=np.array([d["amax"]], np.float32)) if c.gscaled else None
        self.need = K.fwd_ws(lib, c)
        self.WS = Flat(self.need // 4 + 4)
        self.ws_bytes = self.need
        self.nblk = K.expected(c, ncu)[2] if c.stat else 0
        self.P = Flat(sh[0] * self.nblk * c.cout * 2) if c.stat else None
        self.A = Flat(1, 0.0) if c.amax else None
        self.SX = self.MU = self.RS = self.SP = None
        if c.sums:                                                          # TEM_BP_NORM_SUMS: the norm input, its mean / rstd, the rows
            self.SX = _lay(sh + (c.cout,), c.st, None, d["sums_x"])
            self.MU, self.RS = Flat(0, data=d["sums_mean"]), Flat(0, data=d["sums_rstd"])
            self.sums_nblk = K.splitk_stat_blocks(c.nv // sh[0], c.cout)
            self.SP = Flat(sh[0] * self.sums_nblk * c.cout * 2)
        self.delivered = 0

    def pointers(self):
        return {"x": self.X.ptr(), "y": self.Y.ptr(), "w": self.W.ptr(), "ref": _optr(self.REF), "bias": _optr(self.B), "scale": _optr(self.S),
                "shift": _optr(self.T), "coef": _optr(self.CO), "amax": _optr(self.AI)}

    def _bp(self):
        a = lambda t: t.body.data_ptr() if t is not None else 0                                       # noqa: E731
        return K.byproducts(_lib(), self.c, {"out_amax": a(self.A), "sums_x": self.SX.view.data_ptr() if self.SX is not None else 0,
                                             "sums_mean": a(self.MU), "sums_rstd": a(self.RS), "sums_part": a(self.SP)})

    def query(self):
        bp = self._bp()
        return K.query(_lib().load(), self.c, self.pointers(), self.ws_bytes, ctypes.byref(bp) if bp is not None else None)

    def launch(self):
        c, p, lib = self.c, self.pointers(), _lib().load()
        x_ld, y_ld, ref_ld = c.lds()
        assert self.X.view.shape[:4] == self.Y.view.shape[:4] == c.shape and (self.X.Wd, self.Y.Wd) == (x_ld, y_ld), "the extents the launch is told"
        assert self.REF is None or self.REF.Wd == ref_ld
        bp = self._bp()
        rc = lib.tem_conv3d_fwd_ex(p["x"], x_ld, p["scale"], p["shift"], p["w"], p["bias"], p["y"], y_ld, p["ref"], ref_ld, self.WS.ptr(),
                                   self.ws_bytes, *c.shape, c.cin, c.cout, *c.k, c.act, K.use_mfma(c), p["amax"], p["coef"], _optr(self.P),
                                   self.nblk, *c.strides(), ctypes.byref(bp) if bp is not None else None, _stream())
        torch.cuda.synchronize()
        self.delivered = bp.delivered if bp is not None else 0
        return rc

    def inputs_intact(self):
        d = self.d
        return (_holds_any(self.X, d["x"]) and (self.REF is None or _holds(self.REF, d["ref"])) and self.Y.intact() and
                (self.SX is None or _holds(self.SX, d["sums_x"])) and
                all(t is None or t.intact() for t in (self.Wsd, self.W, self.B, self.S, self.T, self.CO, self.AI, self.WS, self.P, self.A,
                                                      self.MU, self.RS, self.SP)))

    def untouched(self):
        return (self.inputs_intact() and bool(torch.isnan(self.Y.view).all()) and (self.P is None or self.P.unwritten())
                and (self.SP is None or self.SP.unwritten()))


def _judge(tag, label, quantity, dt, got, ref, scale, e32, exact):
    kit.judge(LEDGER, M, tag, label, quantity, dt, got, ref, scale, e32, exact, suffix=True)


def _judge_stats(tag, label, c, kernel, got, pk, ncu):
    """pk: the rows as written, [N][nblk][C][2]; got: the tensor as stored"""
    geo = K.stat_geometry(c, kernel, ncu)
    N, C = c.shape[0], c.cout
    if geo[0] == "tile":
        rows, scales = R.block_stats_f64(got, geo[1])
        e32 = R.block_stats_e32(got, geo[1], rows, scales)
        grouped = pk.reshape(N, -1, geo[2], C, 2).sum(axis=2)
    else:
        rows, scales = M.linear_stats_f64(got, geo[1])
        e32 = M.linear_stats_e32(got, geo[1], rows, scales)
        grouped = pk
    assert grouped.shape == rows.shape, f"{tag}: {pk.shape} rows written, the documented geometry has {rows.shape}"
    trow, tscale = M.total_stats_f64(got)
    for j, name in enumerate(("sum y", "sum y^2")):
        _judge(tag, label, name, "f32", grouped[..., j], rows[..., j], scales[..., j], e32[j], False)
        _judge(tag, label, name + " per sample", "f32", pk.sum(axis=1)[..., j], trow[..., j], tscale[..., j], e32[j], False)


def _run(c, option):
    lib = _lib().load()
    for key, value in c.opts.items():
        option(key, value)
    ncu = lib.tem_device_cus()
    d, r = _reference(c)
    tag = f"{c.id} {c.shape} {c.cin}->{c.cout} k={c.k}"
    call = Call(c, d, ncu)
    kernel, inst = call.query()
    ekernel, einst, eblk = K.expected(c, ncu)
    print(f"CONV_MFMA_PATH {tag}: query {K.NAME.get(kernel)} {inst}, intended {K.NAME[c.want]}")
    assert (kernel, inst) == (ekernel, einst), f"{tag}: the rules name {K.NAME[ekernel]} {einst}, the query {K.NAME.get(kernel, kernel)} {inst}"
    assert kernel == c.want, f"{tag}: meant for {K.NAME[c.want]}"
    if c.stat:
        x_ld, y_ld, ref_ld = c.lds()
        assert call.nblk == eblk == lib.tem_conv3d_fwd_stat_blocks_ld(*c.shape, c.cin, c.cout, *c.k, K.use_mfma(c), x_ld, y_ld, ref_ld, 0) > 0, tag
    assert call.launch() == 0, f"{tag}: the launch is accepted: {lib.tem_last_error()}"
    first, got = call.Y.bits(), call.Y.host()
    pfirst = call.P.bits() if call.P is not None else None
    sfirst = call.SP.bits() if call.SP is not None else None
    assert call.SP is None or call.delivered & 4, f"{tag}: the split-K epilogue delivers TEM_BP_NORM_SUMS"
    label = K.NAME[kernel] + f" m{c.mode}"
    if call.A is not None:
        w = int(call.A.bits().item()) & 0xFFFFFFFF
        assert call.delivered & 1, f"{tag}: the launch delivers out_amax"
        assert M.amax_ok(w, got, c.st), f"{tag}: out_amax {w:#x} is not max |y| = {np.abs(got).max()}"
        call.A.body.view(torch.int32).fill_(BIG)
    call.Y.view.fill_(NAN)
    call.WS.body.fill_(NAN)
    if call.P is not None:
        call.P.body.fill_(NAN)
    if call.SP is not None:
        call.SP.body.fill_(NAN)
    assert call.launch() == 0
    assert call.SP is None or torch.equal(sfirst, call.SP.bits()), f"{tag}: the rows of the norm backward are bit-identical too"
    assert torch.equal(first, call.Y.bits()), f"{tag}: a repeated launch is bit-identical"
    assert call.P is None or torch.equal(pfirst, call.P.bits()), f"{tag}: ... and so are its statistics rows"
    assert call.A is None or int(call.A.bits().item()) == BIG, f"{tag}: a larger out_amax stays"
    assert call.inputs_intact(), f"{tag}: wrote outside the elements of y, or to an input"
    exact = c.recipe in ("lattice", "split") and c.act != K.SIGMOID
    q = "y" + (" (sigmoid)" if c.act == K.SIGMOID else "") + (" (dgrad)" if c.dgrad else "")
    if exact:
        _judge(tag, label, q, c.st, got, M.exact_store(r["y"], c.mode, c.st), None, 0.0, True)
    else:
        _judge(tag, label, q, c.st, got, r["y"], r["mag"], r["e32"], False)
    if call.P is not None:
        assert not call.P.unwritten() and bool(torch.isfinite(call.P.body).all()), f"{tag}: every statistics row is written"
        _judge_stats(tag, label, c, kernel, got, call.P.host().reshape(c.shape[0], call.nblk, c.cout, 2), ncu)
    if call.SP is not None:                      # (sum gy, sum gy xn) per block of the split-K epilogue, of the gradient as stored
        assert bool(torch.isfinite(call.SP.body).all()), f"{tag}: every row of the norm backward is written"
        vb = K.splitk_vb(c.cout)
        rows, scales = M.bwd_sums_f64(got, d["sums_x"], d["sums_mean"], d["sums_rstd"], vb)
        e32 = M.bwd_sums_e32(got, d["sums_x"], d["sums_mean"], d["sums_rstd"], vb, rows, scales)
        pk = call.SP.host().reshape(rows.shape)
        for j, name in enumerate(("sum gy", "sum gy xn")):
            _judge(tag, label, name, "f32", pk[..., j], rows[..., j], scales[..., j], e32[j], False)


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.id)
def test_forward_and_data_gradient_against_float64(c, option):
    _run(c, option)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_return_an_error_and_write_nothing(option):
    lib = _lib().load()
    ncu = lib.tem_device_cus()
    sh = (2, 5, 17, 9)
    cases = [
        # statistics where stat_blocks is 0: the patch kernel's split-K launch writes no rows
        ("statistics on a split-K patch launch", K.Case("refuse_stat", -1, (2, 3, 9, 11), 32, 64, K.K333, 2, stat=True, opts={"conv_fwd_variant": 0}), {}),
        # the split-K launch of the z-reuse kernel writes the rows only with its workspace
        ("statistics with a short workspace", K.Case("refuse_ws", -1, (1, 8, 16, 32), 256, 256, K.K333, 2, stat=True), {"ws_bytes": 1024}),
        ("in_amax outside mode 4", K.Case("refuse_amax", -1, sh, 32, 64, K.K333, 2, gscaled=True, dgrad=True, opts={"conv_fwd_variant": 2}), {}),
        ("ref_coef off the z-reuse kernel", K.Case("refuse_coef", -1, (2, 5, 9, 9), 32, 64, K.K333, 2, refnorm=True, dgrad=True,
                                                   opts={"conv_fwd_variant": 1}), {}),
    ]
    for what, c, kw in cases:
        for key, value in c.opts.items():
            option(key, value)
        call = Call(c, K.inputs(c), ncu)
        if c.stat and not call.nblk:                      # a buffer of the size the caller would have sized for rows of the other kernel
            call.nblk = 1 if "ws_bytes" not in kw else K.splitk_stat_blocks(c.nv // c.shape[0], c.cout)
            call.P = Flat(c.shape[0] * call.nblk * c.cout * 2)
        if "ws_bytes" in kw:
            call.ws_bytes = kw["ws_bytes"]
        else:
            assert K.expected(c, ncu)[0] == -1, what
        assert call.query()[0] == -1, what
        rc = call.launch()
        print(f"CONV_MFMA_REFUSAL {what}: rc {rc}: {lib.tem_last_error()}")
        assert rc != 0 and call.untouched() and call.WS.unwritten(), f"{what}: rc {rc}"
        for key in c.opts:
            option(key, K.DEFAULTS[key])
    lib.tem_last_error()
