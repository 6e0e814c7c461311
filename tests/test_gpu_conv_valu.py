"""GPU: every kernel of the VALU convolution family (use_mfma 0: csrc/conv.hip, csrc/conv_small.hip) on every dispatch path,
op by op through tem_conv3d_fwd_ex, tem_conv3d_wgrad, tem_conv3d_wgrad_gnorm_st and tem_conv1x1_out_bwd_st, against the float64
references of oracle/conv_ref.py (which tests/test_conv_valu_cpu.py pins to torch float64 conv3d and its autograd, and whose
judge it tests on planted errors).  Cases: oracle/conv_cases.py.

Rules, none of them measured.
  lattice inputs     small integers, quarters and powers of two, sum |terms| / step < 2^24 (asserted on the CPU): every
                     partial sum is a float32 number in any order, so EVERY output element equals the float64 value -- fp32 as
                     it is, 16-bit as round16 of it; masks are decided on exact zeros (0.0 and -0.0), out_amax is the exact
                     maximum.  No tolerance.
  random inputs and every sigmoid output    errors in units of 2^-23 x the per-element scale (sum |terms| + |bias|; sigmoid:
                     s (1 - s) (sum |terms| + 1) + s after the absolute allowance 2^-126; dw: sum_v |xhat g|); on the same inputs
                     e32 is the worst figure of the numpy float32 restatement (bias first, then (tap, ci) in order; products
                     rounded separately, and contracted) -- a reference, not the code under test.  EVERY fp32 element within
                     MARGIN * max(e32, 1) units, MARGIN of oracle/judge.py: 4; every stored 16-bit element in
                     [round16(ref - band), round16(ref + band)].
  statistics rows    the units rule per (block, channel, quantity) against the float64 sums of the tensor AS STORED (just judged),
                     scales sum |y| and sum y^2, blocks as tem_conv3d_fwd_valu_path documents them.
  out_amax           fp32: the word is the bit pattern of max |y| as stored; 16-bit: round16(word) == max |y stored|.  A word
                     preloaded with 0 receives the value, one preloaded with 2^127 keeps it.
  tem_conv1x1_out_bwd_st   dw / db equal bit for bit to tem_conv3d_wgrad (the two-kernel route) on the same inputs.

Every case asserts and prints the kernel and instantiation the library's own dispatch query (tem_conv3d_fwd_valu_path /
tem_conv3d_wgrad_path) names for exactly the pointers, leading dimensions and operands of the launch.

No test provokes a device fault: the test lays every tensor out itself (oracle/gpu_kit.py: extent asserted against its
buffer, NaN in the unused channels of wide inputs, sentinel fill in those of wide outputs, outputs start as NaN, sentinels
before and after), every launch is one the library accepts or refuses with an error code, and every accepted launch is
repeated into outputs reset to NaN and must return the same bits.

Observed on the MI355X (profiles/conv_valu_op_errors.txt): no element of any lattice case differs from float64 (26.5 million
elements in 1422 judged quantities); worst kernel error / max(e32, 1) = 1.20 (cout1 on random data,
2.03 units where the restatement has 1.69); the sigmoid outputs stay at 1.10 units and below; no 16-bit element outside its
interval; out_bwd equals the two-kernel route in every bit.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_cases as K
from oracle import conv_ref as R
from oracle import gpu_kit as kit
from oracle.gpu_kit import ST, Flat, holds_bits as _holds, lay as _lay, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu
BIG = 0x7F000000                  # the bit pattern of 2^127: more than any |y| here
NAN = float("nan")
LEDGER = kit.Ledger("CONV_VALU_ERR")


def _lattice_totals():
    e = LEDGER.exact
    print(f"CONV_VALU_ERR_SUMMARY lattice: {e['mismatches']} of {e['elements']} elements differ from float64 "
          f"in {e['cases']} judged quantities")


_print_worst = LEDGER.summary_fixture(after=_lattice_totals)


def _mode(pair):
    return (ST[pair[0]] << 8) | (ST[pair[1]] << 12)


def _optr(t):
    return t.ptr() if t is not None else None


def _judge(tag, label, quantity, dt, got, ref, scale, e32, exact):
    """exact: every element equals the float64 value as the storage type holds it; else the units rule"""
    kit.judge(LEDGER, R, tag, label, quantity, dt, got, R.stored(ref, dt) if exact else ref, scale, e32, exact, suffix=True)


_REF = {}


def _cached(key, make):
    if key not in _REF:
        if len(_REF) >= 16:
            _REF.clear()
        _REF[key] = make()
    return _REF[key]


# ------------------------------------------------------------------------------------------ forward
class FwdCall:
    """the tensors of one forward launch, laid out by the test"""

    def __init__(self, c, d):
        self.c, self.d = c, d
        sh = c.shape
        self.X = _lay(sh + (c.cin,), c.pair[0], c.xlay, d["x"])
        self.Y = _lay(sh + (c.cout,), c.pair[1], c.ylay, None, output=True)
        self.REF = _lay(sh + (c.cout,), c.pair[1], c.reflay, d["ref"]) if c.ref else None
        self.W = Flat(0, data=d["w"])
        self.B = Flat(0, data=d["bias"], off=c.bias_off) if c.bias else None
        self.S = Flat(0, data=d["scale"]) if c.norm else None
        self.T = Flat(0, data=d["shift"]) if c.norm else None
        t = K.stat_tile(c)
        self.nblk = -(-sh[1] // t[0]) * -(-sh[2] // t[1]) * -(-sh[3] // t[2]) if c.stat else 0
        self.P = Flat(sh[0] * self.nblk * c.cout * 2) if c.stat else None
        self.A = Flat(1, 0.0) if c.amax else None

    def _args(self):
        c = self.c
        N, D, H, W = c.shape
        return (self.X.ptr(), self.X.Wd, _optr(self.S), _optr(self.T), self.W.ptr(), _optr(self.B), self.Y.ptr(), self.Y.Wd,
                _optr(self.REF), self.REF.Wd if self.REF else 0), (N, D, H, W, c.cin, c.cout) + c.k + (c.act, _mode(c.pair))

    def query(self):
        ptrs, ints = self._args()
        inst = (ctypes.c_int * 4)()
        return _lib().load().tem_conv3d_fwd_valu_path(*ptrs, *ints, int(self.c.stat), inst), list(inst)

    def launch(self):
        ptrs, ints = self._args()
        L = _lib()
        bp = None
        if self.A is not None:
            bp = L.Byproducts()
            bp.out_amax = self.A.body.data_ptr()
        assert self.X.view.shape[:4] == self.Y.view.shape[:4] == self.c.shape, "the extents the launch is told"
        rc = L.load().tem_conv3d_fwd_ex(*ptrs, None, 0, *ints, None, None, _optr(self.P), self.nblk, 0, 0,
                                        ctypes.byref(bp) if bp is not None else None, _stream())
        torch.cuda.synchronize()
        self.delivered = bp.delivered if bp is not None else 0
        return rc

    def inputs_intact(self):
        d = self.d
        return (_holds(self.X, d["x"]) and (self.REF is None or _holds(self.REF, d["ref"])) and self.W.intact() and
                all(t is None or t.intact() for t in (self.B, self.S, self.T)) and self.Y.intact() and
                all(t is None or t.intact() for t in (self.P, self.A)))

    def untouched(self):
        return self.inputs_intact() and bool(torch.isnan(self.Y.view).all()) and (self.P is None or self.P.unwritten())


def _fwd_ref(c):
    key = ("fwd", c.name, c.shape, c.bias, c.norm, c.act, c.ref, c.recipe)
    return _cached(key, lambda: (lambda d: (d, K.fwd_reference(c, d)))(K.fwd_inputs(c)))


def _run_forward(c):
    d, r = _fwd_ref(c)
    tag = f"fwd {c.id} {c.shape} {c.cin}->{c.cout} k={c.k}"
    call = FwdCall(c, d)
    path, inst = call.query()
    epath, einst = K.expected_fwd(c)
    print(f"CONV_VALU_PATH {tag}: query {K.FWD_NAME.get(path)} {inst}, intended {K.FWD_NAME[c.want]}")
    assert (path, inst) == (epath, einst), f"{tag}: the rules name {K.FWD_NAME[epath]} {einst}, the query {K.FWD_NAME.get(path, path)} {inst}"
    assert path == c.want, f"{tag}: meant for {K.FWD_NAME[c.want]}"
    if path < 0:
        rc = call.launch()
        print(f"CONV_VALU_REFUSAL {tag}: rc {rc}")
        assert rc != 0 and call.untouched(), f"{tag}: a refused launch returns an error and writes nothing (rc {rc})"
        _lib().load().tem_last_error()
        return
    assert call.launch() == 0, f"{tag}: the launch is accepted: {_lib().load().tem_last_error()}"
    first, got = call.Y.bits(), call.Y.host()
    pfirst = call.P.bits() if call.P is not None else None
    label = K.FWD_NAME[path]
    if call.A is not None:
        w = int(call.A.bits().item()) & 0xFFFFFFFF
        if path == K.EXPAND:
            assert call.delivered & 1, f"{tag}: the expansion delivers out_amax"
            assert R.amax_ok(w, got, c.pair[1]), f"{tag}: out_amax {w:#x} is not max |y| = {np.abs(got).max()}"
        else:
            assert not (call.delivered & 1) and w == 0
        call.A.body.view(torch.int32).fill_(BIG)
    call.Y.view.fill_(NAN)
    if call.P is not None:
        call.P.body.fill_(NAN)
    assert call.launch() == 0
    assert torch.equal(first, call.Y.bits()), f"{tag}: a repeated launch is bit-identical"
    assert call.P is None or torch.equal(pfirst, call.P.bits()), f"{tag}: ... and so are its statistics rows"
    assert call.A is None or path != K.EXPAND or int(call.A.bits().item()) == BIG, f"{tag}: a larger out_amax stays"
    assert call.inputs_intact(), f"{tag}: wrote outside the elements of y, or to an input"
    exact = c.recipe == "lattice" and c.act != K.SIGMOID
    q = "y" + (" (sigmoid)" if c.act == K.SIGMOID else "") + (" (lattice)" if c.recipe == "lattice" and not exact else "")
    _judge(tag, label, q, c.pair[1], got, r["y"], r["mag"], r["e32"], exact)
    if call.P is not None:
        tile = K.stat_tile(c)
        rows, scales = R.block_stats_f64(got, tile)                 # of the tensor as stored
        e32 = R.block_stats_e32(got, tile, rows, scales)
        pk = call.P.host().reshape(rows.shape)
        for j, name in enumerate(("sum y", "sum y^2")):
            _judge(tag, label, name, "f32", pk[..., j], rows[..., j], scales[..., j], e32[j], False)


FWD_NAMES = sorted({c.name for c in K.FWD}, key=[c.name for c in K.FWD].index)


@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_against_float64(name):
    for c in K.FWD:
        if c.name == name:
            _run_forward(c)


# ------------------------------------------------------------------------------------------ weight gradients
class WgCall:
    def __init__(self, c, d, ws_bytes=None, ylay=None, coef_off=0):
        ylay = ylay or c.ylay
        self.c, self.d = c, d
        sh, lib = c.shape, _lib().load()
        nt = R.ntaps(c.k)
        self.X = _lay(sh + (c.cin,), c.pair[0], c.xlay, d["x"])
        self.G = _lay(sh + (c.cout,), c.pair[1], c.glay, d["g"])
        self.YN = _lay(sh + (c.cout,), c.pair[1], ylay, d["y"]) if c.gnorm else None
        self.C = Flat(0, data=d["coef"], off=coef_off) if c.gnorm else None
        self.S = Flat(0, data=d["scale"]) if c.norm else None
        self.T = Flat(0, data=d["shift"]) if c.norm else None
        self.DW = Flat(nt * c.cin * c.cout)
        self.DB = Flat(c.cout) if c.db else None
        self.need = int(lib.tem_conv3d_wgrad_ws(*sh, c.cin, c.cout, *c.k, 0))
        self.WS = Flat(self.need // 4 + 4)
        self.ws_bytes = self.need if ws_bytes is None else ws_bytes

    def query(self):
        c = self.c
        return _lib().load().tem_conv3d_wgrad_path(
            self.X.ptr(), self.X.Wd, _optr(self.S), _optr(self.T), self.G.ptr(), self.G.Wd, _optr(self.YN), self.YN.Wd if self.YN else 0,
            _optr(self.C), int(c.db), self.ws_bytes, *c.shape, c.cin, c.cout, *c.k, _mode(c.pair), c.sd)

    def launch(self, pair=None):
        c, lib = self.c, _lib().load()
        pair = pair or c.pair
        assert self.X.view.shape[:4] == self.G.view.shape[:4] == c.shape, "the extents the launch is told"
        if c.gnorm:
            rc = lib.tem_conv3d_wgrad_gnorm_st(self.X.ptr(), self.X.Wd, _optr(self.S), _optr(self.T), self.G.ptr(), self.G.Wd, self.YN.ptr(),
                                               self.YN.Wd, self.C.ptr(), self.DW.ptr(), _optr(self.DB), self.WS.ptr(), self.ws_bytes, *c.shape,
                                               c.cin, c.cout, *c.k, c.sd, ST[pair[0]], ST[pair[1]], _stream())
        else:
            rc = lib.tem_conv3d_wgrad(self.X.ptr(), self.X.Wd, _optr(self.S), _optr(self.T), self.G.ptr(), self.G.Wd, self.DW.ptr(),
                                      _optr(self.DB), self.WS.ptr(), self.ws_bytes, *c.shape, c.cin, c.cout, *c.k, _mode(pair), c.sd, _stream())
        torch.cuda.synchronize()
        return rc

    def inputs_intact(self):
        d = self.d
        return (_holds(self.X, d["x"]) and _holds(self.G, d["g"]) and (self.YN is None or _holds(self.YN, d["y"])) and
                all(t is None or t.intact() for t in (self.C, self.S, self.T, self.DW, self.DB, self.WS)))

    def untouched(self):
        return self.inputs_intact() and self.DW.unwritten() and (self.DB is None or self.DB.unwritten())


def _wg_ref(c):
    key = ("wg", c.name, c.shape, c.cin, c.cout, c.k, c.norm, c.gnorm, c.recipe)
    return _cached(key, lambda: (lambda d: (d, K.wg_reference(c, d)))(K.wg_inputs(c)))


def _run_wgrad(c):
    d, r = _wg_ref(c)
    tag = f"wgrad {c.id} {c.shape} {c.cin}->{c.cout} k={c.k}"
    call = WgCall(c, d)
    path = call.query()
    print(f"CONV_VALU_PATH {tag}: query {K.WG_NAME.get(path)}, intended {K.WG_NAME[c.want]}")
    assert path == c.want == K.expected_wgrad(c), f"{tag}: meant for {K.WG_NAME[c.want]}, the query names {K.WG_NAME.get(path, path)}"
    assert call.launch() == 0, f"{tag}: the launch is accepted: {_lib().load().tem_last_error()}"
    first, fdb = call.DW.bits(), call.DB.bits() if call.DB else None
    dw, db = call.DW.host(), call.DB.host() if call.DB else None
    call.DW.body.fill_(NAN)
    call.WS.body.fill_(NAN)
    if call.DB:
        call.DB.body.fill_(NAN)
    assert call.launch() == 0
    assert torch.equal(first, call.DW.bits()) and (fdb is None or torch.equal(fdb, call.DB.bits())), f"{tag}: a repeated launch is bit-identical"
    assert call.inputs_intact(), f"{tag}: wrote outside dw / db / the workspace, or to an input"
    label = K.WG_NAME[path] + (" gnorm" if c.gnorm else "")
    exact = c.recipe == "lattice"
    want, mag = (R.to_sd(r["dw"], c.k), R.to_sd(r["mag"], c.k)) if c.sd else (r["dw"], r["mag"])
    _judge(tag, label, "dw", "f32", dw.reshape(want.shape), want, mag, r["e32"][0], exact)
    if db is not None:
        _judge(tag, label, "db", "f32", db, r["db"], r["dbmag"], r["e32"][1], exact)


WG_NAMES = sorted({c.name for c in K.WG}, key=[c.name for c in K.WG].index)


@pytest.mark.parametrize("name", WG_NAMES)
def test_weight_gradient_against_float64(name):
    for c in K.WG:
        if c.name == name:
            _run_wgrad(c)


# ------------------------------------------------------------------------------------------ out_conv backward in one pass
@pytest.mark.parametrize("cin,cout,pair,recipe", K.OUT_BWD, ids=[f"{a}_{b}-{p[0]}.{p[1]}-{r}" for a, b, p, r in K.OUT_BWD])
def test_out_bwd_against_float64_and_the_two_kernel_route(cin, cout, pair, recipe):
    lib = _lib().load()
    d = K.out_bwd_inputs(cin, cout, recipe)
    NV, sh = K.OUT_BWD_NV, (1, 1, 1, K.OUT_BWD_NV)
    tag = f"out_bwd {cin}->{cout} {pair} {recipe}"
    X, G = _lay(sh + (cin,), pair[0], None, d["x"]), _lay(sh + (cout,), pair[1], None, d["g"])
    GX = _lay(sh + (cin,), pair[0], None, None, output=True)
    Wt, DW, DB, A = Flat(0, data=d["w"]), Flat(cin * cout), Flat(cout), Flat(1, 0.0)
    need = int(lib.tem_conv1x1_out_bwd_ws(cin, cout))
    WS = Flat(need // 4 + 4)

    def launch():
        rc = lib.tem_conv1x1_out_bwd_st(X.ptr(), X.Wd, G.ptr(), G.Wd, Wt.ptr(), GX.ptr(), GX.Wd, DW.ptr(), DB.ptr(), WS.ptr(), need, NV, cin,
                                        cout, A.ptr(), ST[pair[0]], ST[pair[1]], _stream())
        torch.cuda.synchronize()
        return rc
    assert launch() == 0, f"{tag}: {lib.tem_last_error()}"
    first, got = GX.bits(), GX.host()
    dwb, dbb, dw, db = DW.bits(), DB.bits(), DW.host(), DB.host()
    w = int(A.bits().item()) & 0xFFFFFFFF
    assert R.amax_ok(w, got, pair[0]), f"{tag}: out_amax {w:#x} is not max |gx| = {np.abs(got).max()}"
    A.body.view(torch.int32).fill_(BIG)
    for t in (DW, DB, WS):
        t.body.fill_(NAN)
    GX.view.fill_(NAN)
    assert launch() == 0
    assert torch.equal(first, GX.bits()) and torch.equal(dwb, DW.bits()) and torch.equal(dbb, DB.bits()), f"{tag}: a repeated launch is bit-identical"
    assert int(A.bits().item()) == BIG and A.intact(), f"{tag}: a larger out_amax stays"
    assert _holds(X, d["x"]) and _holds(G, d["g"]) and all(t.intact() for t in (Wt, DW, DB, WS, GX)), f"{tag}: inputs and surroundings"
    exact = recipe == "lattice"
    gx, mag = R.out_bwd_f64(d["x"], d["g"], d["w"])
    e32 = 0.0 if exact else max(R.units(R.out_bwd_f32(d["x"], d["g"], d["w"], f), gx, mag + 1e-300) for f in (False, True))
    assert np.isfinite(got).all()
    if exact:
        _judge(tag, "out_bwd", "gx", pair[0], got, gx, mag, e32, True)
    else:                                                          # (the scale is 0 where the mask is: those elements must be 0)
        assert np.all(got[mag == 0] == 0)
        _judge(tag, "out_bwd", "gx", pair[0], np.where(mag == 0, 0.0, got), gx, np.where(mag == 0, 1.0, mag), e32, False)
    rdw, rdb, rmag, rdbmag = R.wgrad_f64(d["x"], d["g"], K.K111)
    e32w = (0.0, 0.0) if exact else R.wgrad_e32(d["x"], d["g"], K.K111, rdw, rdb, rmag, rdbmag)
    _judge(tag, "out_bwd", "dw", "f32", dw.reshape(cout, cin, 1), R.to_sd(rdw, K.K111), R.to_sd(rmag, K.K111), e32w[0], exact)
    _judge(tag, "out_bwd", "db", "f32", db, rdb, rdbmag, e32w[1], exact)
    # the two-kernel route: tem_conv3d_wgrad (the projection's weight-gradient kernel) on the same tensors
    c = K.Wg("two_kernel", K.WG_PROJ, sh, cin, cout, K.K111, pair, sd=1)
    call = WgCall(c, {"x": d["x"], "g": d["g"]})
    assert call.query() == K.WG_PROJ and call.launch() == 0
    diff = int((call.DW.bits() != dwb).sum()) + int((call.DB.bits() != dbb).sum())
    print(f"CONV_VALU_BITS {tag}: {diff} of {dwb.numel() + dbb.numel()} elements of dw / db differ from the two-kernel route")
    assert diff == 0 and call.inputs_intact()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_return_an_error_and_write_nothing():
    lib = _lib().load()
    # a statistics request on a path without rows (the generic kernel), with a buffer of the size the first-layer kernel would fill
    c = K.Fwd("refuse_stat", -1, (2, 5, 9, 11), 5, 8, K.K333, stat=True)
    call = FwdCall(c, K.fwd_inputs(c))
    assert call.nblk > 0 and call.query()[0] == -1
    rc = call.launch()
    print(f"CONV_VALU_REFUSAL statistics on the generic kernel: rc {rc}")
    assert rc != 0 and call.untouched()
    # the storage pair f16 / bf16 (buffers of the larger type's size are never needed: the launch is refused before any access;
    # laid out as fp16 both)
    c = K.Fwd("refuse_pair", -1, (2, 5, 9, 11), 1, 8, K.K333, pair=("f16", "f16"))
    call = FwdCall(c, K.fwd_inputs(c))
    c.pair = ("f16", "bf16")
    assert call.query()[0] == -1
    rc = call.launch()
    print(f"CONV_VALU_REFUSAL forward f16 / bf16: rc {rc}")
    assert rc != 0
    c.pair = ("f16", "f16")
    assert call.untouched()
    # weight gradient: gcoef on a plan that is not cin1; a workspace that is too small; f16 / bf16; misaligned gnx / gcoef
    g = K.Wg("refuse_gcoef", -1, (2, 5, 9, 11), 5, 8, K.K333, gnorm=True)
    for what, c, kw, pair in (("gcoef on the generic plan", g, {}, None),
                              ("a workspace that is too small", K.Wg("refuse_ws", -1, (2, 5, 9, 11), 1, 8, K.K333), dict(ws_bytes=1024), None),
                              ("f16 / bf16", K.Wg("refuse_pair", -1, (2, 5, 9, 11), 1, 8, K.K333, pair=("f16", "f16")), {}, ("f16", "bf16")),
                              ("gnx off its 16-byte rows", K.Wg("refuse_gnx", -1, (2, 5, 9, 11), 1, 8, K.K333, gnorm=True), dict(ylay=(10, 1)), None),
                              ("gcoef off 16 bytes", K.Wg("refuse_coef", -1, (2, 5, 9, 11), 1, 8, K.K333, gnorm=True), dict(coef_off=1), None)):
        call = WgCall(c, K.wg_inputs(c), **kw)
        if pair:
            c.pair = pair
        assert call.query() == -1, what
        if pair:
            c.pair = ("f16", "f16")
        rc = call.launch(pair)
        print(f"CONV_VALU_REFUSAL wgrad {what}: rc {rc}")
        assert rc != 0 and call.untouched(), f"wgrad {what}: rc {rc}"
    lib.tem_last_error()
