"""GPU: every max-pool kernel of csrc/pool_upsample.hip on every dispatch path, op by op through tem_maxpool3d_fwd_st /
tem_maxpool3d_bwd_st, against the float64 references of oracle/maxpool_ref.py (which tests/test_maxpool_cpu.py pins to torch
float64 max_pool3d and its autograd, and whose judge it tests on planted errors).  Cases: oracle/maxpool_cases.py.

Rules, none of them measured.
  forward            a selection: every output equals the float64 window maximum as a value (NaN where the reference has NaN),
                     fp32 and 16-bit alike.
  backward without coefficients   one IEEE add per element: the fp32 output equals float32(gskip + gy) at the arg-max and
                     gskip (or 0) elsewhere, exactly; a 16-bit output equals round16 of that.
  backward with gcoef / ycoef     errors in units of 2^-23 x scale (scale: norm_ref.apply_scale of the skip term, at the
                     arg-max plus that of the pooled term); on the same inputs e32 is the worst figure of the numpy float32
                     restatement (one rounding per operation, each fused apply uncontracted and contracted -- a reference, not
                     the code under test).  EVERY fp32 element within MARGIN * max(e32, 1) units, MARGIN of oracle/judge.py: 4;
                     every stored 16-bit element in [round16(ref - band), round16(ref + band)].
  no element is excluded: arg-max and mask are decided on exact input values (x holds half-integers times powers of two,
                     exact in every storage type), so nothing can flip.
  row partials       the same units rule per (row, channel, quantity).  A 16-bit launch is judged against the float64 sums
                     of the stored values -- which ARE the float64 maxima, by the forward rule asserted just before.  On these
                     tie-rich inputs the sums are exact in float32 (e32 = 0: MARGIN units is all a kernel gets); the cases
                     g2 / g3 run on values whose sums round (e32 up to about 2).
  out_amax           fp32: the word is the bit pattern of max |gx| as stored; 16-bit: round16(word) == max |gx stored|
                     (rounding is monotone).  A word preloaded with 0 receives the value, one preloaded with more keeps it.

Every case asserts and prints the kernel the library's own dispatch query (tem_maxpool3d_fwd_path / _bwd_path) names for
exactly the pointers, leading dimensions and options of the launch, next to the window form (unrolled: at most 8 voxels).
At the two main shapes the 16-bit outputs of the packed-word kernel (pool_vec8 = 2) and of the generic 8-channel kernel
(pool_vec8 = 1) must be equal bit for bit, in every variant.

No test provokes a device fault: the test lays every tensor out itself (oracle/gpu_kit.py: extent asserted against its
buffer, NaN in the unused channels of wide inputs, sentinel fill in those of wide outputs, outputs start as NaN, sentinels
before and after), every launch is one the library accepts or refuses with an error code, and every accepted launch is
repeated and must return the same bits.  The planted -inf / NaN / signed-zero windows are data values.

Observed on the MI355X (profiles/maxpool_op_errors.txt): worst kernel error / max(e32, 1) = 1.00 (OBSERVED_WORST_RATIO below:
the sum of squares of case g2, where kernel and restatement agree to the digit; the fused norm backwards stay at 0.97 and below),
no element of an exact quantity differs, no 16-bit element outside its interval, packed and generic 16-bit kernels equal in
every bit, the C = 2048 launch with 64 KB of dynamic LDS runs.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gpu_kit as kit
from oracle import maxpool_cases as K
from oracle import maxpool_ref as R
from oracle.gpu_kit import DEV, ST, Flat, holds_values as _holds, lay as _lay, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu
MARGIN = R.MARGIN
OBSERVED_WORST_RATIO = 1.00       # informational (profiles/maxpool_op_errors.txt); the assertions use MARGIN
BIG = 0x7F000000                  # the bit pattern of 2^127: more than any |gx| here
LEDGER = kit.Ledger("MAXPOOL_ERR")
_print_worst = LEDGER.summary_fixture()
pool_option = kit.option_fixture()            # a dispatch option ("pool_vec8") for one test


def _plant(L, data):
    """values a Laid's own exactness check cannot take (NaN is not equal to itself)"""
    L.view.copy_(torch.from_numpy(data).to(DEV))
    assert _holds(L, data), "the storage type holds the planted values"


def _label(direction, path, dt, f):
    return f"{direction} {K.PATH_NAME[path]} {'f32' if dt == 'f32' else '16'} {K.form(f)}"


def _judge(tag, label, quantity, dt, got, ref, scale, e32):
    """every element: fp32 within MARGIN * max(e32, 1) units; 16-bit inside the rounded band's closed interval"""
    kit.judge(LEDGER, R, tag, label, quantity, dt, got, ref, scale, e32)


def _judge_exact(tag, label, quantity, got, want):
    """every element equals the exact value, NaN where it has NaN (R.mismatches)"""
    kit.judge(LEDGER, R, tag, label, quantity, None, got, want, exact=True, finite=False)


# ------------------------------------------------------------------------------------------ forward
def _fwd_query(X, Y, shape, f, has_stat, dt):
    N, D, H, W, C = shape
    return _lib().load().tem_maxpool3d_fwd_path(X.ptr(), X.Wd, Y.ptr(), Y.Wd, N, D, H, W, C, f[0], f[1], f[2], int(has_stat), ST[dt])


def _fwd_launch(X, Y, shape, f, part, nblk, st):
    N, D, H, W, C = shape
    assert X.view.shape == shape and Y.view.shape == R.coarse(shape, f), "the extents the launch is told"
    rc = _lib().load().tem_maxpool3d_fwd_st(X.ptr(), X.Wd, Y.ptr(), Y.Wd, N, D, H, W, C, f[0], f[1], f[2],
                                            part.ptr() if part is not None else None, nblk, st, _stream())
    torch.cuda.synchronize()
    return rc


def _run_forward(tag, shape, f, dt, xdata, xlay, stats, want):
    """-> (path, Y, part or None); asserts the query, launches twice, asserts equal bits and intact surroundings"""
    lib = _lib().load()
    N, D, H, W, C = shape
    X = _lay(shape, dt, xlay, np.nan_to_num(xdata, nan=0.0, neginf=0.0))
    if not np.isfinite(xdata).all():
        _plant(X, xdata)
    Y = _lay(R.coarse(shape, f), dt, None, None, output=True)
    nblk = int(lib.tem_maxpool3d_fwd_stat_blocks(D, H, C, f[0], f[1]))
    assert nblk == K.stat_blocks(shape, f), "tem_maxpool3d_fwd_stat_blocks as documented"
    if stats == "none":
        assert nblk == 0 and _fwd_query(X, Y, shape, f, True, dt) == -1, f"{tag}: no row partials for C = {C}"
    part = Flat(N * nblk * C * 2) if stats == "yes" else None
    path = _fwd_query(X, Y, shape, f, part is not None, dt)
    print(f"MAXPOOL_PATH {tag}: query {path} ({K.PATH_NAME.get(path)}, {K.form(f)}), intended {want}")
    assert path == want, f"{tag}: meant for {K.PATH_NAME[want]}, the query names {K.PATH_NAME.get(path, path)}"
    assert _fwd_launch(X, Y, shape, f, part, nblk if part is not None else 0, ST[dt]) == 0, f"{tag}: the launch is accepted"
    first, pfirst = Y.bits(), None if part is None else part.bits()
    Y.view.fill_(float("nan"))
    if part is not None:
        part.body.fill_(float("nan"))
    assert _fwd_launch(X, Y, shape, f, part, nblk if part is not None else 0, ST[dt]) == 0
    assert torch.equal(first, Y.bits()), f"{tag}: a repeated launch is bit-identical"
    assert part is None or (torch.equal(pfirst, part.bits()) and part.intact()), f"{tag}: ... and so are its row partials"
    assert Y.intact(), f"{tag}: wrote outside the elements of y"
    assert _holds(X, xdata), f"{tag}: x is an input"
    return path, Y, part


FWD_CASES = [(name, dt) for name, c in K.FWD.items() for dt in c[2]]


@pytest.mark.parametrize("name,dt", FWD_CASES, ids=[f"{n}-{t}" for n, t in FWD_CASES])
def test_forward_and_row_partials_against_float64(name, dt, pool_option):
    f, shape, dtypes, want, stats, xlay, opts = K.FWD[name]
    recipe = opts.get("x", "ties")
    for key, value in opts.items():
        if key != "x":
            pool_option(key, value)
    N, D, H, W, C = shape
    d = K.inputs(shape, f, recipe)
    tag = f"fwd {name} f={f} {shape} {dt}"
    path, Y, part = _run_forward(tag, shape, f, dt, d["x"], xlay, stats, want[dt])
    label = _label("fwd", path, dt, f)
    got = Y.host()
    _judge_exact(tag, label, "maximum", got, d["y"])
    if part is not None:
        cq = K.cq_of(C, path)
        r = K.fwd_rows(shape, f, cq, recipe)              # the stored y IS the float64 y (just asserted): its sums are the reference
        pk = part.body.double().cpu().numpy().reshape(r["rows"].shape)
        for k, q in enumerate(("sum y", "sum y^2")):
            _judge(tag + f" cq={cq} trips={K.trips(shape, f, path)}", label, q, "f32", pk[..., k], r["rows"][..., k],
                   r["rows_scale"][..., k], r["rows_e32"][k])


# ------------------------------------------------------------------------------------------ backward
def _coef_tensor(coef, layout):
    """-> (tensor that owns the memory, view [N, C, 4] handed to the launch, its row stride in floats)"""
    N, C, _ = coef.shape
    if layout and layout[0] == "xs":                          # the [:, lo:] view of the concat norm's [N, Wd, 4] coefficients
        Wd, lo = layout[1], layout[2]
        full = torch.full((N, Wd, 4), float("nan"), dtype=torch.float32, device=DEV)
        full[:, lo:lo + C] = torch.from_numpy(coef).to(DEV)
        return full, full[:, lo:], Wd * 4
    t = torch.from_numpy(coef).to(DEV).contiguous()
    return t, t, 4 * C


class BwdCall:
    """the tensors of one tem_maxpool3d_bwd_st launch, laid out by the test"""

    def __init__(self, shape, f, dt, layout, xdata, d, variant):
        self.shape, self.f, self.dt, self.xdata, self.d = shape, f, dt, xdata, d
        s, self.mask, g, y = K.VARIANTS[variant]
        kind = layout[0] if layout else None
        spec = (layout[1], layout[2]) if layout else None
        self.GY = _lay(R.coarse(shape, f), dt, None, d["gy"])
        self.X = _lay(shape, dt, spec if kind == "xs" else None, np.nan_to_num(xdata, nan=0.0, neginf=0.0))
        if not np.isfinite(xdata).all():
            _plant(self.X, xdata)
        self.GS = _lay(shape, dt, spec if kind in ("xs", "gskip") else None, d["gskip"]) if s else None
        self.GX = _lay(shape, dt, spec if kind == "gx" else None, None, output=True)
        self.gc = _coef_tensor(d["gcoef"], layout) if g else None
        self.yc = torch.from_numpy(d["ycoef"]).to(DEV).contiguous() if y else None
        assert not layout or kind == "gx" or s, "the layout's tensor is part of the launch"

    def query(self):
        N, D, H, W, C = self.shape
        f, GS = self.f, self.GS
        return _lib().load().tem_maxpool3d_bwd_path(
            self.GY.ptr(), self.GY.Wd, self.X.ptr(), self.X.Wd, GS.ptr() if GS else None, GS.Wd if GS else 0, self.GX.ptr(),
            self.GX.Wd, N, D, H, W, C, f[0], f[1], f[2], int(self.gc is not None), int(self.yc is not None), ST[self.dt])

    def launch(self, amax=None, st=None, gcoef_ld=None):
        N, D, H, W, C = self.shape
        f, GS = self.f, self.GS
        assert self.X.view.shape == self.shape == self.GX.view.shape and self.GY.view.shape == R.coarse(self.shape, f)
        assert GS is None or GS.view.shape == self.shape, "the extents the launch is told"
        assert self.gc is None or self.gc[1].shape[1] >= C and self.gc[1].stride(0) == self.gc[2]
        rc = _lib().load().tem_maxpool3d_bwd_st(
            self.GY.ptr(), self.GY.Wd, self.X.ptr(), self.X.Wd, GS.ptr() if GS else None, GS.Wd if GS else 0, int(self.mask),
            self.GX.ptr(), self.GX.Wd, N, D, H, W, C, f[0], f[1], f[2],
            ctypes.c_void_p(self.gc[1].data_ptr()) if self.gc else None,
            (self.gc[2] if gcoef_ld is None else gcoef_ld) if self.gc else 0,
            ctypes.c_void_p(self.yc.data_ptr()) if self.yc is not None else None,
            amax.ptr() if amax is not None else None, ST[self.dt] if st is None else st, _stream())
        torch.cuda.synchronize()
        return rc

    def inputs_intact(self):
        d = self.d
        return (_holds(self.GY, d["gy"]) and _holds(self.X, self.xdata) and (self.GS is None or _holds(self.GS, d["gskip"]))
                and self.GX.intact())

    def untouched(self):
        return self.inputs_intact() and bool(torch.isnan(self.GX.view).all())


def _run_backward(tag, call, want, with_amax=True):
    """-> (path, gx as stored, its bits); asserts the query, launches twice (the amax word first cleared, then preloaded)"""
    path = call.query()
    print(f"MAXPOOL_PATH {tag}: query {path} ({K.PATH_NAME.get(path)}, {K.form(call.f)}), intended {want}")
    assert path == want, f"{tag}: meant for {K.PATH_NAME[want]}, the query names {K.PATH_NAME.get(path, path)}"
    word = Flat(1, 0.0) if with_amax else None
    assert call.launch(word) == 0, f"{tag}: the launch is accepted"
    first, got = call.GX.bits(), call.GX.host()
    if with_amax:
        w = int(word.bits().item()) & 0xFFFFFFFF
        assert word.intact() and R.amax_ok(w, got, call.dt), f"{tag}: out_amax {w:#x} is not max |gx| = {np.abs(got).max()}"
        word.body.view(torch.int32).fill_(BIG)
    call.GX.view.fill_(float("nan"))
    assert call.launch(word) == 0
    assert torch.equal(first, call.GX.bits()), f"{tag}: a repeated launch is bit-identical"
    assert not with_amax or (int(word.bits().item()) == BIG and word.intact()), f"{tag}: a larger out_amax stays"
    assert call.inputs_intact(), f"{tag}: wrote outside the elements of gx, or to an input"
    return path, got, first


def _bwd_cases():
    out = [(name, dt, v) for name, c in K.BWD.items() for dt in c[2] for v in c[4]]
    out.sort(key=lambda c: (K.BWD[c[0]][1], K.BWD[c[0]][0]))           # cases of one (shape, factor) share their references
    return out


BWD_CASES = _bwd_cases()


@pytest.mark.parametrize("name,dt,variant", BWD_CASES, ids=[f"{n}-{t}-{v}" for n, t, v in BWD_CASES])
def test_backward_against_float64(name, dt, variant, pool_option):
    f, shape, dtypes, want, variants, layout, opts = K.BWD[name]
    for key, value in opts.items():
        pool_option(key, value)
    d = K.inputs(shape, f)
    b = K.bwd_data(shape, f, variant)
    gskip, mask, gcoef, ycoef = K.variant_args(d, variant)
    tag = f"bwd {name} f={f} {shape} {dt} {variant}"
    call = BwdCall(shape, f, dt, layout, d["x"], d, variant)
    path, got, bits = _run_backward(tag, call, want[dt])
    label = _label("bwd", path, dt, f)
    if gcoef is None and ycoef is None:
        _judge_exact(tag, label, "gx (one add)", got, R.add_exact(d["gy"], d["x"], f, gskip, mask, dt))
    else:
        _judge(tag + f" trips={K.trips(shape, f, path)}", label, "gx (norm bwd)", dt, got, b["ref"], b["scale"], b["e32"])
    if name in K.BIT_IDENTITY and dt != "f32":
        pool_option("pool_vec8", 1)
        p1 = call.query()
        assert p1 == K.VEC8, f"{tag}: pool_vec8 = 1 names {K.PATH_NAME.get(p1, p1)}"
        call.GX.view.fill_(float("nan"))
        assert call.launch() == 0 and call.inputs_intact()
        diff = int((call.GX.bits() != bits).sum())
        print(f"MAXPOOL_BITS {tag}: {diff} of {bits.numel()} elements differ between {K.PATH_NAME[path]} and {K.PATH_NAME[p1]}")
        assert diff == 0, f"{tag}: the packed-word kernel is not bit-identical to the generic one ({diff} elements)"


# ------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_special_values(dt):
    """-inf throughout a window, one and two NaNs, an all-equal window, zeros of both signs: judged by equality, NaN positions
    included; no statistics, no amax, no coefficients"""
    f, shape = K.SPECIAL_F, K.SPECIAL_SHAPE
    x, d = K.special_x(), K.inputs(K.SPECIAL_SHAPE, K.SPECIAL_F)
    y, am = R.pool_f64(x, f)
    assert np.isnan(y).any() and np.isneginf(y).any()
    tag = f"special f={f} {shape} {dt}"
    path, Y, _ = _run_forward(tag, shape, f, dt, x, None, "no", K.P4_8[dt])
    _judge_exact(tag, _label("fwd", path, dt, f) + " special", "maximum", Y.host(), y)
    for variant in K.SPECIAL_VARIANTS:
        gskip, mask, _, _ = K.variant_args(d, variant)
        call = BwdCall(shape, f, dt, None, x, d, variant)
        path, got, _ = _run_backward(f"{tag} {variant}", call, K.P16_2[dt], with_amax=False)
        want = R.add_exact(d["gy"], x, f, gskip, mask, dt)
        assert R.mismatches(want, R.bwd_f64(d["gy"], x, f, gskip, mask)[0] if dt == "f32" else want) == 0
        _judge_exact(f"{tag} {variant}", _label("bwd", path, dt, f) + " special", "gx (one add)", got, want)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_return_an_error_and_write_nothing():
    lib = _lib().load()
    f, shape = (2, 2, 2), (1, 2, 4, 6, 8)
    d = K.inputs(shape, f)
    for dt in ("f32", "f16"):
        # forward: buffers of the full size of the shape the launch is told, so that no refusal depends on luck
        X, Y = _lay(shape, dt, None, d["x"]), _lay(shape, dt, None, None, output=True)
        part = Flat(4 * 8 * 2 * 4)

        def fwd(sh, st=ST[dt], p=None, nblk=0):
            N, D, H, W, C = sh
            rc = lib.tem_maxpool3d_fwd_st(X.ptr(), X.Wd, Y.ptr(), Y.Wd, N, D, H, W, C, 2, 2, 2, p.ptr() if p else None, nblk, st, _stream())
            torch.cuda.synchronize()
            ok = bool(torch.isnan(Y.view).all()) and Y.intact() and _holds(X, d["x"]) and bool(torch.isnan(part.body).all()) and part.intact()
            return rc, ok
        small = (1, 3, 2, 2, 8)                                # D = 3; fits the buffers: 12 voxels of 8 channels
        for what, args in {"a shape the factor does not divide": dict(sh=small), "st = 3": dict(sh=shape, st=3),
                           "stat_part with a wrong stat_blocks": dict(sh=shape, p=part, nblk=3)}.items():
            rc, ok = fwd(**args)
            print(f"MAXPOOL_REFUSAL fwd {dt} {what}: rc {rc}")
            assert rc != 0 and ok, f"fwd {dt} {what}: rc {rc}, nothing written: {ok}"
        assert lib.tem_maxpool3d_fwd_path(X.ptr(), X.Wd, Y.ptr(), Y.Wd, *small, 2, 2, 2, 0, ST[dt]) == -1
        assert lib.tem_maxpool3d_fwd_path(X.ptr(), X.Wd, Y.ptr(), Y.Wd, *shape, 2, 2, 2, 0, 3) == -1
        assert lib.tem_maxpool3d_fwd_path(X.ptr(), X.Wd, Y.ptr(), Y.Wd, *shape, 2, 2, 2, 1, ST[dt]) >= 0
        # backward
        for what, variant, kw in (("st = 3", "smb", dict(st=3)), ("gcoef_ld < 4 C", "smb", dict(gcoef_ld=4 * 8 - 4))):
            call = BwdCall(shape, f, dt, None, d["x"], d, variant)
            rc = call.launch(**kw)
            print(f"MAXPOOL_REFUSAL bwd {dt} {what}: rc {rc}")
            assert rc != 0 and call.untouched(), f"bwd {dt} {what}: rc {rc}"
        call = BwdCall(shape, f, dt, None, d["x"], d, "smg")   # gcoef without gskip
        call.GS = None
        assert call.query() == -1
        rc = call.launch()
        print(f"MAXPOOL_REFUSAL bwd {dt} gcoef without gskip: rc {rc}")
        assert rc != 0 and call.untouched()
        call = BwdCall(shape, f, dt, None, d["x"], d, "plain")  # the factor does not divide the shape the launch is told
        call.shape = small
        N, D, H, W, C = small
        assert lib.tem_maxpool3d_bwd_path(call.GY.ptr(), C, call.X.ptr(), C, None, 0, call.GX.ptr(), C, N, D, H, W, C, 2, 2, 2, 0, 0, ST[dt]) == -1
        rc = lib.tem_maxpool3d_bwd_st(call.GY.ptr(), C, call.X.ptr(), C, None, 0, 0, call.GX.ptr(), C, N, D, H, W, C, 2, 2, 2, None, 0,
                                      None, None, ST[dt], _stream())
        torch.cuda.synchronize()
        call.shape = shape
        print(f"MAXPOOL_REFUSAL bwd {dt} a shape the factor does not divide: rc {rc}")
        assert rc != 0 and call.untouched()
    # stat_part for C = 20: tem_maxpool3d_fwd_stat_blocks() is 0, no count of rows is the right one
    sh = K.FWD["c20"][1]
    N, D, H, W, C = sh
    d = K.inputs(sh, f)
    X, Y = _lay(sh, "f32", None, d["x"]), _lay(R.coarse(sh, f), "f32", None, None, output=True)
    rows = (D // 2) * (H // 2)
    part = Flat(N * rows * C * 2)
    assert lib.tem_maxpool3d_fwd_stat_blocks(D, H, C, 2, 2) == 0
    for nblk in (rows, 0):
        rc = lib.tem_maxpool3d_fwd_st(X.ptr(), X.Wd, Y.ptr(), Y.Wd, N, D, H, W, C, 2, 2, 2, part.ptr(), nblk, 0, _stream())
        torch.cuda.synchronize()
        print(f"MAXPOOL_REFUSAL fwd f32 stat_part for C = 20, stat_blocks {nblk}: rc {rc}")
        assert rc != 0 and bool(torch.isnan(Y.view).all()) and Y.intact() and bool(torch.isnan(part.body).all()) and part.intact()
    lib.tem_last_error()

