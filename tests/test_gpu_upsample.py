"""GPU: every upsample kernel of csrc/pool_upsample.hip on every dispatch path, op by op through ops.upsample_fwd /
ops.upsample_bwd / ops.upsample_stats (the `_st` entries), against the float64 references of oracle/upsample_ref.py (which
tests/test_upsample_cpu.py pins to torch float64 interpolate and its autograd, and whose judge it tests on deliberately
wrong outputs).

Rule (oracle/judge.py).  Errors are counted in units of 2^-23 times a per-element
scale -- forward U|x|, adjoint U^T|g|, fused norm backward |a| U^T|g| + |m1| S + |m2r| (U^T U|u| + |mean| S), sum y: sum |y|,
sum y^2: its own float64 value.  On the same inputs the test takes the worst figure e32 of the numpy float32 restatement
(one rounding per operation, float32 weights as ATen computes them -- a reference, not the code under test; at factor 3,
where 1 / f and the source index are rounded, the worse of its separately rounded and its fused evaluation of the source
index: the compiler contracts lin_src's `scale * (o + 0.5) - 0.5` into one fma, which moves the weights' last-bit errors to
other positions, oracle/upsample_ref.py: _src32; at factors 1 and 2 the weights are exact either way); EVERY element
of a fp32 output must stay within MARGIN * max(e32, 1) units, MARGIN of oracle/judge.py: 4.  A 16-bit kernel computes in
fp32 and rounds once on store: every stored element must lie in the closed interval [round16(ref - band), round16(ref + band)]
of the same band (rounding is monotone, so this is exact).  The row statistics of a 16-bit launch describe the tensor as
stored and are judged against the float64 sums of the stored values.

Every case asserts and prints the kernel the library's own dispatch query (tem_upsample_fwd_path / _bwd_path) names for
exactly the pointers, leading dimensions and options of the launch, so a case that drifts to another kernel fails even when
a threshold moves.  Backward cases are the smallest shapes that reach each kernel (oracle/upsample_cases.py; the pair
counts are asserted on the CPU), with odd coarse sizes: every axis has a pair without a second element.

tem_upsample_stats sums per COARSE row of u (sum_x S u, sum_x u (U^T U u)): another partition of the totals than the
per-fine-row-group sums of tem_upsample_fwd_stats.  Its rows are judged against that definition (u_row_stats_f64), and its
totals over the rows against the totals of row_stats_f64(U u), at that quantity's scales.

The 16-bit launches of b4 and b6 (the 8-channel instantiation) are also compared, bit for bit, with the rounded result of
the fp32 launch (the 4-channel instantiation) on the same values: the contract tests/test_gpu_storage16.py states.

No test provokes a device fault: the test lays every tensor out itself and asserts its extent against its buffer before a
launch, unused channels of wide buffers hold NaN on input and keep their fill on output, every tensor sits between
sentinels that must survive, and every launch is repeated and must return the same bits (there are no atomics).

Observed on the MI355X (profiles/upsample_op_errors.txt): worst kernel error / max(e32, 1) = 2.49 (OBSERVED_WORST_RATIO
below: the adjoint of the gather kernel, whose 64 taps form one fma chain; the factor-2 kernels stay at 1.00 and below), no
16-bit element outside its interval, and the 16-bit launches of b4 and b6 equal the rounded fp32 launches in every bit.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import gpu_kit as kit
from oracle import upsample_cases as K
from oracle import upsample_ref as R
from oracle.gpu_kit import DEV, ST, TORCH, lay as _lay, lib as _lib, ops as _ops

pytestmark = pytest.mark.gpu
MARGIN = R.MARGIN
OBSERVED_WORST_RATIO = 2.49       # informational (profiles/upsample_op_errors.txt); the assertions use MARGIN
LEDGER = kit.Ledger("UPSAMPLE_ERR")
_print_worst = LEDGER.summary_fixture()
upsample_option = kit.option_fixture()        # dispatch options ("upsample2_ch8", "upsample_generic") for one test


def _judge(tag, path, quantity, dt, got, ref, scale, e32):
    """every element: fp32 within MARGIN * max(e32, 1) units; 16-bit inside the rounded band's closed interval"""
    kit.judge(LEDGER, R, tag, path, quantity, dt, got, ref, scale, e32)


# ------------------------------------------------------------------------------------------ backward
def _bwd_cases():
    out = []
    for name, (f, shape, dtypes, want, layout, opts) in K.BWD.items():
        for dt in dtypes:
            for norm in (False, True):
                out.append((name, dt, norm))
    # cases of one (shape, factor, value grid) share their float64 reference: keep them together
    out.sort(key=lambda c: (K.BWD[c[0]][1], K.BWD[c[0]][0], K.grid_of(c[1])))
    return out


BWD_CASES = _bwd_cases()


def _bwd_layout(layout, which):
    if layout and layout[0] in (which, "both"):
        return layout[1], layout[2]
    return None


def _launch_bwd(name, dt, shape, f, layout, d, norm):
    """-> (path the query names, GX host float64, bits of GX); launches twice"""
    lib, ops = _lib().load(), _ops()
    N, D, H, W, C = shape
    GY = _lay(K.fine(shape, f), dt, _bwd_layout(layout, "gy"), d["g"])
    GX = _lay(shape, dt, _bwd_layout(layout, "gx"), None, output=True)
    UU = _lay(shape, dt, None, d["u"]) if norm else None
    coef = torch.from_numpy(d["coef"]).to(DEV) if norm else None
    assert GY.view.shape == K.fine(GX.view.shape, f)
    path = lib.tem_upsample_bwd_path(GY.ptr(), GY.Wd, GX.ptr(), GX.Wd, N, D, H, W, C, f[0], f[1], f[2],
                                     UU.ptr() if norm else None, UU.Wd if norm else 0, ST[dt])
    ops.upsample_bwd(GY.view, GX.view, f, norm=(UU.view, coef) if norm else None)
    torch.cuda.synchronize()
    first = GX.bits()
    GX.view.fill_(float("nan"))
    ops.upsample_bwd(GY.view, GX.view, f, norm=(UU.view, coef) if norm else None)
    torch.cuda.synchronize()
    assert torch.equal(first, GX.bits()), f"{name}: a repeated launch is bit-identical"
    assert GX.intact(), f"{name}: wrote outside the elements of gx"
    assert GY.intact() and torch.equal(GY.view.float(), torch.from_numpy(d["g"]).to(DEV)), f"{name}: gy is an input"
    assert not norm or (UU.intact() and torch.equal(UU.view.float(), torch.from_numpy(d["u"]).to(DEV))), f"{name}: u is an input"
    return path, GX.host(), first


@pytest.mark.parametrize("name,dt,norm", BWD_CASES, ids=[f"{n}-{t}-{'norm' if m else 'plain'}" for n, t, m in BWD_CASES])
def test_backward_against_float64(name, dt, norm, upsample_option):
    f, shape, dtypes, want, layout, opts = K.BWD[name]
    for key, value in opts.items():
        upsample_option(key, value)
    d = K.bwd_data(shape, f, K.grid_of(dt))
    path, got, bits = _launch_bwd(name, dt, shape, f, layout, d, norm)
    tag = f"bwd {name} f={f} {shape} {dt} {'norm' if norm else 'plain'} pairs={K.pairs(shape, f)}"
    print(f"UPSAMPLE_PATH {tag}: query {path} ({K.PATH_NAME.get(path)}), intended {want}")
    assert path == want, f"{tag}: meant for {K.PATH_NAME[want]}, the query names {K.PATH_NAME.get(path, path)}"
    q = "nrm" if norm else "adj"
    _judge(tag, f"bwd {K.PATH_NAME[path]} {'f32' if dt == 'f32' else '16'}", "bwd_norm" if norm else "adjoint", dt, got,
           d[q], d[q + "_scale"], d[q + "_e32"])
    if name in ("b4", "b6"):
        # the contract of tests/test_gpu_storage16.py between the 8-channel 16-bit instantiation and the fp32 4-channel one
        p32, got32, _ = _launch_bwd(name + "/fp32", "f32", shape, f, layout, d, norm)
        assert p32 == K.FACTOR2_CH4
        rounded = torch.from_numpy(got32).to(TORCH[dt]).contiguous().view(torch.int16)
        diff = int((rounded != bits.cpu()).sum())
        print(f"UPSAMPLE_BITS {tag}: {diff} of {rounded.numel()} elements differ from the rounded fp32 launch")
        assert diff == 0, f"{tag}: the 16-bit launch is not the rounded fp32 launch on the same values ({diff} elements)"


# ------------------------------------------------------------------------------------------ forward and statistics
FWD_CASES = [(name, dt) for name, c in K.FWD.items() for dt in c[2]]


def _stats64(rows, V, eps=1e-5):
    """mean and rstd per (sample, channel) from float64 row sums [N, R, C, 2]"""
    s = rows.sum(axis=1)
    mean = s[..., 0] / V
    var = s[..., 1] / V - mean * mean
    return mean, 1.0 / np.sqrt(var + eps)


def _check_finalize(tag, part, rows64, V, C):
    """both kinds of partials through tem_norm_finalize_partials, per channel, at the tolerance of tests/test_gpu_ops.py"""
    ops = _ops()
    N = part.shape[0]
    mean, rstd, _, _ = ops.norm_stats_from_partials(part, N, V, C, C, None, None, 1e-5)
    m64, r64 = _stats64(rows64, V)
    em, er = rel_err(mean.cpu().numpy().reshape(N, C), m64), rel_err(rstd.cpu().numpy().reshape(N, C), r64)
    print(f"UPSAMPLE_ERR {tag} finalize: mean rel_err {em:.2e} rstd rel_err {er:.2e}")
    assert em < 2e-6 and er < 2e-6, (tag, em, er)


@pytest.mark.parametrize("name,dt", FWD_CASES, ids=[f"{n}-{t}" for n, t in FWD_CASES])
def test_forward_and_statistics_against_float64(name, dt):
    lib, ops = _lib().load(), _ops()
    f, shape, dtypes, want, want_stats, ylay = K.FWD[name]
    N, D, H, W, C = shape
    d = K.fwd_data(shape, f, K.grid_of(dt))
    X = _lay(shape, dt, None, d["x"])
    Y = _lay(K.fine(shape, f), dt, ylay, None, output=True)
    stats_ok = bool(lib.tem_upsample_fwd_stats_ok(C, *f)) and ops._rows_vec4(X.view, X.Wd, Y.view, Y.Wd)
    assert stats_ok == want_stats, f"{name}: the case table says stats={want_stats}"
    path = lib.tem_upsample_fwd_path(X.ptr(), X.Wd, Y.ptr(), Y.Wd, N, D, H, W, C, f[0], f[1], f[2], int(stats_ok), ST[dt])
    tag = f"fwd {name} f={f} {shape} {dt}"
    print(f"UPSAMPLE_PATH {tag}: query {path} ({K.PATH_NAME.get(path)}), intended {want}")
    assert path == want, f"{tag}: meant for {K.PATH_NAME[want]}, the query names {K.PATH_NAME.get(path, path)}"
    part = ops.upsample_fwd(X.view, Y.view, f, stats=True)
    torch.cuda.synchronize()
    assert (part is not None) == want_stats
    first, part1 = Y.bits(), None if part is None else part.clone()
    Y.view.fill_(float("nan"))
    again = ops.upsample_fwd(X.view, Y.view, f, stats=True)
    torch.cuda.synchronize()
    assert torch.equal(first, Y.bits()), f"{tag}: a repeated launch is bit-identical"
    assert part is None or torch.equal(part1.view(torch.int32), again.view(torch.int32)), f"{tag}: ... and so are its row sums"
    assert Y.intact(), f"{tag}: wrote outside the elements of y"
    assert X.intact() and torch.equal(X.view.float(), torch.from_numpy(d["x"]).to(DEV)), f"{tag}: x is an input"
    kernel = f"fwd {K.PATH_NAME[path]} {'f32' if dt == 'f32' else '16'}"
    got = Y.host()
    _judge(tag, kernel, "forward", dt, got, d["y"], d["y_scale"], d["y_e32"])
    V = D * f[0] * H * f[1] * W * f[2]
    if part is not None:
        assert tuple(part.shape) == (N, D * H, C, 2)
        pk = part.double().cpu().numpy()
        if dt == "f32":
            rows, scale, e32 = d["rows"], d["rows_scale"], d["rows_e32"]
        else:                                               # the sums describe the tensor as stored
            rows, scale = R.row_stats_f64(got, f), R.row_stats_scale(got, f)
            r32 = R.row_stats_f32(got, f)
            e32 = [R.units(r32[..., k], rows[..., k], scale[..., k]) for k in (0, 1)]
        for k, q in enumerate(("sum y", "sum y^2")):
            _judge(tag, kernel, q, "f32", pk[..., k], rows[..., k], scale[..., k], e32[k])
    if name in K.U_STATS:
        assert part is not None
        _check_finalize(tag + " fwd partials", part, rows, V, C)
        upart = ops.upsample_stats(X.view, f)
        torch.cuda.synchronize()
        assert torch.equal(upart.view(torch.int32), ops.upsample_stats(X.view, f).view(torch.int32)), "bit-identical when repeated"
        uk = upart.double().cpu().numpy()
        ukernel = f"stats {'f32' if dt == 'f32' else '16'}"
        for k, q in enumerate(("sum y", "sum y^2")):        # per coarse row of u: the definition of tem_upsample_stats
            _judge(tag, ukernel, "u " + q, "f32", uk[..., k], d["urows"][..., k], d["urows_scale"][..., k], d["urows_e32"][k])
        tot, tot_scale = d["rows"].sum(axis=1), d["rows_scale"].sum(axis=1)
        for k, q in enumerate(("sum y", "sum y^2")):        # the totals: those of the unrounded y = U u
            e32 = R.units(d["urows_f32"].astype(np.float64).sum(axis=1)[..., k], tot[..., k], tot_scale[..., k])
            _judge(tag, ukernel, "u total " + q, "f32", uk.sum(axis=1)[..., k], tot[..., k], tot_scale[..., k], e32)
        _check_finalize(tag + " u partials", upart, d["rows"], V, C)
