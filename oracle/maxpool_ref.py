"""Float64 references of the max-pool kernels (csrc/pool_upsample.hip), op by op (TEST INFRASTRUCTURE, see oracle/__init__.py).

Written from include/tem_hip.h (tem_maxpool3d_fwd / _fwd_stats / _bwd / _bwd_norm / _st) and the comments of the kernels; plain
numpy, no code shared with the kernels, no torch.  tests/test_maxpool_cpu.py pins the float64 functions to torch float64
max_pool3d and its autograd (special values included) and makes the judge fail on planted errors; tests/test_gpu_maxpool.py
judges the kernels with them.

All tensors are channels-last numpy arrays [N, D, H, W, C]; f = (fz, fy, fx).  Window position k = (dz fy + dy) fx + dx.

float64
  pool_f64(x, f)            -> (max [N, Do, Ho, Wo, C], arg-max position k).  The first maximum wins a tie (+0.0 and -0.0 tie);
                            a NaN wins, and the LAST NaN of a window is its arg-max; a window of -inf points at position 0.
  bwd_f64(gy, x, f, gskip, relu_mask, gcoef, ycoef) -> (gx, scale):
                            A = a_s gskip - m1_s - (x - mean_s) m2r_s        (plain gskip, or 0 without it)
                            B = a_y gy - m1_y - (max - mean_y) m2r_y         (plain gy without ycoef), added at the arg-max only
                            gx = 0 where relu_mask and not x > 0
                            coef[n, c] = (a, m1, m2r, mean): the formula is norm_ref.apply_f64, its scale norm_ref.apply_scale;
                            scale = apply_scale(gskip, x, gcoef) (|gskip| without coefficients), at the arg-max plus
                            apply_scale(gy, max, ycoef) (|gy| without)
  row_stats_f64(y)          [N, Do Ho, C, 2]: (sum y, sum y^2) of every output row (n, zo, yo);  row_stats_scale: (sum |y|, sum y^2)

float32, the yardstick e32 "plain fp32 arithmetic" (a reference, not the code under test)
  bwd_f32 / bwd_e32         one rounding per operation; each fused apply in the variants 0 and 3 of norm_ref.apply_f32 (no
                            product contracted / both contracted), e32 = the worst of the combinations
  row_stats_f32 / _e32      norm_ref.partition_sums_f32 in the kernel's documented partition: block = output row, vper = Wo,
                            rows = 256 / cq chains; the worse of fused = False / True (the kernel's sum of squares is an fmaf chain)

The judge
  mismatches(got, want)     the number of elements that differ AS VALUES (+0.0 == -0.0, NaN matches NaN, a wrong shape: all)
  add_exact(gy, x, f, gskip, relu_mask, kind)   what a backward without coefficients must store: float32(gskip + gy) at the
                            arg-max, gskip (or 0) elsewhere, 0 under the mask; 16-bit: round16 of that
  units / within / band / round16 / outside16: oracle/judge.py (units of 2^-23 x scale, no absolute allowance)
  amax_ok(word, stored, kind)   fp32: the word is the bit pattern of max |gx| as stored; 16-bit: round16(word) == max |gx stored|
"""
import numpy as np

from . import judge as J
from . import norm_ref as NR

f32 = np.float32


def _a5(a, dtype=np.float64):
    a = np.asarray(a, dtype)
    assert a.ndim == 5, "channels-last [N, D, H, W, C]"
    return a


def coarse(shape, f):
    N, D, H, W, C = shape
    assert D % f[0] == 0 and H % f[1] == 0 and W % f[2] == 0, "the factor divides the shape"
    return (N, D // f[0], H // f[1], W // f[2], C)


def windows(x, f):
    """[N, D, H, W, C] -> [N, Do, Ho, Wo, C, nwin], position k = (dz fy + dy) fx + dx"""
    N, Do, Ho, Wo, C = coarse(x.shape, f)
    r = x.reshape(N, Do, f[0], Ho, f[1], Wo, f[2], C)
    return r.transpose(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, Do, Ho, Wo, C, f[0] * f[1] * f[2])


def unwindows(w, f):
    """the inverse of windows()"""
    N, Do, Ho, Wo, C, _ = w.shape
    r = w.reshape(N, Do, Ho, Wo, C, f[0], f[1], f[2]).transpose(0, 1, 5, 2, 6, 3, 7, 4)
    return r.reshape(N, Do * f[0], Ho * f[1], Wo * f[2], C)


def _nvc(a):
    return a.reshape(a.shape[0], -1, a.shape[-1])


# ------------------------------------------------------------------------------------------------------- float64
def pool_f64(x, f):
    w = windows(_a5(x), f)
    nan = np.isnan(w)
    nwin = w.shape[-1]
    first_max = np.argmax(np.where(nan, -np.inf, w), axis=-1)             # numpy: the first of equal maxima; all -inf: 0
    last_nan = nwin - 1 - np.argmax(nan[..., ::-1], axis=-1)
    am = np.where(nan.any(axis=-1), last_nan, first_max)
    return np.take_along_axis(w, am[..., None], axis=-1)[..., 0], am


def at_argmax(am, nwin, f):
    """bool [N, D, H, W, C]: the voxel is its window's arg-max"""
    return unwindows(am[..., None] == np.arange(nwin), f)


def spread(y, f):
    """a coarse tensor repeated over its windows: [N, D, H, W, C]"""
    return unwindows(np.repeat(y[..., None], f[0] * f[1] * f[2], axis=-1), f)


def bwd_f64(gy, x, f, gskip=None, relu_mask=False, gcoef=None, ycoef=None):
    gy, x = _a5(gy), _a5(x)
    assert gcoef is None or gskip is not None, "gcoef acts on gskip"
    m, am = pool_f64(x, f)
    hit = at_argmax(am, f[0] * f[1] * f[2], f)
    if gskip is None:
        A, sA = np.zeros_like(x), np.zeros_like(x)
    elif gcoef is None:
        A, sA = _a5(gskip), np.abs(_a5(gskip))
    else:
        A = NR.apply_f64(_nvc(_a5(gskip)), _nvc(x), gcoef, False).reshape(x.shape)
        sA = NR.apply_scale(_nvc(_a5(gskip)), _nvc(x), gcoef).reshape(x.shape)
    if ycoef is None:
        B, sB = gy, np.abs(gy)
    else:
        B = NR.apply_f64(_nvc(gy), _nvc(m), ycoef, False).reshape(gy.shape)
        sB = NR.apply_scale(_nvc(gy), _nvc(m), ycoef).reshape(gy.shape)
    with np.errstate(invalid="ignore"):
        out = np.where(hit, A + spread(B, f), A)
        scale = np.where(hit, sA + spread(sB, f), sA)
        if relu_mask:
            out = np.where(x > 0, out, 0.0)
    return out, scale


def row_stats_f64(y):
    y = _a5(y)
    N, Do, Ho, Wo, C = y.shape
    return np.stack([y.sum(axis=3), (y * y).sum(axis=3)], axis=-1).reshape(N, Do * Ho, C, 2)


def row_stats_scale(y):
    st = row_stats_f64(y)
    st[..., 0] = row_stats_f64(np.abs(_a5(y)))[..., 0]
    return st


# ------------------------------------------------------------------------------------------------------- float32
def bwd_f32(gy, x, f, gskip=None, relu_mask=False, gcoef=None, ycoef=None, va=0, vb=0):
    gy, x = _a5(gy, f32), _a5(x, f32)
    m, am = pool_f64(x, f)
    m = m.astype(f32)
    hit = at_argmax(am, f[0] * f[1] * f[2], f)
    if gskip is None:
        A = np.zeros_like(x)
    elif gcoef is None:
        A = _a5(gskip, f32)
    else:
        A = NR.apply_f32(_nvc(_a5(gskip, f32)), _nvc(x), gcoef, False, va).reshape(x.shape)
    B = gy if ycoef is None else NR.apply_f32(_nvc(gy), _nvc(m), ycoef, False, vb).reshape(gy.shape)
    with np.errstate(invalid="ignore"):
        out = np.where(hit, A + spread(B, f), A)
        if relu_mask:
            out = np.where(x > 0, out, f32(0))
    assert out.dtype == f32
    return out


def bwd_e32(gy, x, f, gskip, relu_mask, gcoef, ycoef, ref, scale):
    """the worst error of the float32 evaluations (each fused apply uncontracted or contracted) against float64"""
    vas = NR.APPLY_VARIANTS if gcoef is not None else (0,)
    vbs = NR.APPLY_VARIANTS if ycoef is not None else (0,)
    return max(units(bwd_f32(gy, x, f, gskip, relu_mask, gcoef, ycoef, va, vb), ref, scale) for va in vas for vb in vbs)


def row_stats_f32(y, cq, fused):
    """[N, Do Ho, C, 2] float32: thread r of the 256 / cq that share a channel group adds the row's voxels r, r + 256 / cq, ...
    in sequence, then the chains are added in sequence"""
    y = _a5(y, f32)
    N, Do, Ho, Wo, C = y.shape
    assert cq <= 256 and 256 % cq == 0, "a thread keeps its channels over its trips"
    v = _nvc(y)
    return NR.partition_sums_f32(v, v, v, 256 // cq, Do * Ho, Wo, fused=fused)


def row_stats_e32(y, cq, ref, scale):
    """[2]: per quantity the worse of the product rounded on its own and the fma chain"""
    out = [0.0, 0.0]
    for fused in (False, True):
        r32 = row_stats_f32(y, cq, fused)
        for k in (0, 1):
            out[k] = max(out[k], units(r32[..., k], ref[..., k], scale[..., k]))
    return out


# ------------------------------------------------------------------------------------------------------- the judge
# oracle/judge.py under the names the tests use; no absolute allowance; an exact quantity may be NaN, and NaN matches NaN
MARGIN = J.MARGIN
round16, round_common16 = J.round16, J.round_common16
units, band, within = J.units, J.band, J.within
outside16, excess16 = J.outside16, J.excess16


def mismatches(got, want):
    return J.mismatches(got, want, nan_equal=True)


def add_exact(gy, x, f, gskip=None, relu_mask=False, kind="f32"):
    """a backward without coefficients is one IEEE add per element: float32(gskip + gy) at the arg-max, exactly"""
    out = bwd_f32(gy, x, f, gskip, relu_mask).astype(np.float64)
    return out if kind == "f32" else round16(out, kind)


def judge_units(got, ref, scale, e32, kind):
    """-> (passes, figure): fp32: every element within MARGIN max(e32, 1) units, figure = the worst units; 16-bit: every
    stored element inside [round16(ref - band), round16(ref + band)], figure = the number outside"""
    if kind == "f32":
        ek = units(got, ref, scale)
        return within(ek, e32), ek
    bad = outside16(got, ref, scale, e32, kind)
    return bad == 0, bad


def amax_ok(word, stored, kind):
    """word: the uint32 the launch left; stored: gx as stored (float64 values)"""
    val = float(np.array([word], np.uint32).view(f32)[0])
    top = float(np.abs(np.asarray(stored, np.float64)).max())
    return val == top if kind == "f32" else float(round16(val, kind)) == top
