"""Float64 references of the upsample kernels (csrc/pool_upsample.hip), op by op (TEST INFRASTRUCTURE, see oracle/__init__.py).

Written from the formulas of include/tem_hip.h (tem_upsample_fwd / _bwd / _bwd_norm / _fwd_stats / _stats) and of ATen's
area_pixel_compute_source_index for align_corners=False; plain numpy, no code shared with the kernels, no torch.
tests/test_upsample_cpu.py pins the float64 functions to torch float64 interpolate and its autograd and tests the judge on
deliberately wrong outputs; tests/test_gpu_upsample.py judges the kernels with them.

All tensors are channels-last numpy arrays [N, D, H, W, C]; f = (fz, fy, fx) are integer factors.

  interp_matrix(n, f)       the dense [n * f, n] matrix U of one axis: src = max((o + 0.5) / f - 0.5, 0), neighbours
                            floor(src) and min(floor(src) + 1, n - 1)
  forward_f64 / adjoint_f64 y = U_z U_y U_x x and U^T g, one matmul per axis;  ones_adjoint_f64: S = U^T 1
  bwd_norm_f64(g, u, coef)  U^T(a g - m1 - (U u - mean) m2r), coef[n, c] = (a, m1, m2r, mean) (include/tem_hip.h);
                            bwd_norm_linear_f64: the same from U^T g by linearity, for the large cases
  row_stats_f64(y, f)       [N][D*H][C][2]: sum y and sum y^2 over the fz * 2 .. fine rows that belong to coarse row (n, z, y)
  u_row_stats_f64(u, f)     [N][D*H][C][2]: sum_x S u and sum_x u (U^T U u) of coarse row (n, z, y) -- what tem_upsample_stats
                            writes per row; only its totals over the rows equal those of row_stats_f64(U u)
  *_scale                   the per-element scales of the judge (the same operators on absolute values)
  *_f32                     the same formulas in numpy float32 with one rounding per operation and float32 weights computed
                            as ATen computes them: the yardstick "plain fp32 arithmetic", a reference and not the code under test
                            (fused=True: the source index with one rounding, see _src32)
  units, within, band, interval16, outside16, excess16, round16, round_common16, FMT, MARGIN: the judge of oracle/judge.py
                            (units of 2^-23 x a per-element scale), here without an absolute allowance
"""
import numpy as np

from . import judge as J

f32 = np.float32


# ------------------------------------------------------------------------------------------------------- float64
def _src64(n, f):
    o = np.arange(n * f, dtype=np.float64)
    src = np.maximum((o + 0.5) / f - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def interp_matrix(n, f):
    i0, i1, l0, l1 = _src64(n, f)
    M = np.zeros((n * f, n), np.float64)
    rows = np.arange(n * f)
    np.add.at(M, (rows, i0), l0)
    np.add.at(M, (rows, i1), l1)
    return M


def _apply_axis(M, a, axis):
    """M along `axis` (1, 2 or 3) of a channels-last [N, D, H, W, C] array: one matmul, no transposed copy"""
    sh = a.shape
    b = a.reshape(sh[:axis] + (sh[axis], -1))
    return np.matmul(M, b).reshape(sh[:axis] + (M.shape[0],) + sh[axis + 1:])


def _a5(a):
    a = np.asarray(a, np.float64)
    assert a.ndim == 5, "channels-last [N, D, H, W, C]"
    return a


def forward_f64(x, f):
    x = _a5(x)
    for axis in (3, 2, 1):                                  # x, then y, then z
        x = _apply_axis(interp_matrix(x.shape[axis], f[axis - 1]), x, axis)
    return x


def adjoint_f64(g, f):
    g = _a5(g)
    for axis in (3, 2, 1):
        n = g.shape[axis] // f[axis - 1]
        assert n * f[axis - 1] == g.shape[axis], "the fine shape is the coarse shape times the factor"
        g = _apply_axis(interp_matrix(n, f[axis - 1]).T, g, axis)
    return g


def ones_adjoint_f64(shape, f):
    """S = U^T 1 as [1, D, H, W, 1] for a coarse shape [N, D, H, W, C]"""
    s = [interp_matrix(shape[a], f[a - 1]).sum(axis=0) for a in (1, 2, 3)]
    return (s[0][:, None, None] * s[1][None, :, None] * s[2][None, None, :])[None, ..., None]


def _coef(coef, dtype):
    c = np.asarray(coef, dtype)
    assert c.ndim == 3 and c.shape[2] == 4, "coef [N, C, 4] = (a, m1, m2r, mean)"
    return [c[:, None, None, None, :, k] for k in range(4)]


def bwd_norm_f64(g, u, coef, f):
    g, u = _a5(g), _a5(u)
    a, m1, m2r, mean = _coef(coef, np.float64)
    return adjoint_f64(a * g - m1 - (forward_f64(u, f) - mean) * m2r, f)


def gram_f64(u, f):
    """U^T U u without the fine tensor: the [n, n] matrix U^T U of each axis on the coarse array (equal to
    adjoint_f64(forward_f64(u)) up to float64 rounding; tests/test_upsample_cpu.py holds the two together)"""
    u = _a5(u)
    for axis in (3, 2, 1):
        M = interp_matrix(u.shape[axis], f[axis - 1])
        u = _apply_axis(M.T @ M, u, axis)
    return u


def bwd_norm_linear_f64(adj, u, coef, f):
    """bwd_norm_f64 by linearity from adj = U^T g: a adj - m1 S - m2r (U^T U u - mean S); differs from the definition by
    float64 rounding only, and spares the references of the large cases two passes over the fine tensors"""
    a, m1, m2r, mean = _coef(coef, np.float64)
    S = ones_adjoint_f64(np.shape(u), f)
    return a * _a5(adj) - m1 * S - m2r * (gram_f64(u, f) - mean * S)


def row_stats_f64(y, f):
    y = _a5(y)
    N, Do, Ho, Wo, C = y.shape
    D, H = Do // f[0], Ho // f[1]
    r = y.reshape(N, D, f[0], H, f[1], Wo, C)
    out = np.stack([r.sum(axis=(2, 4, 5)), (r * r).sum(axis=(2, 4, 5))], axis=-1)
    return out.reshape(N, D * H, C, 2)


def u_row_stats_f64(u, f):
    u = _a5(u)
    N, D, H, W, C = u.shape
    q = adjoint_f64(forward_f64(u, f), f)
    S = ones_adjoint_f64(u.shape, f)
    return np.stack([(S * u).sum(axis=3), (u * q).sum(axis=3)], axis=-1).reshape(N, D * H, C, 2)


# ------------------------------------------------------------------------------------------------------- the scales
def forward_scale(x, f):
    return forward_f64(np.abs(_a5(x)), f)


def adjoint_scale(g, f):
    return adjoint_f64(np.abs(_a5(g)), f)


def bwd_norm_scale(g, u, coef, f, adj_scale=None):
    """|a| U^T|g| + |m1| S + |m2r| (U^T U|u| + |mean| S); adj_scale: U^T|g| where the caller has it"""
    u = _a5(u)
    a, m1, m2r, mean = (np.abs(c) for c in _coef(coef, np.float64))
    S = ones_adjoint_f64(u.shape, f)
    if adj_scale is None:
        adj_scale = adjoint_scale(g, f)
    return a * adj_scale + m1 * S + m2r * (gram_f64(np.abs(u), f) + mean * S)


def row_stats_scale(y, f):
    """sum y: sum |y|; sum y^2: the value itself (every term is non-negative)"""
    st = row_stats_f64(y, f)
    st[..., 0] = row_stats_f64(np.abs(_a5(y)), f)[..., 0]
    return st


def u_row_stats_scale(u, f):
    """sum_x S |u| and sum_x |u| (U^T U |u|): the terms u (U^T U u) may be negative"""
    return u_row_stats_f64(np.abs(_a5(u)), f)


# ------------------------------------------------------------------------------------------------------- float32
def inexact_weights(f):
    """a factor that is no power of two: 1 / f is rounded, and so is the source index"""
    return any(v & (v - 1) for v in f)


def _src32(n, f, fused=False):
    """ATen's float arithmetic: scale = 1 / f, src = scale * (o + 0.5) - 0.5 clamped at 0, l1 = src - i0, l0 = 1 - l1.
    fused: the product and the subtraction rounded once (a fused multiply-add, what a compiler that contracts makes of the
    same expression).  Both are plain fp32 arithmetic; they differ only where 1 / f is inexact, there by up to an ulp of src
    at different positions, and an ulp of src = 8.3 is 2^-20: 6 x 2^-23 of a weight of 1 / 6.  The yardstick e32 of a factor
    that is no power of two is therefore the worse of the two evaluations."""
    o = np.arange(n * f).astype(f32)
    scale = f32(1) / f32(f)
    if fused:     # the product of a 24-bit and a small number is exact in float64, and so is the difference: one rounding
        src = (np.float64(scale) * (o.astype(np.float64) + 0.5) - 0.5).astype(f32)
    else:
        src = scale * (o + f32(0.5)) - f32(0.5)
    src = np.maximum(src, f32(0))
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1) - l1
    assert l0.dtype == f32 and l1.dtype == f32
    return i0, i1, l0, l1


def _fwd_axis32(a, axis, f, fused=False):
    i0, i1, l0, l1 = _src32(a.shape[axis], f, fused)
    sh = [1] * a.ndim
    sh[axis] = -1
    out = l0.reshape(sh) * np.take(a, i0, axis) + l1.reshape(sh) * np.take(a, i1, axis)
    assert out.dtype == f32
    return out


def _adj_axis32(g, axis, f, fused=False):
    """gx[i] += w[o, i] g[o] for o ascending, one product and one sum rounded per term"""
    n = g.shape[axis] // f
    i0, i1, l0, l1 = _src32(n, f, fused)
    g = np.moveaxis(g, axis, 0)
    out = np.zeros((n,) + g.shape[1:], f32)
    for o in range(n * f):
        if i0[o] == i1[o]:
            out[i0[o]] += (l0[o] + l1[o]) * g[o]
            continue
        if l0[o] != 0:
            out[i0[o]] += l0[o] * g[o]
        if l1[o] != 0:
            out[i1[o]] += l1[o] * g[o]
    return np.moveaxis(out, 0, axis)


def forward_f32(x, f, fused=False):
    x = np.asarray(x).astype(f32)
    for axis in (3, 2, 1):
        x = _fwd_axis32(x, axis, f[axis - 1], fused)
    return x


def adjoint_f32(g, f, fused=False):
    g = np.asarray(g).astype(f32)
    for axis in (3, 2, 1):
        g = _adj_axis32(g, axis, f[axis - 1], fused)
    return g


def ones_adjoint_f32(shape, f, fused=False):
    """S = U^T 1 as [1, D, H, W, 1], summed as adjoint_f32 sums"""
    return adjoint_f32(np.ones((1, shape[1] * f[0], shape[2] * f[1], shape[3] * f[2], 1), f32), f, fused)


def bwd_norm_f32(g, u, coef, f, adj=None, fused=False):
    """a U^T g - m1 S - m2r (U^T U u - mean S), every operator and operation in float32; adj: adjoint_f32(g) where the
    caller has it"""
    u = np.asarray(u).astype(f32)
    a, m1, m2r, mean = _coef(coef, f32)
    S = ones_adjoint_f32(u.shape, f, fused)
    if adj is None:
        adj = adjoint_f32(g, f, fused)
    out = a * adj - m1 * S - m2r * (adjoint_f32(forward_f32(u, f, fused), f, fused) - mean * S)
    assert out.dtype == f32
    return out


def _seq_sum32(terms):
    """the float32 sum of `terms` (an iterable of equal-shaped float32 arrays) in sequence, one rounding per addition"""
    acc = None
    for t in terms:
        assert t.dtype == f32
        acc = t.copy() if acc is None else acc + t
    return acc


def row_stats_f32(y, f):
    """float32 sums in sequence over the fz * fy fine rows and their fine x positions: a chain at least as long as the one a
    thread of k_upsample2_fwd adds (ceil(W cq / 256) * fz * 4 terms) before its tree reduction"""
    y = np.asarray(y).astype(f32)
    N, Do, Ho, Wo, C = y.shape
    D, H = Do // f[0], Ho // f[1]
    r = y.reshape(N, D, f[0], H, f[1], Wo, C)
    rows = [r[:, :, a, :, b, x, :] for a in range(f[0]) for b in range(f[1]) for x in range(Wo)]
    out = np.stack([_seq_sum32(rows), _seq_sum32(t * t for t in rows)], axis=-1)
    return out.reshape(N, D * H, C, 2)


def u_row_stats_f32(u, f, fused=False):
    u = np.asarray(u).astype(f32)
    N, D, H, W, C = u.shape
    q = adjoint_f32(forward_f32(u, f, fused), f, fused)
    S = ones_adjoint_f32(u.shape, f, fused)
    out = np.stack([_seq_sum32((S * u)[:, :, :, x, :] for x in range(W)),
                    _seq_sum32((u * q)[:, :, :, x, :] for x in range(W))], axis=-1)
    return out.reshape(N, D * H, C, 2)


# ------------------------------------------------------------------------------------------------------- the judge
# oracle/judge.py under the names the tests use; this module takes no absolute allowance
FMT, MARGIN = J.FMT, J.MARGIN
round16, round_common16 = J.round16, J.round_common16
units, band, within = J.units, J.band, J.within
interval16, outside16, excess16 = J.interval16, J.outside16, J.excess16
