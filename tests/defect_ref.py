"""Oracle of the EM defect augmentation (csrc/defect.hip, torch_em_amd/transform/defect.py): a float64 statement of each op
from explicit inputs -- plan, line endpoints, noise planes -- with the warps going through scipy's `map_coordinates(...,
output=np.float64)`, and a float32 restatement of what the kernels compute (the "f32" column of
profiles/defect_op_errors.txt).  numpy and scipy only; nothing here touches the package's kernels.
"""
import numpy as np
from scipy import ndimage as ndi

from torch_em_amd.transform import _philox
from torch_em_amd.transform import defect as D


# ---------------------------------------------------------------------------
# streaming ops: the float32 expressions of numpy, each step formed in float64 and rounded (exact for +, -, *)
# ---------------------------------------------------------------------------
def _fl(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def low_contrast(x, mean, scale):
    """fl(fl(fl(x - m) * s) + m) for the float32 mean m and the float32 scale s"""
    x, m, s = np.asarray(x, np.float32).astype(np.float64), float(np.float32(mean)), float(np.float32(scale))
    return _fl(_fl(_fl(x - m) * s) + m).astype(np.float32)


def paste(x, art, alpha):
    """fl(fl(x * fl(1 - alpha)) + fl(art * alpha))"""
    x, art, alpha = (np.asarray(v, np.float32).astype(np.float64) for v in (x, art, alpha))
    return _fl(_fl(x * _fl(1.0 - alpha)) + _fl(art * alpha)).astype(np.float32)


# ---------------------------------------------------------------------------
# noise, separable filters
# ---------------------------------------------------------------------------
def noise_plane(seed, row, shape, dtype=np.float64):
    """2u - 1, u = (w0 >> 8) * 2^-24 of stream row `row`, element r * W + c"""
    i = np.arange(shape[0] * shape[1], dtype=np.uint64)
    u = _philox.uniform_co(_philox.words(seed, row, i)[0], np.dtype(dtype).type)
    return (np.dtype(dtype).type(2) * u - np.dtype(dtype).type(1)).reshape(shape)


def smooth(plane):
    """the reference's smoothing of a flow plane, float64"""
    return ndi.gaussian_filter(np.asarray(plane, np.float64), sigma=D.SIGMA, mode="nearest", truncate=D.TRUNCATE)


def coefficients(x):
    """the cubic B-spline coefficients map_coordinates(order=3, mode="constant") interpolates, float64"""
    return ndi.spline_filter(np.asarray(x, np.float64), order=3, mode="mirror", output=np.float64)


def _index(n, radius, border):
    idx = np.arange(n)[:, None] + np.arange(-radius, radius + 1)[None, :]
    if border == "clamp":
        return np.clip(idx, 0, n - 1)
    p = 2 * (n - 1)
    idx = idx % p
    return np.where(idx >= n, p - idx, idx)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def separable(plane, weights, border, dtype=np.float64):
    """The kernels' separable filter: along W, then along H, taps in order, border "clamp" (edge repeat) or "mirror" (whole
    sample).  float64: plain sums; float32: the chain of fused multiply-adds the kernel runs, with float32 weights."""
    x = np.asarray(plane, dtype)
    w = np.asarray(weights, np.float32).astype(dtype)      # the kernels hold the weights in float32
    r = len(w) // 2
    for axis in (1, 0):
        g = np.moveaxis(np.moveaxis(x, axis, -1)[..., _index(x.shape[axis], r, border)], -1, 0)   # [taps, ..., n]
        acc = np.zeros(g.shape[1:], dtype)
        for j in range(len(w)):
            acc = _fma32(np.broadcast_to(w[j], acc.shape), g[j], acc) if dtype == np.float32 else acc + w[j] * g[j]
        x = np.moveaxis(acc, -1, axis)
    return x


def separable_scale(plane, weights, border):
    """sum |w_y| sum |w_x x|: the per-element scale of the filter's rounding error"""
    return separable(np.abs(np.asarray(plane, np.float64)), np.abs(np.asarray(weights, np.float64)), border)


# ---------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------
def warp(x, at_r, at_c, cval=0.0, coef=None):
    """scipy's cubic warp in float64: of the image x (prefiltered by scipy), or of given coefficients"""
    at = (np.asarray(at_r, np.float64).reshape(-1, 1), np.asarray(at_c, np.float64).reshape(-1, 1))
    src, pre = (np.asarray(x, np.float64), True) if coef is None else (np.asarray(coef, np.float64), False)
    return ndi.map_coordinates(src, at, output=np.float64, order=3, mode="constant", cval=cval, prefilter=pre).reshape(np.shape(at_r))


def spline_weights(t):
    """scipy's four weights of the cubic B-spline at offset t from the second coefficient, [4, ...]"""
    z = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2])


def spline_weight_slopes(t):
    """d/dt of `spline_weights`"""
    z = 1.0 - t
    return np.stack([-z * z / 2.0, (3.0 * t * t - 4.0 * t) / 2.0, -(3.0 * z * z - 4.0 * z) / 2.0, t * t / 2.0])


def hand_warp(coef, at_r, at_c, cval=0.0, out_dtype=np.float64, return_scale=False):
    """The formula the warp kernel evaluates (in float64, rounded once to out_dtype): cval outside [0, H-1] x [0, W-1], else
    the 4 x 4 sum of weights times coefficients at mirrored indices.  return_scale: also (sum |weight * coefficient|,
    sum |d weight / d r * coefficient| |r| + sum |d weight / d c * coefficient| |c|): the scales of the sum's rounding
    and of a relative error of the coordinates."""
    coef = np.asarray(coef, np.float64)
    H, W = coef.shape
    at_r, at_c = np.asarray(at_r, np.float64), np.asarray(at_c, np.float64)
    inside = (at_r >= 0) & (at_r <= H - 1) & (at_c >= 0) & (at_c <= W - 1)
    r, c = np.where(inside, at_r, 0.0), np.where(inside, at_c, 0.0)
    fr, fc = np.floor(r), np.floor(c)
    wr, wc = spline_weights(r - fr), spline_weights(c - fc)
    dr, dc = spline_weight_slopes(r - fr), spline_weight_slopes(c - fc)

    def mirror(i, n):
        p = 2 * (n - 1)
        i = i % p
        return np.where(i >= n, p - i, i)
    acc, scale, slope = np.zeros(r.shape), np.zeros(r.shape), np.zeros(r.shape)
    for j in range(4):
        rows = mirror(fr.astype(np.int64) - 1 + j, H)
        for i in range(4):
            v = coef[rows, mirror(fc.astype(np.int64) - 1 + i, W)]
            acc = acc + wr[j] * (wc[i] * v)
            scale = scale + np.abs(wr[j] * wc[i] * v)
            slope = slope + np.abs(dr[j] * wc[i] * v) * np.abs(r) + np.abs(wr[j] * dc[i] * v) * np.abs(c)
    out = np.where(inside, acc, cval).astype(out_dtype)
    return (out, np.where(inside, scale, abs(cval)), np.where(inside, slope, 0.0)) if return_scale else out


def undirected_coordinates(shape, flow_c, flow_r):
    """(rows, columns) the reference samples at: the identity plus the two smoothed planes (square slices)"""
    r, c = np.mgrid[:shape[0], :shape[1]]
    return r + np.asarray(flow_r, np.float64), c + np.asarray(flow_c, np.float64)


def compress_geometry(shape, fixed_x, ends):
    lo, hi = D.line_intervals(*D.line(*ends), shape, fixed_x)
    return D.sides(lo, hi, shape, fixed_x), D.band(lo, hi, shape, fixed_x)


def compress_coordinates(shape, fixed_x, ends, strength, noise_c, noise_r):
    """(rows, columns, band) of a compress slice: the flow is fl32(side * f + noise * (strength / 8)) per axis with the
    float32 f of `compress_flow`, as the reference's in-place float32 addition rounds it"""
    side, zero = compress_geometry(shape, fixed_x, ends)
    pos_c, pos_r = D.compress_flow(ends, strength)
    r, c = np.mgrid[:shape[0], :shape[1]]
    flow_c = _fl(side * np.float64(pos_c) + np.asarray(noise_c, np.float64) * (strength / 8.))
    flow_r = _fl(side * np.float64(pos_r) + np.asarray(noise_r, np.float64) * (strength / 8.))
    return r + flow_r, c + flow_c, zero


def near_range_end(at_r, at_c, shape, eps=1e-3):
    """pixels whose coordinate lies within eps of 0 or n - 1 on an axis: the warp jumps to cval there"""
    out = np.zeros(np.shape(at_r), bool)
    for a, n in ((np.asarray(at_r), shape[0]), (np.asarray(at_c), shape[1])):
        out |= (np.abs(a) < eps) | (np.abs(a - (n - 1)) < eps)
    return out


# ---------------------------------------------------------------------------
# a whole call from a plan and explicit noise planes
# ---------------------------------------------------------------------------
def defect_ref(x, plan, noise, strength, contrast_scale=0.1, mean_val=None, means=None, artifacts=None, smoothed=False):
    """float64 [S, H, W]: the reference's result for the plan (`transform.defect.DefectPlan`).  noise[s] = (plane of the
    column displacement, plane of the row displacement) in [-1, 1) for every deformed slice s (undirected: before the
    strength and the smoothing, unless smoothed: then the finished flow planes); means[s]: the float32 mean of a
    low-contrast slice; artifacts[k] = (artifact, alpha) by index into the source."""
    x = np.asarray(x, np.float32)
    out = x.astype(np.float64)
    for s, action in enumerate(plan.actions):
        if action == D.DROP:
            out[s] = 0
        elif action == D.LOW_CONTRAST:
            out[s] = low_contrast(x[s], means[s], contrast_scale)
        elif action == D.PASTE:
            out[s] = paste(x[s], *artifacts[plan.artifact[s]])
        elif action == D.DEFORM:
            n_c, n_r = noise[s]
            if plan.deform[s][0] == "undirected":
                f_c, f_r = (n_c, n_r) if smoothed else (smooth(np.asarray(n_c, np.float64) * strength), smooth(np.asarray(n_r, np.float64) * strength))
                at_r, at_c = undirected_coordinates(x[s].shape, f_c, f_r)
                out[s] = warp(x[s], at_r, at_c)
            else:
                _, fixed_x, ends = plan.deform[s]
                at_r, at_c, zero = compress_coordinates(x[s].shape, fixed_x, ends, strength, n_c, n_r)
                out[s] = warp(x[s], at_r, at_c, 0.0 if mean_val is None else mean_val)
                out[s][zero] = 0
    return out


class Replay:
    """Stands in for np.random.rand / randint and hands out recorded scalar draws in order"""

    def __init__(self, rand, randint):
        self.rand_, self.randint_ = list(rand), list(randint)

    def rand(self):
        return float(self.rand_.pop(0))

    def randint(self, *a, **k):
        return 0 if "dtype" in k else int(self.randint_.pop(0))   # dtype: the seed of the device fields, not a recorded draw

    def done(self):
        return not (self.rand_ or self.randint_)
