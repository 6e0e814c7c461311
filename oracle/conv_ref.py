"""Float64 references of the VALU convolution kernels (csrc/conv.hip, csrc/conv_small.hip: use_mfma 0), op by op (TEST
INFRASTRUCTURE, see oracle/__init__.py).

Written from the formulas of include/tem_hip.h (tem_conv3d_fwd, tem_conv3d_fwd_stats, tem_conv3d_wgrad, tem_conv3d_wgrad_gnorm,
tem_conv1x1_out_bwd); plain numpy, no code shared with the kernels, no torch.  tests/test_conv_valu_cpu.py pins the float64
functions to torch float64 F.conv3d and its autograd and tests the judge on planted errors; tests/test_gpu_conv_valu.py judges
the kernels with them.

All tensors are channels-last numpy arrays [N, D, H, W, C]; k = (kd, kh, kw) with every entry 1 or 3; weights are the GENERIC
pack w[tap][ci][co], tap = (tz kh + ty) kw + tx, of the correlation y[v] = sum_tap sum_ci xhat[v + tap - k // 2][ci] w[tap][ci].

  xhat64(x, scale, shift)     fma(x, scale[n, ci], shift[n, ci]) BEFORE the zero padding (the fused pre-norm); None: x
  fwd_f64(...)                -> (y, scale): act(conv + bias) masked by ref > 0; the per-element scale of the judge:
                              sum |terms| + |bias|, for a sigmoid s (1 - s) (sum |terms| + |bias| + 1) + s
  wgrad_f64(...)              -> (dw[tap][ci][co], db[co], their scales sum_v |xhat g| and sum_v |g|);  to_sd: [co][ci][tap]
  gnorm_f64(g, y, coef)       g := y > 0 ? a g - m1 - (y - mean) m2r : 0 with coef[n, co] = (a, m1, m2r, mean), and its scale
  out_bwd_f64(x, g, w_sd)     gx = x > 0 ? sum_co g w[co][ci] : 0, and its scale
  block_stats_f64(y, tile)    [N][blocks][C][2]: (sum y, sum y^2) over tiles of tile = (4, 8, tx) voxels, blocks ordered z, y, x
                              with x fastest (tem_conv3d_fwd_valu_path in include/tem_hip.h), and their scales
  *_f32, *_e32                the same formulas in numpy float32, one rounding per operation: the chain bias first, then over
                              (tap, ci) in order, each product once separately rounded and once contracted into the sum (an
                              fma: exact product, one rounding) -- the yardstick "plain fp32 arithmetic", a reference and not
                              the code under test; e32 is the worse of the two against float64, in units
  units / within / outside16 / mismatches / amax_ok    the judge: units of 2^-23 x the per-element scale after the absolute
                              allowance TINY (a sigmoid below 2^-126 is a float32 subnormal), the rule of oracle/judge.py;
                              equality as values for the lattice inputs (oracle/conv_cases.py)
"""
import numpy as np

from . import judge as J

f32 = np.float32
NONE, RELU, SIGMOID = 0, 1, 2            # TEM_ACT_*


# ------------------------------------------------------------------------------------------------------- float64
def ntaps(k):
    return k[0] * k[1] * k[2]


def taps(k):
    """[(tap, dz, dy, dx)]: the voxel offsets of the taps, tap = (tz kh + ty) kw + tx"""
    return [((tz * k[1] + ty) * k[2] + tx, tz - k[0] // 2, ty - k[1] // 2, tx - k[2] // 2)
            for tz in range(k[0]) for ty in range(k[1]) for tx in range(k[2])]


def xhat(x, scale, shift, dtype=np.float64):
    x = np.asarray(x, dtype)
    assert x.ndim == 5, "channels-last [N, D, H, W, C]"
    if scale is None:
        return x
    s, t = (np.asarray(v, dtype)[:, None, None, None, :] for v in (scale, shift))
    return x * s + t


def shifted(a, dz, dy, dx):
    """b[v] = a[v + (dz, dy, dx)], zero outside the volume"""
    N, D, H, W, C = a.shape
    b = np.zeros_like(a)
    z0, z1, y0, y1, x0, x1 = max(0, -dz), min(D, D - dz), max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if z0 < z1 and y0 < y1 and x0 < x1:
        b[:, z0:z1, y0:y1, x0:x1] = a[:, z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def conv_f64(x, w, k, scale=None, shift=None):
    """-> (sum of the terms, sum of their absolute values), [N, D, H, W, Cout]"""
    xh = xhat(x, scale, shift)
    w = np.asarray(w, np.float64)
    assert w.shape[0] == ntaps(k) and w.shape[1] == xh.shape[-1]
    lin = np.zeros(xh.shape[:4] + (w.shape[2],))
    mag = np.zeros_like(lin)
    for tap, dz, dy, dx in taps(k):
        xs = shifted(xh, dz, dy, dx)
        lin += xs @ w[tap]
        mag += np.abs(xs) @ np.abs(w[tap])
    return lin, mag


def fwd_f64(x, w, k, bias=None, scale=None, shift=None, act=NONE, ref=None):
    lin, mag = conv_f64(x, w, k, scale, shift)
    if bias is not None:
        b = np.asarray(bias, np.float64)
        lin, mag = lin + b, mag + np.abs(b)
    if act == RELU:
        y = np.maximum(lin, 0.0)
    elif act == SIGMOID:
        y = sigmoid64(lin)
        mag = y * (1.0 - y) * (mag + 1.0) + y
    else:
        y = lin
    if ref is not None:
        y = np.where(np.asarray(ref, np.float64) > 0.0, y, 0.0)
    return y, mag


def wgrad_f64(x, g, k, scale=None, shift=None):
    xh = xhat(x, scale, shift)
    g = np.asarray(g, np.float64)
    Cin, Cout = xh.shape[-1], g.shape[-1]
    dw, mag = np.zeros((ntaps(k), Cin, Cout)), np.zeros((ntaps(k), Cin, Cout))
    g2, ag2 = g.reshape(-1, Cout), np.abs(g).reshape(-1, Cout)
    for tap, dz, dy, dx in taps(k):
        xs = shifted(xh, dz, dy, dx).reshape(-1, Cin)
        dw[tap] = xs.T @ g2
        mag[tap] = np.abs(xs).T @ ag2
    return dw, g2.sum(axis=0), mag, ag2.sum(axis=0)


def to_sd(dw, k):
    """[tap][ci][co] -> the state_dict order [co][ci][kd][kh][kw]"""
    return np.ascontiguousarray(np.transpose(dw, (2, 1, 0)))


def _coef(coef, dtype=np.float64):
    c = np.asarray(coef, dtype)
    assert c.ndim == 3 and c.shape[2] == 4, "coef [N, C, 4] = (a, m1, m2r, mean)"
    return [c[:, None, None, None, :, j] for j in range(4)]


def gnorm_f64(g, y, coef):
    g, y = np.asarray(g, np.float64), np.asarray(y, np.float64)
    a, m1, m2r, mean = _coef(coef)
    keep = y > 0.0
    val = np.where(keep, a * g - m1 - (y - mean) * m2r, 0.0)
    mag = np.where(keep, np.abs(a * g) + np.abs(m1) + (np.abs(y) + np.abs(mean)) * np.abs(m2r), 0.0)
    return val, mag


def wgrad_gnorm_f64(x, g, y, coef, k, scale=None, shift=None):
    """the weight gradient of gnorm_f64(g, y, coef); scales: the products of the absolute values"""
    gn, gmag = gnorm_f64(g, y, coef)
    dw, db, _, _ = wgrad_f64(x, gn, k, scale, shift)
    ax = np.abs(xhat(x, scale, shift))
    _, _, mag, dbmag = wgrad_f64(ax, gmag, k)
    return dw, db, mag, dbmag


def out_bwd_f64(x, g, w_sd):
    """-> (gx, its scale): w_sd [Cout][Cin]"""
    x, g, w = np.asarray(x, np.float64), np.asarray(g, np.float64), np.asarray(w_sd, np.float64)
    keep = x > 0.0
    return np.where(keep, g @ w, 0.0), np.where(keep, np.abs(g) @ np.abs(w), 0.0)


def _tiles(y, tile):
    """[N, D, H, W, C] -> [N, nZ, tz, nY, ty, nX, tx, C], zero padded to whole tiles"""
    N, D, H, W, C = y.shape
    n = [-(-e // t) for e, t in zip((D, H, W), tile)]
    p = np.zeros((N, n[0] * tile[0], n[1] * tile[1], n[2] * tile[2], C), y.dtype)
    p[:, :D, :H, :W] = y
    return p.reshape(N, n[0], tile[0], n[1], tile[1], n[2], tile[2], C)


def block_stats_f64(y, tile):
    """-> (rows, scales) [N][nZ nY nX][C][2]"""
    y = np.asarray(y, np.float64)
    t = _tiles(y, tile)
    N, C = y.shape[0], y.shape[-1]
    s1, s2, sa = t.sum(axis=(2, 4, 6)), (t * t).sum(axis=(2, 4, 6)), np.abs(t).sum(axis=(2, 4, 6))
    return (np.stack([s1, s2], axis=-1).reshape(N, -1, C, 2), np.stack([sa, s2], axis=-1).reshape(N, -1, C, 2))


def block_stats_e32(y, tile, rows, scales):
    """float32 sums in sequence over the voxels of a tile (a chain far longer than a thread's), squares rounded separately
    and contracted: the worse of the two, per quantity"""
    t = _tiles(np.asarray(y).astype(f32), tile)
    N, nZ, tz, nY, ty, nX, tx, C = t.shape
    v = np.transpose(t, (0, 1, 3, 5, 7, 2, 4, 6)).reshape(N, nZ * nY * nX, C, -1)
    s1, s2a, s2b = (np.zeros(v.shape[:3], f32) for _ in range(3))
    for i in range(v.shape[-1]):
        e = v[..., i]
        s1 = s1 + e
        s2a = s2a + e * e
        s2b = (s2b.astype(np.float64) + e.astype(np.float64) * e.astype(np.float64)).astype(f32)
    return (units(s1, rows[..., 0], scales[..., 0]),
            max(units(s2a, rows[..., 1], scales[..., 1]), units(s2b, rows[..., 1], scales[..., 1])))


# ------------------------------------------------------------------------------------------------------- float32 restatements
def _fma32(a, b, c, fused):
    """a b + c in float32: the product rounded separately, or contracted (the exact product -- 48 bits, float64 holds it --
    added and rounded once, up to float64's own rounding of the sum)"""
    if fused:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    return (a * b).astype(f32) + c


def sigmoid32(v):
    v = np.asarray(v, f32)
    with np.errstate(over="ignore"):
        return (f32(1) / (f32(1) + np.exp(-v).astype(f32))).astype(f32)


def fwd_f32(x, w, k, bias=None, scale=None, shift=None, act=NONE, ref=None, fused=False):
    x = np.asarray(x, f32)
    xh = x
    if scale is not None:
        s, t = (np.asarray(v, f32)[:, None, None, None, :] for v in (scale, shift))
        xh = _fma32(x, np.broadcast_to(s, x.shape), np.broadcast_to(t, x.shape), fused)
    w = np.asarray(w, f32)
    Cin, Cout = w.shape[1], w.shape[2]
    acc = np.zeros(x.shape[:4] + (Cout,), f32)
    if bias is not None:
        acc = acc + np.asarray(bias, f32)
    for tap, dz, dy, dx in taps(k):
        xs = shifted(xh, dz, dy, dx)
        for ci in range(Cin):
            acc = _fma32(xs[..., ci:ci + 1], w[tap, ci][None, None, None, None, :], acc, fused)
    if act == RELU:
        acc = np.maximum(acc, f32(0))
    elif act == SIGMOID:
        acc = sigmoid32(acc)
    if ref is not None:
        acc = np.where(np.asarray(ref, f32) > 0, acc, f32(0))
    return acc


def fwd_e32(x, w, k, y, mag, bias=None, scale=None, shift=None, act=NONE, ref=None):
    return max(units(fwd_f32(x, w, k, bias, scale, shift, act, ref, fused), y, mag) for fused in (False, True))


def wgrad_f32(x, g, k, scale=None, shift=None, fused=False):
    """dw, db as float32 chains over the voxels in order"""
    x = np.asarray(x, f32)
    xh = x
    if scale is not None:
        s, t = (np.asarray(v, f32)[:, None, None, None, :] for v in (scale, shift))
        xh = _fma32(x, np.broadcast_to(s, x.shape), np.broadcast_to(t, x.shape), fused)
    g = np.asarray(g, f32)
    Cin, Cout = xh.shape[-1], g.shape[-1]
    g2 = g.reshape(-1, Cout)
    xs = np.stack([shifted(xh, dz, dy, dx).reshape(-1, Cin) for _, dz, dy, dx in taps(k)], axis=1)     # [NV, tap, ci]
    dw, db = np.zeros((ntaps(k), Cin, Cout), f32), np.zeros(Cout, f32)
    for v in range(g2.shape[0]):
        dw = _fma32(xs[v][:, :, None], g2[v][None, None, :], dw, fused)
        db = db + g2[v]
    return dw, db


def wgrad_e32(x, g, k, dw, db, mag, dbmag, scale=None, shift=None):
    e = [wgrad_f32(x, g, k, scale, shift, fused) for fused in (False, True)]
    return max(units(a, dw, mag) for a, _ in e), max(units(b, db, dbmag) for _, b in e)


def gnorm_f32(g, y, coef, fused=False):
    g, y = np.asarray(g, f32), np.asarray(y, f32)
    a, m1, m2r, mean = _coef(coef, f32)
    b = lambda c: np.broadcast_to(c, g.shape)                                            # noqa: E731
    t = _fma32(b(a), g, -b(m1), fused)
    val = _fma32(-(y - mean).astype(f32), b(m2r), t, fused)
    return np.where(y > 0, val, f32(0)).astype(f32)


def out_bwd_f32(x, g, w_sd, fused=False):
    x, g, w = np.asarray(x, f32), np.asarray(g, f32), np.asarray(w_sd, f32)
    acc = np.zeros(x.shape, f32)
    for co in range(w.shape[0]):
        acc = _fma32(g[..., co:co + 1], w[co][None, None, None, None, :], acc, fused)
    return np.where(x > 0, acc, f32(0))


# ------------------------------------------------------------------------------------------------------- the judge
# oracle/judge.py under the names the tests use; the absolute allowance TINY: a sigmoid below 2^-126 is a float32 subnormal
U, TINY, MARGIN = J.U, J.TINY, J.MARGIN
round16, stored = J.round16, J.stored
band, within = J.band, J.within
interval16, outside16, excess16 = J.interval16, J.outside16, J.excess16
mismatches = J.mismatches                  # a NaN, an element never written, matches nothing


def units(got, ref, scale):
    """judge.units after the absolute allowance TINY"""
    return J.units(got, ref, scale, tiny=TINY)


def amax_ok(word, gx, dt):
    """the out_amax word (bit pattern of a float32) against max |gx| of the tensor as stored"""
    got = float(np.array([word & 0xFFFFFFFF], np.uint32).view(f32)[0])
    want = float(np.abs(np.asarray(gx, np.float64)).max())
    return got == want if dt == "f32" else float(round16(got, dt)) == want


def lattice_bound(mag, step):
    """sum |terms| / step: below 2^24 every partial sum of the terms, in any order and with any contraction, is a float32
    number, so a float32 kernel returns the exact value"""
    return float(np.max(mag)) / step
