"""Float64 references of the matrix-core forward / data-gradient convolution kernels (csrc/conv_zr.hip, conv_pp.hip,
conv_bf16x3.hip, conv_mfma.hip, conv1x1_stream.hip and the split-K epilogues: use_mfma 1 .. 7), op by op (TEST INFRASTRUCTURE,
see oracle/__init__.py).

Written from the formulas of include/tem_hip.h (tem_conv3d_fwd: the modes; tem_conv3d_fwd_stats, _refnorm, _gscaled) and the
comments of csrc/conv_split.h; plain numpy, no code shared with the kernels, no torch.  conv_ref.py's conv_f64 / shifted / taps /
block_stats_f64 and the judge of oracle/judge.py are reused unchanged.

THE OPERAND MODEL.  A mode says which 16-bit (or fp32) numbers the matrix cores multiply.  planes(v, mode, operand) returns those
numbers as float64 arrays, TERMS[mode] the pairs (plane of x, plane of w, accumulator) the mode keeps.  The float64 sum of exactly
these products is the reference: what is left to the kernel is fp32 accumulation.
  xhat     ONE fp32 fma of x, scale, shift before the zero padding (xhat32), then the mode's split
  mode 1   the fp32 values
  5 / 7    round16 to fp16 / bf16 (16-bit storage: x already is that value)
  mode 2   hi = bf16(v), lo = bf16(v - hi); hi hi + hi lo + lo hi
  mode 3   three bf16 planes, p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1); the six terms with i + j <= 2
  mode 4   hi = fp16(v), lo' = fp16((v - hi) 2^12); accumulator 0: hi hi, accumulator 1: hi lo' + lo' hi, joined by ONE fp32 fma
           with 2^-12: y = float32(acc0 + 2^-12 acc1) where both accumulators are exact
  mode 6   x 2^5 clamped to +-2000 x 2^5 and w 2^7 clamped to +-500 x 2^7, split in fp16 (lo unscaled), three terms in one
           accumulator, the result times 2^-12
The bias is added after the accumulation, then the activation, the ref > 0 mask and the rounding of a 16-bit store.
The data gradient (dgrad_model) is stated on its own: gx[u][ci] = sum_tap sum_co g[u - o(tap)][co] W[co][ci][tap] -- the taps
flipped and the channels swapped with respect to the forward -- not the forward helper on a transposed array.

All tensors are channels-last [N, D, H, W, C]; weights come in the state_dict order w_sd[Cout][Cin][taps], tap = (tz kh + ty) kw + tx.
"""
import numpy as np

from . import conv_ref as R
from . import judge as J

f32 = np.float32
NONE, RELU, SIGMOID = R.NONE, R.RELU, R.SIGMOID
FP32, BF16X3, BF16X6, F16X3, F16, F16X3S, BF16 = 1, 2, 3, 4, 5, 6, 7          # TEM_ARITH_*
LO12 = 4096.0                                                                # conv_split.h: F16_LO_SCALE
A_PRE, W_PRE, PRE_INV = 32.0, 128.0, 1.0 / 4096.0                            # F16_A_PRESCALE, F16_W_PRESCALE, F16_PRESCALE_INV
A_CLAMP, W_CLAMP = 2000.0, 500.0
# (plane of x, plane of w, accumulator)
TERMS = {FP32: [(0, 0, 0)], F16: [(0, 0, 0)], BF16: [(0, 0, 0)],
         BF16X3: [(0, 0, 0), (0, 1, 0), (1, 0, 0)],
         BF16X6: [(i, j, 0) for i in range(3) for j in range(3) if i + j <= 2],
         F16X3: [(0, 0, 0), (0, 1, 1), (1, 0, 1)],
         F16X3S: [(0, 0, 0), (0, 1, 0), (1, 0, 0)]}
ACC_SCALE = {F16X3: (1.0, 1.0 / LO12)}                                       # what an accumulator is multiplied by when they are joined
OUT_SCALE = {F16X3S: PRE_INV}


def _r32(v):
    return np.asarray(v, np.float64).astype(f32).astype(np.float64)


def xhat32(x, scale, shift):
    """ONE fp32 fma per element, as float64 values: the exact product (48 bits) plus the shift, rounded once"""
    x = np.asarray(x, np.float64)
    if scale is None:
        return x
    s, t = (np.asarray(v, np.float64)[:, None, None, None, :] for v in (scale, shift))
    return _r32(x * s + t)


def planes(v, mode, operand):
    """the numbers the matrix cores multiply for one operand (operand: "x" | "w"), float64 arrays; v holds float32 values"""
    v = np.asarray(v, np.float64)
    if mode == FP32:
        return [v]
    if mode in (F16, BF16):
        return [J.round16(v, "f16" if mode == F16 else "bf16")]
    if mode in (BF16X3, BF16X6):
        out, rest = [], v
        for _ in range(2 if mode == BF16X3 else 3):
            p = J.round16(rest, "bf16")
            out.append(p)
            rest = _r32(rest - p)                       # (exact: a float32 minus its own rounding)
        return out
    if mode == F16X3:
        hi = J.round16(v, "f16")
        return [hi, J.round16(_r32(_r32(v - hi) * LO12), "f16")]
    if mode == F16X3S:
        pre, lim = (A_PRE, A_CLAMP * A_PRE) if operand == "x" else (W_PRE, W_CLAMP * W_PRE)
        s = np.clip(_r32(v * pre), -lim, lim)
        hi = J.round16(s, "f16")
        return [hi, J.round16(_r32(s - hi), "f16")]
    raise ValueError(mode)


def reproduces(v, mode, operand="x"):
    """the planes of the mode's split add up to v exactly (lattice and split recipes)"""
    p = planes(v, mode, operand)
    if mode == F16X3:
        return bool(np.array_equal(p[0] + p[1] / LO12, np.asarray(v, np.float64)))
    if mode == F16X3S:
        return bool(np.array_equal((p[0] + p[1]) / (A_PRE if operand == "x" else W_PRE), np.asarray(v, np.float64)))
    return bool(np.array_equal(sum(p), np.asarray(v, np.float64)))


def generic(w_sd):
    """w_sd [Cout][Cin][taps] -> the generic pack [tap][ci][co] of the forward"""
    return np.ascontiguousarray(np.transpose(np.asarray(w_sd, np.float64), (2, 1, 0)))


# ------------------------------------------------------------------------------------------------------- accumulation
def _dgrad_lin(g, w_sd, k):
    """sum over (tap, co) of g[u - o(tap)][co] W[co][ci][tap] and of the absolute values, [N, D, H, W, Cin]"""
    g, w = np.asarray(g, np.float64), np.asarray(w_sd, np.float64)
    lin = np.zeros(g.shape[:4] + (w.shape[1],))
    mag = np.zeros_like(lin)
    l2, m2 = lin.reshape(-1, w.shape[1]), mag.reshape(-1, w.shape[1])
    for tap, dz, dy, dx in R.taps(k):
        gs = R.shifted(g, -dz, -dy, -dx).reshape(-1, w.shape[0])
        wt = np.ascontiguousarray(w[:, :, tap])                      # (a contiguous 2-D product is 20 times faster in numpy)
        l2 += gs @ wt
        m2 += np.abs(gs) @ np.abs(wt)
    return lin, mag


def _lin_only(xi, wj, k, dgrad):
    """the sum of one term without its scale (half the work: the exact judgements need no scale)"""
    out = np.zeros(xi.shape[:4] + (wj.shape[1] if dgrad else wj.shape[0],))
    o2 = out.reshape(-1, out.shape[-1])
    for tap, dz, dy, dx in R.taps(k):
        if dgrad:
            o2 += R.shifted(xi, -dz, -dy, -dx).reshape(-1, wj.shape[0]) @ np.ascontiguousarray(wj[:, :, tap])
        else:
            o2 += R.shifted(xi, dz, dy, dx).reshape(-1, wj.shape[1]) @ np.ascontiguousarray(wj[:, :, tap].T)
    return out


def accumulate(xh, w_sd, k, mode, dgrad=False, skip=None, want_mag=True):
    """-> (acc [n_acc] float64 arrays of the exact sums per accumulator, mag: sum |terms| in output units, amag [n_acc]: sum |terms|
    per accumulator in ITS units; want_mag False: zeros).  xh: the operand tensor after the pre-norm (dgrad: the incoming
    gradient); w_sd: state_dict order.  skip(i, j, px, pw) -> (px, pw): a hook for the planted errors of the CPU suite.  A term
    with an all-zero plane (the lo planes of a lattice) is skipped: it adds exact zeros."""
    px, pw = planes(xh, mode, "x"), planes(w_sd, mode, "w")
    nacc = 1 + max(a for _, _, a in TERMS[mode])
    acc, amag = [0.0] * nacc, [0.0] * nacc
    for i, j, a in TERMS[mode]:
        xi, wj = px[i], pw[j]
        if skip is not None:
            xi, wj = skip(i, j, xi, wj)
        if not xi.any() or not wj.any():
            lin = m = np.zeros(xi.shape[:4] + (wj.shape[1] if dgrad else wj.shape[0],))
        elif not want_mag:
            lin, m = _lin_only(xi, wj, k, dgrad), 0.0
        else:
            lin, m = _dgrad_lin(xi, wj, k) if dgrad else R.conv_f64(xi, generic(wj), k)
        acc[a], amag[a] = acc[a] + lin, amag[a] + m
    sc = ACC_SCALE.get(mode, (1.0,) * nacc)
    out = OUT_SCALE.get(mode, 1.0)
    mag = sum(m * s for m, s in zip(amag, sc)) * out
    return acc, mag, amag


def term_bound(xh, w_sd, mode, dgrad=False):
    """an upper bound of sum |terms| per accumulator, in its units, without the convolution: every |x plane| at its maximum
    against the largest column sum of |w plane| over (tap, summed channel)"""
    px, pw = planes(xh, mode, "x"), planes(w_sd, mode, "w")
    out = [0.0] * (1 + max(a for _, _, a in TERMS[mode]))
    for i, j, a in TERMS[mode]:
        out[a] += float(np.abs(px[i]).max()) * float(np.abs(pw[j]).sum(axis=(0, 2) if dgrad else (1, 2)).max())
    return out


def abs_sums32(xh, w_sd, k, mode, dgrad=False):
    """sum |terms| per accumulator in its units, as float32 matrix products of the absolute planes: for the bound of a lattice,
    where three digits are enough and float64 would cost four times the time"""
    px, pw = planes(xh, mode, "x"), planes(w_sd, mode, "w")
    out = [0.0] * (1 + max(a for _, _, a in TERMS[mode]))
    for i, j, a in TERMS[mode]:
        out[a] = out[a] + _lin_only(np.abs(px[i]).astype(f32), np.abs(pw[j]).astype(f32), k, dgrad)
    return out


def join(acc, mode):
    """the exact value of the joined accumulators"""
    sc = ACC_SCALE.get(mode, (1.0,) * len(acc))
    return sum(a * s for a, s in zip(acc, sc)) * OUT_SCALE.get(mode, 1.0)


def gscale(amax):
    """tem_conv3d_fwd_gscaled: the power of two that puts max |x| into [2^14, 2^15) (1 for an all-zero tensor)"""
    if not amax > 0:
        return 1.0
    _, e = np.frexp(float(amax))                         # amax in [2^(e-1), 2^e)
    return float(np.ldexp(1.0, 15 - e))


def fwd_model(x, w_sd, k, mode, bias=None, scale=None, shift=None, act=NONE, ref=None, dgrad=False, coef=None, in_amax=None, skip=None,
              want_mag=True, pre=None):
    """-> dict: y (float64, before the rounding of a 16-bit store), mag (the judge's per-element scale: sum |terms| + |bias|),
    lin (before activation and mask), amag (per accumulator).  coef [N, Cout, 4] = (a, m1, m2r, mean): the refnorm epilogue;
    in_amax: max |x| of the gscaled launch (mode 4).  pre: accumulate()'s result for these operands, computed before (the tests
    share it among the epilogues of one layer; a reference shared among tests is not changed)."""
    xh = xhat32(x, scale, shift)
    p = 1.0
    if in_amax is not None:
        assert mode == F16X3 and bias is None and scale is None
        p = gscale(in_amax)
        xh = xh * p                                      # (a power of two: exact)
    acc, mag, amag = pre if pre is not None else accumulate(xh, w_sd, k, mode, dgrad, skip, want_mag)
    lin, mag = join(acc, mode) / p, mag / p
    if bias is not None:
        b = np.asarray(bias, np.float64)
        lin, mag = lin + b, mag + np.abs(b)
    if coef is not None:
        assert ref is not None and act == NONE
        r = np.asarray(ref, np.float64)
        a, m1, m2r, mean = R._coef(coef)
        y = np.where(r > 0.0, a * lin - m1 - (r - mean) * m2r, 0.0)
        mag = np.where(r > 0.0, np.abs(a) * mag + np.abs(m1) + (np.abs(r) + np.abs(mean)) * np.abs(m2r), 0.0)
        return {"y": y, "mag": mag, "lin": lin, "amag": amag}
    if act == RELU:
        y = np.maximum(lin, 0.0)
    elif act == SIGMOID:
        y = R.sigmoid64(lin)
        mag = y * (1.0 - y) * (mag + 1.0) + y
    else:
        y = lin
    if ref is not None:
        y = np.where(np.asarray(ref, np.float64) > 0.0, y, 0.0)
    return {"y": y, "mag": mag, "lin": lin, "amag": amag}


# ------------------------------------------------------------------------------------------------------- the fp32 yardstick
def model_e32(x, w_sd, k, mode, y, mag, bias=None, scale=None, shift=None, act=NONE, ref=None, dgrad=False, sample=None):
    """e32: a numpy float32 restatement ON THE MODELLED TERMS -- bias first, then one chain over (tap, ci, term), products once
    rounded separately and once contracted; the worse of the two against y, in units.  A yardstick, not a check of elements:
    `sample` (an index array into the flattened voxels) evaluates it on a fixed subset of the voxels."""
    xh = xhat32(x, scale, shift)
    px, pw = planes(xh, mode, "x"), planes(w_sd, mode, "w")
    sc = ACC_SCALE.get(mode, (1.0, 1.0))
    out = OUT_SCALE.get(mode, 1.0)
    nv = int(np.prod(y.shape[:4]))
    idx = np.arange(nv) if sample is None else np.asarray(sample)
    yy, mm = y.reshape(nv, -1)[idx], mag.reshape(nv, -1)[idx]
    rr = None if ref is None else np.asarray(ref, np.float64).reshape(nv, -1)[idx]
    worst = 0.0
    for fused in (False, True):
        acc = np.zeros(yy.shape, f32)
        if bias is not None:
            acc = acc + np.asarray(bias, f32)
        for tap, dz, dy, dx in R.taps(k):
            for i, j, a in TERMS[mode]:
                if dgrad:
                    xs = R.shifted(px[i], -dz, -dy, -dx).reshape(nv, -1)[idx].astype(f32)
                    wt = (pw[j][:, :, tap] * sc[a] * out).astype(f32)                      # [co][ci]: rows are the summed channel
                else:
                    xs = R.shifted(px[i], dz, dy, dx).reshape(nv, -1)[idx].astype(f32)
                    wt = (pw[j][:, :, tap].T * sc[a] * out).astype(f32)                    # [ci][co]
                for c in range(wt.shape[0]):
                    acc = R._fma32(xs[:, c:c + 1], wt[c][None, :], acc, fused)
        if act == RELU:
            acc = np.maximum(acc, f32(0))
        elif act == SIGMOID:
            acc = R.sigmoid32(acc)
        if rr is not None:
            acc = np.where(rr > 0, acc, f32(0))
        worst = max(worst, R.units(acc, yy, mm))
    return worst


# ------------------------------------------------------------------------------------------------------- statistics rows
def total_stats_f64(y):
    """per (n, channel): (sum y, sum y^2) of the tensor as stored and their scales (sum |y|, sum y^2), [N][C][2]"""
    y = np.asarray(y, np.float64)
    s1, s2, sa = y.sum(axis=(1, 2, 3)), (y * y).sum(axis=(1, 2, 3)), np.abs(y).sum(axis=(1, 2, 3))
    return np.stack([s1, s2], axis=-1), np.stack([sa, s2], axis=-1)


def linear_stats_f64(y, vb):
    """the rows of the split-K epilogue: blocks of vb consecutive voxels of a sample, [N][ceil(V / vb)][C][2], and their scales"""
    y = np.asarray(y, np.float64)
    N, C = y.shape[0], y.shape[-1]
    v = y.reshape(N, -1, C)
    nb = -(-v.shape[1] // vb)
    p = np.zeros((N, nb * vb, C))
    p[:, :v.shape[1]] = v
    p = p.reshape(N, nb, vb, C)
    s1, s2, sa = p.sum(axis=2), (p * p).sum(axis=2), np.abs(p).sum(axis=2)
    return np.stack([s1, s2], axis=-1), np.stack([sa, s2], axis=-1)


def linear_stats_e32(y, vb, rows, scales):
    """conv_ref.block_stats_e32 for the rows of linear_stats_f64: float32 sums in sequence over the vb voxels of a row, squares
    rounded separately and contracted; the worse of the two, per quantity"""
    y = np.asarray(y).astype(f32)
    N, C = y.shape[0], y.shape[-1]
    v = y.reshape(N, -1, C)
    nb = -(-v.shape[1] // vb)
    p = np.zeros((N, nb * vb, C), f32)
    p[:, :v.shape[1]] = v
    p = p.reshape(N, nb, vb, C)
    s1, s2a, s2b = (np.zeros((N, nb, C), f32) for _ in range(3))
    for i in range(vb):
        e = p[:, :, i]
        s1 = s1 + e
        s2a = s2a + e * e
        s2b = (s2b.astype(np.float64) + e.astype(np.float64) * e.astype(np.float64)).astype(f32)
    return (R.units(s1, rows[..., 0], scales[..., 0]),
            max(R.units(s2a, rows[..., 1], scales[..., 1]), R.units(s2b, rows[..., 1], scales[..., 1])))


def _blocks(a, vb):
    """[N, D, H, W, C] -> [N, ceil(V / vb), vb, C], zero padded"""
    N, C = a.shape[0], a.shape[-1]
    v = a.reshape(N, -1, C)
    nb = -(-v.shape[1] // vb)
    p = np.zeros((N, nb * vb, C), a.dtype)
    p[:, :v.shape[1]] = v
    return p.reshape(N, nb, vb, C)


def bwd_sums_f64(g, xin, mean, rstd, vb):
    """TEM_BP_NORM_SUMS of a split-K data gradient (tem_hip.h): per block of vb consecutive voxels and channel the rows
    (sum g, sum g xn) of the gradient AS STORED, xn = (xin - mean) rstd of the norm the gradient lands behind, mean / rstd
    [N][G] with C / G consecutive channels per group.  -> (rows, scales) [N][blocks][C][2], scales (sum |g|, sum |g xn|)"""
    g, xin = np.asarray(g, np.float64), np.asarray(xin, np.float64)
    C = g.shape[-1]
    rep = C // np.asarray(mean).shape[1]
    mu, rs = (np.repeat(np.asarray(v, np.float64), rep, axis=1)[:, None, None, None, :] for v in (mean, rstd))
    t = g * ((xin - mu) * rs)
    bg, bt = _blocks(g, vb), _blocks(t, vb)
    return (np.stack([bg.sum(axis=2), bt.sum(axis=2)], axis=-1), np.stack([np.abs(bg).sum(axis=2), np.abs(bt).sum(axis=2)], axis=-1))


def bwd_sums_e32(g, xin, mean, rstd, vb, rows, scales):
    """the float32 restatement: xn = (xin - mean) rstd with one rounding per operation, then chains over the voxels of a
    block, the product g xn rounded separately and contracted; the worse of the two, per quantity"""
    g32, x32 = np.asarray(g).astype(f32), np.asarray(xin).astype(f32)
    rep = g32.shape[-1] // np.asarray(mean).shape[1]
    mu, rs = (np.repeat(np.asarray(v, f32), rep, axis=1)[:, None, None, None, :] for v in (mean, rstd))
    xn = ((x32 - mu).astype(f32) * rs).astype(f32)
    bg, bx = _blocks(g32, vb), _blocks(xn, vb)
    s0, s1a, s1b = (np.zeros(bg.shape[:2] + bg.shape[3:], f32) for _ in range(3))
    for i in range(vb):
        s0 = s0 + bg[:, :, i]
        s1a = R._fma32(bg[:, :, i], bx[:, :, i], s1a, False)
        s1b = R._fma32(bg[:, :, i], bx[:, :, i], s1b, True)
    return (R.units(s0, rows[..., 0], scales[..., 0]),
            max(R.units(s1a, rows[..., 1], scales[..., 1]), R.units(s1b, rows[..., 1], scales[..., 1])))


# ------------------------------------------------------------------------------------------------------- the judge
U, MARGIN = J.U, J.MARGIN
round16, stored = J.round16, J.stored
band, within = J.band, J.within
interval16, outside16, excess16 = J.interval16, J.outside16, J.excess16
mismatches = J.mismatches
units, amax_ok, lattice_bound = R.units, R.amax_ok, R.lattice_bound


def exact_store(r, mode, dt):
    """what a kernel that accumulates exactly stores: the joined value rounded to fp32 once (mode 4: the joining fma; every other
    lattice / split case: already a float32 number), then the rounding of a 16-bit store"""
    return J.stored(_r32(r), dt)
