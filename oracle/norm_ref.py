"""Float64 references of the norm kernels (csrc/norm.hip), op by op (TEST INFRASTRUCTURE, see oracle/__init__.py).

Written from the formulas of include/tem_hip.h (tem_norm_stats / _finalize_partials / _finalize_partials2 / tem_norm_bwd /
_coef / _st) and the comments of csrc/norm.hip; plain numpy, no code shared with the kernels, no torch.
tests/test_norm_cpu.py pins the float64 functions to torch float64 group_norm and its autograd, checks every band formula
below by perturbing the inputs of the float64 formula to the band ends, and tests the judge on deliberately wrong
results; tests/test_gpu_norm.py judges the kernels with them.

Tensors are LOGICAL numpy arrays [N, V, C]; per-channel results [N, C(, k)], per-group results [N, G]; cg = C / G,
cnt = V cg.  Partial rows are [N, nblk, C, 2].

float64
  channel_sums_f64(x)                 [N, C, 2] = (sum x, sum x^2);  channel_sums_scale: (sum |x|, sum x^2)
  bwd_sums_f64(g, x, mean, rstd)      [N, C, 2] = (sum g, sum g xn), xn = (x - mean) rstd of the channel's group, for the
                                      float32-valued mean / rstd the kernel receives;  bwd_sums_scale: (sum |g|, sum |g xn|)
  stats_f64(sums, V, G, ...)          mean = s / cnt, var = max(ss / cnt - mean^2, 0), rstd = 1 / sqrt(var + eps) per group,
                                      scale = rstd gamma, shift = beta - mean rstd gamma per channel
  rows_f64(part) / concat_rows_f64    the float64 sum over partial rows; the concat form: channels [0, CA) from one set of
                                      rows, [CA, C) from another
  coef_f64(bsums, V, G, gamma, ...)   [N, C, 4] = (a, m1, m2r, mean): a = rstd gamma, m1 = rstd S1 / cnt, m2r = rstd^2 S2 / cnt
                                      with S1 = sum_{c in group} gamma_c sum g, S2 = sum_{c in group} gamma_c sum g xn
  affine_grads_f64(bsums)             dgamma[c] = sum_n sum g xn, dbeta[c] = sum_n sum g
  apply_f64(g, x, coef, relu_mask)    gx = a g - m1 - (x - mean) m2r, 0 where relu_mask and not x > 0 (so at 0.0, -0.0);
                                      apply_scale: |a g| + |m1| + |(x - mean) m2r|

float32, the yardstick e32 "plain fp32 arithmetic" (a reference, not the code under test)
  partition_sums_f32(a, pa, pb, rows, nblk, vper, fused)
                                      the partition the header of norm.hip documents -- fp32 per-thread partials -> fp32
                                      per-block partials -> fp64 merge -- with the chain lengths of the geometry query:
                                      block b owns voxels [b vper, min((b + 1) vper, V)), chain r of it adds voxels
                                      b vper + r, + rows, + 2 rows, ... in sequence (sum a; sum pa pb with the product rounded
                                      on its own, or fused = one rounding per fma), then the `rows` chains are added in
                                      sequence.  -> float32 rows [N, nblk, C, 2]; the merge over nblk is float64 (rows_f64).
                                      NOT np.sum over a strided float32 axis: that is one sequential chain over all of V.
  xn_f32                              (x - mean) rstd with two roundings
  apply_f32(g, x, coef, relu, v)      one rounding per operation; v & 1: a g - m1 as one fma, v & 2: u - d m2r as one fma.
                                      The compiler is free to contract: e32 of the apply is the worse of v = 0 and v = 3.

The judge: errors in units of 2^-23 x a per-quantity scale (units / within / band / MARGIN of oracle/judge.py, no absolute
allowance); every element within MARGIN max(e32, 1) units.  Scales:
  sum x: sum |x|      sum x^2: its value      sum g: sum |g|      sum g xn: sum |g xn|
  mean: sum |x| / cnt                          var as computed (ss / cnt - m^2): E[x^2] + 2 |m| E|x|
Derived quantities get the first-order propagation of the bands dm, dv, dS0, dS1 (ABSOLUTE half-widths, band(e32) x scale)
of what they are built from, plus one rounding to float32, RND |value| with RND = 2^-24 (1 + 2^-20):
  rstd    the closed interval [f32(1 / sqrt(var + dv + eps)), f32(1 / sqrt(max(var - dv, 0) + eps))]: the map is
          monotone, so this is exact, like the 16-bit rule;  dr = the larger distance of an UNROUNDED end from rstd
  scale   |gamma| dr + RND |scale|
  shift   |rstd gamma| dm + |mean gamma| dr + RND |shift|
  a       RND |a|                       (rstd and gamma are given: one exact product, one rounding)
  m1      rstd / cnt sum_{c in group} |gamma_c| dS0_c + RND |m1|
  m2r     rstd^2 / cnt sum_{c in group} |gamma_c| dS1_c + RND |m2r|
  mean    0                             (coef[3] is the given float32 mean, bit for bit)
  dbeta   sum_n dS0 + RND |dbeta|;  dgamma  sum_n dS1 + RND |dgamma|
  gx end to end   band(e32 apply) x apply_scale + |g| da + dm1 + |x - mean| dm2r   (the bands of a, m1, m2r above, their
          rounding included: the coef the kernel applies is the rounded one)
  16-bit gx: the closed interval [round16(ref - B), round16(ref + B)] of the same absolute band B.
"""
import numpy as np

from . import judge as J

f32 = np.float32
RND = 2.0 ** -24 * (1.0 + 2.0 ** -20)
# oracle/judge.py under the names the tests use; no absolute allowance
MARGIN = J.MARGIN
round16, round_common16 = J.round16, J.round_common16
units, band, within = J.units, J.band, J.within
outside_interval, outside16_abs = J.outside_interval, J.outside16_abs


def _nvc(a, dtype=np.float64):
    a = np.asarray(a, dtype)
    assert a.ndim == 3, "logical [N, V, C]"
    return a


def group_sum(a, G):
    """[N, C] -> [N, G]"""
    a = np.asarray(a)
    return a.reshape(a.shape[0], G, a.shape[1] // G).sum(axis=2)


def per_channel(a, C):
    """[N, G] -> [N, C]"""
    a = np.asarray(a)
    return np.repeat(a, C // a.shape[1], axis=1)


def _vec(v, C, fill):
    return np.full(C, fill, np.float64) if v is None else np.asarray(v, np.float64).reshape(C)


# ------------------------------------------------------------------------------------------------------- float64
def channel_sums_f64(x):
    x = _nvc(x)
    return np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=-1)


def channel_sums_scale(x):
    x = _nvc(x)
    return np.stack([np.abs(x).sum(axis=1), (x * x).sum(axis=1)], axis=-1)


def xn_f64(x, mean, rstd):
    x = _nvc(x)
    C = x.shape[2]
    m, r = per_channel(np.asarray(mean, np.float64), C), per_channel(np.asarray(rstd, np.float64), C)
    return (x - m[:, None, :]) * r[:, None, :]


def bwd_sums_f64(g, x, mean, rstd):
    g, xn = _nvc(g), xn_f64(x, mean, rstd)
    return np.stack([g.sum(axis=1), (g * xn).sum(axis=1)], axis=-1)


def bwd_sums_scale(g, x, mean, rstd):
    g, xn = _nvc(g), xn_f64(x, mean, rstd)
    return np.stack([np.abs(g).sum(axis=1), np.abs(g * xn).sum(axis=1)], axis=-1)


def stats_f64(sums, V, G, gamma=None, beta=None, eps=1e-5):
    """sums [N, C, 2] -> dict(mean, var, rstd [N, G]; scale, shift [N, C])"""
    sums = np.asarray(sums, np.float64)
    N, C, _ = sums.shape
    cnt = float(V) * (C // G)
    mean = group_sum(sums[..., 0], G) / cnt
    var = np.maximum(group_sum(sums[..., 1], G) / cnt - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    ga, be = _vec(gamma, C, 1.0), _vec(beta, C, 0.0)
    scale = per_channel(rstd, C) * ga
    return {"mean": mean, "var": var, "rstd": rstd, "scale": scale, "shift": be - per_channel(mean, C) * scale}


def rows_f64(part):
    part = np.asarray(part, np.float64)
    assert part.ndim == 4 and part.shape[3] == 2, "partial rows [N, nblk, C, 2]"
    return part.sum(axis=1)


def rows_scale(part):
    """(sum over rows of |s|, sum of ss): what the rows say about sum |x| (a lower bound of it) and sum x^2"""
    part = np.asarray(part, np.float64)
    return np.stack([np.abs(part[..., 0]).sum(axis=1), part[..., 1].sum(axis=1)], axis=-1)


def concat_rows_f64(part_a, part_b, fn=rows_f64):
    return np.concatenate([fn(part_a), fn(part_b)], axis=1)


def coef_f64(bsums, V, G, gamma, mean, rstd):
    bsums = np.asarray(bsums, np.float64)
    N, C, _ = bsums.shape
    cnt = float(V) * (C // G)
    ga = _vec(gamma, C, 1.0)
    r, m = per_channel(np.asarray(rstd, np.float64), C), per_channel(np.asarray(mean, np.float64), C)
    s1 = per_channel(group_sum(bsums[..., 0] * ga, G), C)
    s2 = per_channel(group_sum(bsums[..., 1] * ga, G), C)
    return np.stack([r * ga, r * s1 / cnt, r * r * s2 / cnt, m], axis=-1)


def affine_grads_f64(bsums):
    bsums = np.asarray(bsums, np.float64)
    return bsums[..., 1].sum(axis=0), bsums[..., 0].sum(axis=0)


def _coef(coef, dtype):
    c = np.asarray(coef, dtype)
    assert c.ndim == 3 and c.shape[2] == 4, "coef [N, C, 4] = (a, m1, m2r, mean)"
    return [c[:, None, :, k] for k in range(4)]


def apply_f64(g, x, coef, relu_mask):
    g, x = _nvc(g), _nvc(x)
    a, m1, m2r, mean = _coef(coef, np.float64)
    out = a * g - m1 - (x - mean) * m2r
    return np.where(x > 0, out, 0.0) if relu_mask else out


def apply_scale(g, x, coef):
    g, x = _nvc(g), _nvc(x)
    a, m1, m2r, mean = _coef(coef, np.float64)
    return np.abs(a * g) + np.abs(m1) + np.abs((x - mean) * m2r)


# ------------------------------------------------------------------------------------------------------- float32
def xn_f32(x, mean, rstd):
    x = _nvc(x, f32)
    C = x.shape[2]
    m, r = per_channel(np.asarray(mean, f32), C), per_channel(np.asarray(rstd, f32), C)
    out = (x - m[:, None, :]) * r[:, None, :]
    assert out.dtype == f32
    return out


def partition_sums_f32(a, pa, pb, rows, nblk, vper, fused=False):
    """-> float32 rows [N, nblk, C, 2] = (sum a, sum pa pb) in the documented partition (module docstring)"""
    a, pa, pb = _nvc(a, f32), _nvc(pa, f32), _nvc(pb, f32)
    N, V, C = a.shape
    rows, nblk, vper = int(rows), int(nblk), int(vper)
    assert nblk * vper >= V and rows >= 1
    b0 = np.arange(nblk, dtype=np.int64) * vper
    b1 = np.minimum(b0 + vper, V)
    r = np.arange(rows, dtype=np.int64)
    acc0, acc1 = np.zeros((N, nblk, rows, C), f32), np.zeros((N, nblk, rows, C), f32)
    for t in range(-(-vper // rows)):
        v = b0[:, None] + r[None, :] + t * rows
        ok = (v < b1[:, None])[None, :, :, None]
        vi = np.minimum(v, V - 1)
        new0 = acc0 + a[:, vi, :]
        if fused:     # the product of two 24-bit numbers is exact in float64: the sum is rounded once (to 53, then 24 bits)
            new1 = (pa[:, vi, :].astype(np.float64) * pb[:, vi, :].astype(np.float64) + acc1.astype(np.float64)).astype(f32)
        else:
            new1 = acc1 + pa[:, vi, :] * pb[:, vi, :]
        assert new0.dtype == f32 and new1.dtype == f32
        acc0, acc1 = np.where(ok, new0, acc0), np.where(ok, new1, acc1)
    s0, s1 = np.zeros((N, nblk, C), f32), np.zeros((N, nblk, C), f32)
    for rr in range(rows):
        s0, s1 = s0 + acc0[:, :, rr, :], s1 + acc1[:, :, rr, :]
    assert s0.dtype == f32
    return np.stack([s0, s1], axis=-1)


APPLY_VARIANTS = (0, 3)       # no product contracted, both contracted


def apply_f32(g, x, coef, relu_mask, variant=0):
    g, x = _nvc(g, f32), _nvc(x, f32)
    a, m1, m2r, mean = _coef(coef, f32)
    d = x - mean
    if variant & 1:
        u = (a.astype(np.float64) * g.astype(np.float64) - m1.astype(np.float64)).astype(f32)
    else:
        u = a * g - m1
    if variant & 2:
        out = (u.astype(np.float64) - d.astype(np.float64) * m2r.astype(np.float64)).astype(f32)
    else:
        out = u - d * m2r
    assert out.dtype == f32
    return np.where(x > 0, out, f32(0)) if relu_mask else out


def apply_e32(g, x, coef, relu_mask, ref=None, scale=None):
    """the worse error of the two float32 evaluations against the float64 evaluation from the same coef"""
    ref = apply_f64(g, x, coef, relu_mask) if ref is None else ref
    scale = apply_scale(g, x, coef) if scale is None else scale
    return max(units(apply_f32(g, x, coef, relu_mask, v), ref, scale) for v in APPLY_VARIANTS)


# ------------------------------------------------------------------------------------------------------- the bands
def stats_scales(sums_scale, V, G):
    """-> (scale of mean, scale of var) [N, G] from [N, C, 2] = (sum |x|, sum x^2)"""
    sums_scale = np.asarray(sums_scale, np.float64)
    cnt = float(V) * (sums_scale.shape[1] // G)
    eabs, esq = group_sum(sums_scale[..., 0], G) / cnt, group_sum(sums_scale[..., 1], G) / cnt
    return eabs, esq, cnt


def var_scale(mean, eabs, esq):
    return esq + 2.0 * np.abs(mean) * eabs


def stats_e32(rows32, ref, sums_scale, V, G):
    """the errors of the restatement's rows (float32 [N, nblk, C, 2], merged in float64) in units: dict sum0, sum1, mean, var"""
    s = rows_f64(rows32)
    C = s.shape[1]
    eabs, esq, cnt = stats_scales(sums_scale, V, G)
    mean = group_sum(s[..., 0], G) / cnt
    var = group_sum(s[..., 1], G) / cnt - mean * mean                    # as computed, before the clamp
    ref_var = group_sum(ref["sums"][..., 1], G) / cnt - ref["mean"] ** 2
    return {"sum0": units(s[..., 0], ref["sums"][..., 0], sums_scale[..., 0]),
            "sum1": units(s[..., 1], ref["sums"][..., 1], sums_scale[..., 1]),
            "mean": units(mean, ref["mean"], eabs), "var": units(var, ref_var, var_scale(ref["mean"], eabs, esq))}


def stats_bands(ref, sums_scale, V, G, gamma=None, beta=None, eps=1e-5, e32=None):
    """ref: stats_f64's dict -> dict of the absolute bands and the rstd interval (module docstring); e32: dict mean, var"""
    e32 = e32 or {}
    C = ref["scale"].shape[1]
    eabs, esq, cnt = stats_scales(sums_scale, V, G)
    ga = np.abs(_vec(gamma, C, 1.0))
    dm = band(e32.get("mean", 0.0)) * eabs
    dv = band(e32.get("var", 0.0)) * var_scale(ref["mean"], eabs, esq)
    lo, hi = 1.0 / np.sqrt(ref["var"] + dv + eps), 1.0 / np.sqrt(np.maximum(ref["var"] - dv, 0.0) + eps)
    dr = np.maximum(hi - ref["rstd"], ref["rstd"] - lo)
    d_scale = ga * per_channel(dr, C) + RND * np.abs(ref["scale"])
    d_shift = (np.abs(ref["scale"]) * per_channel(dm, C) + np.abs(per_channel(ref["mean"], C)) * ga * per_channel(dr, C)
               + RND * np.abs(ref["shift"]))
    return {"mean_scale": eabs, "dm": dm, "dv": dv, "dr": dr, "d_scale": d_scale, "d_shift": d_shift,
            "rstd_lo": lo.astype(f32).astype(np.float64), "rstd_hi": hi.astype(f32).astype(np.float64)}


def coef_bands(coef, bscale, V, G, gamma, rstd, e32=None, rounding=True):
    """coef: coef_f64's result; bscale [N, C, 2] = (sum |g|, sum |g xn|); e32: dict sum0, sum1 -> [N, C, 4] absolute bands
    and (d dgamma, d dbeta) [C]"""
    e32 = e32 or {}
    coef, bscale = np.asarray(coef, np.float64), np.asarray(bscale, np.float64)
    N, C, _ = coef.shape
    cnt = float(V) * (C // G)
    ga = np.abs(_vec(gamma, C, 1.0))
    r = per_channel(np.asarray(rstd, np.float64), C)
    d0, d1 = band(e32.get("sum0", 0.0)) * bscale[..., 0], band(e32.get("sum1", 0.0)) * bscale[..., 1]
    rnd = RND if rounding else 0.0
    out = np.zeros_like(coef)
    out[..., 0] = rnd * np.abs(coef[..., 0])
    out[..., 1] = r / cnt * per_channel(group_sum(ga * d0, G), C) + rnd * np.abs(coef[..., 1])
    out[..., 2] = r * r / cnt * per_channel(group_sum(ga * d1, G), C) + rnd * np.abs(coef[..., 2])
    return out, d0, d1


def affine_bands(dgamma, dbeta, d0, d1):
    return d1.sum(axis=0) + RND * np.abs(dgamma), d0.sum(axis=0) + RND * np.abs(dbeta)


def gx_band(g, x, coef, dcoef, e32_apply, scale=None):
    """the absolute band of gx end to end: the apply band plus the coef bands through gx = a g - m1 - (x - mean) m2r"""
    g, x = _nvc(g), _nvc(x)
    scale = apply_scale(g, x, coef) if scale is None else scale
    a, m1, m2r, mean = _coef(coef, np.float64)
    da, dm1, dm2r, _ = _coef(dcoef, np.float64)
    return band(e32_apply) * scale + np.abs(g) * da + dm1 + np.abs(x - mean) * dm2r


# ------------------------------------------------------------------------------------------------------- the judge
def ratio_units(got, ref, scale, e32):
    """kernel units / max(e32, 1): at most MARGIN passes"""
    return units(got, ref, scale) / max(float(e32), 1.0)


def ratio_band(got, ref, d):
    """MARGIN x the worst |got - ref| / d over every element (0 / 0 = 0; a non-finite value or an error where the band is 0:
    infinite): at most MARGIN passes, the convention of ratio_units"""
    got, ref, d = (np.asarray(v, np.float64) for v in (got, ref, d))
    if got.shape != ref.shape:
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / np.broadcast_to(d, ref.shape))
    q = np.where(np.isfinite(got), q, np.inf)
    return MARGIN * float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max()) if q.size else 0.0


def judge_stats(got, ref, sums_scale, V, G, gamma=None, beta=None, eps=1e-5, e32=None):
    """got: dict mean, rstd [N, G], scale, shift [N, C] (the kernel's float32 outputs) -> dict quantity -> ratio (at most
    MARGIN passes; rstd: infinite outside its interval, else MARGIN x |error| / (dr + one rounding), for the record)"""
    e32 = e32 or {}
    b = stats_bands(ref, sums_scale, V, G, gamma, beta, eps, e32)
    out = {"mean": ratio_units(got["mean"], ref["mean"], b["mean_scale"], e32.get("mean", 0.0))}
    bad = outside_interval(got["rstd"], b["rstd_lo"], b["rstd_hi"])
    out["rstd"] = float("inf") if bad else ratio_band(got["rstd"], ref["rstd"], b["dr"] + RND * b["rstd_hi"])
    out["scale"] = ratio_band(got["scale"], ref["scale"], b["d_scale"])
    out["shift"] = ratio_band(got["shift"], ref["shift"], b["d_shift"])
    return out


def passes(ratios):
    return all(v <= MARGIN for v in ratios.values())
