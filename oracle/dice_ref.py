"""Float64 references of the Dice kernels (csrc/dice.hip), op by op (TEST INFRASTRUCTURE, see oracle/__init__.py).

Written from the formulas of include/tem_hip.h (tem_dice_sums / _finalize / _grad and their *2 forms) and of the reference's
loss/dice.py; no code is shared with the kernels.  tests/test_dice_cpu.py pins the float64 functions to torch float64
autograd and to the reference-made fixtures; tests/test_gpu_dice.py judges the kernels with them.

All tensors are LOGICAL numpy arrays [N, C, V] (any trailing shape is flattened), whatever layout the kernel reads.

  dice_sums_f64      -> [C, 3 | 4]: sum p t, sum p^2, sum t^2 (p, t multiplied by the mask first; p = sigmoid(x) under
                        LOGITS) and, under BCE, the summed binary cross entropy of the UNMASKED prediction
  dice_finalize_f64  -> (out, ca, cb): the score / loss and the coefficients of d out / d p = ca t + cb p
  dice_grad_f64      -> the gradient for the float32-valued ca / cb / gout / weights the kernel receives (one-step error)
  *_f32              the same three in numpy float32 with one rounding per operation: the yardstick "plain fp32
                     arithmetic" of the tests, a reference and not the code under test
  grad_scale, sums_units, grad_units, finalize_units, within: the judge (oracle/judge.py: units of 2^-23 x a per-quantity
                     scale, here after the absolute allowance TINY)
"""
import numpy as np

from . import judge as J

LOGITS, BCE = 1, 2                      # TEM_DICE_LOGITS, TEM_DICE_BCE
REDUCE = {None: 0, "none": 0, "sum": 1, "mean": 2, "max": 3, "min": 4}
BCE_EPS = float(np.float32(1e-12))      # aten binary_cross_entropy_backward: a float constant


def _ncv(a, dtype):
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1), dtype=dtype)      # the layout must not matter


def _per_channel(a, C, dtype):
    """None -> 1; a scalar or a 1-element array -> broadcast; [C] -> per channel: as [1, C, 1]"""
    if a is None:
        return np.ones((1, 1, 1), dtype)
    a = np.asarray(a, dtype).reshape(-1)
    assert a.size in (1, C)
    return a.reshape(1, -1, 1)


# ------------------------------------------------------------------------------------------------------- float64
def sigmoid_f64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def dice_sums_f64(p, t, mask=None, flags=0):
    x, tv = _ncv(p, np.float64), _ncv(t, np.float64)
    pv = sigmoid_f64(x) if flags & LOGITS else x
    cols = []
    if flags & BCE:
        assert mask is None, "the BCE term has no masked form"
        with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
            if flags & LOGITS:
                ce = np.maximum(x, 0.0) - x * tv + np.log1p(np.exp(-np.abs(x)))
            else:
                ce = -(tv * np.maximum(np.log(pv), -100.0) + (1.0 - tv) * np.maximum(np.log(1.0 - pv), -100.0))
        cols = [ce]
    if mask is not None:
        m = _ncv(mask, np.float64)
        pv, tv = pv * m, tv * m
    cols = [pv * tv, pv * pv, tv * tv] + cols
    return np.stack([c.sum(axis=(0, 2)) for c in cols], axis=1)


def dice_finalize_f64(sums, eps=1e-7, channelwise=True, invert=True, reduce="sum"):
    """-> (out [C] for channelwise reduce None, else [1]; ca [C]; cb [C]), float64.  score = 2 num / max(den, eps);
    cb = 0 where den < eps (the clamp's gradient); `reduce` is ignored in the flat mode, as in the reference."""
    s = np.asarray(sums, np.float64)
    C = s.shape[0]
    sgn = -1.0 if invert else 1.0
    num, den = s[:, 0], s[:, 1] + s[:, 2]
    if not channelwise:
        num, den = np.array([num.sum()]), np.array([den.sum()])
    cd = np.maximum(den, eps)
    score = 2.0 * num / cd
    val = 1.0 - score if invert else score
    ca = sgn * 2.0 / cd
    cb = np.where(den >= eps, -sgn * 4.0 * num / (cd * cd), 0.0)
    if not channelwise:
        return val, np.repeat(ca, C), np.repeat(cb, C)
    r = REDUCE[reduce]
    if r == 0:
        return val, ca, cb
    if r == 1:
        return np.array([val.sum()]), ca, cb
    if r == 2:
        return np.array([val.sum() / C]), ca / C, cb / C
    arg = int(np.argmax(val) if r == 3 else np.argmin(val))
    keep = np.arange(C) == arg
    return np.array([val[arg]]), np.where(keep, ca, 0.0), np.where(keep, cb, 0.0)


def dice_grad_f64(p, t, mask, ca, cb, gout=None, per_channel=False, flags=0, w_dice=1.0, w_bce=0.0):
    """gout (w_dice (ca t + cb p) [sigma'] + w_bce dBCEsum/dx), p and t masked first and the result masked again; every
    scalar at the float32 value the C ABI carries."""
    x, tv = _ncv(p, np.float64), _ncv(t, np.float64)
    C = x.shape[1]
    a, b = _per_channel(ca, C, np.float64), _per_channel(cb, C, np.float64)
    go = _per_channel(gout, C, np.float64)
    assert per_channel or go.size == 1
    wd, wb = float(np.float32(w_dice)), float(np.float32(w_bce))
    if not flags:
        m = 1.0 if mask is None else _ncv(mask, np.float64)
        return go * (a * (tv * m) + b * (x * m)) * m
    assert mask is None, "the logits / BCE members have no masked form"
    pv = sigmoid_f64(x) if flags & LOGITS else x
    d = wd * (a * tv + b * pv)
    if flags & LOGITS:
        d = d * (pv * sigmoid_f64(-x))
    if flags & BCE:
        d = d + wb * ((pv - tv) if flags & LOGITS else (pv - tv) / np.maximum(pv * (1.0 - pv), BCE_EPS))
    return go * d


def grad_scale(p, t, mask, ca, cb, gout=None, flags=0, w_dice=1.0, w_bce=0.0):
    """|gout| (w_dice (|ca t| + |cb p|) s + |w_bce| b) [m]: s = 1, or sigma(x) under LOGITS (not sigma (1 - sigma): one ulp of
    sigma near 1 is all of 1 - sigma, and that is the true fp32 limit there); b = sigma + |t| under LOGITS, else
    (|p| + |t|) / max(p (1 - p), 1e-12)."""
    x, tv = _ncv(p, np.float64), _ncv(t, np.float64)
    C = x.shape[1]
    a, b = _per_channel(ca, C, np.float64), _per_channel(cb, C, np.float64)
    go = np.abs(_per_channel(gout, C, np.float64))
    wd, wb = abs(float(np.float32(w_dice))), abs(float(np.float32(w_bce)))
    m = 1.0 if mask is None else _ncv(mask, np.float64)
    pv = sigmoid_f64(x) if flags & LOGITS else x * m
    tm = tv * m
    s = pv if flags & LOGITS else 1.0
    sc = wd * (np.abs(a * tm) + np.abs(b * pv)) * s
    if flags & BCE:
        bb = (pv + np.abs(tv)) if flags & LOGITS else (np.abs(pv) + np.abs(tv)) / np.maximum(pv * (1.0 - pv), BCE_EPS)
        sc = sc + wb * bb
    return go * sc * m


# ------------------------------------------------------------------------------------------------------- float32
f32 = np.float32


def sigmoid_f32(x):
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore"):
        return f32(1) / (f32(1) + np.exp(-x, dtype=f32))


def dice_sums_f32(p, t, mask=None, flags=0):
    """float32 terms (one rounding per operation), float32 sums over (n, v) in numpy's pairwise order"""
    x, tv = _ncv(p, f32), _ncv(t, f32)
    pv = sigmoid_f32(x) if flags & LOGITS else x
    cols = []
    if flags & BCE:
        assert mask is None
        with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
            if flags & LOGITS:
                ce = (np.maximum(x, f32(0)) - x * tv) + np.log1p(np.exp(-np.abs(x), dtype=f32), dtype=f32)
            else:
                ce = -(tv * np.maximum(np.log(pv, dtype=f32), f32(-100)) +
                       (f32(1) - tv) * np.maximum(np.log(f32(1) - pv, dtype=f32), f32(-100)))
        cols = [ce]
    if mask is not None:
        m = _ncv(mask, f32)
        pv, tv = pv * m, tv * m
    cols = [pv * tv, pv * pv, tv * tv] + cols
    assert all(c.dtype == f32 for c in cols)
    rows = [np.ascontiguousarray(c.transpose(1, 0, 2)).reshape(c.shape[1], -1) for c in cols]   # pairwise along a contiguous row
    return np.stack([r.sum(axis=1, dtype=f32) for r in rows], axis=1)


def dice_finalize_f32(sums, eps=1e-7, channelwise=True, invert=True, reduce="sum"):
    """dice_finalize_f64's steps on float32 values (the sums rounded first)"""
    s = np.asarray(sums).astype(f32)
    C = s.shape[0]
    sgn = f32(-1 if invert else 1)
    num, den = s[:, 0], s[:, 1] + s[:, 2]
    if not channelwise:
        num, den = np.array([num.sum(dtype=f32)]), np.array([den.sum(dtype=f32)])
    cd = np.maximum(den, f32(eps))
    score = f32(2) * num / cd
    val = f32(1) - score if invert else score
    ca = sgn * f32(2) / cd
    cb = np.where(den >= f32(eps), -sgn * f32(4) * num / (cd * cd), f32(0)).astype(f32)
    if not channelwise:
        return val, np.repeat(ca, C), np.repeat(cb, C)
    r = REDUCE[reduce]
    if r == 0:
        return val, ca, cb
    if r == 1:
        return np.array([val.sum(dtype=f32)]), ca, cb
    if r == 2:
        return np.array([val.sum(dtype=f32) / f32(C)]), ca / f32(C), cb / f32(C)
    arg = int(np.argmax(val) if r == 3 else np.argmin(val))
    keep = np.arange(C) == arg
    return np.array([val[arg]]), np.where(keep, ca, f32(0)), np.where(keep, cb, f32(0))


def dice_grad_f32(p, t, mask, ca, cb, gout=None, per_channel=False, flags=0, w_dice=1.0, w_bce=0.0):
    x, tv = _ncv(p, f32), _ncv(t, f32)
    C = x.shape[1]
    a, b = _per_channel(ca, C, f32), _per_channel(cb, C, f32)
    go = _per_channel(gout, C, f32)
    wd, wb = f32(w_dice), f32(w_bce)
    if not flags:
        if mask is None:
            return go * (a * tv + b * x)
        m = _ncv(mask, f32)
        return go * (a * (tv * m) + b * (x * m)) * m
    assert mask is None
    pv = sigmoid_f32(x) if flags & LOGITS else x
    d = wd * (a * tv + b * pv)
    if flags & LOGITS:
        d = d * (pv * (f32(1) - pv))
    if flags & BCE:
        d = d + wb * ((pv - tv) if flags & LOGITS else (pv - tv) / np.maximum(pv * (f32(1) - pv), f32(1e-12)))
    out = go * d
    assert out.dtype == f32
    return out


# ------------------------------------------------------------------------------------------------------- the judge
# oracle/judge.py under the names the tests use; the absolute allowance TINY: sigmoid(-90) is a float32 subnormal
U, TINY, MARGIN, within = J.U, J.TINY, J.MARGIN, J.within


def _units(got, ref, scale):
    """judge.units after the absolute allowance TINY"""
    return J.units(got, ref, scale, tiny=TINY)


def sums_units(got, ref):
    """per column: every term of a column is non-negative, so the column's own float64 value is its scale"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return [float("inf")] * ref.shape[1]
    return [_units(got[:, k], ref[:, k], np.abs(ref[:, k])) for k in range(ref.shape[1])]


def grad_units(got, ref, scale):
    return _units(_ncv(got, np.float64), ref, scale)


def finalize_units(got, ref):
    """the float32 rounding of the float64 result: units of 2^-23 |value|"""
    return _units(got, ref, np.abs(np.asarray(ref, np.float64)))
