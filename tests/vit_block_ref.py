"""The definitions the transformer-block ops (csrc/vit_block.hip) are judged against: numpy, float64, and restated with every
operation in float32 for e32 (`dtype=np.float32`; erf there is math.erf rounded once to float32).

    LN(x) = xhat gamma + beta      xhat = (x - mean_c x) rstd      rstd = 1 / sqrt(mean_c (x - mean_c x)^2 + eps)
    layer_norm_windows   xw = partition(pad(LN(x)))                   segment_anything's window_partition; pad tokens are 0
    window_merge_norm    x1 = shortcut + crop(unpartition(y))   xn = LN(x1), from the UNROUNDED x1
    LN backward          gh = g gamma    dx = rstd (gh - mean_c gh - xhat mean_c(gh xhat))    dgamma = sum_tokens g xhat    dbeta = sum_tokens g
    bias_gelu            z = h + b   y = 0.5 z (1 + erf(z / sqrt 2))   dh = dy (Phi(z) + z phi(z))   db = sum_rows dh

Per-element scales (sums of magnitudes; the judge's units are 2^-23 x scale):
    forward (xw, xn)     |gamma| rstd (|x| + mean_c |x|) + |beta|        (xn: |x| = |shortcut| + |y|;   x1: |shortcut| + |y|)
    dx                   rstd (|gh| + mean_c |gh| + |xhat| mean_c |gh xhat|)      (dshortcut, dy: + |dx1|)
    dgamma               sum_tokens |g xhat|            dbeta   sum_tokens |g|
    GELU forward         0.5 |z| (1 + |erf|)            GELU backward   |dy| (Phi + |z| phi)            db   sum_rows of the latter
One 16-bit rounding off the reference's path: k_win_merge_ln_bwd recomputes xhat from the STORED x1 = x1 (1 + d), |d| <= 2^-p, so
xhat moves by rstd |x1| 2^-p and, to first order (`stored_x1_sensitivity`, multiplied by 2^-p in the tests),
    dshortcut, dy        rstd^2 (|x1| |mean_c(gh xhat)| + |xhat| mean_c(|gh| |x1|))            dgamma   sum_tokens |g| rstd |x1|
"""
import math

import numpy as np

_erf = np.frompyfunc(math.erf, 1, 1)


def partition(t, ws):
    """[B, H, W, C] -> [B nWh nWw, ws, ws, C], zero-padded at the bottom and the right (ws = 0: t itself)"""
    if ws == 0:
        return t
    B, H, W, C = t.shape
    ph, pw = -H % ws, -W % ws
    t = np.pad(t, ((0, 0), (0, ph), (0, pw), (0, 0)))
    return t.reshape(B, (H + ph) // ws, ws, (W + pw) // ws, ws, C).transpose(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, C)


def merge(tw, ws, B, H, W):
    if ws == 0:
        return tw
    nh, nw = -(-H // ws), -(-W // ws)
    return tw.reshape(B, nh, nw, ws, ws, -1).transpose(0, 1, 3, 2, 4, 5).reshape(B, nh * ws, nw * ws, -1)[:, :H, :W]


def pad_mask(ws, B, H, W):
    """True at the pad tokens of the window layout"""
    return partition(np.ones((B, H, W, 1)), ws)[..., 0] == 0


def _ln(x, gamma, beta, eps, dt):
    x, gamma, beta = (np.asarray(t, dt) for t in (x, gamma, beta))
    C = dt(x.shape[-1])
    d = x - x.sum(-1, keepdims=True, dtype=dt) / C
    rstd = dt(1) / np.sqrt((d * d).sum(-1, keepdims=True, dtype=dt) / C + dt(eps))
    xhat = d * rstd
    return xhat * gamma + beta, xhat, rstd


def _ln_bwd(g, xhat, rstd, gamma, dt):
    g, gamma = np.asarray(g, dt), np.asarray(gamma, dt)
    C = dt(g.shape[-1])
    gh = g * gamma
    dx = rstd * (gh - gh.sum(-1, keepdims=True, dtype=dt) / C - xhat * ((gh * xhat).sum(-1, keepdims=True, dtype=dt) / C))
    return dx, (g * xhat).sum((0, 1, 2), dtype=dt), g.sum((0, 1, 2), dtype=dt)


def layer_norm_windows(x, gamma, beta, eps, ws, dtype=np.float64):
    return partition(_ln(x, gamma, beta, eps, dtype)[0], ws)


def layer_norm_windows_bwd(g, x, gamma, eps, ws, dtype=np.float64):
    """g in window layout -> (dx, dgamma, dbeta)"""
    _, xhat, rstd = _ln(x, gamma, 0 * np.asarray(gamma), eps, dtype)
    return _ln_bwd(merge(np.asarray(g, dtype), ws, *x.shape[:3]), xhat, rstd, gamma, dtype)


def window_merge_norm(y, shortcut, gamma, beta, eps, ws, dtype=np.float64):
    x1 = np.asarray(shortcut, dtype) + merge(np.asarray(y, dtype), ws, *shortcut.shape[:3])
    return x1, _ln(x1, gamma, beta, eps, dtype)[0]


def window_merge_norm_bwd(dx1, dxn, y, shortcut, gamma, eps, ws, dtype=np.float64):
    """-> (dy in window layout, dshortcut, dgamma, dbeta)"""
    x1 = np.asarray(shortcut, dtype) + merge(np.asarray(y, dtype), ws, *shortcut.shape[:3])
    _, xhat, rstd = _ln(x1, gamma, 0 * np.asarray(gamma), eps, dtype)
    dx, dgamma, dbeta = _ln_bwd(dxn, xhat, rstd, gamma, dtype)
    t = np.asarray(dx1, dtype) + dx
    return partition(t, ws), t, dgamma, dbeta


def forward_scale(absx, gamma, beta, rstd):
    return np.abs(gamma) * rstd * (absx + absx.mean(-1, keepdims=True)) + np.abs(beta)


def ln_bwd_scales(g, x, gamma, eps):
    """-> (scale of dx, of dgamma, of dbeta) and (xhat, rstd, gh) for the callers that need more"""
    _, xhat, rstd = _ln(x, gamma, 0 * np.asarray(gamma), eps, np.float64)
    gh = np.abs(g * gamma)
    sdx = rstd * (gh + gh.mean(-1, keepdims=True) + np.abs(xhat) * (gh * np.abs(xhat)).mean(-1, keepdims=True))
    return (sdx, np.abs(g * xhat).sum((0, 1, 2)), np.abs(g).sum((0, 1, 2))), (xhat, rstd, gh)


def stored_x1_sensitivity(dxn, x1, gamma, eps):
    """d(dshortcut) and d(dgamma) per unit of relative change of x1 inside xhat (module docstring)"""
    _, xhat, rstd = _ln(x1, gamma, 0 * np.asarray(gamma), eps, np.float64)
    gh = dxn * gamma
    a = rstd ** 2 * (np.abs(x1) * np.abs((gh * xhat).mean(-1, keepdims=True)) + np.abs(xhat) * (np.abs(gh) * np.abs(x1)).mean(-1, keepdims=True))
    return a, (np.abs(dxn) * rstd * np.abs(x1)).sum((0, 1, 2))


def _gelu_parts(h, b, dt):
    z = np.asarray(h, dt) + np.asarray(b, dt)
    erf = _erf(z * dt(math.sqrt(0.5))).astype(dt)
    return z, erf, np.exp(dt(-0.5) * z * z) * dt(1 / math.sqrt(2 * math.pi))


def bias_gelu(h, b, dtype=np.float64):
    z, erf, _ = _gelu_parts(h, b, dtype)
    return dtype(0.5) * z * (dtype(1) + erf)


def bias_gelu_bwd(dy, h, b, dtype=np.float64):
    z, erf, phi = _gelu_parts(h, b, dtype)
    dh = np.asarray(dy, dtype) * (dtype(0.5) * (dtype(1) + erf) + z * phi)
    return dh, dh.sum(0, dtype=dtype)


def gelu_scales(dy, h, b):
    """-> (forward, dh, db)"""
    z, erf, phi = _gelu_parts(h, b, np.float64)
    sdh = np.abs(dy) * (0.5 * (1 + erf) + np.abs(z) * phi)
    return 0.5 * np.abs(z) * (1 + np.abs(erf)), sdh, sdh.sum(0)
