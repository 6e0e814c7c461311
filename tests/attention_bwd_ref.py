"""The gradients ops.attention's backward is judged against (numpy; float64, restated in float32 for e32), on
attention_ref.logits.  With dO the incoming gradient, L the rows' log-sum-exp:

    P = exp(S - L)    delta[i] = dO[i] . O[i]    dP = dO v^T    dS = P (dP - delta)
    dV = P^T dO       dK = scale dS^T q          dBh[i][x] = sum_{j: hj = x} dS[i][j]    dBw[i][y] = sum_{j: wj = y} dS[i][j]
    dQ[i] = scale (dS k)[i] + sum_x dBh[i][x] Rh[hi - x + H-1] + sum_y dBw[i][y] Rw[wi - y + W-1]
    dRh[r] = sum_{b, a} sum_{i, x: hi - x + H-1 = r} dBh[i][x] q[i]                      dRw likewise
"""
import numpy as np

import attention_ref as R


def _assemble(P, dS, q, k, dO, grid, scale, rel_pos, dtype):
    """(dq, dk, dv, dRh, dRw) from P and dS: the last five lines of the definition"""
    H, W = grid
    B, nH, N, D = q.shape
    sc = dtype(D ** -0.5 if scale is None else scale)
    dv = P.swapaxes(-1, -2) @ dO
    dk = sc * (dS.swapaxes(-1, -2) @ q)
    dq = sc * (dS @ k)
    if rel_pos is None:
        return dq, dk, dv, None, None
    out = [dq, dk, dv]
    d6 = dS.reshape(B, nH, N, H, W)
    tok = np.arange(N)
    for table, dB, coord, side in ((rel_pos[0], d6.sum(-1), tok // W, H), (rel_pos[1], d6.sum(-2), tok % W, W)):
        table = np.asarray(table, dtype)
        rows = coord[:, None] - np.arange(side)[None, :] + side - 1                      # [N, side]: the table row of (i, x)
        out[0] = out[0] + np.einsum("baix,ixc->baic", dB, table[rows])
        dT = np.zeros_like(table)
        np.add.at(dT, rows, np.einsum("baix,baic->ixc", dB, q))
        out.append(dT)
    return tuple(out)


def _softmax(q, k, grid, scale, rel_pos, dtype):
    S = R.logits(q, k, grid, scale, rel_pos, dtype)
    P = np.exp(S - S.max(-1, keepdims=True))
    return P / P.sum(-1, keepdims=True)


def backward(q, k, v, dO, grid, scale=None, rel_pos=None, dtype=np.float64):
    q, k, v, dO = (np.asarray(t, dtype) for t in (q, k, v, dO))
    P = _softmax(q, k, grid, scale, rel_pos, dtype)
    delta = (dO * (P @ v)).sum(-1, keepdims=True)
    dS = P * (dO @ v.swapaxes(-1, -2) - delta)
    return _assemble(P, dS, q, k, dO, grid, scale, rel_pos, dtype)


def magnitudes(q, k, v, dO, grid, scale=None, rel_pos=None, logit_factor=False):
    """the same formulae on magnitudes: A_dS = P (|dO| . |v| + |dO| . (P |v|)) in place of dS, |q|, |k|, |R| in place of the
    operands; with `logit_factor` every row i of P and A_dS carries the forward's factor 1 + max_j logits(|q|, |k|, |R|)[i]"""
    dt = np.float64
    aq, ak, av, ag = (np.abs(np.asarray(t, dt)) for t in (q, k, v, dO))
    arel = None if rel_pos is None else tuple(np.abs(np.asarray(t, dt)) for t in rel_pos)
    P = _softmax(q, k, grid, scale, rel_pos, dt)
    A = P * (ag @ av.swapaxes(-1, -2) + (ag * (P @ av)).sum(-1, keepdims=True))
    if logit_factor:
        f = 1.0 + R.logits(aq, ak, grid, scale, arel).max(-1, keepdims=True)
        P, A = f * P, f * A
    return _assemble(P, A, aq, ak, ag, grid, abs(aq.shape[-1] ** -0.5 if scale is None else scale), arel, dt)
