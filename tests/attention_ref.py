"""The definition ops.attention is judged against (numpy; float64, and restated with every operation in float32 for e32).

    S[b,a,i,j] = scale * sum_c q[b,a,i,c] k[b,a,j,c] + sum_c q[b,a,i,c] Rh[hi - hj + H-1, c] + sum_c q[b,a,i,c] Rw[wi - wj + W-1, c]
    P = softmax_j(S)        O[b,a,i,c] = sum_j P[b,a,i,j] v[b,a,j,c]             token i = hi * W + wi
"""
import numpy as np


def logits(q, k, grid, scale=None, rel_pos=None, dtype=np.float64):
    H, W = grid
    q, k = np.asarray(q, dtype), np.asarray(k, dtype)
    B, nH, N, D = q.shape
    S = dtype(D ** -0.5 if scale is None else scale) * (q @ k.swapaxes(-1, -2))
    if rel_pos is not None:
        Rh, Rw = (np.asarray(t, dtype) for t in rel_pos)
        r = q.reshape(B, nH, H, W, D)
        rel_h = np.einsum("bahwc,hkc->bahwk", r, Rh[np.arange(H)[:, None] - np.arange(H)[None, :] + H - 1])
        rel_w = np.einsum("bahwc,wkc->bahwk", r, Rw[np.arange(W)[:, None] - np.arange(W)[None, :] + W - 1])
        S = (S.reshape(B, nH, H, W, H, W) + rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, nH, N, N)
    return S


def attention(q, k, v, grid, scale=None, rel_pos=None, dtype=np.float64):
    S = logits(q, k, grid, scale, rel_pos, dtype)
    P = np.exp(S - S.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)) @ np.asarray(v, dtype)


def attention32(q, k, v, grid, scale=None, rel_pos=None):
    return attention(q, k, v, grid, scale, rel_pos, dtype=np.float32)
