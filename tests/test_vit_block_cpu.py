"""CPU: the host logic of the transformer-block entry points (csrc/vit_block.hip) and the reference of tests/vit_block_ref.py."""
import numpy as np
import pytest

import vit_block_ref as R
from oracle import judge

LN_BWD, MERGE_BWD, GELU_BWD = 0, 1, 2


@pytest.mark.parametrize("B,H,W,C,ws", [(1, 64, 64, 768, 14), (2, 40, 37, 40, 14), (2, 9, 6, 1280, 0), (3, 5, 3, 2048, 4)])
def test_workspace_size(B, H, W, C, ws):
    from torch_em_amd import _lib
    lib = _lib.load()
    Hp, Wp = (-(-H // ws) * ws, -(-W // ws) * ws) if ws else (H, W)
    assert lib.tem_vit_block_ws(LN_BWD, B, H, W, C, ws) == 8 * C * -(-B * H * W // 32)
    assert lib.tem_vit_block_ws(MERGE_BWD, B, H, W, C, ws) == 8 * C * -(-B * Hp * Wp // 32)
    M = B * H * W
    assert lib.tem_vit_block_ws(GELU_BWD, M, 1, 1, 4 * C, 0) == 4 * 4 * C * min(-(-M // 16), 1024)


def test_refusals_before_any_hip_call():
    from torch_em_amd import _lib
    lib = _lib.load()
    for args, msg in (((LN_BWD, 1, 4, 4, 36, 0), b"multiple of 8"), ((MERGE_BWD, 1, 4, 4, 2056, 0), b"exceeds 2048"),
                      ((LN_BWD, 1, 4, 4, 64, -1), b"negative window"), ((LN_BWD, 0, 4, 4, 64, 0), b"positive"),
                      ((MERGE_BWD, 1 << 20, 64, 64, 64, 0), b"tokens exceed"), ((GELU_BWD, 4, 1, 1, 20, 0), b"multiple of 8"),
                      ((7, 1, 4, 4, 64, 0), b"unknown operation")):
        assert lib.tem_vit_block_ws(*args) == -1 and msg in lib.tem_last_error(), args
    assert lib.tem_vit_block_ws(GELU_BWD, 4, 1, 1, 1 << 20, 0) > 0            # no upper limit on C4
    a = 4096                                                                   # an aligned non-null address; nothing is launched
    assert lib.tem_ln_windows_fwd(*[None] * 6, 1, 4, 4, 64, 0, 1e-6, 0, None) == -1 and b"null pointer" in lib.tem_last_error()
    assert lib.tem_ln_windows_fwd(a, a, a, a + 8, None, None, 1, 4, 4, 64, 0, 1e-6, 0, None) == -1 and b"aligned" in lib.tem_last_error()
    assert lib.tem_ln_windows_fwd(a, a, a, a, None, None, 1, 4, 4, 36, 0, 1e-6, 0, None) == -1 and b"multiple of 8" in lib.tem_last_error()
    assert lib.tem_ln_windows_fwd(a, a, a, a, None, None, 1, 4, 4, 64, 0, 1e-6, 3, None) == -1 and b"storage type" in lib.tem_last_error()
    assert lib.tem_window_merge_ln_fwd(*[a] * 6, a, None, 1, 4, 4, 64, 2, 1e-6, 0, None) == -1 and b"pair" in lib.tem_last_error()
    assert lib.tem_window_merge_ln_fwd(*[a] * 8, 1, 4, 4, 64, -2, 1e-6, 0, None) == -1 and b"negative window" in lib.tem_last_error()
    need = lib.tem_vit_block_ws(LN_BWD, 1, 4, 4, 64, 0)
    assert lib.tem_ln_windows_bwd(*[a] * 8, 1, 4, 4, 64, 0, 0, a, need - 1, None) == -3 and b"workspace too small" in lib.tem_last_error()
    need = lib.tem_vit_block_ws(MERGE_BWD, 1, 4, 4, 64, 3)
    assert lib.tem_window_merge_ln_bwd(*[a] * 10, 1, 4, 4, 64, 3, 0, a, need - 1, None) == -3 and b"workspace too small" in lib.tem_last_error()
    assert lib.tem_bias_gelu_fwd(a, a, a, 4, 20, 0, None) == -1 and b"multiple of 8" in lib.tem_last_error()
    assert lib.tem_bias_gelu_bwd(*[a] * 5, 4, 24, 0, a, 4 * 24 - 1, None) == -3 and b"workspace too small" in lib.tem_last_error()


def _inputs(seed=0, B=2, H=3, W=5, C=6, ws=2):
    rng = np.random.default_rng(seed)
    x, s = rng.standard_normal((2, B, H, W, C))
    gamma, beta = 1 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    y = R.partition(rng.standard_normal((B, H, W, C)), ws) + rng.standard_normal(R.partition(x, ws).shape)   # pad tokens hold values too
    return rng, x, s, y, gamma, beta, ws


def _numeric(loss, ops):
    out = []
    for t in ops:
        num = np.zeros_like(t)
        for idx in np.ndindex(t.shape):
            keep = t[idx]
            t[idx] = keep + 1e-5
            up = loss()
            t[idx] = keep - 1e-5
            num[idx] = (up - loss()) / 2e-5
            t[idx] = keep
        out.append(num)
    return out


def test_reference_gradients_equal_central_differences():
    rng, x, s, y, gamma, beta, ws = _inputs()
    close = lambda a, n: np.abs(a - n).max() <= 1e-8 * (1 + np.abs(n).max())
    g = rng.standard_normal(y.shape)
    got = R.layer_norm_windows_bwd(g, x, gamma, 1e-3, ws)
    num = _numeric(lambda: float((R.layer_norm_windows(x, gamma, beta, 1e-3, ws) * g).sum()), [x, gamma, beta])
    assert all(close(a, n) for a, n in zip(got, num))
    d1, dn = rng.standard_normal((2,) + x.shape)
    got = R.window_merge_norm_bwd(d1, dn, y, s, gamma, 1e-3, ws)
    num = _numeric(lambda: float(sum((o * d).sum() for o, d in zip(R.window_merge_norm(y, s, gamma, beta, 1e-3, ws), (d1, dn)))), [y, s, gamma, beta])
    assert all(close(a, n) for a, n in zip(got, num))
    assert np.all(got[0][R.pad_mask(ws, *x.shape[:3])] == 0)
    h, b, dy = 3 * rng.standard_normal((4, 5)), rng.standard_normal(5), rng.standard_normal((4, 5))
    num = _numeric(lambda: float((R.bias_gelu(h, b) * dy).sum()), [h, b])
    assert all(close(a, n) for a, n in zip(R.bias_gelu_bwd(dy, h, b), num))


def test_float32_restatement_stays_within_the_band():
    rng, x, s, y, gamma, beta, ws = _inputs(1, 2, 9, 6, 40, 4)
    f32 = lambda *ts: [t.astype(np.float32).astype(np.float64) for t in ts]
    x, s, y, gamma, beta = f32(x, s, y, gamma, beta)
    g, dn = f32(rng.standard_normal(y.shape), rng.standard_normal(x.shape))
    rstd = 1 / np.sqrt(x.var(-1, keepdims=True) + 1e-6)
    pairs = [(R.layer_norm_windows(x, gamma, beta, 1e-6, ws, np.float32), R.layer_norm_windows(x, gamma, beta, 1e-6, ws),
              R.partition(R.forward_scale(np.abs(x), gamma, beta, rstd), ws))]
    scales, _ = R.ln_bwd_scales(R.merge(g, ws, *x.shape[:3]), x, gamma, 1e-6)
    pairs += list(zip(R.layer_norm_windows_bwd(g, x, gamma, 1e-6, ws, np.float32), R.layer_norm_windows_bwd(g, x, gamma, 1e-6, ws), scales))
    h, b, dy = f32(np.linspace(-6, 6, 400).reshape(50, 8), 0.1 * rng.standard_normal(8), rng.standard_normal((50, 8)))
    sf, sdh, sdb = R.gelu_scales(dy, h, b)
    pairs += [(R.bias_gelu(h, b, np.float32), R.bias_gelu(h, b), sf)]
    # backward: Phi = 0.5 (1 + erf) cancels for negative z and the scale of dh carries no (1 + |erf|) term, so the restatement
    # leaves the band there by construction (the GPU suite's band is e32's own); it is held to the band for z >= -1
    h = np.abs(h + 1) - 1
    sf, sdh, sdb = R.gelu_scales(dy, h, b)
    pairs += list(zip(R.bias_gelu_bwd(dy, h, b, np.float32), R.bias_gelu_bwd(dy, h, b), (sdh, sdb)))
    for a32, a64, sc in pairs:
        assert a32.dtype == np.float32 and judge.within(judge.units(a32, a64, sc), 1.0), judge.units(a32, a64, sc)
