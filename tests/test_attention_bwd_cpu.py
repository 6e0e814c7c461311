"""CPU: the float64 gradients of tests/attention_bwd_ref.py against central differences, and the host logic of the backward's
entry points."""
import numpy as np
import pytest

import attention_bwd_ref as RB
import attention_ref as R


def test_reference_equals_central_differences():
    H, W, D = 3, 2, 4
    rng = np.random.default_rng(0)
    q, k, v, dO = (rng.standard_normal((2, 2, H * W, D)) for _ in range(4))
    rel = (rng.standard_normal((2 * H - 1, D)), rng.standard_normal((2 * W - 1, D)))
    got = RB.backward(q, k, v, dO, (H, W), 0.3, rel)
    ops = [q, k, v, rel[0], rel[1]]
    loss = lambda: float((R.attention(ops[0], ops[1], ops[2], (H, W), 0.3, (ops[3], ops[4])) * dO).sum())
    eps = 1e-5
    for name, x, g in zip(("dq", "dk", "dv", "dRh", "dRw"), ops, got):
        num = np.zeros_like(x)
        for idx in np.ndindex(x.shape):
            keep = x[idx]
            x[idx] = keep + eps
            up = loss()
            x[idx] = keep - eps
            num[idx] = (up - loss()) / (2 * eps)
            x[idx] = keep
        assert np.abs(g - num).max() <= 1e-8 * (1 + np.abs(num).max()), name


@pytest.mark.parametrize("B,nH,H,W,D", [(2, 3, 14, 14, 64), (1, 16, 64, 64, 80), (25, 12, 5, 3, 64)])
def test_backward_workspace_size(B, nH, H, W, D):
    from torch_em_amd import _lib
    lib = _lib.load()
    N = H * W
    assert lib.tem_attention_bwd_ws(B, nH, H, W, D, 0) == 4 * B * nH * N
    assert lib.tem_attention_bwd_ws(B, nH, H, W, D, 1) == 4 * B * nH * N + 2 * 4 * B * nH * N * (H + W) + 4 * B * nH * (2 * H - 1 + 2 * W - 1) * D


def test_refusals_before_any_hip_call():
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_attention_bwd_ws(1, 1, 2, 2, 48, 1) == -1 and b"head width" in lib.tem_last_error()
    assert lib.tem_attention_bwd_ws(1, 1, 256, 65, 64, 1) == -1 and b"exceeds" in lib.tem_last_error()
    assert lib.tem_attention_bwd_ws(1, 1, 256, 64, 64, 1) > 0
    rc = lib.tem_attention_bwd(*[None] * 21, 1, 1, 2, 2, 64, 0.125, 0, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.tem_last_error()
    rc = lib.tem_attention_fwd_ex(*[None] * 10, 1, 1, 2, 2, 64, 0.125, 0, None, 0, None, None)
    assert rc == -1 and b"null pointer" in lib.tem_last_error()
