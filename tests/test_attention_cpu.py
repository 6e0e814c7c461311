"""CPU: the host logic of the attention entry points and the float64 reference of tests/attention_ref.py."""
import math

import numpy as np
import pytest

import attention_ref as R


@pytest.mark.parametrize("B,nH,H,W,D", [(2, 3, 14, 14, 64), (1, 16, 64, 64, 80), (25, 12, 5, 3, 64)])
def test_workspace_size(B, nH, H, W, D):
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_attention_ws(B, nH, H, W, D, 1) == B * nH * H * W * (H + W) * 4
    assert lib.tem_attention_ws(B, nH, H, W, D, 0) == 0


def test_null_pointers_are_refused_before_any_hip_call():
    from torch_em_amd import _lib
    lib = _lib.load()
    rc = lib.tem_attention_fwd(None, None, None, None, None, None, None, None, None, None, 1, 1, 2, 2, 64, 0.125, 0, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.tem_last_error()
    assert lib.tem_attention_ws(1, 1, 2, 2, 48, 1) == -1 and b"head width" in lib.tem_last_error()
    assert lib.tem_attention_ws(1, 1, 257, 2, 64, 1) == -1 and b"exceeds" in lib.tem_last_error()


def test_reference_equals_a_direct_evaluation():
    H, W, D = 3, 2, 4
    rng = np.random.default_rng(0)
    q, k, v = (rng.standard_normal((1, 2, H * W, D)) for _ in range(3))
    Rh, Rw = rng.standard_normal((2 * H - 1, D)), rng.standard_normal((2 * W - 1, D))
    got = R.attention(q, k, v, (H, W), scale=0.3, rel_pos=(Rh, Rw))
    for a in range(2):
        for i in range(H * W):
            s = [sum(float(q[0, a, i, c]) * (0.3 * float(k[0, a, j, c]) + float(Rh[i // W - j // W + H - 1, c])
                                              + float(Rw[i % W - j % W + W - 1, c])) for c in range(D)) for j in range(H * W)]
            p = [math.exp(x - max(s)) for x in s]
            for c in range(D):
                want = sum(pj * float(v[0, a, j, c]) for j, pj in enumerate(p)) / sum(p)
                assert abs(got[0, a, i, c] - want) <= 1e-14 * (1 + abs(want)), (a, i, c)
