"""CPU: the float64 Dice oracle (oracle/dice_ref.py) pinned to torch float64 autograd and to the reference-made fixtures, the
judge of tests/test_gpu_dice.py tested on deliberately wrong "kernel outputs", and the host-side refusals of the Dice C ABI.

The wrong outputs are built on the CPU from the float32 restatement, on the smallest shapes tests/test_gpu_dice.py uses
(V = 63 and 257, two samples, three channels); the unmodified restatement is accepted on the same inputs, so every
rejection is due to the planted mistake.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_err
from oracle import dice_ref as R
from oracle import loss_ref
from oracle.dice_cases import FLAG_SETS, anchors, coefficients, flag_name, gout_variant, make_inputs

f32 = np.float32


# ------------------------------------------------------------------------------------------ the oracle against torch
def _oracle_loss_and_grad(p, t, m, flags, alpha, beta, channelwise, reduce, eps=1e-7):
    """value and gradient of alpha * dice + beta * mean BCE through the three oracle functions, float64 throughout"""
    sums = R.dice_sums_f64(p, t, m, flags)
    out, ca, cb = R.dice_finalize_f64(sums, eps, channelwise, True, reduce)
    per_channel = channelwise and reduce is None
    w_bce = beta / p.size if flags & R.BCE else 0.0
    val = alpha * out
    if flags & R.BCE:
        val = val + beta * sums[:, 3].sum() / p.size
    gout = np.ones(p.shape[1]) if per_channel else None
    grad = R.dice_grad_f64(p, t, m, ca, cb, gout, per_channel, flags, alpha, w_bce)
    return val, grad


def _torch_loss_and_grad(p, t, m, flags, alpha, beta, channelwise, reduce, eps=1e-7):
    x = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    tt = torch.from_numpy(t.astype(np.float64))
    pv = torch.sigmoid(x) if flags & R.LOGITS else x
    if m is not None:
        mm = torch.from_numpy(m.astype(np.float64))
        val = loss_ref.dice_loss(pv * mm, tt * mm, channelwise=channelwise, eps=eps, reduce_channel=reduce)
    else:
        val = loss_ref.dice_loss(pv, tt, channelwise=channelwise, eps=eps, reduce_channel=reduce)
    val = alpha * val
    if flags & R.BCE:
        val = val + beta * (F.binary_cross_entropy_with_logits(x, tt) if flags & R.LOGITS else F.binary_cross_entropy(x, tt))
    val.sum().backward()
    return val.detach().numpy().reshape(-1), x.grad.numpy()


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_oracle_matches_torch_float64_autograd(flags, soft):
    """all four family members, every reduction, flat and channel-wise, masked (the plain member), soft and binary targets.
    512 elements and power-of-two weights: beta / count is exact in float32, so the float-valued weights of the oracle are
    torch's.  Elementwise: 1e-10 relative (float64 round-off of two evaluation orders) plus 1e-15 of the largest gradient."""
    N, C, V = 2, 4, 64
    p, t, m = make_inputs(N, C, V, 3 + flags, bool(flags & R.LOGITS), soft)
    alpha, beta = (1.0, 0.0) if not flags & R.BCE else (0.5, 2.0)
    for channelwise in (True, False):
        for reduce in ("sum", "mean", "max", "min", None) if channelwise else ("sum",):
            if reduce is None and flags & R.BCE:
                continue                                      # a per-channel loss plus a scalar: not a member of the family
            for mask in ((None, m) if flags == 0 else (None,)):
                got_v, got_g = _oracle_loss_and_grad(p, t, mask, flags, alpha, beta, channelwise, reduce)
                ref_v, ref_g = _torch_loss_and_grad(p, t, mask, flags, alpha, beta, channelwise, reduce)
                what = (flag_name(flags, mask is not None), channelwise, reduce)
                assert np.allclose(got_v, ref_v, rtol=1e-12, atol=1e-13), what
                tol = 1e-10 * np.abs(ref_g) + 1e-15 * np.abs(ref_g).max()
                assert (np.abs(got_g.reshape(ref_g.shape) - ref_g) <= tol).all(), what
                if mask is not None:
                    assert not got_g.reshape(ref_g.shape)[mask == 0].any()


def test_oracle_eps_branch_matches_torch():
    """den < eps: the clamp is active, its gradient is zero -- one channel, and all channels"""
    p, t, _ = make_inputs(2, 3, 63, 5, False, True, masked=False)
    for dead in ([1], [0, 1, 2]):
        q, s = p.copy(), t.copy()
        q[:, dead], s[:, dead] = q[:, dead] * f32(1e-6), s[:, dead] * f32(1e-6)
        for channelwise in (True, False):
            got_v, got_g = _oracle_loss_and_grad(q, s, None, 0, 1.0, 0.0, channelwise, "sum")
            ref_v, ref_g = _torch_loss_and_grad(q, s, None, 0, 1.0, 0.0, channelwise, "sum")
            assert np.allclose(got_v, ref_v, rtol=1e-12)
            assert np.allclose(got_g.reshape(ref_g.shape), ref_g, rtol=1e-10, atol=1e-300)
        sums = R.dice_sums_f64(q, s)
        _, ca, cb = R.dice_finalize_f64(sums, 1e-7, True, True, "sum")
        assert (sums[dead, 1] + sums[dead, 2] < 1e-7).all() and not cb[dead].any() and (ca[dead] == -2.0 / 1e-7).all()


# ------------------------------------------------------------------------------------------ the oracle against the fixtures
def test_oracle_matches_the_reference_fixture_g5():
    """tolerances of tests/test_oracle_golden.py::test_dice_oracle_matches_reference"""
    g = dict(np.load(os.path.join(GOLDEN, "g5_dice.npz")))
    p, t = g["p"], g["t"]
    for cw in (True, False):
        for red in ("sum", "mean", "max", "min"):
            val, grad = _oracle_loss_and_grad(p, t, None, 0, 1.0, 0.0, cw, red)
            assert abs(float(val[0]) - float(g[f"loss_{int(cw)}_{red}"])) < 1e-6
            assert rel_err(grad.reshape(p.shape), g[f"grad_{int(cw)}_{red}"]) < 1e-5
    score, _, _ = R.dice_finalize_f64(R.dice_sums_f64(p, t), 1e-7, True, False, None)
    assert rel_err(score, g["score_none"]) < 1e-6
    pm, tm = g["pm"], g["tm"]
    c = pm.shape[1]
    val, grad = _oracle_loss_and_grad(pm, tm[:, :c], tm[:, c:], 0, 1.0, 0.0, True, "sum")
    assert abs(float(val[0]) - float(g["loss_masked"])) < 1e-6
    assert rel_err(grad.reshape(pm.shape), g["grad_masked"]) < 1e-5


def test_oracle_matches_the_reference_fixture_g5b():
    """tolerances of tests/test_gpu_ops.py::test_dice_family_against_reference_golden"""
    g = np.load(os.path.join(GOLDEN, "g5b_dice_variants.npz"))
    t = g["target"]
    L, B = R.LOGITS, R.BCE
    cases = {"dwl_default": (L, 1.0, 0.0, True, "sum"), "dwl_mean": (L, 1.0, 0.0, True, "mean"),
             "dwl_flat": (L, 1.0, 0.0, False, "sum"), "bce_default": (B, 1.0, 1.0, True, "sum"),
             "bce_weighted": (B, 0.7, 1.3, True, "sum"), "bce_flat": (B, 0.5, 2.0, False, "sum"),
             "bcel_default": (L | B, 1.0, 1.0, True, "sum"), "bcel_weighted": (L | B, 1.5, 0.25, False, "sum")}
    for name, (flags, alpha, beta, cw, red) in cases.items():
        x = g["logits" if flags & L else "probs"]
        val, grad = _oracle_loss_and_grad(x, t, None, flags, alpha, beta, cw, red)
        ref = float(g[f"{name}.loss"])
        assert abs(float(val[0]) - ref) < 3e-6 * max(1.0, abs(ref)), name
        assert rel_err(grad.reshape(x.shape), g[f"{name}.grad"]) < 5e-6, name


# ------------------------------------------------------------------------------------------ the judge
SMALL = [(2, 3, 63), (2, 3, 257)]


def _sums_verdict(got, p, t, m, flags):
    ref = R.dice_sums_f64(p, t, m, flags)
    e32 = R.sums_units(R.dice_sums_f32(p, t, m, flags), ref)
    ek = R.sums_units(got, ref)
    return all(R.within(k, e) for k, e in zip(ek, e32)), ek, e32


def _grad_verdict(got, p, t, m, ca, cb, gout, per_channel, flags, wd, wb):
    ref = R.dice_grad_f64(p, t, m, ca, cb, gout, per_channel, flags, wd, wb)
    scale = R.grad_scale(p, t, m, ca, cb, gout, flags, wd, wb)
    e32 = R.grad_units(R.dice_grad_f32(p, t, m, ca, cb, gout, per_channel, flags, wd, wb), ref, scale)
    ek = R.grad_units(got, ref, scale)
    return R.within(ek, e32), ek, e32


def _sums_dropping(p, t, m, flags, keep):
    """float32 sums of a kernel that loses the voxels `keep`: onwards of the LAST sample"""
    head = R.dice_sums_f32(p[:-1], t[:-1], None if m is None else m[:-1], flags)
    tail = R.dice_sums_f32(p[-1:, :, :keep], t[-1:, :, :keep], None if m is None else m[-1:, :, :keep], flags)
    return head + tail


def _weights(flags, n):
    return (f32(0.75), f32(2.0 / n)) if flags & R.BCE else (f32(1.0), f32(0.0))


@pytest.mark.parametrize("N,C,V", SMALL)
def test_judge_accepts_plain_float32_and_stays_within_the_documented_figures(N, C, V):
    """the restatement itself: <= 1.9 units for the sums and <= 2.8 for the gradients (the figures that back MARGIN)"""
    for flags in FLAG_SETS:
        for masked in ((False, True) if flags == 0 else (False,)):
            p, t, m = make_inputs(N, C, V, 17 + flags, bool(flags & R.LOGITS), soft=bool(flags & 1) ^ (V > 100), masked=masked)
            ok, ek, _ = _sums_verdict(R.dice_sums_f32(p, t, m, flags), p, t, m, flags)
            assert ok and max(ek) <= 1.9, (flags, masked, ek)
            ca, cb = coefficients(p, t, m, flags)
            wd, wb = _weights(flags, p.size)
            for kind in (0, 1, 2):
                gout, per = gout_variant(kind, C, 5)
                got = R.dice_grad_f32(p, t, m, ca, cb, gout, per, flags, wd, wb)
                ok, ek, _ = _grad_verdict(got, p, t, m, ca, cb, gout, per, flags, wd, wb)
                assert ok and ek <= 2.8, (flags, masked, kind, ek)
            # the channel with ca = cb = 0: exactly zero, or exactly the cross-entropy part
            g = R.dice_grad_f32(p, t, m, ca, cb, None, False, flags, wd, wb)
            if not flags & R.BCE:
                assert not g[:, -1].any()


@pytest.mark.parametrize("N,C,V", SMALL)
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_judge_rejects_dropped_voxels_in_the_sums(N, C, V, flags):
    p, t, _ = make_inputs(N, C, V, 23 + flags, bool(flags & R.LOGITS), soft=False, masked=False)
    ok, _, _ = _sums_verdict(_sums_dropping(p, t, None, flags, V), p, t, None, flags)
    assert ok, "nothing dropped: the split float32 sum is accepted"
    for keep in (V - 1, anchors(V)[0]):                       # the last voxel; the last 256-voxel tile
        ok, ek, e32 = _sums_verdict(_sums_dropping(p, t, None, flags, keep), p, t, None, flags)
        assert not ok, (keep, ek, e32)
        assert all(not R.within(k, e) for k, e in zip(ek, e32)), "every column notices"


@pytest.mark.parametrize("N,C,V", SMALL)
def test_judge_rejects_the_mask_missing_on_the_target(N, C, V):
    p, t, m = make_inputs(N, C, V, 29, False, soft=True)
    wrong = R.dice_sums_f32(p * m, t, None, 0)                # p masked, t not
    ok, ek, e32 = _sums_verdict(wrong, p, t, m, 0)
    assert not ok and not R.within(ek[2], e32[2]), "sum t^2 took the unmasked target"
    ca, cb = coefficients(p, t, m, 0)
    a, b = ca.reshape(1, -1, 1), cb.reshape(1, -1, 1)
    wrong = (a * t + b * (p * m)) * m * m                     # the final mask hides it ...
    ok, _, _ = _grad_verdict(wrong, p, t, m, ca, cb, None, False, 0, 1.0, 0.0)
    assert ok, "... for a binary mask t m m == t m: only the sums can see this mistake"
    soft_mask = (m * f32(0.5) + f32(0.25)).astype(f32)
    wrong = (a * t + b * (p * soft_mask)) * soft_mask
    ok, _, _ = _grad_verdict(wrong, p, t, soft_mask, ca, cb, None, False, 0, 1.0, 0.0)
    assert not ok, "with a fractional mask the gradient shows it too"


@pytest.mark.parametrize("N,C,V", SMALL)
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_judge_rejects_wrong_gradients(N, C, V, flags):
    logits = bool(flags & R.LOGITS)
    p, t, m = make_inputs(N, C, V, 31 + flags, logits, soft=True, masked=(flags == 0))
    ca, cb = coefficients(p, t, m, flags, special=False)
    wd, wb = _weights(flags, p.size)
    gout, per = gout_variant(2, C, 7)
    args = (p, t, m, ca, cb, gout, per, flags, wd, wb)
    good = R.dice_grad_f32(*args)
    assert _grad_verdict(good, *args)[0]

    def rejected(wrong):
        return not _grad_verdict(wrong, *args)[0]

    for stale in (np.nan, 0.0):                               # the last voxel never written / written as zero
        w = good.copy()
        w[-1, :, -1] = stale
        assert rejected(w), stale
    w = good.copy()
    w[:, :, anchors(V)[0]:] = 0.0                             # the last 256-voxel tile
    assert rejected(w)
    assert rejected(R.dice_grad_f32(p, t, m, np.roll(ca, -1), np.roll(cb, -1), gout, per, flags, wd, wb)), "neighbour's ca, cb"
    assert rejected(R.dice_grad_f32(p, t, m, ca, cb, np.roll(gout, 1), per, flags, wd, wb)), "neighbour's gout"
    if logits:
        a, b, go = ca.reshape(1, -1, 1), cb.reshape(1, -1, 1), gout.reshape(1, -1, 1)
        s = R.sigmoid_f32(p)
        w = wd * (a * t + b * s)                              # sigma' omitted
        if flags & R.BCE:
            w = w + wb * (s - t)
        assert rejected(go * w)
    if flags & R.BCE:
        assert rejected(R.dice_grad_f32(p, t, m, ca, cb, gout, per, flags, wd, wb * f32(N))), "w_bce off by the factor N"


def test_judge_rejects_wrong_finalize_outputs():
    rng = np.random.RandomState(41)
    C = 12
    sums = np.stack([rng.uniform(10, 20, C), rng.uniform(30, 40, C), rng.uniform(20, 30, C)], 1)
    sums[4] = [1e-9, 2e-8, 3e-8]                              # den = 5e-8 < eps
    for reduce in ("sum", "max"):
        ref = R.dice_finalize_f64(sums, 1e-7, True, True, reduce)
        good = [v.astype(f32) for v in ref]
        assert all(R.finalize_units(a, b) <= 1.0 for a, b in zip(good, ref))
    ref = R.dice_finalize_f64(sums, 1e-7, True, True, "sum")
    _, ca32, cb32 = R.dice_finalize_f32(sums, 1e-7, True, True, "sum")
    assert cb32[4] == 0 and ref[2][4] == 0
    wrong = cb32.copy()
    wrong[4] = f32(4) * f32(sums[4, 0]) / (f32(1e-7) * f32(1e-7))   # the clamp's gradient not zeroed
    assert R.finalize_units(cb32, ref[2]) < 4 and R.finalize_units(wrong, ref[2]) == float("inf")
    ref = R.dice_finalize_f64(sums, 1e-7, True, True, "max")
    assert list(np.flatnonzero(ref[1])) == [4], "the dead channel has the largest loss"
    assert R.finalize_units(ca32, ref[1]) == float("inf"), "non-arg channels not zeroed"
    out_min = R.dice_finalize_f64(sums, 1e-7, True, True, "min")[0]
    assert R.finalize_units(out_min.astype(f32), ref[0]) > 1e5, "min where max was asked"


def test_judge_counts_missing_and_non_finite_values_as_infinite():
    ref = np.array([[1.0, 2.0, 3.0]])
    assert R.sums_units(ref, ref) == [0.0, 0.0, 0.0]
    assert R.sums_units(np.array([[1.0, np.nan, np.inf]]), ref) == [0.0, float("inf"), float("inf")]
    assert R.sums_units(ref[:, :2], ref) == [float("inf")] * 3
    assert R._units(np.array([1e-39]), np.array([0.0]), np.array([0.0])) == 0.0, "inside the absolute allowance"
    assert R._units(np.array([1e-30]), np.array([0.0]), np.array([0.0])) == float("inf"), "an error where nothing may be"
    assert R.within(4.0, 0.2) and not R.within(4.01, 0.2) and R.within(8.0, 2.0) and not R.within(float("nan"), 1.0)


# ------------------------------------------------------------------------------------------ the C ABI refuses on the host
def test_dice_c_abi_refuses_bad_arguments_before_any_launch():
    """every argument check of csrc/dice.hip precedes its launch: -1 (TEM_EINVAL) or -3 (TEM_EWS) and a message, on a
    machine without a GPU as well.  The non-null pointers are host buffers nobody dereferences."""
    from torch_em_amd import _lib
    lib = _lib.load()
    host = np.zeros(64, np.float64)
    P = host.ctypes.data_as(ctypes.c_void_p).value
    N, C, V = 2, 3, 100
    ws = lib.tem_dice_ws(N, V, C)
    assert ws == 2048 * C * 4 * 4 and lib.tem_dice_ws(1, 1, 1024) == 2048 * 1024 * 16
    s = (C * V, V, 1)

    def sums(p=P, t=P, mask=None, n=N, c=C, v=V, out=P, wsp=P, nbytes=ws):
        return lib.tem_dice_sums(p, *s, t, *s, mask, n, c, v, out, wsp, nbytes, None)

    def sums2(flags, n=N, c=C, nbytes=ws):
        return lib.tem_dice_sums2(P, *s, P, *s, n, c, V, P, P, nbytes, flags, None)

    for kw in (dict(p=None), dict(t=None), dict(out=None), dict(wsp=None)):
        assert sums(**kw) == -1 and b"null pointer" in lib.tem_last_error(), kw
    for c in (0, 1025, -1):
        assert sums(c=c, nbytes=1 << 40) == -1 and b"bad shape" in lib.tem_last_error(), c
        assert sums2(0, c=c, nbytes=1 << 40) == -1
    assert sums(n=0) == -1 and sums(v=0) == -1
    assert sums(n=2049, nbytes=1 << 40) == -1 and b"batch too large" in lib.tem_last_error()
    assert sums2(3, n=2049, nbytes=1 << 40) == -1 and b"batch too large" in lib.tem_last_error()
    assert sums(nbytes=ws - 1) == -3 and b"workspace too small" in lib.tem_last_error()
    assert sums2(2, nbytes=ws - 1) == -3
    for flags in (4, 8, -1, 1 << 30):
        assert sums2(flags) == -1 and b"unknown flags" in lib.tem_last_error(), flags

    def finalize(sums_=P, c=C, reduce=1, out=P, ca=P, cb=P):
        return lib.tem_dice_finalize(sums_, c, 1e-7, 1, 1, reduce, out, ca, cb, None)

    for kw in (dict(sums_=None), dict(out=None), dict(ca=None), dict(cb=None), dict(c=0)):
        assert finalize(**kw) == -1 and b"bad arguments" in lib.tem_last_error(), kw
    for reduce in (5, -1):
        assert finalize(reduce=reduce) == -1 and b"Unsupported channel reduction" in lib.tem_last_error()
        assert lib.tem_dice_finalize2(P, 4, C, 1e-7, 1, 1, reduce, P, P, P, None) == -1
    for ncol in (2, 5, 0):
        assert lib.tem_dice_finalize2(P, ncol, C, 1e-7, 1, 1, 1, P, P, P, None) == -1
        assert b"ncol must be 3 or 4" in lib.tem_last_error()

    def grad(p=P, t=P, ca=P, cb=P, gp=P, n=N, c=C, v=V):
        return lib.tem_dice_grad(p, *s, t, *s, None, ca, cb, None, 0, gp, *s, n, c, v, None)

    for kw in (dict(p=None), dict(t=None), dict(ca=None), dict(cb=None), dict(gp=None), dict(n=0), dict(c=0), dict(v=0)):
        assert grad(**kw) == -1 and b"bad arguments" in lib.tem_last_error(), kw
    for flags in (4, -1):
        assert lib.tem_dice_grad2(P, *s, P, *s, P, P, None, 0, P, *s, N, C, V, flags, 1.0, 0.0, None) == -1
        assert b"unknown flags" in lib.tem_last_error()
    assert lib.tem_dice_grad2(None, *s, P, *s, P, P, None, 0, P, *s, N, C, V, 1, 1.0, 0.0, None) == -1
    with pytest.raises(ValueError, match="unknown flags"):
        _lib.check(sums2(4), "tem_dice_sums2")
    with pytest.raises(_lib.TemError, match="workspace too small"):
        _lib.check(sums(nbytes=0), "tem_dice_sums")
    assert host.sum() == 0.0
