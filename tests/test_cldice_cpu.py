"""CPU: the clDice oracle -- a torch-op restatement of the soft skeleton and the score, and an explicit GATHER-FORM
gradient that implements PyTorch's tie rules by hand (no autograd) -- checked against the reference's recorded runs
(tests/golden/g13_cldice.npz, written by gen_golden_cldice.py), plus the host-side surface of the new classes.

Tie rules of the hand-written gradient (the ones csrc/cldice.hip implements):
  pools       the gradient of a window goes to its FIRST extremum in (d, h, w) scan order (strict comparison)
  min(a, b)   the smaller operand takes it; on equality each takes half (3-D min(min(p_z, p_y), p_x): 1/4, 1/4, 1/2)
  relu        passes iff its argument is > 0
"""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

G13 = os.path.join(GOLDEN, "g13_cldice.npz")
FIELDS = ("x", "y", "num_iter", "alpha", "exclude_background", "kind", "skel_x", "skel_y", "loss", "loss32", "grad",
          "grad32_dev")
TIE_CASES = ("quant3d", "plateau3d", "quant2d", "plateau2d", "odd2d", "exbg2d_soft", "line_overlap", "line_apart")


def golden():
    return np.load(G13)


def case_names():
    return sorted({k.split(".")[0] for k in golden().files})


def load_case(name):
    g = golden()
    return {f: g[f"{name}.{f}"] for f in FIELDS}


# ---- restatement with torch ops (any dtype) ------------------------------------------------------------------------
def erode(x):
    if x.dim() == 4:
        return torch.min(-F.max_pool2d(-x, (3, 1), 1, (1, 0)), -F.max_pool2d(-x, (1, 3), 1, (0, 1)))
    p1 = -F.max_pool3d(-x, (3, 1, 1), 1, (1, 0, 0))
    p2 = -F.max_pool3d(-x, (1, 3, 1), 1, (0, 1, 0))
    p3 = -F.max_pool3d(-x, (1, 1, 3), 1, (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def dilate(x):
    return F.max_pool2d(x, 3, 1, 1) if x.dim() == 4 else F.max_pool3d(x, 3, 1, 1)


def skel_restate(x, num_iter):
    """e_{j+1} = erode(e_j), delta_j = relu(e_j - dilate(e_{j+1})), skel += relu(delta - skel * delta)"""
    e1 = erode(x)
    skel = F.relu(x - dilate(e1))
    for _ in range(num_iter):
        x, e1 = e1, erode(e1)
        delta = F.relu(x - dilate(e1))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def cldice_restate(x, y, num_iter, invert=False, eps=1e-7):
    sx, sy = skel_restate(x, num_iter), skel_restate(y, num_iter)
    tp = (sx * y).sum() / sx.sum().clamp(min=eps)
    ts = (sy * x).sum() / sy.sum().clamp(min=eps)
    score = 2.0 * (tp * ts) / (tp + ts).clamp(min=eps)
    return 1.0 - score if invert else score


def loss_restate(x, y, kind, num_iter, alpha, exclude_background, eps=1e-7):
    if exclude_background:
        x, y = x[:, 1:], y[:, 1:]
    cl = cldice_restate(x, y, num_iter, True, eps)
    if kind == 0:
        return cl
    dice = 1.0 - 2.0 * (x * y).sum() / ((x * x).sum() + (y * y).sum()).clamp(min=eps)
    return (1.0 - alpha) * dice + alpha * cl


# ---- explicit gather-form gradient (numpy float64, no autograd) ----------------------------------------------------
def _shift(a, off, fill=0.0):
    """b[..., v] = a[..., v - off] over the trailing len(off) axes; `fill` where v - off is outside"""
    b = np.full_like(a, fill)
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    for k, o in enumerate(off):
        ax = a.ndim - len(off) + k
        n = a.shape[ax]
        if abs(o) >= n:
            return b
        dst[ax] = slice(max(o, 0), n + min(o, 0))
        src[ax] = slice(max(-o, 0), n + min(-o, 0))
    b[tuple(dst)] = a[tuple(src)]
    return b


def _axis_off(nd, ax, o):
    return tuple(o if k == ax else 0 for k in range(nd))


def np_erode_parts(e, nd):
    """per spatial axis: (line minimum p_a, position 0/1/2 of its FIRST minimum)"""
    parts = []
    for ax in range(nd):
        best = _shift(e, _axis_off(nd, ax, 1), np.inf)          # e[v - 1]
        pos = np.zeros(e.shape, np.int8)
        for k, cand in ((1, e), (2, _shift(e, _axis_off(nd, ax, -1), np.inf))):
            better = cand < best
            best = np.where(better, cand, best)
            pos[better] = k
        parts.append((best, pos))
    return parts


def np_erode(e, nd):
    out = None
    for p, _ in np_erode_parts(e, nd):
        out = p if out is None else np.minimum(out, p)
    return out


def np_dilate_first(e, nd):
    """(window maximum, index of its FIRST maximum in scan order)"""
    best = np.full(e.shape, -np.inf)
    idx = np.full(e.shape, -1, np.int8)
    for k, o in enumerate(itertools.product((-1, 0, 1), repeat=nd)):
        cand = _shift(e, tuple(-c for c in o), -np.inf)          # e[v + o]
        better = cand > best
        best = np.where(better, cand, best)
        idx[better] = k
    return best, idx


def np_dilate_bwd(e, h, nd):
    """out[v] = sum over the window u of v of h[u] * [first maximum of window(u) is v]"""
    _, idx = np_dilate_first(e, nd)
    out = np.zeros_like(h)
    for k, o in enumerate(itertools.product((-1, 0, 1), repeat=nd)):
        out += _shift(np.where(idx == k, h, 0.0), o)             # u selected u + o = v
    return out


def np_erode_bwd(e, g, nd):
    """out[v] = sum over axes a and the line u of v of g[u] * w_a(u) * [first minimum of line_a(u) is v]"""
    parts = np_erode_parts(e, nd)

    def split(a, b):   # torch.min(a, b): the smaller takes the gradient, half / half on equality
        return np.where(a < b, 1.0, np.where(a > b, 0.0, 0.5))

    if nd == 3:
        (pz, _), (py, _), (px, _) = parts
        wz1 = split(pz, py)
        wm = split(np.minimum(pz, py), px)
        weights = [wz1 * wm, (1.0 - wz1) * wm, 1.0 - wm]
    else:
        (py, _), (px, _) = parts
        wy = split(py, px)
        weights = [wy, 1.0 - wy]
    out = np.zeros_like(g)
    for ax, ((_, pos), w) in enumerate(zip(parts, weights)):
        for k in range(3):
            out += _shift(np.where(pos == k, g * w, 0.0), _axis_off(nd, ax, k - 1))
    return out


def np_skel_forward(x, num_iter):
    nd = x.ndim - 2
    es = [x]
    for _ in range(num_iter + 1):
        es.append(np_erode(es[-1], nd))
    pres = [es[j] - np_dilate_first(es[j + 1], nd)[0] for j in range(num_iter + 1)]
    skels = [np.maximum(pres[0], 0.0)]
    for j in range(1, num_iter + 1):
        d = np.maximum(pres[j], 0.0)
        skels.append(skels[-1] + np.maximum(d - skels[-1] * d, 0.0))
    return es, pres, skels


def np_skel_bwd(x, num_iter, gs):
    """d / d x of sum(skel * gs), rounds in reverse: point, dilate, erode"""
    nd = x.ndim - 2
    es, pres, skels = np_skel_forward(x, num_iter)
    a = None
    for j in range(num_iter, -1, -1):
        if j:
            s, d = skels[j - 1], np.maximum(pres[j], 0.0)
            gr = np.where(d - s * d > 0, gs, 0.0)
            gd = gr - gr * s
            gs = gs - gr * d
        else:
            gd = gs
        h = np.where(pres[j] > 0, -gd, 0.0)
        g = np_dilate_bwd(es[j + 1], h, nd)
        if a is not None:
            g = a + g
        a = -h + np_erode_bwd(es[j], g, nd)
    return a


def np_loss_and_grad(x, y, kind, num_iter, alpha, exclude_background, eps=1e-7):
    x, y = x.astype(np.float64), y.astype(np.float64)
    full = x.shape
    if exclude_background:
        x, y = x[:, 1:], y[:, 1:]
    sx, sy = np_skel_forward(x, num_iter)[2][-1], np_skel_forward(y, num_iter)[2][-1]
    A, B, C, D = (sx * y).sum(), sx.sum(), (sy * x).sum(), sy.sum()
    Bc, Dc = max(B, eps), max(D, eps)
    tp, ts = A / Bc, C / Dc
    S = tp + ts
    Sc = max(S, eps)
    loss = 1.0 - 2.0 * tp * ts / Sc
    dS = -2.0 * tp * ts / Sc ** 2 if S >= eps else 0.0            # clamp(min) passes its gradient iff arg >= min
    dtp, dts = -(2.0 * ts / Sc + dS), -(2.0 * tp / Sc + dS)
    ca, cb = dtp / Bc, (-dtp * A / Bc ** 2 if B >= eps else 0.0)
    grad = dts / Dc * sy + np_skel_bwd(x, num_iter, ca * y + cb)
    if kind == 1:
        num, den = (x * y).sum(), (x * x).sum() + (y * y).sum()
        denc = max(den, eps)
        gd = -2.0 * y / denc + (4.0 * num * x / denc ** 2 if den >= eps else 0.0)
        loss, grad = (1.0 - alpha) * (1.0 - 2.0 * num / denc) + alpha * loss, (1.0 - alpha) * gd + alpha * grad
    if exclude_background:
        out = np.zeros(full)
        out[:, 1:] = grad
        grad = out
    return loss, grad


# ---- fixtures ------------------------------------------------------------------------------------------------------
def test_fixture_is_complete():
    names = case_names()
    g = golden()
    for n in names:
        for f in FIELDS:
            assert f"{n}.{f}" in g.files, (n, f)
        c = load_case(n)
        assert c["x"].shape == c["y"].shape == c["skel_x"].shape == c["grad"].shape
        assert c["x"].dtype == np.float32 and c["grad"].dtype == np.float64 and c["loss"].dtype == np.float64
        assert np.isfinite(c["grad"]).all() and 0 <= float(c["grad32_dev"]) < 1e-5
    dims = {load_case(n)["x"].ndim for n in names}
    assert dims == {4, 5}
    assert {int(load_case(n)["num_iter"]) for n in names} >= {0, 3, 5}
    assert {int(load_case(n)["kind"]) for n in names} == {0, 1}
    assert any(int(load_case(n)["exclude_background"]) and load_case(n)["x"].shape[1] == 3 for n in names)
    assert any(any(s % 2 for s in load_case(n)["x"].shape[2:]) and load_case(n)["x"].shape[-1] % 4 for n in names)
    assert set(TIE_CASES) <= set(names)
    assert os.path.getsize(G13) < 1 << 20


def test_tie_cases_do_have_ties():
    """the quantised and plateau cases exercise the tie rules: many voxels share their value with a neighbour"""
    for n in ("quant3d", "plateau3d", "quant2d", "plateau2d"):
        x = load_case(n)["x"]
        assert float((x == np.roll(x, 1, -1)).mean()) > 0.05, n


@pytest.mark.parametrize("name", case_names())
def test_restated_skeleton_is_bit_equal_to_reference(name):
    c = load_case(name)
    k = int(c["num_iter"])
    assert torch.equal(skel_restate(torch.from_numpy(c["x"]), k), torch.from_numpy(c["skel_x"]))
    assert torch.equal(skel_restate(torch.from_numpy(c["y"]), k), torch.from_numpy(c["skel_y"]))
    # the numpy forward of the hand-written gradient agrees with it in float64
    ref64 = skel_restate(torch.from_numpy(c["x"]).double(), k).numpy()
    assert np.array_equal(np_skel_forward(c["x"].astype(np.float64), k)[2][-1], ref64)


@pytest.mark.parametrize("name", case_names())
def test_restated_loss_matches_reference_float64(name):
    c = load_case(name)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    loss = loss_restate(x, torch.from_numpy(c["y"]).double(), int(c["kind"]), int(c["num_iter"]), float(c["alpha"]),
                        bool(c["exclude_background"]))
    loss.backward()
    assert abs(loss.item() - float(c["loss"])) < 1e-12
    assert np.abs(x.grad.numpy() - c["grad"]).max() <= 1e-12 * max(np.abs(c["grad"]).max(), 1e-30)
    x32 = torch.from_numpy(c["x"])
    l32 = loss_restate(x32, torch.from_numpy(c["y"]), int(c["kind"]), int(c["num_iter"]), float(c["alpha"]),
                       bool(c["exclude_background"]))
    assert abs(float(l32) - float(c["loss32"])) < 1e-6


@pytest.mark.parametrize("name", case_names())
def test_hand_written_gradient_matches_reference(name):
    """gather form + hand-written tie rules == the reference's float64 autograd, to float64 round-off, on every case
    (quantised, plateau and line cases included: a wrong tie rule moves single voxels by O(1) of max |grad|)"""
    c = load_case(name)
    loss, grad = np_loss_and_grad(c["x"], c["y"], int(c["kind"]), int(c["num_iter"]), float(c["alpha"]),
                                  bool(c["exclude_background"]))
    assert abs(loss - float(c["loss"])) < 1e-12
    scale = max(np.abs(c["grad"]).max(), 1e-30)
    assert np.abs(grad - c["grad"]).max() <= 1e-10 * scale, np.abs(grad - c["grad"]).max() / scale


def test_pool_and_min_tie_rules_are_pytorchs():
    """the rules the gather form relies on, observed on this build of torch"""
    x = torch.ones(1, 1, 1, 1, 3, dtype=torch.float64, requires_grad=True)
    F.max_pool3d(x, (1, 1, 3), 1, (0, 0, 1)).sum().backward()
    assert x.grad.flatten().tolist() == [2.0, 1.0, 0.0]
    a, b, c = (torch.ones(1, dtype=torch.float64, requires_grad=True) for _ in range(3))
    torch.min(torch.min(a, b), c).sum().backward()
    assert (float(a.grad), float(b.grad), float(c.grad)) == (0.25, 0.25, 0.5)
    z = torch.zeros(1, requires_grad=True)
    F.relu(z).sum().backward()
    assert float(z.grad) == 0.0
    # and the hand-written pieces agree on an all-equal volume (every voxel a tie)
    e = np.ones((1, 1, 3, 3, 3))
    t = torch.from_numpy(e).requires_grad_(True)
    erode(t).sum().backward()
    assert np.array_equal(np_erode_bwd(e, np.ones_like(e), 3), t.grad.numpy())
    t = torch.from_numpy(e).requires_grad_(True)
    dilate(t).sum().backward()
    assert np.array_equal(np_dilate_bwd(e, np.ones_like(e), 3), t.grad.numpy())
    e2 = np.ones((1, 1, 4, 5))
    t = torch.from_numpy(e2).requires_grad_(True)
    erode(t).sum().backward()
    assert np.array_equal(np_erode_bwd(e2, np.ones_like(e2), 2), t.grad.numpy())


# ---- host-side surface ---------------------------------------------------------------------------------------------
def test_loss_package_exports_the_reference_list():
    import torch_em_amd.loss as L
    for name in ("AffinitySideLoss", "SoftSkeletonize", "cldice_score", "SoftclDiceLoss", "CombinedclDiceLoss",
                 "CombinedLoss", "ContrastiveLoss", "DiceLoss", "dice_score", "SPOCOLoss", "ApplyAndRemoveMask",
                 "ApplyMask", "LossWrapper", "MaskIgnoreLabel", "DistanceLoss", "DiceBasedDistanceLoss"):
        assert hasattr(L, name), name


def test_constructors_and_init_kwargs():
    from torch_em_amd.loss import CombinedclDiceLoss, SoftSkeletonize, SoftclDiceLoss
    assert SoftSkeletonize().num_iter == 5 and SoftSkeletonize(num_iter=2).num_iter == 2
    s = SoftclDiceLoss()
    assert s.init_kwargs == {"num_iter": 5, "eps": 1e-7, "exclude_background": False}
    c = CombinedclDiceLoss()
    assert c.init_kwargs == {"num_iter": 5, "alpha": 0.5, "eps": 1e-7, "exclude_background": False}
    c = CombinedclDiceLoss(3, 0.25, 1e-6, True)
    assert (c.num_iter, c.alpha, c.eps, c.exclude_background) == (3, 0.25, 1e-6, True)
    assert isinstance(c, SoftclDiceLoss)
    again = CombinedclDiceLoss(**c.init_kwargs)
    assert again.init_kwargs == c.init_kwargs
    for m in (SoftSkeletonize(), s, c):
        assert isinstance(m, torch.nn.Module)
    for attr in ("soft_erode", "soft_dilate", "soft_open", "soft_skel", "forward"):
        assert callable(getattr(SoftSkeletonize(), attr))


def test_shape_mismatch_raises_value_error_and_cpu_tensors_runtime_error():
    from torch_em_amd.loss import CombinedclDiceLoss, SoftSkeletonize, SoftclDiceLoss, cldice_score
    x, y = torch.rand(1, 1, 32, 32), torch.rand(1, 2, 32, 32)
    for fn in (CombinedclDiceLoss(), SoftclDiceLoss(), cldice_score):
        with pytest.raises(ValueError, match="same shape"):
            fn(x, y)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SoftSkeletonize()(x)


def test_cldice_c_abi_validates_before_any_hip_call():
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_cldice_ws(2, 2, 1000, 5, 0) == 1024 * 4 * 8
    assert lib.tem_cldice_ws(2, 2, 1000, 5, 1) == 2 * 4000 * 4
    assert lib.tem_cldice_ws(2, 2, 1000, 5, 2) == 11 * 4000 * 4
    assert lib.tem_cldice_ws(2, 2, 1000, 5, 3) == 4 * 4000 * 4
    assert lib.tem_cldice_ws(2, 2, 1000, 5, 9) == -1
    rc = lib.tem_cldice_step(None, 0, 0, 0, None, None, None, None, None, 1, 1, 4, 4, 4, 3, 0, None)
    assert rc == -1 and b"null input" in lib.tem_last_error()
    rc = lib.tem_cldice_step(None, 0, 0, 0, None, None, None, None, None, 1, 1, 4, 4, 4, 2, 0, None)
    assert rc == -1 and b"bad shape" in lib.tem_last_error()
    assert lib.tem_cldice_dilate_bwd(None, 0, 0, 0, None, None, None, 1, 1, 1, 4, 4, 2, None) == -1
    assert lib.tem_cldice_erode_bwd(None, 0, 0, 0, None, None, None, None, None, None, 0, 0, 0, 1, 1, 1, 4, 4, 2, None) == -1
    assert lib.tem_cldice_sums(None, None, None, 0, 0, 0, None, 0, 0, 0, 1, 1, 16, None, 0, None) == -1
    assert lib.tem_cldice_finalize(None, 1e-7, 1, None, None, None, None) == -1
    assert lib.tem_cldice_grad(None, 0, 0, 0, None, None, None, 1, 1, 16, None) == -1
    with pytest.raises(ValueError):
        _lib.check(-1, "tem_cldice_grad")


class _Const(torch.nn.Module):
    def __init__(self, v):
        super().__init__()
        self.v = v

    def forward(self, x, y):
        return (x - y).sum() * 0 + self.v


def test_combined_loss_weights():
    from torch_em_amd.loss import CombinedLoss
    x, y = torch.rand(3), torch.rand(3)
    c = CombinedLoss(_Const(1.0), _Const(3.0))
    assert c.loss_weights == [0.5, 0.5] and float(c(x, y)) == 2.0
    c = CombinedLoss(_Const(1.0), _Const(3.0), loss_weights=[2.0, 1.0])
    assert float(c(x, y)) == 5.0 and len(c.losses) == 2 and isinstance(c.losses, torch.nn.ModuleList)
    with pytest.raises(AssertionError):
        CombinedLoss(_Const(1.0), loss_weights=[1.0, 2.0])
    empty = CombinedLoss()
    assert empty.loss_weights is None
    with pytest.raises(AssertionError):
        empty(x, y)
    m = torch.nn.MSELoss()
    c = CombinedLoss(m, torch.nn.L1Loss(), loss_weights=[0.25, 0.75])
    assert torch.allclose(c(x, y), 0.25 * m(x, y) + 0.75 * (x - y).abs().mean())
