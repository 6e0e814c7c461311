"""GPU: the kernels of csrc/defect.hip op by op, and EMDefectAugmentation on CUDA tensors, against tests/defect_ref.py.

Rules, none of them measured.
  drop, keep, paste, low contrast    equal bits with numpy's float32 expressions; the low-contrast mean is the one the device
                     returned, and that lies within n 2^-24 mean|x| of the float64 mean (float64 accumulation of n terms
                     and one rounding to float32: 2^-24 |mean| + n 2^-53 mean|x| in fact).
  noise planes       the flow kernel with the one weight 1.0 returns noise * strength: equal bits with _philox.py.
  smoothed flow, coefficients    errors in units of 2^-23 x sum |w_y| sum |w_x v| of the element (v: the filtered plane),
                     against scipy's float64 gaussian_filter / spline_filter on the same words / pixels; f32 is the numpy
                     float32 restatement (the same chains of fused multiply-adds, float32 weights) on the same inputs.
  warp               "warp": against scipy's float64 map_coordinates of the DEVICE's coefficients at the DEVICE's flow (the op
                     alone), unit 2^-23 sum |weight * coefficient| (|cval| outside); the kernel forms coordinates, weights and
                     the sum in float64, so coordinates are exact and the unit has no coordinate term.
                     "slice": the finished slice against defect_ref from the same plan and the same words (scipy from the
                     pixels and the noise on), unit 2^-23 (sum |weight * coefficient| + sum |d weight * coefficient| |coordinate|):
                     the float32 flow planes carry a relative coordinate error.  f32: the float32 restatement of the chain.
  every figure       kernel / max(f32, 1) <= 4.
  range ends         pixels whose float64 coordinate lies within 1e-3 of 0 or n - 1 are left out of "slice" (the result jumps
                     to cval there); at most 0.5 % of a slice, asserted; everywhere else inside / outside agree exactly.
  band of compress   exactly 0.
Every op runs twice and returns equal bits; the input is compared with its copy after every call.  No test provokes a fault:
the tables the kernels index with are checked on the host (ops.DefectTables) before they are copied.
Observed on the MI355X: profiles/defect_op_errors.txt.
"""
import functools

import numpy as np
import pytest
import torch

import defect_ref as R
from oracle import gpu_kit as kit
from oracle.gpu_kit import ops as _ops
from oracle.judge import MARGIN
from torch_em_amd.transform import EMDefectAugmentation, get_raw_transform
from torch_em_amd.transform import defect as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# A property of the inputs, computable without a device: under this seed no 5 x 5 slice of the cases below has a pixel within
# 1e-3 of a range end (one pixel would be 4 % of such a slice, against the 0.5 % that may be left out); the largest share
# left out in any slice is 0.1 %.
SEED = 0x1234_5678_9ABC_DEF1
LEDGER = kit.Ledger("DEFECT_ERR")
_note = LEDGER.note
_print_worst = LEDGER.summary_fixture()


# ---------------------------------------------------------------------------------------------------------------- cases
SHAPES = [(32, 32), (33, 33), (40, 40), (24, 40), (5, 5)]
ORDER = [("deform", "undirected"), (D.LOW_CONTRAST,), (D.PASTE,), (D.DROP,), (D.KEEP,), ("deform", "rows"), ("deform", "cols"),
         (D.LOW_CONTRAST,)]
N_ART = 3


def _line(rs, shape, fixed_x):
    H, W = shape
    n = W if fixed_x else H
    a, b = (int(v) for v in rs.randint(1, n - 2, 2))
    return (0, a, H - 1, b) if fixed_x else (a, 0, b, W - 1)


def _plan(shape, S, kind, variant=0):
    """kind "none": no slice deformed; "all": every slice; "each": one of each action, as far as S reaches"""
    rs = np.random.RandomState(1000 * shape[0] + 10 * S + variant)
    square = shape[0] == shape[1]
    actions, deform, artifact = [], [], []
    for s in range(S):
        if kind == "none":
            what = [(D.KEEP,), (D.DROP,), (D.LOW_CONTRAST,), (D.PASTE,)][(s + variant) % 4]
        elif kind == "all":
            what = [("deform", "undirected"), ("deform", "rows"), ("deform", "cols")][(s + variant) % 3]
        else:
            what = ORDER[(s + variant) % len(ORDER)]
        if what[0] == "deform":
            mode = what[1] if square or what[1] != "undirected" else "rows"
            actions.append(D.DEFORM)
            deform.append(("undirected",) if mode == "undirected" else ("compress", mode == "rows", _line(rs, shape, mode == "rows")))
        else:
            actions.append(what[0])
            deform.append(None)
        artifact.append(int(rs.randint(N_ART)) if what[0] == D.PASTE else -1)
    return D.DefectPlan(shape, actions, deform, artifact, SEED)


@functools.lru_cache(maxsize=None)
def _data(shape, S):
    rs = np.random.RandomState(shape[0] * 100 + shape[1] + S)
    x = rs.uniform(-1, 1, (S,) + shape).astype(np.float32)
    art = rs.randn(N_ART, *shape).astype(np.float32)
    alpha = rs.rand(N_ART, *shape).astype(np.float32)
    return x, art, alpha


def _dev(a, off=0):
    """the array on the device; off: its base pointer moved `off` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    return t


class Source:
    def __init__(self, art, alpha):
        self.items = [(torch.from_numpy(a[None]), torch.from_numpy(m[None])) for a, m in zip(art, alpha)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _aug(shape, S, strength=4.0, mean_val=None, **kw):
    _, art, alpha = _data(shape, S)
    return EMDefectAugmentation(0.1, 0.1, 0.3, p_paste_artifact=0.2, contrast_scale=0.3, deformation_mode="all",
                                deformation_strength=strength, artifact_source=Source(art, alpha), mean_val=mean_val, **kw)


def _tables(aug, plan):
    ptab, rec, tables, chosen = aug.plan_tables(plan)
    return _ops().DefectTables(ptab, rec, tables, plan.n_slices, plan.shape[0], plan.shape[1], len(chosen), DEV), rec, chosen


def _twice(fn):
    a = fn()
    b = fn()
    assert torch.equal(a, b), "two runs of one op differ"
    return a.cpu().numpy()


def _units(got, ref, scale):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (2.0 ** -23 * np.maximum(scale, 1e-300))).max())


# ------------------------------------------------------------------------------------------------------- the ops, one by one
def _check_streaming(x, xd, plan, aug, tab, chosen, off):
    ops = _ops()
    S, (H, W) = plan.n_slices, plan.shape
    _, art, alpha = _data(plan.shape, S)
    artd = alphad = None
    if chosen:
        artd, alphad = _dev(art[chosen], off), _dev(alpha[chosen], (off + 2) % 4)
    mean = _twice(lambda: ops.defect_mean(xd, tab))
    y = ops.defect_apply(xd, tab, torch.from_numpy(mean).to(DEV), artd, alphad)
    y2 = ops.defect_apply(xd, tab, torch.from_numpy(mean).to(DEV), artd, alphad)
    keep = [s for s in range(S) if plan.actions[s] != D.DEFORM]
    assert torch.equal(y[keep], y2[keep])
    yh = y.cpu().numpy()
    for s, a in enumerate(plan.actions):
        if a == D.LOW_CONTRAST:
            m64 = x[s].astype(np.float64).mean()
            bound = H * W * 2.0 ** -24 * np.abs(x[s].astype(np.float64)).mean()
            print(f"mean {plan.shape} slice {s}: device {mean[s]!r} float64 {m64!r} |diff| {abs(mean[s] - m64):.3e} bound {bound:.3e}")
            assert abs(float(mean[s]) - m64) <= bound
            assert yh[s].tobytes() == R.low_contrast(x[s], mean[s], aug.contrast_scale).tobytes()
        else:
            assert mean[s] == 0
        if a == D.KEEP:
            assert yh[s].tobytes() == x[s].tobytes()
        elif a == D.DROP:
            assert not yh[s].any() and not np.signbit(yh[s]).any()
        elif a == D.PASTE:
            k = plan.artifact[s]
            want = x[s] * (np.float32(1.) - alpha[k]) + art[k] * alpha[k]
            assert want.dtype == np.float32 and yh[s].tobytes() == want.tobytes() == R.paste(x[s], art[k], alpha[k]).tobytes()
    return y


def _check_deformed(x, xd, y, plan, aug, tab, rec):
    ops = _ops()
    S, shape = plan.n_slices, plan.shape
    strength = np.float32(aug.deformation_strength)
    gw, sw = D.gaussian_weights(), D.spline_fir_weights()
    fill = 0.0 if aug.mean_val is None else aug.mean_val      # of a compressed slice; an undirected warp fills with 0
    # coefficients
    coef = _twice(lambda: ops.defect_prefilter(xd, tab, sw))
    coefd = torch.from_numpy(coef).to(DEV)
    for d, s in enumerate(plan.deformed):
        ref = R.coefficients(x[s])
        scale = R.separable_scale(x[s], sw, "mirror")
        ek = _units(coef[d], ref, scale)
        e32 = _units(R.separable(x[s], sw, "mirror", np.float32), ref, scale)
        assert _note("prefilter", "coefficients", ek, e32) <= MARGIN, (shape, s, ek, e32)
    # noise and flow
    und = [d for d, s in enumerate(plan.deformed) if plan.deform[s][0] == "undirected"]
    flowd = torch.zeros((tab.D, 2) + shape, dtype=torch.float32, device=DEV)
    if und:
        noise = _twice(lambda: ops.defect_flow(tab, SEED, float(strength), [1.0], out=torch.zeros_like(flowd)))
        flow = _twice(lambda: ops.defect_flow(tab, SEED, float(strength), gw, out=torch.zeros_like(flowd)))
        flowd = torch.from_numpy(flow).to(DEV)
        for d, s in enumerate(plan.deformed):
            if d not in und:
                assert not noise[d].any() and not flow[d].any()     # compress records are skipped
                continue
            for f in (0, 1):
                n32 = R.noise_plane(SEED, D.stream_row(s, f), shape, np.float32)
                assert n32.dtype == np.float32 and noise[d, f].tobytes() == (n32 * strength).tobytes()
                v64 = R.noise_plane(SEED, D.stream_row(s, f), shape) * float(strength)
                ref, scale = R.smooth(v64), R.separable_scale(v64, gw, "clamp")
                ek = _units(flow[d, f], ref, scale)
                e32 = _units(R.separable(n32 * strength, gw, "clamp", np.float32), ref, scale)
                assert _note("flow", "smoothed plane", ek, e32) <= MARGIN, (shape, s, f, ek, e32)
    # warp
    before = y.clone()
    out = _twice(lambda: ops.defect_warp(coefd, flowd, before.clone(), tab, SEED, float(aug.deformation_strength) / 8.))
    untouched = [s for s in range(S) if plan.actions[s] != D.DEFORM]
    assert out[untouched].tobytes() == before[untouched].cpu().numpy().tobytes()
    rr, cc = np.mgrid[:shape[0], :shape[1]]
    for d, s in enumerate(plan.deformed):
        zero, cval = np.zeros(shape, bool), (0.0 if plan.deform[s][0] == "undirected" else fill)
        if plan.deform[s][0] == "undirected":
            at_r, at_c = R.undirected_coordinates(shape, flowd[d, 0].cpu().numpy(), flowd[d, 1].cpu().numpy())
            n64 = [R.noise_plane(SEED, D.stream_row(s, f), shape) for f in (0, 1)]
            ref_r, ref_c = R.undirected_coordinates(shape, R.smooth(n64[0] * float(strength)), R.smooth(n64[1] * float(strength)))
            n32 = [R.noise_plane(SEED, D.stream_row(s, f), shape, np.float32) * strength for f in (0, 1)]
            r32_r, r32_c = R.undirected_coordinates(shape, R.separable(n32[0], gw, "clamp", np.float32), R.separable(n32[1], gw, "clamp", np.float32))
        else:
            _, fixed_x, ends = plan.deform[s]
            n64 = [R.noise_plane(SEED, D.stream_row(s, f), shape) for f in (0, 1)]
            at_r, at_c, zero = R.compress_coordinates(shape, fixed_x, ends, aug.deformation_strength, n64[0], n64[1])
            ref_r, ref_c, r32_r, r32_c = at_r, at_c, at_r, at_c
        assert not out[s][zero].any(), "the band of a compress line is zero"
        live = ~zero
        # the op alone: scipy at the device's coefficients and coordinates
        want = R.warp(None, at_r, at_c, cval, coef=coef[d])
        hand, scale, _ = R.hand_warp(coef[d], at_r, at_c, cval, np.float32, return_scale=True)
        inside = (at_r >= 0) & (at_r <= shape[0] - 1) & (at_c >= 0) & (at_c <= shape[1] - 1)
        assert (out[s][live & ~inside] == np.float32(cval)).all()
        if (live & inside).any():
            m = live & inside
            ek, e32 = _units(out[s][m], want[m], scale[m]), _units(hand[m], want[m], scale[m])
            assert _note("warp", plan.deform[s][0], ek, e32) <= MARGIN, (shape, s, ek, e32)
        # the finished slice: defect_ref from the plan and the words
        near = R.near_range_end(ref_r, ref_c, shape) & live
        assert near.mean() <= 0.005, (shape, s, float(near.mean()))
        cmp = live & ~near
        ref_in = (ref_r >= 0) & (ref_r <= shape[0] - 1) & (ref_c >= 0) & (ref_c <= shape[1] - 1)
        assert (inside[cmp] == ref_in[cmp]).all(), "inside / outside differs away from the ends of the range"
        want = R.warp(x[s], ref_r, ref_c, cval)
        _, scale, slope = R.hand_warp(R.coefficients(x[s]), ref_r, ref_c, cval, return_scale=True)
        chain = R.hand_warp(R.separable(x[s], sw, "mirror", np.float32), r32_r, r32_c, cval, np.float32)
        m = cmp & ref_in
        if m.any():
            ek, e32 = _units(out[s][m], want[m], (scale + slope)[m]), _units(chain[m], want[m], (scale + slope)[m])
            assert _note("slice", plan.deform[s][0], ek, e32) <= MARGIN, (shape, s, ek, e32)
    return out


# off = 1: the base pointer of the slices sits 4 bytes past a 16-byte boundary
CASES = [(shape, S, kind, 0) for shape in SHAPES for S in (1, 3, 8) for kind in ("none", "all", "each")] \
    + [(shape, 3, kind, 1) for shape in SHAPES for kind in ("none", "each")]


@pytest.mark.parametrize("shape,S,kind,off", CASES)
def test_ops_one_by_one(shape, S, kind, off):
    x, _, _ = _data(shape, S)
    for strength, mean_val in ((4.0, None), (10.0, 0.5)) if kind != "none" else ((4.0, None),):
        aug = _aug(shape, S, strength, mean_val)
        plan = _plan(shape, S, kind)
        tab, rec, chosen = _tables(aug, plan)
        xd = _dev(x, off)
        y = _check_streaming(x, xd, plan, aug, tab, chosen, off)
        if plan.deformed:
            out = _check_deformed(x, xd, y, plan, aug, tab, rec)
            # the class gives the same bits as the ops in sequence
            assert aug.apply_plan(xd, plan).cpu().numpy().tobytes() == out.tobytes()
        else:
            assert torch.equal(aug.apply_plan(xd, plan), y)
        assert xd.cpu().numpy().tobytes() == x.tobytes(), "the input changed"


# ------------------------------------------------------------------------------------------------------- whole calls
def test_no_deformed_slice_launches_no_warp_kernels(monkeypatch):
    shape, S = (33, 33), 8
    x, _, _ = _data(shape, S)
    aug, plan = _aug(shape, S), _plan(shape, S, "none")
    calls = []
    for name in ("defect_prefilter", "defect_flow", "defect_warp"):
        monkeypatch.setattr(_ops(), name, lambda *a, _n=name, **k: calls.append(_n))
    xd = _dev(x)
    y = aug.apply_plan(xd, plan).cpu().numpy()
    assert not calls
    monkeypatch.undo()
    tab, _, chosen = _tables(aug, plan)
    assert y.tobytes() == _check_streaming(x, xd, plan, aug, tab, chosen, 0).cpu().numpy().tobytes()


@pytest.mark.parametrize("shape", [(32, 32), (24, 40)])
def test_a_slice_does_not_depend_on_the_other_slices(shape):
    S = 8
    x, _, _ = _data(shape, S)
    xd = _dev(x)
    aug = _aug(shape, S, 10.0)
    a, b = _plan(shape, S, "each", 0), _plan(shape, S, "all", 1)
    ya, yb = aug.apply_plan(xd, a).cpu().numpy(), aug.apply_plan(xd, b).cpu().numpy()
    # give slice s of plan b the action of plan a, keep everything else of b
    for s in range(S):
        c = D.DefectPlan(shape, list(b.actions), list(b.deform), list(b.artifact), SEED)
        c.actions[s], c.deform[s], c.artifact[s] = a.actions[s], a.deform[s], a.artifact[s]
        yc = aug.apply_plan(xd, c).cpu().numpy()
        assert yc[s].tobytes() == ya[s].tobytes(), s
        rest = [t for t in range(S) if t != s]
        assert yc[rest].tobytes() == yb[rest].tobytes(), s
    assert xd.cpu().numpy().tobytes() == x.tobytes()


def test_per_sample_equals_the_flat_batch():
    shape, N, Z = (32, 32), 2, 4
    x, _, _ = _data(shape, N * Z)
    aug, flat = _aug(shape, N * Z, per_sample=True), _aug(shape, N * Z)
    plan = _plan(shape, N * Z, "each")
    want = flat.apply_plan(_dev(x), plan).cpu().numpy()
    for view in ((N, Z) + shape, (N, 1, Z) + shape):
        got = aug.apply_plan(_dev(x.reshape(view)), plan)
        assert tuple(got.shape) == view and got.cpu().numpy().tobytes() == want.tobytes()
    np.random.seed(3)
    a = aug(_dev(x.reshape((N, Z) + shape)))
    np.random.seed(3)
    b = aug.apply_plan(_dev(x.reshape((N, Z) + shape)), aug.sample_plan(N * Z, shape))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        flat(_dev(x.reshape((N, Z) + shape)))


@pytest.mark.parametrize("mode,shape", [("undirected", (32, 32)), ("compress", (24, 40)), ("all", (40, 40))])
def test_call_is_sample_plan_then_apply_plan(mode, shape):
    Z = 8
    x, art, alpha = _data(shape, Z)
    aug = EMDefectAugmentation(0.15, 0.15, 0.4, p_paste_artifact=0.2, deformation_mode=mode, deformation_strength=10.0,
                               artifact_source=Source(art, alpha), mean_val=0.25)
    xd = _dev(x)
    np.random.seed(11)
    y = aug(xd)
    after = np.random.rand()
    np.random.seed(11)
    plan = aug.sample_plan(Z, shape)
    assert after == np.random.rand()
    assert torch.equal(y, aug.apply_plan(xd, plan)) and torch.equal(y, aug.apply_plan(xd, plan, plan.seed))
    assert y.dtype == torch.float32 and y.shape == xd.shape and xd.cpu().numpy().tobytes() == x.tobytes()
    assert len(set(plan.actions)) >= 3 and plan.deformed
    if plan.seed is not None:
        other = aug.apply_plan(xd, plan, plan.seed + 1)
        d = plan.deformed
        assert not torch.equal(other[d], y[d])
    # against the oracle, loosely: the whole call does what the reference's class does (the figures are judged above)
    noise = {s: tuple(R.noise_plane(plan.seed, D.stream_row(s, f), shape) for f in (0, 1)) for s in plan.deformed}
    means = {s: x[s].astype(np.float64).mean() for s, a in enumerate(plan.actions) if a == D.LOW_CONTRAST}
    ref = R.defect_ref(x, plan, noise, np.float32(10.0), aug.contrast_scale, 0.25, means, list(zip(art, alpha)))
    yh = y.cpu().numpy()
    bad = np.abs(yh - ref) > 1e-4
    assert bad.mean() <= 0.005     # the range-end pixels may jump to cval


def test_raw_transform_and_prefetcher():
    from torch_em_amd.trainer.input_pipeline import DevicePrefetcher
    shape, Z = (32, 32), 8
    x, art, alpha = _data(shape, Z)
    aug = EMDefectAugmentation(0.1, 0.2, 0.5, deformation_mode="all", deformation_strength=4.0)
    np.random.seed(1)
    y = get_raw_transform(augmentation1=aug)(_dev(x))
    assert y.is_cuda and y.shape == (Z,) + shape and bool(torch.isfinite(y).all())
    batch = EMDefectAugmentation(0.1, 0.2, 0.5, deformation_mode="all", deformation_strength=4.0, per_sample=True)
    xs = [torch.from_numpy(x.reshape(2, 1, 4, *shape)).clone() for _ in range(2)]
    loader = [(b, torch.zeros(2, 1, 4, *shape)) for b in xs]
    np.random.seed(2)
    got = [bx.clone() for bx, _ in DevicePrefetcher(loader, DEV, prepass=lambda bx, by: (batch(bx), by))]
    torch.cuda.synchronize()
    np.random.seed(2)
    want = [batch(b.to(DEV)) for b in xs]
    assert len(got) == 2 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert not torch.equal(got[0], got[1])


def test_refusals():
    ops = _ops()
    aug = _aug((32, 32), 3)
    with pytest.raises(RuntimeError):
        aug(torch.zeros(3, 32, 32))
    with pytest.raises(ValueError):
        aug(torch.zeros(3, 3, 3, device=DEV))
    with pytest.raises(ValueError):
        aug(torch.zeros(2, 3, 32, 32, device=DEV))
    plan = _plan((32, 32), 3, "all")
    with pytest.raises(ValueError):
        aug.apply_plan(torch.zeros(4, 32, 32, device=DEV), plan)
    ptab, rec, tables, chosen = aug.plan_tables(_plan((32, 32), 3, "each"))
    bad = rec.copy()
    bad[0, 0] = 7
    with pytest.raises(ValueError):
        ops.DefectTables(ptab, bad, tables, 3, 32, 32, len(chosen), DEV)
    bad = ptab.copy()
    bad[2, 1] = 5
    with pytest.raises(ValueError):
        ops.DefectTables(bad, rec, tables, 3, 32, 32, len(chosen), DEV)
    cplan = _plan((32, 32), 3, "all")
    ptab, rec, tables, chosen = aug.plan_tables(cplan)
    with pytest.raises(ValueError):
        ops.DefectTables(ptab, rec, tables[:-1], 3, 32, 32, 0, DEV)
    bad = tables.copy()
    bad[0] = 40 | (41 << 16)
    with pytest.raises(ValueError):
        ops.DefectTables(ptab, rec, bad, 3, 32, 32, 0, DEV)
    tab = ops.DefectTables(ptab, rec, tables, 3, 32, 32, 0, DEV)
    with pytest.raises(ValueError):
        ops.defect_flow(tab, SEED, 4.0, [1.0] * 35)
    with pytest.raises(ValueError):
        ops.defect_mean(torch.zeros(3, 32, 33, device=DEV), tab)
