"""CPU: the numpy branch of EMDefectAugmentation and the oracle tests/defect_ref.py against the fixture recorded from the
reference's class (tests/golden/gen_golden_defect.py), and the host geometry (line, interval table, band, filter weights)
against scipy."""
import importlib.util
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import defect_ref as R
from conftest import GOLDEN
from torch_em_amd.transform import EMDefectAugmentation
from torch_em_amd.transform import defect as D

_spec = importlib.util.spec_from_file_location("gen_golden_defect", os.path.join(GOLDEN, "gen_golden_defect.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)


@pytest.fixture(scope="module")
def fx():
    return np.load(GEN.FIXTURE)


def _aug(name, fx):
    shape, seed, kwargs = GEN.RUNS[name]
    kwargs = dict(kwargs)
    if kwargs.get("p_paste_artifact"):
        kwargs["artifact_source"] = GEN.make_artifacts(shape[1:])
    return EMDefectAugmentation(**kwargs), shape, seed, kwargs


def _replay(monkeypatch, fx, name):
    """the recorded scalar draws in place of numpy's: `sample_plan` must consume exactly these, in this order"""
    rp = R.Replay(fx[f"{name}_rand"], fx[f"{name}_randint"])
    monkeypatch.setattr(np.random, "rand", rp.rand)
    monkeypatch.setattr(np.random, "randint", rp.randint)
    return rp


@pytest.mark.parametrize("name", list(GEN.RUNS))
def test_numpy_branch_equals_the_reference(fx, name):
    """same seed -> the reference's output bit for bit (the same scipy calls on the same draws in the same order)"""
    aug, shape, seed, _ = _aug(name, fx)
    x = fx[f"{name}_x"]
    np.random.seed(seed)
    y = aug(x.copy())
    assert y.dtype == np.float32 and y.tobytes() == fx[f"{name}_out"].tobytes()
    assert (x == fx[f"{name}_x"]).all()
    assert (y != x).any()


@pytest.mark.parametrize("name", list(GEN.RUNS))
def test_sample_plan_consumes_the_stream_in_the_documented_order(fx, name, monkeypatch):
    """per slice r, the coin of mode "all", rand / randint / randint of a compress line, the artifact index -- exactly the
    reference's scalar draws in its order, and one seed at the end iff a slice deforms"""
    aug, shape, seed, _ = _aug(name, fx)
    rp = _replay(monkeypatch, fx, name)
    plan = aug.sample_plan(shape[0], shape[1:])
    assert rp.done()
    assert (plan.seed is not None) == bool(plan.deformed)
    planes = sum(2 for s in plan.deformed)
    assert planes == len(fx[f"{name}_uniform"])
    changed = (fx[f"{name}_out"] != fx[f"{name}_x"]).reshape(shape[0], -1).any(1)
    assert [a != D.KEEP for a in plan.actions] == changed.tolist()


def test_sample_plan_draws_from_numpys_global_state():
    aug = EMDefectAugmentation(0.1, 0.1, 0.5, deformation_mode="all")
    np.random.seed(5)
    p1 = aug.sample_plan(12, (32, 32))
    after = np.random.rand()
    np.random.seed(5)
    p2 = aug.sample_plan(12, (32, 32))
    assert p1.actions == p2.actions and p1.deform == p2.deform and p1.seed == p2.seed and after == np.random.rand()
    assert {d[0] for d in p1.deform if d} == {"undirected", "compress"}


@pytest.mark.parametrize("name", list(GEN.RUNS))
def test_oracle_equals_the_reference(fx, name, monkeypatch):
    """float32(defect_ref(...)) from the recorded draws equals the fixture bit for bit"""
    aug, shape, seed, kwargs = _aug(name, fx)
    _replay(monkeypatch, fx, name)
    plan = aug.sample_plan(shape[0], shape[1:])
    monkeypatch.undo()
    x = fx[f"{name}_x"]
    planes = list(fx[f"{name}_uniform"])
    noise = {s: (planes.pop(0), planes.pop(0)) for s in plan.deformed}
    means = {s: x[s].mean() for s, a in enumerate(plan.actions) if a == D.LOW_CONTRAST}
    arts = list(zip(fx[f"{name}_artifacts"], fx[f"{name}_alphas"])) if f"{name}_artifacts" in fx else None
    y = R.defect_ref(x, plan, noise, kwargs["deformation_strength"], kwargs.get("contrast_scale", 0.1), kwargs.get("mean_val"),
                     means, arts)
    assert y.dtype == np.float64 and y.astype(np.float32).tobytes() == fx[f"{name}_out"].tobytes()


def test_fixture_covers_every_action(fx, monkeypatch):
    seen, modes = set(), set()
    for name in GEN.RUNS:
        aug, shape, _, _ = _aug(name, fx)
        _replay(monkeypatch, fx, name)
        plan = aug.sample_plan(shape[0], shape[1:])
        monkeypatch.undo()
        seen |= set(plan.actions)
        modes |= {(d[0], d[1] if len(d) > 1 else None) for d in plan.deform if d}
    assert seen == {D.KEEP, D.DROP, D.LOW_CONTRAST, D.DEFORM, D.PASTE}
    assert {m[0] for m in modes} == {"undirected", "compress"}


def test_hand_formula_agrees_with_scipy():
    """mirror coefficients, B-spline weights and the range test reproduce map_coordinates(order=3, mode="constant") in
    float64 to 1e-12 relative, in and out of range and at the ends of the range"""
    rs = np.random.RandomState(0)
    for shape in ((32, 32), (24, 40), (5, 5), (4, 7)):
        x = rs.randn(*shape)
        at_r = rs.uniform(-1.5, shape[0] + 0.5, 400)
        at_c = rs.uniform(-1.5, shape[1] + 0.5, 400)
        at_r[:8] = [0, shape[0] - 1, 0.5, shape[0] - 1, 0, 1e-9, shape[0] - 1 - 1e-9, 2]
        at_c[:8] = [0, shape[1] - 1, shape[1] - 1, 0.25, 3, 2, 1, shape[1] - 1]
        for cval in (0.0, 0.5):
            want = R.warp(x, at_r, at_c, cval)
            got = R.hand_warp(R.coefficients(x), at_r, at_c, cval)
            inside = (at_r >= 0) & (at_r <= shape[0] - 1) & (at_c >= 0) & (at_c <= shape[1] - 1)
            assert inside.sum() > 40 and (~inside).sum() > 20
            assert (got[~inside] == cval).all() and (want[~inside] == cval).all()
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _lines(shape):
    H, W = shape
    for fixed_x in (True, False):
        n = W if fixed_x else H
        for a in range(1, n - 2):
            for b in range(1, n - 2):
                yield fixed_x, ((0, a, H - 1, b) if fixed_x else (a, 0, b, W - 1))


def _fixture_lines(fx, monkeypatch):
    for name in GEN.RUNS:
        aug, shape, _, _ = _aug(name, fx)
        _replay(monkeypatch, fx, name)
        plan = aug.sample_plan(shape[0], shape[1:])
        monkeypatch.undo()
        for d in plan.deform:
            if d and d[0] == "compress":
                yield shape[1:], d[1], d[2]


def _check_line(shape, fixed_x, ends):
    rr, cc = D.line(*ends)
    mask = np.zeros(shape, bool)
    mask[rr, cc] = True
    assert (rr[0], cc[0], rr[-1], cc[-1]) == ends and mask.sum() == len(rr)
    lab, n = ndi.label(~mask)
    assert n == 2
    neg, pos = (lab[0, 0], lab[-1, -1]) if fixed_x else (lab[-1, -1], lab[0, 0])
    lo, hi = D.line_intervals(rr, cc, shape, fixed_x)
    assert (D.sides(lo, hi, shape, fixed_x) == (lab == pos).astype(int) - (lab == neg).astype(int)).all()
    assert (D.band(lo, hi, shape, fixed_x) == ndi.binary_dilation(mask, iterations=10)).all()
    assert (D.band(lo, hi, shape, fixed_x, 2) == ndi.binary_dilation(mask, iterations=2)).all()


def test_interval_table_and_band_on_the_fixture_lines(fx, monkeypatch):
    lines = list(_fixture_lines(fx, monkeypatch))
    assert len(lines) >= 4 and {l[1] for l in lines} == {True, False}
    for shape, fixed_x, ends in lines:
        _check_line(tuple(shape), fixed_x, ends)


@pytest.mark.parametrize("shape", [(8, 8), (8, 12), (12, 8)])
def test_interval_table_and_band_exhaustively(shape):
    """every line the reference can draw at this shape, both orientations: sides equal scipy.ndimage.label's components, the
    closed-form diamond equals binary_dilation"""
    n = 0
    for fixed_x, ends in _lines(shape):
        _check_line(shape, fixed_x, ends)
        n += 1
    assert n == (shape[1] - 3) ** 2 + (shape[0] - 3) ** 2


def test_line_is_symmetric_under_endpoint_swap():
    rs = np.random.RandomState(1)
    for _ in range(300):
        r0, c0, r1, c1 = (int(v) for v in rs.randint(0, 40, 4))
        rr, cc = D.line(r0, c0, r1, c1)
        r2, c2 = D.line(r1, c1, r0, c0)
        assert (rr[::-1] == r2).all() and (cc[::-1] == c2).all()
        assert (rr[0], cc[0], rr[-1], cc[-1]) == (r0, c0, r1, c1) and len(rr) == max(abs(r1 - r0), abs(c1 - c0)) + 1
        assert (np.abs(np.diff(rr)) <= 1).all() and (np.abs(np.diff(cc)) <= 1).all()
        # no pixel is farther than half a pixel from the ideal line along the minor axis
        if abs(r1 - r0) >= abs(c1 - c0) and r1 != r0:
            assert (np.abs(cc - (c0 + (rr - r0) * (c1 - c0) / (r1 - r0))) <= 0.5 + 1e-12).all()


@pytest.mark.parametrize("n", [4, 5, 7, 32, 33])
def test_fir_prefilter_equals_spline_filter(n):
    """The truncated two-sided impulse response on the mirrored signal equals scipy's recursion.  Bound: the dropped taps
    sum to 2 sqrt(3) |z|^17 / (1 - |z|) = 9.0e-10 per pass and unit of max |x|; the pass along H sees values up to 3 max |x|
    (the filter's gain sum |h| = 3): 4 * 9.0e-10 = 3.6e-9 max |x| in all."""
    x = np.random.RandomState(n).randn(n, n + 3)
    got = R.separable(x, D.spline_fir_weights().astype(np.float64), "mirror")
    # separable() rounds the weights to float32 as the kernels do; here the float64 weights are wanted
    w = D.spline_fir_weights()
    g = x
    for axis in (1, 0):
        idx = R._index(g.shape[axis], len(w) // 2, "mirror")
        g = np.moveaxis((np.moveaxis(g, axis, -1)[..., idx] * w).sum(-1), -1, axis)
    want = ndi.spline_filter(x, order=3, mode="mirror", output=np.float64)
    z = abs(D.SPLINE_POLE)
    bound = 4 * 2 * np.sqrt(3) * z ** 17 / (1 - z) * np.abs(x).max()
    assert np.abs(g - want).max() <= bound
    assert np.abs(got - want).max() <= bound + 3 * 2.0 ** -24 * 3 * np.abs(x).max()   # + the float32 rounding of the weights
    assert len(w) == 33 and abs(w.sum() - 1.0) < 1e-9


def test_gaussian_weights_are_scipys():
    w = D.gaussian_weights()
    assert len(w) == 25
    x = np.zeros(61)
    x[30] = 1.0
    assert np.abs(ndi.gaussian_filter(x, sigma=3.0, mode="nearest", truncate=4.0)[18:43] - w[::-1]).max() < 1e-17


def test_f32_restatement_of_the_filters_is_close():
    rs = np.random.RandomState(3)
    x = rs.uniform(-1, 1, (33, 40))
    for w, border, ref in ((D.gaussian_weights(), "clamp", R.smooth(x)), (D.spline_fir_weights(), "mirror", R.coefficients(x))):
        got = R.separable(x.astype(np.float32), w, border, np.float32)
        unit = 2.0 ** -23 * R.separable_scale(x.astype(np.float32), w, border)
        assert got.dtype == np.float32 and (np.abs(got - (ref if border == "clamp" else R.coefficients(x.astype(np.float32)))) / unit).max() < 8


def test_arguments_and_scope():
    with pytest.raises(AssertionError):
        EMDefectAugmentation(0.5, 0.3, 0.3)
    with pytest.raises(AssertionError):
        EMDefectAugmentation(0.1, 0.1, 0.1, p_paste_artifact=0.1)
    with pytest.raises(AssertionError):
        EMDefectAugmentation(0.1, 0.1, 0.1, deformation_mode="shear")
    assert EMDefectAugmentation(0.1, 0.1, 0.1, deformation_mode=["compress", "undirected"]).deformation_mode == "all"
    aug = EMDefectAugmentation(0.0, 0.0, 0.99, deformation_mode="undirected")
    with pytest.raises(ValueError):
        aug(np.zeros((2, 8, 12), np.float32))
    with pytest.raises(ValueError):
        aug.sample_plan(2, (8, 12))
    with pytest.raises(ValueError):
        aug.sample_plan(2, (3, 3))
    assert EMDefectAugmentation(0.0, 0.0, 0.99, deformation_mode="compress").sample_plan(2, (8, 12)).deformed == [0, 1]
    import torch_em_amd.transform.defect as mod
    assert not hasattr(mod, "get_artifact_source")


def test_plan_tables():
    from torch_em_amd import ops
    aug = EMDefectAugmentation(0.2, 0.2, 0.4, deformation_mode="compress", deformation_strength=4.0, mean_val=0.5, contrast_scale=0.3)
    np.random.seed(2)
    plan = aug.sample_plan(16, (24, 40))
    ptab, rec, tables, chosen = aug.plan_tables(plan)
    assert ptab.shape == (16, 4) and rec.shape == (len(plan.deformed), 8) and not chosen
    assert (ptab[:, 2].view(np.float32) == np.float32(0.3)).all()
    assert sorted(set(ptab[:, 0])) == [ops.DEFECT_KEEP, ops.DEFECT_DROP, ops.DEFECT_LOW, ops.DEFECT_DEFORM]
    for d, s in enumerate(plan.deformed):
        _, fixed_x, ends = plan.deform[s]
        n = 24 if fixed_x else 40
        t = tables[rec[d, 2]:rec[d, 2] + n]
        lo, hi = D.line_intervals(*D.line(*ends), (24, 40), fixed_x)
        assert rec[d, 0] == s and rec[d, 1] == (1 if fixed_x else 2) and rec[d, 3] == 2 * s
        assert ((t & 0xffff) == lo).all() and ((t >> 16) == hi).all()
        assert rec.view(np.float32)[d, 6] == np.float32(0.5)
    assert len(tables) == sum(24 if plan.deform[s][1] else 40 for s in plan.deformed)
