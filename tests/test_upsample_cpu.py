"""CPU: the float64 oracle of the upsample kernels (oracle/upsample_ref.py) against torch float64, its judge against
deliberately wrong outputs, and the arithmetic of the case tables (oracle/upsample_cases.py).  No GPU.

E32_LIMIT / E32_LIMIT_FACTOR3: the numpy float32 restatement stays below these figures, in units of 2^-23 x the
per-element scale, on every case of the tables.  This run, factors 1 and 2 (exact weights 0.25 / 0.75): forward 1.84, adjoint
1.60, bwd_norm 2.05, sum y 3.56, sum y^2 11.18 (the 560-term sequential chain of f5), sums from u 1.33 / 2.08.  Factor 3
(1 / 3 and the source index are rounded; the worse of the separately rounded and the fused evaluation, upsample_ref._src32):
forward 16.87, adjoint 3.47, bwd_norm 3.01, sum y 2.23, sum y^2 3.17, sums from u 1.46 / 1.10.  So the bound
MARGIN * max(e32, 1) of tests/test_gpu_upsample.py has room for the reference and no case loosens it unnoticed.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import upsample_cases as K
from oracle import upsample_ref as R

E32_LIMIT = {"forward": 2.0, "adjoint": 1.75, "bwd_norm": 2.25, "sum y": 4.0, "sum y^2": 12.0, "u sum y": 1.5, "u sum y^2": 2.25}
E32_LIMIT_FACTOR3 = {"forward": 18.0, "adjoint": 3.75, "bwd_norm": 3.25, "sum y": 2.5, "sum y^2": 3.5, "u sum y": 1.6, "u sum y^2": 1.25}

FACTORS = [(2, 2, 2), (1, 2, 2), (1, 3, 3), (3, 1, 2)]
SHAPES = [(2, 3, 4, 5, 3), (1, 1, 1, 1, 2), (1, 1, 5, 1, 4), (2, 4, 1, 3, 1)]


def _ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 4, 1, 2, 3)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


def _interp(x, f):
    return F.interpolate(x, scale_factor=tuple(float(v) for v in f), mode="trilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ the oracle against torch
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_adjoint_against_torch_float64(shape, f):
    rng = np.random.RandomState(sum(shape) + 10 * sum(f))
    x, g = rng.randn(*shape), rng.randn(*K.fine(shape, f))
    xt = _ncdhw(x).requires_grad_(True)
    yt = _interp(xt, f)
    gxt, = torch.autograd.grad(yt, xt, _ncdhw(g))
    y, gx = R.forward_f64(x, f), R.adjoint_f64(g, f)
    assert y.shape == K.fine(shape, f) and gx.shape == shape
    assert np.abs(y - _cl(yt.detach())).max() <= 1e-14 * max(1.0, np.abs(y).max())
    assert np.abs(gx - _cl(gxt)).max() <= 1e-14 * max(1.0, np.abs(gx).max())
    S = R.ones_adjoint_f64(shape, f)
    assert np.abs(R.adjoint_f64(np.ones(K.fine(shape, f)), f) - S).max() <= 1e-14 * S.max()
    # <U x, g> = <x, U^T g>
    assert abs((y * g).sum() - (x * gx).sum()) <= 1e-12 * (np.abs(y) * np.abs(g)).sum()


@pytest.mark.parametrize("f", FACTORS)
def test_bwd_norm_against_autograd_of_its_definition(f):
    shape = (2, 3, 4, 5, 3)
    rng = np.random.RandomState(5 + sum(f))
    u, g, coef = rng.randn(*shape), rng.randn(*K.fine(shape, f)), K.make_coef(shape[0], shape[4], 9).astype(np.float64)
    ut = _ncdhw(u).requires_grad_(True)
    yt = _interp(ut, f)
    a, m1, m2r, mean = (torch.from_numpy(coef[:, :, k])[:, :, None, None, None] for k in range(4))
    h = (a * _ncdhw(g) - m1 - (yt - mean) * m2r).detach()                 # the norm backward of the fine tensors ...
    want, = torch.autograd.grad((h * yt).sum(), ut)                          # ... through U^T
    got = R.bwd_norm_f64(g, u, coef, f)
    assert np.abs(got - _cl(want)).max() <= 1e-14 * np.abs(got).max()
    scale = R.bwd_norm_scale(g, u, coef, f)
    assert (scale >= np.abs(got) * (1 - 1e-12)).all(), "the scale bounds the value"
    # the forms the large cases use: U^T U per axis on the coarse tensor, and the result by linearity from U^T g
    assert np.abs(R.gram_f64(u, f) - R.adjoint_f64(R.forward_f64(u, f), f)).max() <= 1e-14 * np.abs(u).max()
    assert np.abs(R.bwd_norm_linear_f64(R.adjoint_f64(g, f), u, coef, f) - got).max() <= 1e-14 * scale.max()
    assert np.array_equal(R.bwd_norm_scale(g, u, coef, f, adj_scale=R.adjoint_scale(g, f)), scale)
    assert np.array_equal(R.bwd_norm_f32(g, u, coef, f, adj=R.adjoint_f32(g, f)), R.bwd_norm_f32(g, u, coef, f))


@pytest.mark.parametrize("f", FACTORS)
def test_row_stats_against_direct_sums(f):
    shape = (2, 3, 4, 5, 3)
    N, D, H, W, C = shape
    y = np.random.RandomState(3).randn(*K.fine(shape, f))
    got = R.row_stats_f64(y, f)
    assert got.shape == (N, D * H, C, 2)
    for n in range(N):
        for z in range(D):
            for r in range(H):
                blk = y[n, z * f[0]:(z + 1) * f[0], r * f[1]:(r + 1) * f[1]].reshape(-1, C)
                assert np.allclose(got[n, z * H + r, :, 0], blk.sum(0), rtol=1e-13, atol=1e-13)
                assert np.allclose(got[n, z * H + r, :, 1], (blk * blk).sum(0), rtol=1e-13, atol=0)
    # the sums from u alone: another partition of the same totals
    u = np.random.RandomState(4).randn(*shape)
    a, b = R.u_row_stats_f64(u, f).sum(axis=1), R.row_stats_f64(R.forward_f64(u, f), f).sum(axis=1)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12)


def test_fused_source_index_differs_only_where_the_factor_is_inexact():
    for n in (1, 4, 9, 70):
        for f in (1, 2, 4):
            for a, b in zip(R._src32(n, f), R._src32(n, f, fused=True)):
                assert np.array_equal(a, b)
        a, b, e = R._src32(n, 3), R._src32(n, 3, fused=True), R._src64(n, 3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])
        for v in (a, b):
            assert np.abs(v[3] - e[3]).max() <= 2.0 ** -23 * max(n, 1) and np.abs(v[2] - e[2]).max() <= 2.0 ** -23 * max(n, 1)
    assert not R.inexact_weights((1, 2, 2)) and not R.inexact_weights((2, 2, 2)) and R.inexact_weights((1, 3, 3))


def test_round16_against_the_types():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.randn(20000) * 10.0 ** rng.uniform(-9, 4, 20000), [0.0, 1.0, 65504.0, 2.0 ** -24, 2.0 ** -25 * 1.0001]])
    assert np.array_equal(R.round16(x, "f16"), x.astype(np.float16).astype(np.float64))
    assert np.array_equal(R.round16(x, "bf16"), torch.from_numpy(x).to(torch.bfloat16).double().numpy())
    c = R.round_common16(x)
    assert np.array_equal(R.round16(c, "f16"), c) and np.array_equal(R.round16(c, "bf16"), c)
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    s = np.sort(x)
    assert (np.diff(R.round16(s, "f16")) >= 0).all() and (np.diff(R.round16(s, "bf16")) >= 0).all(), "monotone"


# ------------------------------------------------------------------------------------------------ the judge
F2, SH = (2, 2, 2), (1, 3, 5, 7, 8)               # odd coarse sizes: every axis has a pair without a second element


def _bwd_small(grid="f32"):
    d = K.bwd_data(SH, F2, grid)
    return d["g"], d["adj"], d["adj_scale"], d["adj_e32"]


def test_judge_passes_the_float32_restatement():
    g, ref, scale, e32 = _bwd_small()
    assert R.within(R.units(R.adjoint_f32(g, F2), ref, scale), e32)
    assert R.within(R.units(ref.astype(np.float32), ref, scale), e32)


def test_judge_fails_clamp_weight_on_the_wrong_coarse_voxel():
    """the last fine plane reads coarse D - 1 with weight 0.75 + 0.25 (its clamped neighbour); the 0.25 goes to D - 2 instead"""
    g, ref, scale, e32 = _bwd_small()
    last = g[:, -1:].astype(np.float64)
    for axis in (3, 2):
        last = R._apply_axis(R.interp_matrix(SH[axis], 2).T, last, axis)
    wrong = ref.copy()
    wrong[:, -1:] -= 0.25 * last
    wrong[:, -2:-1] += 0.25 * last
    assert not R.within(R.units(wrong.astype(np.float32), ref, scale), e32)
    assert np.isclose(wrong.sum(), ref.sum()), "the planted error keeps the total: only a per-element judge sees it"


def test_judge_fails_dropped_second_element_of_an_odd_pair():
    g, ref, scale, e32 = _bwd_small()
    wrong = ref.astype(np.float32)
    wrong[:, :, :, -1, :] = 0.0
    assert not R.within(R.units(wrong, ref, scale), e32)


def test_judge_fails_two_swapped_channels():
    g, ref, scale, e32 = _bwd_small()
    wrong = ref.astype(np.float32)
    wrong[..., [1, 2]] = wrong[..., [2, 1]]
    assert not R.within(R.units(wrong, ref, scale), e32)
    wrong = ref.astype(np.float32)
    wrong[..., [0, 5]] = wrong[..., [5, 0]]           # two channels of the same scale
    assert not R.within(R.units(wrong, ref, scale), e32)


def test_judge_fails_a_nan_and_a_wrong_shape():
    g, ref, scale, e32 = _bwd_small()
    wrong = ref.astype(np.float32)
    wrong[0, 1, 2, 3, 4] = np.nan
    assert R.units(wrong, ref, scale) == float("inf")
    assert R.units(ref[:, :-1], ref, scale) == float("inf")
    wrong = R.round16(ref, "f16")
    wrong[0, 1, 2, 3, 4] = np.nan
    assert R.outside16(wrong, ref, scale, e32, "f16") == 1 and R.outside16(ref[:, :-1], ref, scale, e32, "f16") == ref.size


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_judge_fails_one_16bit_element_one_ulp_outside_its_interval(kind):
    g, ref, scale, e32 = _bwd_small("16")
    lo, hi = R.interval16(ref, scale, e32, kind)
    good = R.round16(ref, kind)
    assert R.outside16(good, ref, scale, e32, kind) == 0
    assert R.outside16(lo, ref, scale, e32, kind) == 0 and R.outside16(hi, ref, scale, e32, kind) == 0, "a closed interval"
    p, emin = R.FMT[kind]
    for sign, edge in ((1.0, hi), (-1.0, lo)):
        wrong = edge.copy()
        v = wrong[0, 2, 4, 6, 3]
        ulp = 2.0 ** (max(np.frexp(v)[1] - 1, emin) - (p - 1))
        wrong[0, 2, 4, 6, 3] = v + sign * ulp
        assert R.round16(wrong, kind)[0, 2, 4, 6, 3] == wrong[0, 2, 4, 6, 3], "a value of the type"
        assert R.outside16(wrong, ref, scale, e32, kind) == 1


def test_judge_fails_sum_of_squares_missing_one_voxel():
    d = K.fwd_data(SH, F2, "f32")
    y, ref, scale, e32 = d["y"], d["rows"], d["rows_scale"], d["rows_e32"]
    good = R.row_stats_f32(R.forward_f32(d["x"], F2), F2)
    for k in (0, 1):
        assert R.within(R.units(good[..., k], ref[..., k], scale[..., k]), e32[k])
    wrong = good.astype(np.float64)
    n, z, r = 0, 1, 2
    wrong[n, z * SH[2] + r, :, 1] -= y[n, 2 * z + 1, 2 * r + 1, 2 * SH[3] - 1, :] ** 2      # the row's last fine voxel
    assert not R.within(R.units(wrong[..., 1], ref[..., 1], scale[..., 1]), e32[1])
    assert R.within(R.units(wrong[..., 0], ref[..., 0], scale[..., 0]), e32[0])


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_table_pair_counts_against_the_thresholds():
    for name, (f, shape, dtypes, path, layout, opts) in K.BWD.items():
        n = K.pairs(shape, f)
        if name in K.BWD_PAIRS:
            assert n == K.BWD_PAIRS[name], (name, n)
        factor2 = f[1:] == (2, 2) and f[0] in (1, 2) and shape[4] % 4 == 0 and not opts.get("upsample_generic")
        if path == K.FACTOR2_CH8:
            assert factor2 and n >= K.PAIRS_CH8 and shape[4] % 8 == 0 and "f32" not in dtypes, name
        elif path == K.FACTOR2_CH4:
            assert factor2 and n >= K.PAIRS_CH4, name
            # below the 8-channel threshold, or kept off that kernel by the option or by rows that are only 8-byte aligned
            assert n < K.PAIRS_CH8 or opts.get("upsample2_ch8") == 0 or (layout and layout[2] % 8), name
        else:
            assert not factor2 or n < K.PAIRS_CH4 or layout, name
        for dim, fac in zip(shape[1:4], f):
            assert dim == 1 or fac == 1 or dim % 2 == 1, (name, "odd coarse sizes: a pair without a second element on every axis")
    assert K.pairs(*K.BWD["b1"][1::-1]) == K.PAIRS_CH4 and K.pairs(*K.BWD["b2"][1::-1]) < K.PAIRS_CH4
    assert K.pairs(*K.BWD["b4"][1::-1]) == K.PAIRS_CH8
    assert {c[3] for c in K.BWD.values()} == {0, 1, 2, 3} and {c[3] for c in K.FWD.values()} == {0, 1, 2, 3}
    # f5: cq = 64 is the widest channel-group count the lane reduction takes, a thread makes 18 trips; b7: two trips, a tail of 2
    f, shape = K.FWD["f5"][:2]
    assert shape[4] // 4 == 64 and -(-shape[3] * 64 // 256) == 18
    f, shape = K.BWD["b7"][:2]
    assert shape[4] // 4 == 6 and -(-shape[3] // 2) * 6 == 258


def _grids(dtypes):
    return sorted({K.grid_of(d) for d in dtypes})


def test_float32_restatement_stays_below_its_stated_error_on_every_case():
    worst = {False: {k: 0.0 for k in E32_LIMIT}, True: {k: 0.0 for k in E32_LIMIT}}      # [1 / f inexact][quantity]
    seen = set()

    def note(f, q, v):
        w = worst[R.inexact_weights(f)]
        w[q] = max(w[q], v)
    for name, (f, shape, dtypes, path, layout, opts) in sorted(K.BWD.items(), key=lambda kv: kv[1][1]):
        for grid in _grids(dtypes):
            if (shape, f, grid) in seen:
                continue
            seen.add((shape, f, grid))
            d = K.bwd_data(shape, f, grid)
            note(f, "adjoint", d["adj_e32"])
            note(f, "bwd_norm", d["nrm_e32"])
    for name, (f, shape, dtypes, path, stats, layout) in K.FWD.items():
        for grid in _grids(dtypes):
            d = K.fwd_data(shape, f, grid)
            note(f, "forward", d["y_e32"])
            for k, q in enumerate(("sum y", "sum y^2")):
                note(f, q, d["rows_e32"][k])
                note(f, "u " + q, d["urows_e32"][k])
    for inexact, limit in ((False, E32_LIMIT), (True, E32_LIMIT_FACTOR3)):
        print(f"UPSAMPLE_E32 {'factor 3' if inexact else 'factors 1, 2'} " + " ".join(f"{k}: {v:.2f}" for k, v in worst[inexact].items()))
        for k, v in worst[inexact].items():
            assert v < limit[k], (inexact, k, v)
