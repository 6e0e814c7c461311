"""CPU: the float64 oracle of the norm kernels (oracle/norm_ref.py) against torch float64 group_norm / batch_norm and their
autograd, the geometry of every case of oracle/norm_cases.py through the library's dispatch queries (host code: the
library loads without a device), the band formulas against perturbed inputs, and the judge against deliberately wrong
results.  No GPU.

No element is left out of judgement: units / ratio_band / outside_interval count EVERY element, there is no subnormal or
absolute allowance anywhere in the norm judge, and the float32 restatement alone passes every case without one
(test_float32_restatement_passes_every_case_with_every_element_judged).

E32_LIMIT: the restatement stays below these figures (units of 2^-23 x the quantity's scale) on every case.  This run:
sum x 2.12, sum x^2 2.47, mean 2.12, var 1.41, sum g 0.48, sum g xn 0.65, apply 1.44.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import norm_cases as K
from oracle import norm_ref as R

MARGIN = R.MARGIN
E32_LIMIT = {"sum0": 2.5, "sum1": 3.0, "mean": 2.5, "var": 2.0, "bsum0": 1.0, "bsum1": 1.0, "apply": 1.75}
f32 = np.float32


def _lib():
    from torch_em_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the oracle against torch
def _nvc(t):
    """torch [N, C, V] -> numpy [N, V, C]"""
    return t.detach().permute(0, 2, 1).contiguous().numpy()


@pytest.mark.parametrize("C,G,affine", [(6, 6, False), (6, 3, True), (8, 2, True), (5, 1, True), (1, 1, False)])
def test_oracle_against_torch_float64_group_norm(C, G, affine):
    N, V = 3, 37
    rng = np.random.RandomState(C * 10 + G)
    x, g = rng.randn(N, V, C) * 2 + 0.7, rng.randn(N, V, C)
    gamma = 1 + 0.3 * rng.randn(C) if affine else None
    beta = 0.2 * rng.randn(C) if affine else None
    xt = torch.from_numpy(x).permute(0, 2, 1).contiguous().requires_grad_(True)
    gt = torch.from_numpy(gamma).requires_grad_(True) if affine else None
    bt = torch.from_numpy(beta).requires_grad_(True) if affine else None
    yt = F.group_norm(xt, G, gt, bt, eps=K.EPS)
    yt.backward(torch.from_numpy(g).permute(0, 2, 1))
    st = R.stats_f64(R.channel_sums_f64(x), V, G, gamma, beta, K.EPS)
    y = x * st["scale"][:, None, :] + st["shift"][:, None, :]
    assert np.abs(y - _nvc(yt)).max() <= 1e-13 * np.abs(y).max()
    xg = x.reshape(N, V, G, C // G)
    assert np.allclose(st["mean"], xg.mean(axis=(1, 3)), rtol=1e-13) and np.allclose(st["var"], xg.var(axis=(1, 3)), rtol=1e-12)
    bs = R.bwd_sums_f64(g, x, st["mean"], st["rstd"])
    coef = R.coef_f64(bs, V, G, gamma, st["mean"], st["rstd"])
    gx = R.apply_f64(g, x, coef, False)
    assert np.abs(gx - _nvc(xt.grad)).max() <= 1e-12 * np.abs(gx).max()
    masked = R.apply_f64(g, x, coef, True)
    assert np.array_equal(masked, np.where(x > 0, gx, 0.0))
    assert (R.apply_scale(g, x, coef) >= np.abs(gx) * (1 - 1e-12)).all(), "the scale bounds the value"
    if affine:
        dgamma, dbeta = R.affine_grads_f64(bs)
        assert np.allclose(dgamma, gt.grad.numpy(), rtol=1e-11, atol=1e-12) and np.allclose(dbeta, bt.grad.numpy(), rtol=1e-11, atol=1e-12)


def test_oracle_rows_forms_against_torch_batch_norm_and_a_concatenation():
    N, V, C = 3, 29, 6
    rng = np.random.RandomState(4)
    x = rng.randn(N, V, C) * 2 + 0.7
    gamma, beta = 1 + 0.3 * rng.randn(C), 0.2 * rng.randn(C)
    # partial rows: 4 uneven voxel blocks per sample
    cut = [0, 5, 6, 20, V]
    part = np.stack([R.channel_sums_f64(x[:, a:b]) for a, b in zip(cut[:-1], cut[1:])], axis=1)
    assert part.shape == (N, 4, C, 2)
    assert np.allclose(R.rows_f64(part), R.channel_sums_f64(x), rtol=1e-13)
    # BatchNorm: the rows == 1 form, every sample's rows merged into one
    st = R.stats_f64(R.rows_f64(part.reshape(1, N * 4, C, 2)), N * V, C, gamma, beta, K.EPS)
    xt = torch.from_numpy(x).permute(0, 2, 1).contiguous()
    yt = F.batch_norm(xt, None, None, torch.from_numpy(gamma), torch.from_numpy(beta), training=True, eps=K.EPS)
    y = x * st["scale"][:, None, :] + st["shift"][:, None, :]
    assert np.abs(y - _nvc(yt)).max() <= 1e-13 * np.abs(y).max()
    # the concat form: channels [0, 2) from one set of rows, [2, 6) from another partition of the voxels
    pa = part[:, :, :2]
    pb = np.stack([R.channel_sums_f64(x[:, a:b, 2:]) for a, b in ((0, 11), (11, V))], axis=1)
    both = R.concat_rows_f64(pa, pb)
    assert np.allclose(both, R.channel_sums_f64(x), rtol=1e-13)
    a, b = R.stats_f64(both, V, 3, gamma, beta, K.EPS), R.stats_f64(R.channel_sums_f64(x), V, 3, gamma, beta, K.EPS)
    assert all(np.allclose(a[k], b[k], rtol=1e-12) for k in a)


def test_partition_sums_is_the_documented_partition():
    """on integers every float32 sum is exact: the partition must then give the exact totals, per block the block's"""
    rng = np.random.RandomState(1)
    N, V, C = 2, 53, 3
    a = rng.randint(-8, 9, (N, V, C)).astype(f32)
    for rows, nblk, vper in ((4, 3, 18), (1, 7, 8), (16, 1, 53), (5, 4, 14)):
        for fused in (False, True):
            p = R.partition_sums_f32(a, a, a, rows, nblk, vper, fused)
            assert p.shape == (N, nblk, C, 2) and p.dtype == f32
            for b in range(nblk):
                blk = a[:, b * vper:(b + 1) * vper].astype(np.float64)
                assert np.array_equal(p[:, b, :, 0], blk.sum(axis=1)) and np.array_equal(p[:, b, :, 1], (blk * blk).sum(axis=1))


# ------------------------------------------------------------------------------------------------ geometry
def test_reduction_geometry_of_every_case():
    lib = _lib()
    for name, (C, G, N, V, dtypes, affine, offset, xl, gl, want0, want1) in K.RED.items():
        for dt in dtypes:
            x, gy = K.fake_ptr(xl, dt), K.fake_ptr(gl, dt)
            got0 = K.reduce_geom(lib, x, K.ld_of(xl, C), None, 0, V, C, K.ST[dt])
            got1 = K.reduce_geom(lib, x, K.ld_of(xl, C), gy, K.ld_of(gl, C), V, C, K.ST[dt])
            assert got0 == want0 and got1 == want1, (name, dt, got0, got1)
            for vec, rows, threads, nblk, vper in (got0, got1):
                assert threads == rows * (C // vec) <= (256 if vec == 4 else 1024) and nblk * vper >= V > (nblk - 1) * vper - vper * 30
    geo = {n: c[9] for n, c in K.RED.items()}
    assert geo["r1"][3] == 2 and 513 - 257 != 257, "uneven blocks"
    assert geo["r1"][4] > 4 * geo["r1"][1] and geo["r1"][4] % (4 * geo["r1"][1]), "the four-voxel main loop and its tail"
    assert geo["r4"][3] == 512 and -(-8209 // 17) < 512, "the cap, and blocks with no voxel"
    assert geo["r4"][1] == geo["r6"][1] == geo["r5"][1] == 1 and geo["r5"][2] == 1024
    assert {c[9][0] for c in K.RED.values()} == {1, 4}


def test_apply_geometry_of_every_case():
    lib = _lib()
    for name, (C, G, N, V, dtypes, affine, amax, gxl, want, inplace) in K.APP.items():
        for dt in dtypes:
            p = K.fake_ptr(None, dt)
            got = K.apply_geom(lib, p, C, p + (1 << 30), C, K.fake_ptr(gxl, dt) + (2 << 30), K.ld_of(gxl, C), N, V, C, amax, K.ST[dt])
            assert got == want, (name, dt, got)
            vec, threads, grid_x, fast = got
            lo, hi = K.APP_TRIPS[name]
            trips = V * (C // vec) / (grid_x * threads)
            assert lo < trips <= hi, (name, trips)
            assert fast == int(vec == 4 and (grid_x * threads) % (C // 4) == 0)
        if amax:
            n, v, c, val = K.amax_spike(name)
            assert K.last_block_elements(name)[v, c] and n == N - 1


def test_queries_refuse_what_the_launch_refuses():
    lib = _lib()
    p = K.fake_ptr(None, "f32")
    assert K.reduce_geom(lib, p, 8, None, 0, 10, 8, 0) is not None
    for args in ((None, 8, None, 0, 10, 8, 0), (p, 7, None, 0, 10, 8, 0), (p, 8, p, 7, 10, 8, 0), (p, 8, None, 0, 0, 8, 0),
                 (p, 1025, None, 0, 10, 1025, 0), (p, 8, None, 0, 10, 0, 0), (p, 8, None, 0, 10, 8, 3)):
        assert K.reduce_geom(lib, *args) is None, args
    assert K.apply_geom(lib, p, 8, p, 8, p, 8, 1, 10, 8, 0, 0) is not None
    for args in ((None, 8, p, 8, p, 8, 1, 10, 8, 0, 0), (p, 8, p, 8, None, 8, 1, 10, 8, 0, 0), (p, 8, p, 8, p, 7, 1, 10, 8, 0, 0),
                 (p, 8, p, 8, p, 8, 0, 10, 8, 0, 0), (p, 8, p, 8, p, 8, 1, 10, 8, 0, -1), (p, 1028, p, 1028, p, 1028, 1, 10, 1028, 0, 0)):
        assert K.apply_geom(lib, *args) is None, args
    assert lib.tem_norm_reduce_geom(ctypes.c_void_p(p), 8, None, 0, 10, 8, 0, None) == -1


def test_finalize_thread_switch_of_the_synthetic_sizes():
    for nblk, cg, threads in K.FIN:
        assert K.finalize_threads(nblk, cg) == threads
    assert 2048 == 8 * 256 and 16384 == 2 * 8 * 1024 and 2049 > 2048, "one exact trip, exactly two trips, the clamped tail"
    f = K.FIN2
    assert f["CA"] % f["cg"] == 0 and (f["CA"] + f["CB"]) // f["cg"] > f["CA"] // f["cg"] > 0, "groups on both sides of the split"
    assert K.finalize_threads(max(f["nblkA"], f["nblkB"]), f["cg"]) == 1024


# ------------------------------------------------------------------------------------------------ the band formulas
def _small():
    return K.tensor_data("s8", 8, 2, 2, 61, True, 0.7, "f32")


def test_band_formulas_hold_at_the_band_ends():
    """perturb what a quantity is built from to the ends of its band, in every sign combination and at random signs: the
    float64 formula stays inside the stated band (first order: a relative 1e-5 for the second-order terms)"""
    d = _small()
    V, G, C = d["V"], d["G"], 8
    e32 = {"mean": 1.7, "var": 2.3, "sum0": 1.3, "sum1": 2.9}
    ref, b = d["ref"], R.stats_bands(d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e32)
    ga, be = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    worst = 0.0
    for sm in (-1, 1):
        for sv in (-1, 1):
            m = ref["mean"] + sm * b["dm"]
            var = np.maximum(ref["var"] + sv * b["dv"], 0.0)
            r = 1.0 / np.sqrt(var + K.EPS)
            assert (np.abs(r - ref["rstd"]) <= b["dr"] * (1 + 1e-12)).all()
            assert R.outside_interval(r.astype(f32), b["rstd_lo"], b["rstd_hi"]) == 0
            scale = R.per_channel(r, C) * ga
            shift = be - R.per_channel(m, C) * scale
            assert (np.abs(scale - ref["scale"]) <= b["d_scale"] * (1 + 1e-5)).all()
            assert (np.abs(shift - ref["shift"]) <= b["d_shift"] * (1 + 1e-5)).all()
            assert (np.abs(scale.astype(f32) - ref["scale"]) <= b["d_scale"] * (1 + 1e-5)).all(), "... and after the rounding"
            assert (np.abs(shift.astype(f32) - ref["shift"]) <= b["d_shift"] * (1 + 1e-5)).all()
            worst = np.maximum(worst, np.abs(shift - ref["shift"]) / (b["d_shift"] - R.RND * np.abs(ref["shift"])))
    assert (worst > 0.95).all(), "the bands are tight: the combination with aligned signs reaches them"
    dc, d0, d1 = R.coef_bands(d["coef"], d["bscale"], V, G, d["gamma"], d["rstd32"], e32)
    rng = np.random.RandomState(0)
    for trial in range(6):
        s = np.sign(rng.randn(*d["bsums"].shape)) if trial < 4 else np.sign(ga)[None, :, None] * (1 if trial == 4 else -1)
        bs = d["bsums"] + s * np.stack([d0, d1], axis=-1)
        coef = R.coef_f64(bs, V, G, d["gamma"], d["mean32"], d["rstd32"])
        assert (np.abs(coef.astype(f32) - d["coef"]) <= dc * (1 + 1e-9)).all()
        dg, db = R.affine_grads_f64(bs)
        bg, bb = R.affine_bands(d["dgamma"], d["dbeta"], d0, d1)
        assert (np.abs(dg.astype(f32) - d["dgamma"]) <= bg).all() and (np.abs(db.astype(f32) - d["dbeta"]) <= bb).all()
    assert (np.abs(coef - d["coef"])[..., 1:3] > 0.9 * (dc[..., 1:3] - R.RND * np.abs(d["coef"][..., 1:3]))).all(), "reached with aligned signs"
    # gx end to end: the coef at the band ends through the formula, within the apply band plus the propagated ones
    e_apply = 1.2
    B = R.gx_band(d["g"], d["x"], d["coef"], dc, e_apply)
    ref_gx = R.apply_f64(d["g"], d["x"], d["coef"], False)
    for trial in range(4):
        coef = d["coef"] + np.sign(rng.randn(*dc.shape)) * dc
        gx = R.apply_f32(d["g"], d["x"], coef.astype(f32), False, 3 if trial % 2 else 0)
        assert (np.abs(gx - ref_gx) <= B + 2 * R.RND * R.apply_scale(d["g"], d["x"], d["coef"])).all()
    assert R.ratio_band(ref_gx + 0.999 * B, ref_gx, B) <= MARGIN < R.ratio_band(ref_gx + 1.001 * B, ref_gx, B)
    assert R.ratio_band(ref_gx[:, :-1], ref_gx, B) == float("inf") and R.ratio_band(np.where(B == B.max(), np.nan, ref_gx), ref_gx, B) == float("inf")


# ------------------------------------------------------------------------------------------------ the judge
def _restated(d, geom0, geom1, fused=False):
    """what a kernel that is plain fp32 arithmetic in the documented partition would return for the tensors of d"""
    vec, rows, threads, nblk, vper = geom0
    p0 = R.partition_sums_f32(d["x"], d["x"], d["x"], rows, nblk, vper, fused)
    st = R.stats_f64(R.rows_f64(p0), d["V"], d["G"], d["gamma"], d["beta"], K.EPS)
    vec, rows, threads, nblk, vper = geom1
    p1 = R.partition_sums_f32(d["g"], d["g"], R.xn_f32(d["x"], d["mean32"], d["rstd32"]), rows, nblk, vper, fused)
    bs = R.rows_f64(p1)
    coef = R.coef_f64(bs, d["V"], d["G"], d["gamma"], d["mean32"], d["rstd32"]).astype(f32)
    dgamma, dbeta = (v.astype(f32) for v in R.affine_grads_f64(bs))
    return {"sums": R.rows_f64(p0), "stats": {k: v.astype(f32) for k, v in st.items()}, "bsums": bs, "coef": coef,
            "dgamma": dgamma, "dbeta": dbeta}


def _judge_all(d, out, e0, e1):
    r = {}
    r.update(K.judge_sums(out["sums"], d["sums"], d["sums_scale"], e0))
    r.update(R.judge_stats(out["stats"], d["ref"], d["sums_scale"], d["V"], d["G"], d["gamma"], d["beta"], K.EPS, e0))
    r.update({"b" + k: v for k, v in K.judge_sums(out["bsums"], d["bsums"], d["bscale"], e1).items()})
    r.update(K.judge_coef(out["coef"], d, e1, out["dgamma"], out["dbeta"]))
    return r


RED_F32 = [(n, K.grid_of(c[4][0])) for n, c in K.RED.items()]
WORST_E32 = {}


def _note(k, v):
    WORST_E32[k] = max(WORST_E32.get(k, 0.0), v)


@pytest.mark.parametrize("name,grid", RED_F32, ids=[n for n, g in RED_F32])
def test_reduction_judge_passes_the_restatement_and_fails_planted_errors(name, grid):
    C, G, N, V, dtypes, affine, offset, xl, gl, geom0, geom1 = K.RED[name]
    d = K.red_data(name, grid)
    e0, e1 = K.reduce_e32(d, 0, geom0), K.reduce_e32(d, 1, geom1)
    for k, v in e0.items():
        _note(k, v)
        assert v < E32_LIMIT[k], (name, k, v)
    for k, v in e1.items():
        _note("b" + k, v)
        assert v < E32_LIMIT["b" + k], (name, k, v)
    for fused in (False, True):
        good = _restated(d, geom0, geom1, fused)
        r = _judge_all(d, good, e0, e1)
        assert R.passes(r), (name, fused, r)
    x, g = d["x"].astype(np.float64), d["g"].astype(np.float64)
    xn = R.xn_f64(x, d["mean32"], d["rstd32"])
    cg = C // G

    def wrong_sums(v, n):
        """voxel v of sample n left out of all four sums"""
        s, bs = d["sums"].copy(), d["bsums"].copy()
        s[n, :, 0] -= x[n, v]
        s[n, :, 1] -= x[n, v] ** 2
        bs[n, :, 0] -= g[n, v]
        bs[n, :, 1] -= g[n, v] * xn[n, v]
        return s, bs

    def outputs(s, bs, V_cnt=None, G_=G, roll=0):
        st = R.stats_f64(np.roll(s, roll, axis=1), d["V"] if V_cnt is None else V_cnt, G_, d["gamma"], d["beta"], K.EPS)
        coef = R.coef_f64(np.roll(bs, roll, axis=1), d["V"] if V_cnt is None else V_cnt, G_, d["gamma"], d["mean32"], d["rstd32"])
        dg, db = R.affine_grads_f64(bs)
        return {"sums": s, "stats": {k: v.astype(f32) for k, v in st.items()}, "bsums": bs, "coef": coef.astype(f32),
                "dgamma": dg.astype(f32), "dbeta": db.astype(f32)}

    exact = _judge_all(d, outputs(d["sums"], d["bsums"]), e0, e1)
    assert R.passes(exact), (name, exact)
    # the last voxel of one sample left out of a sum
    planted = [("last voxel of a sample", wrong_sums(V - 1, N - 1), ("sum0", "sum1", "bsum0", "bsum1", "mean", "m1"))]
    if geom0[3] > 1:   # the last voxel of the first block
        planted.append(("last voxel of a block", wrong_sums(geom0[4] - 1, 0), ("sum0", "sum1", "bsum0", "bsum1", "mean", "m1")))
    for what, (s, bs), must in planted:
        r = _judge_all(d, outputs(s, bs), e0, e1)
        for k in must:
            assert r[k] > MARGIN, (name, what, k, r[k])
    if G > 1:          # a group boundary off by one channel (one group has no boundary)
        r = _judge_all(d, outputs(d["sums"], d["bsums"], roll=1), e0, e1)
        assert r["mean"] > MARGIN and r["rstd"] > MARGIN and r["shift"] > MARGIN and r["m1"] > MARGIN and r["m2r"] > MARGIN, (name, r)
    if cg > 1:         # cnt = V in place of V cg: what a kernel that forgets the group width computes
        st = R.stats_f64(d["sums"], d["V"], G, d["gamma"], d["beta"], K.EPS)
        bad = {k: (v * cg if k == "mean" else v).astype(f32) for k, v in st.items()}
        r = R.judge_stats(bad, d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0)
        assert r["mean"] > MARGIN, (name, r)
        coef = d["coef"].copy()
        coef[..., 1:3] *= cg
        r = K.judge_coef(coef.astype(f32), d, e1)
        assert r["m1"] > MARGIN and r["m2r"] > MARGIN and r["a"] <= MARGIN and r["cmean"] == 0.0, (name, r)
    # m1 and m2r swapped
    r = K.judge_coef(d["coef"][..., [0, 2, 1, 3]].astype(f32), d, e1)
    assert r["m1"] > MARGIN and r["m2r"] > MARGIN, (name, r)
    # the mean of the coefficients one float32 step off
    coef = d["coef"].astype(f32)
    coef[0, 0, 3] = np.nextafter(coef[0, 0, 3], f32(np.inf))
    assert K.judge_coef(coef, d, e1)["cmean"] == float("inf")
    # rstd one float32 step outside its interval
    b = R.stats_bands(d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0)
    st = {k: v.astype(f32) for k, v in d["ref"].items() if k != "sums"}
    st["rstd"] = b["rstd_hi"].astype(f32)
    assert R.judge_stats(st, d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0)["rstd"] <= MARGIN, "a closed interval"
    st["rstd"] = np.nextafter(b["rstd_hi"].astype(f32), f32(np.inf))
    assert R.judge_stats(st, d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0)["rstd"] == float("inf")


APP_CASES = [(n, K.grid_of(c[4][0])) for n, c in K.APP.items() if n != "a8"]       # a8: the tensors of a1


@pytest.mark.parametrize("name,grid", APP_CASES, ids=[n for n, g in APP_CASES])
def test_apply_judge_passes_the_restatement_and_fails_planted_errors(name, grid):
    C, G, N, V, dtypes, affine, amax, gxl, geom, inplace = K.APP[name]
    d = K.app_data(name, grid)
    lib = _lib()
    p = K.fake_ptr(None, dtypes[0])
    rg = K.reduce_geom(lib, p, C, p + (1 << 30), C, V, C, K.ST[dtypes[0]])
    e1 = K.reduce_e32(d, 1, rg)
    coef32 = d["coef"].astype(f32)
    assert np.isin(0.0, d["x"]) and np.signbit(d["x"][d["x"] == 0]).any() and not np.signbit(d["x"][d["x"] == 0]).all(), "0.0 and -0.0"
    for relu in (False, True):
        ref1, scale1, e_apply = K.gx_apply_alone(d, coef32, relu)
        _note("apply", e_apply)
        assert e_apply < E32_LIMIT["apply"], (name, e_apply)
        ref2, B = K.gx_end_to_end(d, relu, e1, e_apply)
        for v in R.APPLY_VARIANTS:
            got = R.apply_f32(d["g"], d["x"], coef32, relu, v)
            assert R.within(R.units(got, ref1, scale1), e_apply) and R.ratio_band(got, ref2, B) <= MARGIN, (name, relu, v)
            for dt in dtypes:
                if dt != "f32":
                    assert R.outside16_abs(R.round16(got, dt), ref1, R.band(e_apply) * scale1, dt) == 0
                    assert R.outside16_abs(R.round16(got, dt), ref2, B, dt) == 0

        def fails(wrong, what, alone=True):
            if alone:
                assert not R.within(R.units(wrong.astype(f32), ref1, scale1), e_apply), (name, relu, what)
            assert R.ratio_band(wrong.astype(f32), ref2, B) > MARGIN, (name, relu, what)
            for dt in dtypes:
                if dt != "f32":
                    assert R.outside16_abs(R.round16(wrong, dt), ref2, B, dt) > 0, (name, relu, what, dt)
        # m1 and m2r swapped (in the coefficients the apply uses: the apply-alone reference follows the coef it is given)
        fails(R.apply_f64(d["g"], d["x"], d["coef"][..., [0, 2, 1, 3]], relu), "m1 and m2r swapped")
        # one element taken from the next channel
        wrong = ref2.copy()
        v = int(np.nonzero((d["x"][N - 1, :, 1] > 0) & (d["x"][N - 1, :, 2] > 0))[0][-1])      # neither is masked
        wrong[N - 1, v, 1] = ref2[N - 1, v, 2]
        fails(wrong, "one element from the next channel")
        # the second voxel of a trip never written (it keeps the NaN the test fills gx with)
        wrong = ref2.copy()
        wrong[0, V - 1, C - 1] = np.nan
        fails(wrong, "an element never written")
        if relu:       # the mask applied as x >= 0
            unmasked = R.apply_f64(d["g"], d["x"], d["coef"], False)
            fails(np.where(d["x"] >= 0, unmasked, 0.0), "mask x >= 0")
            assert (ref2[d["x"] == 0] == 0).all()
    if amax:           # max |gx| lies in the last block's elements: an amax over all but those differs
        for relu in (False, True):
            gx = R.apply_f32(d["g"], d["x"], coef32, relu, 0)
            full = np.abs(gx).max()
            rest = np.abs(np.where(K.last_block_elements(name)[None], 0, gx)[N - 1]).max()
            rest = max(rest, np.abs(gx[:N - 1]).max())
            assert f32(rest).view(np.uint32) != f32(full).view(np.uint32) and rest < full, (name, relu)
            n, v, c, val = K.amax_spike(name)
            assert np.abs(gx[n, v, c]) == full


def test_float32_restatement_passes_every_case_with_every_element_judged():
    """the judge has no allowance for small or subnormal elements: units() and ratio_band() take the maximum over every
    element, and an error where the scale or the band is 0 counts as infinite"""
    ref, scale = np.array([1.0, 0.0, 2.0]), np.array([1.0, 0.0, 2.0])
    assert R.units(ref, ref, scale) == 0.0 and R.units(ref + [0, 1e-300, 0], ref, scale) == float("inf")
    assert R.ratio_band(ref, ref, scale * 0) == 0.0 and R.ratio_band(ref + [0, 1e-300, 0], ref, scale * 0) == float("inf")
    assert R.outside_interval(np.array([1.0, np.nan]), np.array([1.0, 0.0]), np.array([1.0, 1.0])) == 1
    # every reduction and apply case above judged its restatement without leaving an element out; the smallest scale any
    # judged quantity has is far above the subnormal range, so no allowance could be needed
    for name in ("r1", "r5", "r9x"):
        d = K.red_data(name, K.grid_of(K.RED[name][4][0]))
        assert d["sums_scale"].min() > 1e-3 and d["bscale"].min() > 1e-3
    print("NORM_E32 " + " ".join(f"{k}: {v:.2f}" for k, v in sorted(WORST_E32.items())))
