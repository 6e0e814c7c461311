"""CPU: the float64 oracle of the max-pool kernels (oracle/maxpool_ref.py) against torch float64 max_pool3d and its autograd
(special values included), the fused coefficient path against norm_ref.apply_f64 composed by hand, the judge against
deliberately wrong outputs, and the arithmetic of the case tables (oracle/maxpool_cases.py).  No GPU.

E32_LIMIT: the numpy float32 restatement of a backward with coefficients stays below this figure, in units of 2^-23 x the
per-element scale, on every case of the table (this run: at most 1.51); the row partials of the recipe's tensors are exact
in float32 (e32 = 0: half-integers times powers of two), so a kernel passes them only with exact sums; the forward cases g2 / g3
run on values whose sums round (ROWS_E32_LIMIT; this run: sum y 0.44, sum y^2 2.38).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import maxpool_cases as K
from oracle import maxpool_ref as R
from oracle import norm_ref as NR
from oracle import upsample_cases as UK

E32_LIMIT = 2.0
ROWS_E32_LIMIT = 4.0
FACTORS = [(2, 2, 2), (1, 2, 2), (1, 3, 3), (3, 3, 3), (1, 1, 1), (2, 1, 1), (1, 1, 2)]


def _ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 4, 1, 2, 3)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


def _flat_index(am, shape, f):
    """the oracle's window position as the index into D * H * W that torch returns"""
    N, D, H, W, C = shape
    zo, yo, xo = np.meshgrid(np.arange(D // f[0]), np.arange(H // f[1]), np.arange(W // f[2]), indexing="ij")
    dz, dy, dx = am // (f[1] * f[2]), (am // f[2]) % f[1], am % f[2]
    e = (None, ..., None)
    return ((zo[e] * f[0] + dz) * H + yo[e] * f[1] + dy) * W + xo[e] * f[2] + dx


def _torch_pool(x, f):
    xt = _ncdhw(x).requires_grad_(True)
    yt, idx = F.max_pool3d(xt, f, return_indices=True)
    return xt, yt, idx


def _same(a, b):
    return R.mismatches(a, b) == 0


# ------------------------------------------------------------------------------------------------ the oracle against torch
@pytest.mark.parametrize("f", FACTORS)
def test_pool_and_backward_against_torch_float64(f):
    shape = (2, 2 * f[0], 3 * f[1], 2 * f[2], 5)
    d = K.inputs(shape, f)
    x, gy, gskip = d["x"], d["gy"], d["gskip"]
    xt, yt, idx = _torch_pool(x, f)
    y, am = R.pool_f64(x, f)
    assert _same(y, _cl(yt.detach()))
    assert np.array_equal(_flat_index(am, shape, f), _cl(idx)), "the first of equal maxima, as ATen"
    g, = torch.autograd.grad(yt, xt, _ncdhw(gy))
    g = _cl(g)
    out, scale = R.bwd_f64(gy, x, f)
    assert _same(out, g) and _same(scale, np.abs(g))
    out, scale = R.bwd_f64(gy, x, f, gskip, True)
    assert _same(out, (g + gskip) * (x > 0))
    assert _same(R.add_exact(gy, x, f, gskip, True), out), "inputs on the 16-bit grid: the float32 add is exact here"
    assert _same(R.unwindows(R.windows(x, f), f), x)


def test_special_values_against_torch_float64():
    f, shape = K.SPECIAL_F, K.SPECIAL_SHAPE
    x = K.special_x()
    assert np.isnan(x).sum() == 3 * shape[4] and np.isneginf(x).sum() == 8 * shape[4] and np.signbit(x[x == 0]).any()
    xt, yt, idx = _torch_pool(x, f)
    y, am = R.pool_f64(x, f)
    assert R.mismatches(y, _cl(yt.detach())) == 0 and np.isnan(y).sum() == 2 * shape[4]
    assert np.array_equal(_flat_index(am, shape, f), _cl(idx)), "the last NaN, the first of equal maxima, position 0 for -inf"
    assert (am[0, 0, 0, 0] == 0).all() and (am[0, 0, 0, 1] == 3).all() and (am[0, 0, 1, 0] == 5).all()
    assert (am[0, 0, 1, 1] == 0).all() and (am[0, 0, 0, 2] == 0).all()
    d = K.inputs(shape, f)
    g, = torch.autograd.grad(yt, xt, _ncdhw(d["gy"]))
    g = _cl(g)
    assert _same(R.bwd_f64(d["gy"], x, f)[0], g)
    with np.errstate(invalid="ignore"):
        want = np.where(x > 0, g + d["gskip"], 0.0)
    assert _same(R.bwd_f64(d["gy"], x, f, d["gskip"], True)[0], want)
    assert R.mismatches(np.array([np.nan, 0.0, 1.0]), np.array([np.nan, -0.0, 1.0])) == 0
    assert R.mismatches(np.array([np.nan, 0.0]), np.array([0.0, np.nan])) == 2


def _by_hand(d, f, variant, *, am=None, second=False, mask_ge=False, swap=False, voxel=False):
    """bwd_f64 composed from norm_ref.apply_f64 and torch's scatter; the keywords plant one error each"""
    x, gy = d["x"].astype(np.float64), d["gy"].astype(np.float64)
    gskip, mask, gcoef, ycoef = K.variant_args(d, variant)
    nvc = lambda a: a.reshape(a.shape[0], -1, a.shape[-1])                                      # noqa: E731
    if swap and gcoef is not None:
        gcoef = gcoef[..., [0, 1, 3, 2]]
    y, am0 = R.pool_f64(x, f)
    am = am0 if am is None else am
    A = np.zeros_like(x) if gskip is None else gskip.astype(np.float64)
    if gcoef is not None:
        A = NR.apply_f64(nvc(A), nvc(x), gcoef, False).reshape(x.shape)
    hit = R.at_argmax(am, K.nwin(f), f)
    if second:                                                # ... and the next tied position
        w = R.windows(x, f)
        tied = (w == y[..., None]) & (np.arange(K.nwin(f)) > am[..., None])
        nxt = np.where(tied.any(-1), np.argmax(tied, axis=-1), am)
        hit = hit | R.at_argmax(nxt, K.nwin(f), f)
    B = R.spread(gy, f)
    if ycoef is not None:
        # (the voxel AT the arg-max is the maximum: the planted error takes the window's first voxel, as a kernel would that
        # applied the coefficients before its arg-max loop had run)
        at = R.spread(R.windows(x, f)[..., 0], f) if voxel else R.spread(y, f)
        B = NR.apply_f64(nvc(B), nvc(at), ycoef, False).reshape(x.shape)
    out = np.where(hit, A + B, A)
    if mask:
        out = np.where(x >= 0 if mask_ge else x > 0, out, 0.0)
    return out


@pytest.mark.parametrize("variant", sorted(K.VARIANTS))
@pytest.mark.parametrize("name", sorted(K.MAIN))
def test_coefficient_path_composed_by_hand(name, variant):
    f, shape = K.MAIN[name]
    d, b = K.inputs(shape, f), K.bwd_data(shape, f, variant)
    hand = _by_hand(d, f, variant)
    assert np.abs(hand - b["ref"]).max() <= 1e-14 * max(1.0, np.abs(b["ref"]).max())
    xt, yt, idx = _torch_pool(d["x"], f)
    gskip, mask, gcoef, ycoef = K.variant_args(d, variant)
    By = d["gy"].astype(np.float64)
    if ycoef is not None:
        By = NR.apply_f64(By.reshape(shape[0], -1, shape[4]), _cl(yt.detach()).reshape(shape[0], -1, shape[4]), ycoef, False).reshape(By.shape)
    g, = torch.autograd.grad(yt, xt, _ncdhw(By))
    A = np.zeros(shape) if gskip is None else gskip.astype(np.float64)
    if gcoef is not None:
        A = NR.apply_f64(A.reshape(shape[0], -1, shape[4]), d["x"].reshape(shape[0], -1, shape[4]), gcoef, False).reshape(shape)
    total = A + _cl(g)                                        # the pooled norm's backward arrives through torch's scatter
    if mask:
        total = np.where(d["x"] > 0, total, 0.0)
    assert np.abs(total - b["ref"]).max() <= 1e-14 * max(1.0, np.abs(b["ref"]).max())
    assert (b["scale"] >= 0).all() and (b["scale"][b["ref"] != 0] > 0).all()
    if gcoef is None and ycoef is None:
        assert b["e32"] == 0.0
    else:
        assert 0.0 < b["e32"] <= E32_LIMIT, (name, variant, b["e32"])


# ------------------------------------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("shape,f", K.TIE_CASES, ids=[f"{s}-{f}" for s, f in K.TIE_CASES])
def test_windows_are_full_of_ties(shape, f):
    x = K.inputs(shape, f)["x"]
    tied, later = K.tie_share(x, f)
    print(f"MAXPOOL_TIES {shape} {f}: {tied:.2f} of the windows attain their maximum more than once, {later:.2f} with the first not at 0")
    assert tied >= K.TIE_MIN
    assert later > 0.05, "what tells the first maximum from the last and from position 0"


def _fwd_tensors(shape, layout):
    return [layout or (shape[4], 0), (shape[4], 0)]


def _bwd_tensors(shape, layout, variant):
    C = shape[4]
    t = {"gy": (C, 0), "x": (C, 0), "gx": (C, 0)}
    if K.VARIANTS[variant][0]:
        t["gskip"] = (C, 0)
    if layout:
        for k in {"xs": ("x", "gskip"), "gskip": ("gskip",), "gx": ("gx",)}[layout[0]]:
            assert k in t, "the layout's tensor is part of the launch"
            t[k] = (layout[1], layout[2])
    return list(t.values())


def test_forward_table_follows_the_documented_selector():
    seen = set()
    for name, (f, shape, dtypes, want, stats, layout, opts) in K.FWD.items():
        for dt in dtypes:
            path = K.expected_path("fwd", f, shape[4], dt, _fwd_tensors(shape, layout), opts.get("pool_vec8", 2))
            assert path == want[dt], (name, dt, K.PATH_NAME[path])
            if opts.get("x") == "randn16":
                e32 = K.fwd_rows(shape, f, K.cq_of(shape[4], path), "randn16")["rows_e32"]
                print(f"MAXPOOL_E32 {name} {dt}: row partials of the restatement {e32[0]:.2f} / {e32[1]:.2f}")
                assert 0.25 < max(e32) <= ROWS_E32_LIMIT, (name, dt, e32)
            seen.add((path, K.form(f)))
            cq = K.cq_of(shape[4], path)
            if (name, dt) in K.FWD_TRIPS:
                assert K.trips(shape, f, path) == K.FWD_TRIPS[(name, dt)], (name, dt)
            assert (K.stat_blocks(shape, f) == 0) == (stats == "none"), name
            if stats == "yes":
                assert cq <= 256 and 256 % cq == 0 and K.stat_blocks(shape, f) == shape[1] // f[0] * (shape[2] // f[1])
    assert K.form((2, 2, 2)) == "unrolled" and K.form((1, 3, 3)) == "loop" and K.form((1, 1, 1)) == "unrolled"
    assert {(p, fm) for p in (K.VEC4, K.VEC8) for fm in ("unrolled", "loop")} | {(K.VEC1, "unrolled")} <= seen
    assert max(K.FWD_TRIPS.values()) == 3


def test_backward_table_follows_the_documented_selector():
    seen = set()
    for name, (f, shape, dtypes, want, variants, layout, opts) in K.BWD.items():
        for dt in dtypes:
            for v in variants:
                path = K.expected_path("bwd", f, shape[4], dt, _bwd_tensors(shape, layout, v), opts.get("pool_vec8", 2))
                assert path == want[dt], (name, dt, v, K.PATH_NAME[path])
                seen.add((path, K.form(f), dt != "f32"))
            if (name, dt) in K.BWD_TRIPS:
                assert K.trips(shape, f, want[dt]) == K.BWD_TRIPS[(name, dt)], (name, dt)
    for p in (K.VEC1, K.VEC4, K.VEC8, K.PACKED16_FZ1, K.PACKED16_FZ2):
        assert any(s[0] == p for s in seen), K.PATH_NAME[p]
    assert (K.VEC8, "loop", True) in seen and (K.VEC4, "loop", False) in seen
    assert (K.VEC4, "unrolled", True) in seen and (K.VEC8, "unrolled", True) in seen and (K.VEC1, "unrolled", False) in seen
    assert set(K.BWD["m1"][4]) | set(K.BWD["m1r"][4]) == set(K.VARIANTS) == set(K.BWD["m2"][4]) | set(K.BWD["m2r"][4])
    assert K.cq_of(24, K.PACKED16_FZ2) == 3 and 2 * 2048 * 16 == 65536 and K.BWD["c512"][1][4] > 256


def test_restatement_stays_below_its_limit_on_every_backward_case():
    worst = 0.0
    for name, (f, shape, dtypes, want, variants, layout, opts) in K.BWD.items():
        for v in variants:
            worst = max(worst, K.bwd_data(shape, f, v)["e32"])
    print(f"MAXPOOL_E32 worst restatement error over the backward table: {worst:.2f}")
    assert worst <= E32_LIMIT


# ------------------------------------------------------------------------------------------------ the judge
def _verdicts(d, f, variant, wrong):
    """the judge's verdict on `wrong`, stored as fp32, fp16 and bf16"""
    shape = d["x"].shape
    b = K.bwd_data(shape, f, variant)
    gskip, mask, gcoef, ycoef = K.variant_args(d, variant)
    out = []
    for kind in ("f32", "f16", "bf16"):
        stored = wrong.astype(np.float32).astype(np.float64) if kind == "f32" else R.round16(wrong.astype(np.float32), kind)
        if gcoef is None and ycoef is None:
            out.append(R.mismatches(stored, R.add_exact(d["gy"], d["x"], f, gskip, mask, kind)) == 0)
        else:
            out.append(R.judge_units(stored, b["ref"], b["scale"], b["e32"], kind)[0])
    return out


@pytest.mark.parametrize("variant", sorted(K.VARIANTS))
def test_judge_passes_the_restatement_and_fails_planted_errors(variant):
    f, shape = K.MAIN["m1"]
    d = K.inputs(shape, f)
    gskip, mask, gcoef, ycoef = K.variant_args(d, variant)
    vs = NR.APPLY_VARIANTS
    for va in (vs if gcoef is not None else (0,)):
        for vb in (vs if ycoef is not None else (0,)):
            assert all(_verdicts(d, f, variant, R.bwd_f32(d["gy"], d["x"], f, gskip, mask, gcoef, ycoef, va, vb)))
    w = R.windows(d["x"].astype(np.float64), f)
    last = K.nwin(f) - 1 - np.argmax((w == d["y"][..., None])[..., ::-1], axis=-1)
    planted = {"last maximum": dict(am=last), "a second tied position": dict(second=True)}
    if mask:
        planted["mask from x >= 0"] = dict(mask_ge=True)
    if gcoef is not None:
        planted["mean and m2r swapped"] = dict(swap=True)
    if ycoef is not None:
        planted["ycoef at the window's first voxel"] = dict(voxel=True)
    for what, kw in planted.items():
        if mask and what in ("last maximum", "a second tied position") and ycoef is None:
            continue           # under the mask alone a tie at 0 hides both: the variants without it and with ycoef tell
        assert not any(_verdicts(d, f, variant, _by_hand(d, f, variant, **kw))), (variant, what)


def test_judge_of_the_forward_and_the_row_partials():
    f, shape = K.MAIN["m1"]
    d = K.inputs(shape, f)
    y = d["y"]
    assert R.mismatches(y, y) == 0
    lastval = R.windows(d["x"].astype(np.float64), f)[..., -1]
    assert R.mismatches(lastval, y) > 0 and R.mismatches(y[:, :, :, :-1], y) == y.size
    bad = y.copy()
    bad[1, 1, 2, 3, 7] = np.nan
    assert R.mismatches(bad, y) == 1
    for cq in (4, 8):
        r = K.fwd_rows(shape, f, cq)
        for k in (0, 1):
            for fused in (False, True):
                got = R.row_stats_f32(y, cq, fused)[..., k]
                assert R.within(R.units(got, r["rows"][..., k], r["rows_scale"][..., k]), r["rows_e32"][k])
            wrong = r["rows"][..., k].copy()
            wrong[1, 3, 5] = wrong[1, 3, 6]                   # one partial row holds the neighbour channel's sum
            assert wrong[1, 3, 5] != r["rows"][1, 3, 5, k]
            assert not R.within(R.units(wrong, r["rows"][..., k], r["rows_scale"][..., k]), r["rows_e32"][k])
    naive = np.stack([y.sum(axis=3), (y * y).sum(axis=3)], -1).reshape(r["rows"].shape)
    assert np.array_equal(naive, r["rows"])


def test_amax_rule():
    got = np.array([0.5, -3.25, 2.0])
    word = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])                          # noqa: E731
    assert R.amax_ok(word(3.25), got, "f32") and not R.amax_ok(word(3.2500002), got, "f32") and not R.amax_ok(word(2.0), got, "f32")
    assert R.amax_ok(word(3.2501), got, "bf16") and R.amax_ok(word(3.2501), got, "f16") and not R.amax_ok(word(3.26), got, "f16")


def test_inputs_are_exact_in_every_storage_type():
    for f, shape in K.MAIN.values():
        d = K.inputs(shape, f)
        for k in ("x", "gy", "gskip"):
            assert np.array_equal(R.round_common16(d[k]), d[k]) and d[k].dtype == np.float32
        assert (d["x"] >= 0).all() and (d["x"] == 0).mean() > 0.4
    assert UK.make_coef(2, 8, 1).shape == (2, 8, 4)
