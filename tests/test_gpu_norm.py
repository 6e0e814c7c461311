"""GPU: every kernel of csrc/norm.hip on every dispatch path, op by op through ops.norm_stats / norm_stats_from_partials /
norm_stats_from_partials2 / norm_bwd_coef / norm_bwd (the `_st` entries), against the float64 references of
oracle/norm_ref.py (which tests/test_norm_cpu.py pins to torch float64 group_norm / batch_norm and their autograd, and whose
judge it tests on deliberately wrong results).

Rule (oracle/judge.py).  Errors are counted in units of 2^-23 times a
per-quantity scale -- sum x: sum |x|, sum x^2: its value, sum g: sum |g|, sum g xn: sum |g xn|, mean: sum |x| / cnt.  On the
same inputs the test takes the worst figure e32 of the numpy float32 restatement (a reference, not the code under test): for
the reductions the partition the header of norm.hip documents, fp32 chains -> fp32 per-block rows -> fp64 merge, with the
chain lengths (`rows`, `vper`, `nblk`) the dispatch query names for the launch; for the apply one rounding per operation, the
worse of the products rounded on their own and contracted into fmas.  EVERY element must stay within MARGIN * max(e32, 1)
units, MARGIN of oracle/judge.py: 4.  The partial rows are read from the workspace the launch wrote.  Quantities derived
from those (rstd, scale, shift, the coef entries, dgamma, dbeta, gx end to end) get the propagated bands stated in the
docstring of oracle/norm_ref.py: rstd the closed float32 interval of the var band (scale E[x^2] + 2 |m| E|x|: what
ss / cnt - m^2 can lose), the others first order plus one rounding.  gx is judged twice: the apply alone against the float64
formula from the float32 coef a coef_out call returned on the same inputs (scale |a g| + |m1| + |(x - mean) m2r|), and end to
end against the float64 gx.  16-bit outputs: the closed rounded interval of the same band.  out_amax: the exact bit pattern of
max |gx| of the tensor as stored; a larger preset stays, a smaller non-zero one is replaced.

The backward is given float32(mean), float32(rstd) of the float64 statistics, so every reference is computed once per tensor
set, before any launch.  Every case asserts and prints the geometry the library's dispatch queries (tem_norm_reduce_geom,
tem_norm_apply_geom) name for exactly the pointers and leading dimensions of the launch; tests/test_norm_cpu.py asserts the
same table without a device.  Cases are the smallest shapes that reach each path (oracle/norm_cases.py).

No test provokes a device fault: the test lays every tensor out itself and asserts its extent against its buffer before a
launch (oracle/gpu_kit.py), unused channels of wide buffers hold NaN on input and keep their fill on output, every tensor
sits between sentinels that must survive, and every launch is repeated and must return the same bits (the reductions have no
atomics; the one atomic of out_amax is a max).

Observed on the MI355X (profiles/norm_op_errors.txt): worst ratio 1.27 (OBSERVED_WORST_RATIO below: the mean of r9, whose
float32 rounding is half a unit of its scale; every sum equals the restatement's figure or stays below it), no 16-bit element
outside its interval, the 16-bit launches of a7 equal the rounded fp32 launches in every bit, out_amax exact.  r9 / r9x
(|mean| / sigma up to 9.6 / 15.6): rstd is 16 / 47 x 2^-23 off relatively, inside a band of 550 / 1460 -- what the fp32 partials
of ss / cnt - m^2 cost; the finalize itself is in double and loses nothing more.
"""
import numpy as np
import pytest
import torch

from oracle import gpu_kit as kit
from oracle import norm_cases as K
from oracle import norm_ref as R
from oracle.gpu_kit import DEV, TORCH, lib as _lib, ops as _ops

pytestmark = pytest.mark.gpu
MARGIN = R.MARGIN
OBSERVED_WORST_RATIO = 1.27       # informational (profiles/norm_op_errors.txt); the assertions use MARGIN
f32 = np.float32
EXACT = ("a", "cmean")            # quantities whose band is one rounding or none: not part of the worst ratio
LEDGER = kit.Ledger("NORM_ERR")
_print_worst = LEDGER.summary_fixture(
    legend=" (kernel, f32: units of 2^-23 x scale, ratio = kernel / max(f32, 1); band quantities: ratio = MARGIN x error / band; "
           "at most MARGIN passes)",
    left_out=lambda q: q in EXACT,
    footnote=f" (without a and cmean: a is one correctly rounded product, whose band is half a float32 step, so up to {MARGIN:.0f} "
             f"by construction; cmean is 0 or infinite)")


def _note(path, ratios, e32):
    """e32: the restatement's figure for the quantities judged in units (ratio = kernel units / max(e32, 1)); the others
    are MARGIN x error / band"""
    for q, v in ratios.items():
        e = e32.get(q)
        LEDGER.note(path, q, None if e is None else v * max(e, 1.0), e, ratio=v)


def _check(tag, path, ratios, e32=None):
    e32 = e32 or {}
    print(f"NORM_ERR {tag} -> {path}: " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items())
          + (" | f32: " + " ".join(f"{k} {v:.2f}" for k, v in e32.items()) if e32 else ""))
    _note(path, ratios, e32)
    bad = {k: v for k, v in ratios.items() if not v <= MARGIN}
    assert not bad, f"{tag}: beyond MARGIN x the float32 restatement: {bad}"


# ------------------------------------------------------------------------------------------ helpers
def _lay(N, V, C, dt, layout, data=None, output=False):
    data = None if data is None else np.ascontiguousarray(data.reshape(N, 1, 1, V, C))
    return kit.lay((N, 1, 1, V, C), dt, layout, data, output)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(*ts):
    return [t.detach().clone().view(torch.int32) for t in ts if t is not None]


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def _rows(N, V, C, nblk):
    """the partial rows [N, nblk, C, 2] the reduction pass of the last launch left at the head of the workspace"""
    lib, ops = _lib().load(), _ops()
    ws = ops._workspace(lib.tem_norm_ws(N, V, C), DEV)
    n = N * nblk * C * 2
    assert n * 4 <= lib.tem_norm_ws(N, V, C) <= ws.numel()
    torch.cuda.synchronize()
    return ws[:n * 4].view(torch.float32).view(N, nblk, C, 2).clone()


def _unchanged(tag, L, data):
    assert L.intact() and torch.equal(L.view.float().reshape(data.shape), torch.from_numpy(data).to(DEV)), f"{tag}: an input changed"


# ------------------------------------------------------------------------------------------ reduction
RED_CASES = [(name, dt) for name, c in K.RED.items() for dt in c[4]]


@pytest.mark.parametrize("name,dt", RED_CASES, ids=[f"{n}-{t}" for n, t in RED_CASES])
def test_reductions_against_float64(name, dt):
    lib, ops = _lib().load(), _ops()
    C, G, N, V, dtypes, affine, offset, xl, gl, want0, want1 = K.RED[name]
    d = K.red_data(name, K.grid_of(dt))
    st = K.ST[dt]
    X, GY = _lay(N, V, C, dt, xl, d["x"]), _lay(N, V, C, dt, gl, d["g"])
    gamma, beta = _dev(d["gamma"]), _dev(d["beta"])
    tag = f"reduce {name} C={C} G={G} N={N} V={V} {dt}"
    # ---- MODE 0: norm_stats
    geom0 = K.reduce_geom(lib, X.ptr(), X.Wd, None, 0, V, C, st)
    print(f"NORM_PATH {tag} stats: query (vec, rows, threads, nblk, vper) = {geom0}, intended {want0}")
    assert geom0 == want0, f"{tag}: meant for {want0}, the query names {geom0}"
    e0 = K.reduce_e32(d, 0, geom0)
    out = ops.norm_stats(X.view, G, gamma, beta, K.EPS)
    rows = _rows(N, V, C, geom0[3])
    again = ops.norm_stats(X.view, G, gamma, beta, K.EPS)
    assert _same(_bits(*out, rows), _bits(*again, _rows(N, V, C, geom0[3]))), f"{tag}: a repeated launch is bit-identical"
    path = f"stats vec{geom0[0]} rows{geom0[1]} {'f32' if dt == 'f32' else '16'}"
    ratios = K.judge_sums(R.rows_f64(_np(rows)), d["sums"], d["sums_scale"], e0)
    got = dict(zip(("mean", "rstd", "scale", "shift"), (_np(t) for t in out)))
    ratios.update(R.judge_stats(got, d["ref"], d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0))
    _check(tag, path, ratios, e0)
    if offset > 1:     # the conditioning of ss / cnt - m^2, for the record
        ref = d["ref"]
        rel = np.abs(got["rstd"].astype(np.float64) - ref["rstd"]) / ref["rstd"] / 2.0 ** -23
        b = R.stats_bands(ref, d["sums_scale"], V, G, d["gamma"], d["beta"], K.EPS, e0)
        print(f"NORM_COND {tag}: |mean| / sigma up to {np.abs(ref['mean'] / np.sqrt(ref['var'])).max():.2f}; rstd error "
              f"{rel.max():.2f} x 2^-23 relative (band {(b['dr'] / ref['rstd']).max() / 2.0 ** -23:.0f}); var scale / var up to "
              f"{(R.var_scale(ref['mean'], *R.stats_scales(d['sums_scale'], V, G)[:2]) / ref['var']).max():.0f}; f32 var error {e0['var']:.2f} units")
    # ---- MODE 1: the backward reduction, through coef_out
    geom1 = K.reduce_geom(lib, X.ptr(), X.Wd, GY.ptr(), GY.Wd, V, C, st)
    print(f"NORM_PATH {tag} bwd: query = {geom1}, intended {want1}")
    assert geom1 == want1, f"{tag}: meant for {want1}, the query names {geom1}"
    e1 = K.reduce_e32(d, 1, geom1)
    mean, rstd = _dev(d["mean32"]), _dev(d["rstd32"])
    dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    coef = ops.norm_bwd_coef(GY.view, X.view, G, gamma, mean, rstd, dgamma, dbeta)
    rows1 = _rows(N, V, C, geom1[3])
    first = _bits(coef, dgamma, dbeta, rows1)
    dg2, db2 = torch.full_like(dgamma, float("nan")), torch.full_like(dbeta, float("nan"))
    coef2 = ops.norm_bwd_coef(GY.view, X.view, G, gamma, mean, rstd, dg2, db2)
    assert _same(first, _bits(coef2, dg2, db2, _rows(N, V, C, geom1[3]))), f"{tag}: a repeated launch is bit-identical"
    path = f"bwd reduce vec{geom1[0]} rows{geom1[1]} {'f32' if dt == 'f32' else '16'}"
    ratios = {"b" + k: v for k, v in K.judge_sums(R.rows_f64(_np(rows1)), d["bsums"], d["bscale"], e1).items()}
    ratios.update(K.judge_coef(_np(coef), d, e1, _np(dgamma), _np(dbeta)))
    _check(tag, path, ratios, {"b" + k: v for k, v in e1.items()})
    _unchanged(tag, X, d["x"])
    _unchanged(tag, GY, d["g"])


# ------------------------------------------------------------------------------------------ finalize on synthetic rows
def _judge_finalize(tag, path, out, sums, scale, V, G, gamma, beta):
    got = dict(zip(("mean", "rstd", "scale", "shift"), (_np(t) for t in out)))
    ref = R.stats_f64(sums, V, G, gamma, beta, K.EPS)
    _check(tag, path, R.judge_stats(got, ref, scale, V, G, gamma, beta, K.EPS))
    return got, ref


@pytest.mark.parametrize("nblk,cg,threads", K.FIN, ids=[f"{n}x{c}" for n, c, t in K.FIN])
def test_finalize_on_synthetic_rows(nblk, cg, threads):
    ops = _ops()
    C, G, V = 2 * cg, 2, nblk * 8
    assert K.finalize_threads(nblk, cg) == threads
    gamma, beta = K.make_affine(C, 5)
    for N, rows in ((2, 2), (3, 1)):          # per sample; BatchNorm: the rows of every sample merge into one
        part = K.make_rows(N, nblk, C, 100 + nblk + N, V)
        pt = _dev(part)
        out = ops.norm_stats_from_partials(pt, rows, V, C, G, _dev(gamma), _dev(beta), K.EPS)
        again = ops.norm_stats_from_partials(pt, rows, V, C, G, _dev(gamma), _dev(beta), K.EPS)
        assert _same(_bits(*out), _bits(*again)) and torch.equal(pt, _dev(part))
        p = part if rows == N else part.reshape(1, N * nblk, C, 2)
        tag = f"finalize nblk={nblk} cg={cg} N={N} rows={rows} ({threads} threads)"
        _judge_finalize(tag, f"finalize {threads} threads" + (" batch" if rows == 1 else ""), out, R.rows_f64(p), R.rows_scale(p),
                        V * (N if rows == 1 else 1), G, gamma, beta)


@pytest.mark.parametrize("lower", [False, True], ids=["var-zero", "var-negative"])
def test_finalize_clamps_the_variance(lower):
    """every x equal (0.75: the rows and the mean are exact): ss / cnt - m^2 is exactly 0, or -- ss one float32 step lower --
    negative, and clamps; rstd = float32(1 / sqrt(eps)) in every bit"""
    ops = _ops()
    nblk, cg, N = 7, 3, 2
    C, G, V = 2 * cg, 2, nblk * 16
    part = K.make_rows(N, nblk, C, 0, V, equal=True)
    if lower:
        part[..., 1] = np.nextafter(part[..., 1], f32(0))
    assert ((R.rows_f64(part)[..., 1] / V - (R.rows_f64(part)[..., 0] / V) ** 2 < 0) == lower).all()
    out = ops.norm_stats_from_partials(_dev(part), N, V, C, G, None, None, K.EPS)
    got, ref = _judge_finalize(f"finalize clamp lower={lower}", "finalize clamp", out, R.rows_f64(part), R.rows_scale(part), V, G, None, None)
    assert (ref["var"] == 0).all() and (got["rstd"] == f32(1.0 / np.sqrt(K.EPS))).all() and (got["mean"] == f32(0.75)).all()


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_finalize_of_a_concatenation(affine):
    ops = _ops()
    f = K.FIN2
    CA, CB, cg, N = f["CA"], f["CB"], f["cg"], f["N"]
    C, G, V = CA + CB, (CA + CB) // cg, f["nblkB"] * 8
    pa, pb = K.make_rows(N, f["nblkA"], CA, 21, V), K.make_rows(N, f["nblkB"], CB, 22, V)
    gamma, beta = K.make_affine(C, 6, affine)
    args = (_dev(pa), _dev(pb), N, V, G, _dev(gamma), _dev(beta), K.EPS)
    out = ops.norm_stats_from_partials2(*args)
    assert _same(_bits(*out), _bits(*ops.norm_stats_from_partials2(*args)))
    _judge_finalize(f"finalize2 CA={CA} CB={CB} cg={cg} nblk {f['nblkA']} / {f['nblkB']} affine={affine}", "finalize2", out,
                    R.concat_rows_f64(pa, pb), R.concat_rows_f64(pa, pb, R.rows_scale), V, G, gamma, beta)


@pytest.mark.parametrize("nblk,N", K.BWD_STAGE, ids=[f"{b}x{n}" for b, n in K.BWD_STAGE])
def test_backward_stages_on_synthetic_rows(nblk, N):
    """k_norm_bwd_finalize and k_norm_bwd_affine on given rows (sum g, sum g xn): gy and x are not read"""
    ops = _ops()
    C, cg = K.BWD_STAGE_CG
    G, V = C // cg, 64
    part = K.make_bwd_rows(N, nblk, C, 300 + nblk + N)
    rng = np.random.RandomState(nblk + N)
    mean32, rstd32 = (0.7 + 0.2 * rng.randn(N, G)).astype(f32), rng.uniform(0.5, 2.0, (N, G)).astype(f32)
    X, GY = _lay(N, V, C, "f32", None, np.zeros((N, V, C), f32)), _lay(N, V, C, "f32", None, np.zeros((N, V, C), f32))
    for affine in (False, True):
        gamma, _ = K.make_affine(C, 7, affine)
        bs = R.rows_f64(part)
        dd = {"coef": R.coef_f64(bs, V, G, gamma, mean32, rstd32), "bscale": np.abs(part.astype(np.float64)).sum(axis=1), "V": V,
              "G": G, "gamma": gamma, "rstd32": rstd32}
        dd["dgamma"], dd["dbeta"] = R.affine_grads_f64(bs)
        outs = []
        for _ in range(2):
            dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
            coef = ops.norm_bwd_coef(GY.view, X.view, G, _dev(gamma), _dev(mean32), _dev(rstd32), dgamma, dbeta, sums=_dev(part))
            outs.append(_bits(coef, dgamma, dbeta))
        assert _same(*outs), "a repeated launch is bit-identical"
        _check(f"bwd stages nblk={nblk} N={N} affine={affine}", "bwd finalize / affine", K.judge_coef(_np(coef), dd, {}, _np(dgamma), _np(dbeta)))
    assert X.intact() and GY.intact()


# ------------------------------------------------------------------------------------------ apply
APP_CASES = [(name, dt, relu) for name, c in K.APP.items() for dt in c[4] for relu in (False, True)]
APP_CASES.sort(key=lambda c: (K.APP[c[0]][:4], K.grid_of(c[1]), K.APP[c[0]][6]))      # cases of one tensor set together
_ALONE = {}


def _apply_refs(d, coef_k, relu, e1):
    """the references of one (tensor set, mask): shared by the storage types and launches whose coef_out call returned the
    same bits"""
    key = (id(d), relu, coef_k.tobytes())
    if key not in _ALONE or _ALONE[key][0] is not d:
        if len(_ALONE) >= 2:
            _ALONE.clear()
        ref1, scale1, e_apply = K.gx_apply_alone(d, coef_k, relu)
        ref2, B = K.gx_end_to_end(d, relu, e1, e_apply)
        _ALONE[key] = (d, ref1, scale1, e_apply, ref2, B)
    return _ALONE[key][1:]


def _launch_apply(name, dt, relu, d, amax_preset=None, inplace=False):
    """-> dict: gx (host float64 [N, V, C]), bits, coef (numpy float32 from the coef_out call), word, geometry"""
    lib, ops = _lib().load(), _ops()
    C, G, N, V, dtypes, affine, amax, gxl, want, _ = K.APP[name]
    X, GY = _lay(N, V, C, dt, None, d["x"]), _lay(N, V, C, dt, None, d["g"])
    GX = GY if inplace else _lay(N, V, C, dt, gxl, None, output=True)
    gamma, mean, rstd = _dev(d["gamma"]), _dev(d["mean32"]), _dev(d["rstd32"])
    st = K.ST[dt]
    ag = K.apply_geom(lib, GY.ptr(), GY.Wd, X.ptr(), X.Wd, GX.ptr(), GX.Wd, N, V, C, amax, st)
    rg = K.reduce_geom(lib, X.ptr(), X.Wd, GY.ptr(), GY.Wd, V, C, st)
    coef = ops.norm_bwd_coef(GY.view, X.view, G, gamma, mean, rstd)
    assert _same(_bits(coef), _bits(ops.norm_bwd_coef(GY.view, X.view, G, gamma, mean, rstd))), "coef_out is bit-identical when repeated"
    words = []
    for rep in range(2):
        if rep and not inplace:
            GX.view.fill_(float("nan"))
        if rep and inplace:
            GY = GX = _lay(N, V, C, dt, None, d["g"])
        word = None
        if amax:
            word = torch.tensor([0 if amax_preset is None else int(f32(amax_preset).view(np.uint32))], dtype=torch.int32, device=DEV)
        ops.norm_bwd(GY.view, X.view, G, gamma, mean, rstd, relu, GX.view, out_amax=word)
        torch.cuda.synchronize()
        if rep == 0:
            first = GX.bits()
        words.append(None if word is None else int(word.item()))
    assert torch.equal(first, GX.bits()) and words[0] == words[1], f"{name}: a repeated launch is bit-identical"
    assert GX.intact(), f"{name}: wrote outside the elements of gx"
    _unchanged(name, X, d["x"])
    if not inplace:
        _unchanged(name, GY, d["g"])
    return {"gx": GX.host().reshape(N, V, C), "bits": first, "coef": _np(coef), "word": words[0], "ag": ag, "rg": rg}


@pytest.mark.parametrize("name,dt,relu", APP_CASES, ids=[f"{n}-{t}-{'relu' if m else 'plain'}" for n, t, m in APP_CASES])
def test_apply_against_float64(name, dt, relu):
    C, G, N, V, dtypes, affine, amax, gxl, want, inplace = K.APP[name]
    d = K.app_data(name, K.grid_of(dt))
    r = _launch_apply(name, dt, relu, d)
    tag = f"apply {name} C={C} G={G} N={N} V={V} {dt} relu={int(relu)}"
    print(f"NORM_PATH {tag}: query (vec, threads, grid_x, fast) = {r['ag']}, intended {want}; reduction {r['rg']}")
    assert r["ag"] == want, f"{tag}: meant for {want}, the query names {r['ag']}"
    e1 = K.reduce_e32(d, 1, r["rg"])
    vec, threads, grid_x, fast = r["ag"]
    path = f"apply vec{vec} {'fast' if fast else 'slow'} {threads} {'f32' if dt == 'f32' else '16'}"
    _check(tag, path, K.judge_coef(r["coef"], d, e1))
    ref1, scale1, e_apply, ref2, B = _apply_refs(d, r["coef"], relu, e1)
    got = r["gx"]
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} elements of gx were never written or are not finite"
    if dt == "f32":
        ratios = {"gx alone": R.ratio_units(got, ref1, scale1, e_apply), "gx": R.ratio_band(got, ref2, B)}
        _check(tag, path, ratios, {"gx alone": e_apply})
    else:
        bad1, bad2 = R.outside16_abs(got, ref1, R.band(e_apply) * scale1, dt), R.outside16_abs(got, ref2, B, dt)
        print(f"NORM_ERR {tag} -> {path}: {bad1} / {bad2} of {got.size} stored elements outside their interval (apply alone / end to end)")
        assert bad1 == 0 and bad2 == 0, f"{tag}: stored elements outside [round16(ref - band), round16(ref + band)]"
        # the contract of tests/test_gpu_storage16.py: the 16-bit launch is the rounded fp32 launch on the same values
        r32 = _launch_apply(name, "f32", relu, d)
        assert np.array_equal(r32["coef"], r["coef"]), f"{tag}: the reduction of the same values gives the same coef bits"
        rounded = torch.from_numpy(r32["gx"]).to(TORCH[dt]).contiguous().view(torch.int16).reshape(-1)
        diff = int((rounded != r["bits"].cpu().reshape(-1)).sum())
        print(f"NORM_BITS {tag}: {diff} of {rounded.numel()} elements differ from the rounded fp32 launch")
        assert diff == 0, f"{tag}: the 16-bit launch is not the rounded fp32 launch on the same values ({diff} elements)"
    if inplace:        # gx aliasing gy, the way the engine calls it
        ri = _launch_apply(name, dt, relu, d, inplace=True)
        assert torch.equal(ri["bits"], r["bits"]) and ri["ag"] == r["ag"], f"{tag}: in place (gx = gy) gives the same bits"
    if amax:
        want_bits = int(f32(np.abs(got).max()).view(np.uint32))
        n, v, c, val = K.amax_spike(name)
        assert np.abs(got[n, v, c]) == np.abs(got).max(), f"{tag}: max |gx| is an element of the last block"
        print(f"NORM_AMAX {tag}: word {r['word']:#x}, max |gx| as stored {want_bits:#x}")
        assert r["word"] == want_bits, f"{tag}: out_amax {r['word']:#x} is not the bit pattern of max |gx| {want_bits:#x}"
        big, small = 3.0e4, 1.0e-3
        assert small < np.abs(got).max() < big
        assert _launch_apply(name, dt, relu, d, amax_preset=big)["word"] == int(f32(big).view(np.uint32)), f"{tag}: a larger word stays"
        assert _launch_apply(name, dt, relu, d, amax_preset=small)["word"] == want_bits, f"{tag}: a smaller word is replaced"
