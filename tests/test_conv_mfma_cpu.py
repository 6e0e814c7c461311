"""The float64 references of the matrix-core forward / data-gradient convolutions (oracle/conv_mfma_ref.py), the case table of
tests/test_gpu_conv_mfma.py (oracle/conv_mfma_cases.py) and the judge, without a GPU.

  * the operand model of every mode and the independently stated data gradient against torch float64 conv3d /
    torch.nn.grad.conv3d_input ON THE MODELLED OPERANDS, within 1e-12 of the scale;
  * for every case of the table: the kernel and instantiation it is meant for, the restated dispatch rules and the library's own
    query (tem_conv3d_fwd_mfma_path: host code, no device) agree; REQUIRED -- the instantiations the suite undertakes to reach;
    DESIGN.md names the ones it leaves out -- is reached by lattice cases and the table reaches nothing that is not listed; every
    lattice and split case has sum |terms| / step < 2^24 and inputs its split reproduces exactly;
  * the judge rejects planted errors and accepts the float32 restatement.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_mfma_cases as K
from oracle import conv_mfma_ref as M
from oracle import conv_ref as R


def _lib():
    from torch_em_amd import _lib
    return _lib


def _close(a, b, scale):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / (np.asarray(scale) + 1e-300))) <= 1e-12


def _ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 4, 1, 2, 3)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------------- float64 against torch
@pytest.mark.parametrize("mode", sorted(M.TERMS))
@pytest.mark.parametrize("k", (K.K333, K.K133, K.K111), ids=lambda k: "".join(map(str, k)))
def test_operand_models_against_torch(mode, k):
    rng = np.random.RandomState(3 + mode + sum(k))
    N, D, H, W, Cin, Cout = 2, 3, 5, 4, 3, 4
    x = rng.randn(N, D, H, W, Cin).astype(np.float32)
    w_sd = (0.3 * rng.randn(Cout, Cin, R.ntaps(k))).astype(np.float32)
    scale, shift = rng.uniform(0.5, 2, (N, Cin)).astype(np.float32), rng.randn(N, Cin).astype(np.float32)
    bias = rng.randn(Cout).astype(np.float32)
    pad = tuple(s // 2 for s in k)
    xh = M.xhat32(x, scale, shift)
    assert np.array_equal(xh, xh.astype(np.float32).astype(np.float64)), "xhat is a float32 number"
    fm = (x.astype(np.float64) * scale.astype(np.float64)[:, None, None, None, :] + shift.astype(np.float64)[:, None, None, None, :])
    assert np.max(np.abs(xh - fm)) <= 2.0 ** -24 * np.max(np.abs(fm)) * 1.0001, "... one rounding away from the exact fma"
    px, pw = M.planes(xh, mode, "x"), M.planes(w_sd, mode, "w")
    # the planes are numbers of the mode's element type and add up to the operand within the mode's precision
    kind = {1: None, 2: "bf16", 3: "bf16", 4: "f16", 5: "f16", 6: "f16", 7: "bf16"}[mode]
    for p in px + pw:
        assert kind is None or np.array_equal(M.round16(p, kind), p)
    if mode == M.F16X3:
        assert np.max(np.abs(px[0] + px[1] / 4096 - xh)) <= 2.0 ** -21 * np.max(np.abs(xh))
    if mode in (M.BF16X3, M.BF16X6):
        assert np.max(np.abs(sum(px) - xh)) <= 2.0 ** (-15 if mode == M.BF16X3 else -22) * np.max(np.abs(xh))
    # the terms, by torch float64 conv3d on the modelled operands
    want = [0.0, 0.0]
    for i, j, a in M.TERMS[mode]:
        wt = torch.from_numpy(pw[j]).reshape(Cout, Cin, *k)
        want[a] = want[a] + _cl(F.conv3d(_ncdhw(px[i]), wt, None, padding=pad))
    acc, mag, _ = M.accumulate(xh, w_sd, k, mode)
    for a in range(len(acc)):
        assert _close(acc[a], want[a], mag / M.OUT_SCALE.get(mode, 1.0) / M.ACC_SCALE.get(mode, (1, 1))[a] + 1e-300), f"accumulator {a}"
    r = M.fwd_model(x, w_sd, k, mode, bias, scale, shift, R.RELU, None)
    sc = M.ACC_SCALE.get(mode, (1.0, 1.0))
    lin = (want[0] * sc[0] + (want[1] * sc[1] if len(acc) > 1 else 0.0)) * M.OUT_SCALE.get(mode, 1.0) + bias.astype(np.float64)
    assert _close(r["y"], np.maximum(lin, 0), r["mag"]) and np.all(r["mag"] >= np.abs(r["lin"]) * (1 - 1e-12))
    if mode in (1, 3):
        full, fmag = R.fwd_f64(x, M.generic(w_sd), k, bias, scale, shift)
        assert np.max(np.abs(r["lin"] - full) / fmag) < 2.0 ** -20, "fp32-class modes reproduce the fp32 convolution"
    # the data gradient, stated on its own, against torch's conv3d_input on the modelled operands
    g = rng.randn(N, D, H, W, Cout).astype(np.float32)
    pg = M.planes(g, mode, "x")
    wantd = [0.0, 0.0]
    for i, j, a in M.TERMS[mode]:
        wt = torch.from_numpy(pw[j]).reshape(Cout, Cin, *k)
        wantd[a] = wantd[a] + _cl(torch.nn.grad.conv3d_input((N, Cin, D, H, W), wt, _ncdhw(pg[i]), padding=pad))
    accd, magd, _ = M.accumulate(g, w_sd, k, mode, dgrad=True)
    for a in range(len(accd)):
        assert _close(accd[a], wantd[a], magd / M.OUT_SCALE.get(mode, 1.0) / M.ACC_SCALE.get(mode, (1, 1))[a] + 1e-300), f"dgrad accumulator {a}"


def test_refnorm_gscaled_and_statistics_rows():
    rng = np.random.RandomState(9)
    c = K.BY_ID["zr_rag-m2f32-macd"]
    d = K.inputs(c)
    r = K.model(c, d)
    plain = M.fwd_model(d["x"], d["w_sd"], c.k, c.mode, dgrad=True)["y"]
    a, m1, m2r, mean = (d["coef"][..., j].astype(np.float64)[:, None, None, None, :] for j in range(4))
    ref = d["ref"].astype(np.float64)
    assert np.array_equal(r["y"], np.where(ref > 0, a * plain - m1 - (ref - mean) * m2r, 0.0))
    assert M.gscale(4.0) == 2.0 ** 12 and M.gscale(7.9) == 2.0 ** 12 and M.gscale(8.0) == 2.0 ** 11 and M.gscale(0.0) == 1.0
    cg = K.BY_ID["zr_rag-m4f32-gd"]
    dg = K.inputs(cg)
    assert np.array_equal(K.model(cg, dg)["y"], M.fwd_model(dg["x"], dg["w_sd"], cg.k, 4, dgrad=True)["y"]), "exact on the lattice"
    y = rng.randn(2, 5, 9, 11, 4)
    rows, scales = M.linear_stats_f64(y, 64)
    v = y.reshape(2, -1, 4)
    assert rows.shape == (2, -(-495 // 64), 4, 2) and np.allclose(rows[1, 3, :, 0], v[1, 192:256].sum(axis=0), rtol=1e-13, atol=1e-13)
    assert np.allclose(rows[0, -1, :, 1], (v[0, 448:] ** 2).sum(axis=0), rtol=1e-13)
    t, ts = M.total_stats_f64(y)
    assert np.allclose(rows.sum(axis=1), t, rtol=1e-12, atol=1e-12) and np.all(ts[..., 0] >= np.abs(t[..., 0]))


# ------------------------------------------------------------------------------------------------------- the table
@pytest.fixture
def options():
    L, old = _lib(), {}

    def set_all(opts):
        for key, value in opts.items():
            old.setdefault(key, L.get_option(key))
            L.set_option(key, value)
    yield set_all
    for key, value in old.items():
        L.set_option(key, value)


def test_table_rules_and_query_agree_and_reach_every_instantiation(options):
    L = _lib()
    lib = L.load()
    assert {k: L.get_option(k) for k in K.DEFAULTS} == K.DEFAULTS, "the defaults the rules are restated for"
    ncu = lib.tem_device_cus()
    ncu = ncu if ncu > 0 else 256
    reached, bad = set(), []
    for c in K.CASES:
        options({**K.DEFAULTS, **c.opts})
        bp = K.fake_byproducts(L, c)
        kernel, inst = K.query(lib, c, K.fake_pointers(c), bp=ctypes.byref(bp) if bp is not None else None)
        ekernel, einst, eblk = K.expected(c, ncu)
        if (kernel, inst) != (ekernel, einst) or kernel != c.want:
            bad.append((c.id, K.NAME.get(kernel), inst, K.NAME.get(ekernel), einst, K.NAME[c.want]))
        if c.recipe == "lattice" and kernel > 0:
            reached.add((kernel, K.signature(kernel, inst)))
        if c.stat:
            x_ld, y_ld, ref_ld = c.lds()
            assert eblk == lib.tem_conv3d_fwd_stat_blocks_ld(*c.shape, c.cin, c.cout, *c.k, K.use_mfma(c), x_ld, y_ld, ref_ld, 0) > 0, c.id
        # about 10 GFLOP of float64 work per case, except on the split-K launch of the z-reuse kernel: it needs units x ks >= 2 per CU
        # with at least two 16-channel chunks per slice, i.e. NV Cin Cout >= 2^28 -- 14.5 GFLOP per term with 27 taps, three terms
        # on the split recipe (measured: 3 to 6 s for the case that sums such a layer first, shared by the cases behind it)
        assert c.flops64() < (50e9 if c.want == K.ZR_SPLITK or c.name == "zk" else 10e9), f"{c.id}: {c.flops64() / 1e9:.1f} GFLOP of float64 work"
    assert not bad, f"{len(bad)} cases: (id, query, inst, rules, inst, table) {bad[:6]}"
    missing = [(K.NAME[k], s) for k, s in K.REQUIRED if (k, s) not in reached]
    assert not missing, f"instantiations no lattice case reaches: {missing}"
    extra = [(K.NAME[k], s) for k, s in sorted(reached) if (k, s) not in K.REQUIRED]
    assert not extra, f"instantiations reached but not listed in REQUIRED: {extra}"
    print(f"\nCONV_MFMA_TABLE {len(K.CASES)} cases reach {len(reached)} instantiations, all {len(K.REQUIRED)} required ones")
    # every family forward and as a data gradient on the lattice, on wide buffers, and on random data; the split families on `split`
    for fam in (K.ZR, K.ZR_SPLITK, K.PP, K.PATCH, K.PATCH_FP32, K.STREAM):
        cs = [c for c in K.CASES if c.want == fam]
        assert any(c.dgrad and c.recipe == "lattice" for c in cs) and any(not c.dgrad and c.recipe == "lattice" for c in cs), K.NAME[fam]
        assert any(c.recipe == "random" for c in cs), K.NAME[fam]
        assert any(c.wide and c.ref for c in cs), f"{K.NAME[fam]}: x, y and ref as channels [8, 8 + C) of wider buffers"
        if fam != K.PATCH_FP32:
            assert any(c.recipe == "split" for c in cs), K.NAME[fam]
    assert any(c.ybuf for c in K.CASES if c.want == K.ZR_SPLITK), "y as a channel slice of a wider buffer"
    sk = [c for c in K.CASES if c.want == K.ZR_SPLITK and c.recipe == "split"]
    assert {c.mode for c in sk} == {2, 4} and any(c.dgrad for c in sk), "non-zero lo planes through the two-plane KSPLIT kernels"
    assert any(c.cs and c.dgrad for c in K.CASES) and any(c.cs and c.stat for c in K.CASES), "the chunk-stride layout"
    ksc = K.BY_ID["pt_ksc-m2f32-b"]
    assert K.expected(ksc, ncu)[1][K.KS] == 8 and K.patch_tiling(K.Case("x", 0, ksc.shape, 128, 256, K.K133, 2))["ks"] == 4, "fwd_ksplit_chunks"
    # the bwd_sums epilogue needs rows of its own geometry: any other sums_nblk gets the plain epilogue (and delivers nothing)
    su = K.BY_ID["zk-m2f32-mdu"]
    options({**K.DEFAULTS, **su.opts})
    bp = K.fake_byproducts(L, su)
    assert K.query(lib, su, K.fake_pointers(su), bp=ctypes.byref(bp))[1][K.EPI] == K.BWD_SUMS
    bp.sums_nblk += 1
    assert K.query(lib, su, K.fake_pointers(su), bp=ctypes.byref(bp))[1][K.EPI] == K.PLAIN
    # a team walks a second unit; the split-K slices of two chunks and of three
    walk = K.BY_ID["zr_walk-m2f32-brt"]
    assert K.zr_geometry(walk, 256)["nunits"] == 576 > 2 * 256 and K.expected(walk, 256)[0] == K.ZR, "more units than teams on 256 CUs"
    assert K.expected(K.BY_ID["zk-m2f32-b"], ncu)[1][K.KS] == 8 and K.expected(K.BY_ID["zk_odd-m5f32-b"], ncu)[1][K.KS] == 4
    # what the query refuses
    options(K.DEFAULTS)
    for c in (K.Case("x", -1, (2, 5, 17, 9), 32, 64, K.K333, 2, gscaled=True, opts={"conv_fwd_variant": 2}),
              K.Case("x", -1, (2, 5, 9, 9), 32, 64, K.K333, 2, refnorm=True, opts={"conv_fwd_variant": 1}),
              K.Case("x", -1, (2, 3, 9, 11), 32, 64, K.K333, 2, stat=True, opts={"conv_fwd_variant": 0}),
              K.Case("x", -1, (2, 3, 9, 11), 32, 64, K.K333, 2, st="f16"),
              K.Case("x", -1, (2, 5, 9, 9), 64, 64, K.K333, 5, st="f16", cs=True, opts={"conv_fwd_variant": 0}),      # chunk strides off the z-reuse kernel
              K.Case("x", -1, (2, 5, 17, 9), 64, 64, K.K333, 5, st="f16", cs=True, ref=True, opts={"conv_fwd_variant": 2}),
              K.Case("x", -1, (2, 3, 9, 11), 24, 64, K.K333, 2)):
        options({**K.DEFAULTS, **c.opts})
        assert K.query(lib, c, K.fake_pointers(c))[0] == -1 == K.expected(c, ncu)[0], c.id
    options(K.DEFAULTS)
    zk = K.BY_ID["zk-m2f32-brt"]
    assert K.query(lib, zk, K.fake_pointers(zk), ws_bytes=1024)[0] == -1, "statistics of the split-K launch need its workspace"
    zk = K.BY_ID["zk-m2f32-b"]
    assert K.query(lib, zk, K.fake_pointers(zk), ws_bytes=0)[0] == K.PATCH, "without a workspace the patch kernel runs, unsplit"
    lib.tem_last_error()


def test_lattice_and_split_cases_are_exact_in_float32():
    worst, seen, checked = {}, {}, set()
    for c in K.CASES:
        if c.recipe == "random":
            continue
        key = (c.name, c.shape, c.cin, c.cout, c.k, c.bias, c.norm, c.refnorm, c.gscaled, c.dgrad, c.recipe, c.mode if c.recipe == "split" else 0)
        if key not in seen:
            d = K.inputs(c)
            seen[key] = (K.lattice_bounds(c, d), d)
        bounds, d = seen[key]
        for b in bounds:
            assert b < 2 ** 24, f"{c.id}: sum |terms| / step = 2^{np.log2(b):.2f}"
            worst[c.recipe, c.mode if c.recipe == "split" else 0] = max(worst.get((c.recipe, c.mode if c.recipe == "split" else 0), 0), b)
        okey = (c.name, c.shape, c.cin, c.cout, c.k, c.dgrad, c.recipe, c.norm, c.mode)       # the operands and the mode that splits them
        if okey in checked:
            continue
        checked.add(okey)
        xh = M.xhat32(d["x"], d["scale"], d["shift"])
        px, pw = M.planes(xh, c.mode, "x"), M.planes(d["w_sd"], c.mode, "w")
        assert M.reproduces(xh, c.mode, "x") and M.reproduces(d["w_sd"], c.mode, "w"), f"{c.id}: the split reproduces the operands"
        if c.recipe == "lattice":
            for key in ("x", "w_sd", "bias", "scale", "shift", "ref", "coef", "sums_x", "sums_mean", "sums_rstd"):
                if d[key] is not None:
                    assert np.array_equal(R.round16(R.round16(d[key], "f16"), "bf16"), d[key]), f"{c.id}: {key} is exact in every type"
            assert all(not p.any() for p in px[1:] + pw[1:]), f"{c.id}: the lo planes are zero"
        else:
            assert all(p.any() for p in px + pw), f"{c.id}: the lo planes are not zero"
    for (recipe, mode), b in sorted(worst.items()):
        print(f"\nCONV_MFMA_LATTICE {recipe}{' mode %d' % mode if mode else ''}: worst sum |terms| / step = 2^{np.log2(b):.1f}")


# ------------------------------------------------------------------------------------------------------- the judge on planted errors
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def test_the_judge_rejects_planted_errors_and_accepts_the_restatement():
    c = K.BY_ID["zr_rag-m2f32-"]
    d = K.inputs(c)
    y = K.model(c, d)["y"]
    want = M.exact_store(y, c.mode, "f32")
    assert M.mismatches(_f32(y), want) == 0, "the exact value passes"
    x64, w = d["x"].astype(np.float64), M.generic(d["w_sd"])
    # 1. a missing tap at one border voxel
    term = None
    for v in [(n, z, yy, xx) for n in (0, 1) for z in (0, 4) for yy in (0, 16) for xx in (0, 8)]:
        for tap, dz, dy, dx in R.taps(c.k):
            z2, y2, x2 = v[1] + dz, v[2] + dy, v[3] + dx
            if 0 <= z2 < 5 and 0 <= y2 < 17 and 0 <= x2 < 9 and x64[v[0], z2, y2, x2, 0] * w[tap, 0, 0] != 0:
                term = (v, x64[v[0], z2, y2, x2, 0] * w[tap, 0, 0])
    bad = y.copy()
    bad[term[0] + (0,)] -= term[1]
    assert M.mismatches(_f32(bad), want) == 1, "one missing tap at a border voxel"
    # 2. one lo hi cross term dropped in one 16-channel chunk (the split recipe: on the lattice the lo planes are zero)
    cs = K.BY_ID["zr_split-m2f32--split"]
    ds = K.inputs(cs)
    ys = M.exact_store(K.model(cs, ds)["y"], 2, "f32")

    def drop(i, j, px, pw):
        if (i, j) == (1, 0):
            px = px.copy()
            px[..., 16:32] = 0.0
        return px, pw
    assert M.mismatches(_f32(K.model(cs, ds, skip=drop)["y"]), ys) > 0.5 * ys.size, "a lo hi term dropped in one chunk"
    lat = M.mismatches(_f32(K.model(c, d, skip=drop)["y"]), want)
    assert lat == 0, "(the lattice does not see it: that is what the split recipe is for)"
    # 3. one chunk skipped in one split-K slice: channels [16, 32) of every term never reach the sum
    def chunk(i, j, px, pw):
        px = px.copy()
        px[..., 16:32] = 0.0
        return px, pw
    assert M.mismatches(_f32(K.model(c, d, skip=chunk)["y"]), want) > 0.5 * want.size, "a chunk skipped"
    # 4. a halo plane reused one step late in z: output plane 2 reads plane 2 where it should read plane 3
    late = d["x"].copy()
    late[:, 3] = late[:, 2]
    ylate = y.copy()
    ylate[:, 2] = M.fwd_model(late, d["w_sd"], c.k, c.mode)["y"][:, 2]
    assert M.mismatches(_f32(ylate), want) > 0, "a halo plane one step late"
    # 5. >= for > in the mask (ref holds 0 and -0.0)
    cm = K.BY_ID["zr_rag-m2f32-m"]
    dm = K.inputs(cm)
    ym = K.model(cm, dm)["y"]
    assert np.signbit(dm["ref"][dm["ref"] == 0]).any() and (dm["ref"] == 0).any()
    assert M.mismatches(_f32(np.where(dm["ref"] >= 0, y, 0.0)), M.exact_store(ym, 2, "f32")) > 0, ">= for > in the mask"
    assert M.mismatches(_f32(np.where(dm["ref"] > 0, y, 0.0)), M.exact_store(ym, 2, "f32")) == 0
    # 6. a statistic of the unrounded 16-bit value
    cr = K.BY_ID["zr_rnd16-m5f16-b-random"]
    rr = K.reference(cr)
    st = M.stored(_f32(rr["y"]), "f16")
    rows, scales = R.block_stats_f64(st, (4, 16, 8))
    e32 = R.block_stats_e32(st, (4, 16, 8), rows, scales)
    unr, _ = R.block_stats_f64(_f32(rr["y"]), (4, 16, 8))
    for q in (0, 1):
        assert M.within(M.units(_f32(rows[..., q]), rows[..., q], scales[..., q]), e32[q]), "float32 sums of the stored values pass"
        assert not M.within(M.units(unr[..., q], rows[..., q], scales[..., q]), e32[q]), "sums of the unrounded values"
    # 7. the data gradient with unflipped taps
    cd = K.BY_ID["zr_tile-m2f32-d"]
    dd = K.inputs(cd)
    yd = M.exact_store(K.model(cd, dd)["y"], 2, "f32")
    unflipped, _ = R.conv_f64(dd["x"], np.transpose(dd["w_sd"].astype(np.float64), (2, 0, 1)), cd.k)      # [tap][co of the layer][ci]
    flipped, _ = R.conv_f64(dd["x"], np.transpose(dd["w_sd"].astype(np.float64), (2, 0, 1))[::-1], cd.k)
    assert M.mismatches(_f32(flipped), yd) == 0 and M.mismatches(_f32(unflipped), yd) > 0.5 * yd.size, "dgrad with unflipped taps"
    # 8. an 8-ulp scale on one output channel, on a lattice
    s8 = _f32(y)
    s8[..., 3] = (s8[..., 3].astype(np.float32) * np.float32(1 + 8 * 2.0 ** -23)).astype(np.float64)
    assert M.mismatches(s8, want) > 0, "8 ulp on one channel"
    # mode 4 joins its accumulators with ONE rounding: float32(exact), not the sum of two rounded parts
    c4 = K.BY_ID["zr_split-m4f32--split"]
    d4 = K.inputs(c4)
    x4 = M.xhat32(d4["x"], None, None)
    acc, _, _ = M.accumulate(x4, d4["w_sd"], c4.k, 4)
    y4 = M.exact_store(M.join(acc, 4), 4, "f32")
    assert M.mismatches(_f32(K.model(c4, d4)["y"]), y4) == 0
    assert M.mismatches(_f32(acc[0]), y4) > 0.5 * y4.size, "the 2^-12 rejoin left out"
    # the float32 restatement on random data is accepted; 64 ulp on one channel is not; a 16-bit element outside its interval
    cq = K.BY_ID["zr_rnd-m2f32-bnrt-random"]
    dq = K.inputs(cq)
    rq = K.reference(cq, dq)
    assert M.within(rq["e32"], rq["e32"]) and M.within(M.units(_f32(rq["y"]), rq["y"], rq["mag"]), rq["e32"])
    ud = M.units(_f32(K.model(cq, dq, skip=drop)["y"]), rq["y"], rq["mag"])
    print(f"\nCONV_MFMA_JUDGE {cq.id}: e32 {rq['e32']:.2f}; a lo hi term dropped in one chunk: {ud:.1f} units")
    assert not M.within(ud, rq["e32"]), "a lo hi term dropped in one chunk, on random data"
    st16 = M.stored(rr["y"], "f16")
    assert M.outside16(st16, rr["y"], rr["mag"], rr["e32"], "f16") == 0
    st16[0, 0, 3, 3, 1] += 2 * abs(st16[0, 0, 3, 3, 1]) * 2.0 ** -10 + 2.0 ** -20
    assert M.outside16(st16, rr["y"], rr["mag"], rr["e32"], "f16") == 1
