"""The float64 references of the VALU convolution kernels (oracle/conv_ref.py), the case tables of tests/test_gpu_conv_valu.py
(oracle/conv_cases.py) and the judge, without a GPU.

  * conv_ref's float64 functions against torch float64 F.conv3d and its autograd, at every kernel size, within 1e-12 of the scale;
  * for every case of the tables: the kernel it is meant for, the documented selector rules and the library's own dispatch
    query (tem_conv3d_fwd_valu_path / tem_conv3d_wgrad_path: host code, no device) name the same kernel and instantiation, every
    instantiation and loop trip is reached by a lattice case, and for every lattice case sum |terms| / step < 2^24 (so that
    equality with float64 is the right judge for a float32 kernel);
  * the judge rejects planted errors.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_cases as K
from oracle import conv_ref as R

ST = {"f32": 0, "f16": 1, "bf16": 2}


def _mode(pair):
    return (ST[pair[0]] << 8) | (ST[pair[1]] << 12)              # TEM_MFMA_STX | TEM_MFMA_STY over use_mfma 0


def _w_torch(w, k):
    """[tap][ci][co] -> torch's [co][ci][kd][kh][kw]"""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(w, (2, 1, 0)))).reshape(w.shape[2], w.shape[1], *k)


def _cl(t):
    """torch [N, C, D, H, W] -> numpy channels-last"""
    return t.detach().permute(0, 2, 3, 4, 1).contiguous().numpy()


def _close(a, b, scale):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / (np.asarray(scale) + 1e-300))) <= 1e-12


# ------------------------------------------------------------------------------------------------------- float64 against torch
@pytest.mark.parametrize("k", K.KSIZES, ids=lambda k: "".join(map(str, k)))
def test_float64_references_against_torch(k):
    rng = np.random.RandomState(5 + sum(k))
    N, D, H, W, Cin, Cout = 2, 3, 5, 4, 3, 4
    x, g = rng.randn(N, D, H, W, Cin), rng.randn(N, D, H, W, Cout)
    w, bias = rng.randn(R.ntaps(k), Cin, Cout), rng.randn(Cout)
    scale, shift = rng.uniform(0.5, 2, (N, Cin)), rng.randn(N, Cin)
    ref = rng.randn(N, D, H, W, Cout)
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3)
    xh = (xt * torch.from_numpy(scale)[:, :, None, None, None] + torch.from_numpy(shift)[:, :, None, None, None]).requires_grad_(True)
    wt, bt = _w_torch(w, k).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    lin = F.conv3d(xh, wt, bt, padding=tuple(s // 2 for s in k))
    for act, fn in ((R.NONE, lambda t: t), (R.RELU, torch.relu), (R.SIGMOID, torch.sigmoid)):
        y, mag = R.fwd_f64(x, w, k, bias, scale, shift, act, None)
        assert _close(y, _cl(fn(lin)), mag), f"forward, act {act}"
        ym, _ = R.fwd_f64(x, w, k, bias, scale, shift, act, ref)
        assert _close(ym, _cl(fn(lin)) * (ref > 0), mag), f"forward with ref, act {act}"
    y0, m0 = R.fwd_f64(x, w, k)
    assert _close(y0, _cl(F.conv3d(xt, _w_torch(w, k), None, padding=tuple(s // 2 for s in k))), m0), "no bias, no pre-norm"
    # weight and bias gradient: autograd of sum(conv * g)
    (lin * torch.from_numpy(g).permute(0, 4, 1, 2, 3)).sum().backward()
    dw, db, mag, dbmag = R.wgrad_f64(x, g, k, scale, shift)
    assert _close(R.to_sd(dw, k), wt.grad.reshape(Cout, Cin, -1).numpy(), R.to_sd(mag, k)), "dw in state_dict order"
    assert _close(dw, np.transpose(wt.grad.reshape(Cout, Cin, -1).numpy(), (2, 1, 0)), mag), "dw tap-major"
    assert _close(db, bt.grad.numpy(), dbmag), "db"
    # the norm backward on load: the gradient a ReLU + affine-free norm passes down, as a formula
    coef = np.stack([rng.uniform(0.5, 2, (N, Cout)), rng.randn(N, Cout), rng.randn(N, Cout), rng.randn(N, Cout)], axis=-1)
    yv = rng.randn(N, D, H, W, Cout)
    a, m1, m2r, mean = (torch.from_numpy(coef[..., j])[:, None, None, None, :] for j in range(4))
    gn_t = torch.where(torch.from_numpy(yv) > 0, a * torch.from_numpy(g) - m1 - (torch.from_numpy(yv) - mean) * m2r, torch.zeros(()).double())
    gn, gmag = R.gnorm_f64(g, yv, coef)
    assert _close(gn, gn_t.numpy(), gmag + 1e-300) and np.all(gn[yv <= 0] == 0)
    dwg, dbg, magg, dbmagg = R.wgrad_gnorm_f64(x, g, yv, coef, k, scale, shift)
    dw2, db2, _, _ = R.wgrad_f64(x, gn_t.numpy(), k, scale, shift)
    assert _close(dwg, dw2, magg) and _close(dbg, db2, dbmagg) and np.all(magg >= np.abs(dwg) * (1 - 1e-12))


def test_out_bwd_and_block_statistics_against_torch():
    rng = np.random.RandomState(11)
    NV, Cin, Cout = 50, 6, 3
    x, g, w = rng.randn(1, 1, 1, NV, Cin), rng.randn(1, 1, 1, NV, Cout), rng.randn(Cout, Cin)
    x[0, 0, 0, :5] = 0.0
    xt = torch.from_numpy(x).requires_grad_(True)
    (F.linear(torch.relu(xt), torch.from_numpy(w)) * torch.from_numpy(g)).sum().backward()
    gx, mag = R.out_bwd_f64(x, g, w)
    assert _close(gx, xt.grad.numpy(), mag + 1e-300)
    dw, db, _, _ = R.wgrad_f64(np.maximum(x, 0), g, K.K111)
    wt = torch.from_numpy(w).requires_grad_(True)
    (F.linear(torch.relu(torch.from_numpy(x)), wt) * torch.from_numpy(g)).sum().backward()
    assert _close(R.to_sd(dw, K.K111)[..., 0], wt.grad.numpy(), 1.0 + np.abs(wt.grad.numpy()))
    y = rng.randn(2, 5, 9, 35, 4)
    for tile in ((4, 8, 8), (4, 8, 32)):
        rows, scales = R.block_stats_f64(y, tile)
        nz, ny, nx = 2, 2, -(-35 // tile[2])
        assert rows.shape == (2, nz * ny * nx, 4, 2)
        blk = y[1, 4:8, 8:16, tile[2]:2 * tile[2]]                  # block (z 1, y 1, x 1): x fastest
        i = (1 * ny + 1) * nx + 1
        assert np.allclose(rows[1, i, :, 0], blk.sum(axis=(0, 1, 2)), rtol=1e-13, atol=1e-13)
        assert np.allclose(rows[1, i, :, 1], (blk * blk).sum(axis=(0, 1, 2)), rtol=1e-13)
        assert np.allclose(rows.sum(axis=1)[..., 0], y.sum(axis=(1, 2, 3)), rtol=1e-12, atol=1e-12)
        assert np.all(scales[..., 0] >= np.abs(rows[..., 0]) - 1e-12)


# ------------------------------------------------------------------------------------------------------- the tables
def _lib():
    from torch_em_amd import _lib
    return _lib.load()


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


def fwd_query(lib, c):
    """the query for the addresses a Laid layout of the case's tensors has"""
    N, D, H, W = c.shape
    x_ld, y_ld, ref_ld = c.lds()
    inst = (ctypes.c_int * 4)()
    path = lib.tem_conv3d_fwd_valu_path(
        _p(K.address(c.pair[0], (c.xlay or (0, 0))[1])), x_ld, _p(K.BASE if c.norm else 0), _p(K.BASE if c.norm else 0), _p(K.BASE),
        _p(K.address("f32", 0, c.bias_off) if c.bias else 0), _p(K.address(c.pair[1], (c.ylay or (0, 0))[1])), y_ld,
        _p(K.address(c.pair[1], (c.reflay or (0, 0))[1]) if c.ref else 0), ref_ld, N, D, H, W, c.cin, c.cout, *c.k, c.act, _mode(c.pair),
        int(c.stat), inst)
    return path, list(inst)


def test_every_forward_case_names_its_kernel():
    lib = _lib()
    reached, bad = set(), []
    for c in K.FWD:
        path, inst = fwd_query(lib, c)
        epath, einst = K.expected_fwd(c)
        if c.recipe == "lattice" and path >= 0:
            reached.add((path, tuple(inst)))
        if (path, inst) != (epath, einst) or path != c.want or (c.inst and inst != c.inst):
            bad.append((c.id, K.FWD_NAME.get(path), inst, K.FWD_NAME.get(epath), einst, c.want))
        assert c.bytes_moved() < 40e6, f"{c.id}: a case moves less than 40 MB"
        if c.stat and path >= 0:
            assert K.stat_blocks(c) == lib.tem_conv3d_fwd_stat_blocks(*c.shape, c.cin, c.cout, *c.k, _mode(c.pair)) > 0, c.id
    assert not bad, f"{len(bad)} cases: (id, query, inst, rules, inst, table) {bad[:8]}"
    missing = [(K.FWD_NAME[p], i) for p, i in K.FWD_REQUIRED if (p, i) not in reached]
    assert not missing, f"instantiations no lattice case reaches: {missing}"
    # the loop trips the issue names
    ids = {c.name: c for c in K.FWD}
    assert ids["projr_2_1_trip2"].nv > 4096 * 32 and ids["projr_16_2_trip2"].nv > 4096 * 32, "past the 4096-block cap"
    assert ids["expand_q_carry"].nv * 9 > 4096 * 256 and (4096 * 256) % 9, "cq = 9 does not divide the stride"
    assert ids["generic_co_carry"].nv * 5 > 4096 * 256 and (4096 * 256) % 5, "Cout = 5 does not divide the stride"
    assert lib.tem_conv3d_fwd_stat_blocks(2, 5, 9, 11, 1, 12, 3, 3, 3, 0) == 0 and ids["cin1_nostat"].want == -1


def wg_query(lib, c, ws_bytes=None):
    N, D, H, W = c.shape
    x_ld = (c.xlay or (c.cin,))[0]
    ws = lib.tem_conv3d_wgrad_ws(N, D, H, W, c.cin, c.cout, *c.k, 0) if ws_bytes is None else ws_bytes
    return lib.tem_conv3d_wgrad_path(
        _p(K.address(c.pair[0], (c.xlay or (0, 0))[1])), x_ld, _p(K.BASE if c.norm else 0), _p(K.BASE if c.norm else 0),
        _p(K.address(c.pair[1], (c.glay or (0, 0))[1])), (c.glay or (c.cout,))[0],
        _p(K.address(c.pair[1], (c.ylay or (0, 0))[1]) if c.gnorm else 0), (c.ylay or (c.cout,))[0], _p(K.BASE if c.gnorm else 0), int(c.db), ws,
        N, D, H, W, c.cin, c.cout, *c.k, _mode(c.pair), c.sd)


def test_every_weight_gradient_case_names_its_kernel():
    lib = _lib()
    bad, reached = [], set()
    for c in K.WG:
        path = wg_query(lib, c)
        if path != c.want or path != K.expected_wgrad(c):
            bad.append((c.id, K.WG_NAME.get(path), K.WG_NAME.get(K.expected_wgrad(c)), c.want))
        if c.recipe == "lattice":
            reached.add((path, c.cin, c.cout, c.k[0]))
            if c.gnorm:
                reached.add(("gnorm", c.cin, c.cout, c.k[0], c.shape))
        assert c.bytes_moved() < 40e6
    assert not bad, f"{len(bad)} cases: (id, query, rules, table) {bad[:8]}"
    for cin in (1, 2, 3, 4):
        for cout in (4, 8, 16, 32, 64):
            assert (K.WG_CIN1, cin, cout, 3) in reached and (K.WG_CIN1, cin, cout, 1) in reached
            assert all(("gnorm", cin, cout, kd, (2, 5, 9, 11)) in reached for kd in (1, 3)), "the norm backward on load at the same shapes"
    assert ("gnorm", 1, 4, 3, (1, 4, 264, 256)) in reached, "... and where workgroups walk two patches"
    # every fast path also runs on buffers wider than its tensors (a kernel that strode by C instead of ld would pass the dense cases)
    wide = {c.want for c in K.FWD if c.recipe == "lattice" and c.xlay and c.ylay and c.lds()[0] > c.cin and c.lds()[1] > c.cout}
    assert wide >= {K.C1ROWS, K.CIN1, K.COUT1, K.PROJ_R, K.PROJ, K.EXPAND}
    assert any(c.reflay and c.lds()[2] > c.cout and c.want == K.EXPAND for c in K.FWD)
    assert {c.want for c in K.WG if c.xlay and c.glay and c.glay[0] > c.cout} >= {K.WG_CIN1, K.WG_PROJ}
    assert any(c.gnorm and c.ylay and c.ylay[0] > c.cout for c in K.WG)
    n = 0
    for nj in (1, 2, 4):
        for co in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32):
            if K.proj_wgrad_takes(32 * nj, co):
                n += 1
                assert (K.WG_PROJ, 32 * nj, co, 1) in reached
    assert n == 24, "the 24 <COUT, NJ> instantiations of k_conv1x1_proj_wgrad"
    two = K.WG_BY_ID["wc1_two_patches-f32.f32-sd1b"]
    assert -(-two.shape[1] // 4) * -(-two.shape[2] // 8) * -(-two.shape[3] // 8) > 1024, "workgroups walk two patches"
    assert K.WG_BY_ID["pw_2_1_trip2-f32.f32-sd1b"].nv > 1024 * 32
    # what the query refuses: gcoef on a plan that is not cin1, a workspace that is too small, the pair f16 / bf16
    c = K.WG_BY_ID["wgen_333-f32.f32-sd0b"]
    assert wg_query(lib, c, 16) == -1
    g = K.Wg("x", -1, c.shape, c.cin, c.cout, c.k, gnorm=True)
    assert K.expected_wgrad(g) == -1 and wg_query(lib, g) == -1
    assert wg_query(lib, K.Wg("x", -1, (2, 5, 9, 11), 1, 8, K.K333, pair=("f16", "bf16"))) == -1
    assert fwd_query(lib, K.Fwd("x", -1, (2, 5, 9, 11), 1, 8, K.K333, pair=("f16", "bf16")))[0] == -1
    assert {(ci // 32, co) for ci, co, _, r in K.OUT_BWD if r == "lattice"} == {(j, o) for j in (1, 2) for o in (1, 2, 3, 4)}
    for ci, co, _, _ in K.OUT_BWD:
        assert lib.tem_conv1x1_out_bwd_ok(ci, co) == 1


def test_lattice_cases_are_exact_in_float32():
    worst = 0.0
    for c in K.FWD:
        if c.recipe == "lattice" and c.want != -1:
            d = K.fwd_inputs(c)
            b = K.fwd_lattice_bound(c, d)
            worst = max(worst, b)
            assert b < 2 ** 24, f"{c.id}: sum |terms| / step = {b}"
            for key in ("x", "w", "bias", "scale", "shift", "ref"):
                if d[key] is not None:
                    assert np.array_equal(R.round16(R.round16(d[key], "f16"), "bf16"), d[key]), f"{c.id}: {key} is exact in every type"
    for c in K.WG:
        if c.recipe == "lattice":
            r = K.wg_reference(c)
            b = max(R.lattice_bound(r["mag"], K.wg_step(c)), R.lattice_bound(r["dbmag"], K.wg_step(c)))
            worst = max(worst, b)
            assert b < 2 ** 24, f"{c.id}: sum |terms| / step = {b}"
            q = r["dw"] / K.wg_step(c)
            assert np.array_equal(q, np.rint(q)), f"{c.id}: every dw is a multiple of the step"
    for cin, cout, _, recipe in K.OUT_BWD:
        if recipe == "lattice":
            d = K.out_bwd_inputs(cin, cout, recipe)
            _, mag = R.out_bwd_f64(d["x"], d["g"], d["w"])
            assert R.lattice_bound(mag, 0.25) < 2 ** 24
            assert np.signbit(d["x"][d["x"] == 0]).any() and (d["x"] < 0).any(), "x holds -0.0 and negative values"
    print(f"\nCONV_VALU_LATTICE worst sum |terms| / step = 2^{np.log2(worst):.1f}")


# ------------------------------------------------------------------------------------------------------- the judge on planted errors
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def test_the_judge_rejects_planted_errors():
    c = K.FWD_BY_ID["c1r_b32-f32.f32-b"]
    d = K.fwd_inputs(c)
    y = K.fwd_reference(c, d)["y"]
    assert R.mismatches(_f32(y), y) == 0, "the exact value passes"
    # 1. one missing tap at a border voxel
    xh = R.xhat(d["x"], d["scale"], d["shift"])
    term = None
    for v in [(n, z, yy, x) for n in range(2) for z in (0, 4) for yy in (0, 8) for x in (0, 40)]:
        for tap, dz, dy, dx in R.taps(c.k):
            z2, y2, x2 = v[1] + dz, v[2] + dy, v[3] + dx
            if 0 <= z2 < 5 and 0 <= y2 < 9 and 0 <= x2 < 41 and xh[v[0], z2, y2, x2, 0] * d["w"][tap, 0, 0] != 0:
                term = (v, xh[v[0], z2, y2, x2, 0] * d["w"][tap, 0, 0])
    assert term is not None
    bad = y.copy()
    bad[term[0] + (0,)] -= term[1]
    assert R.mismatches(_f32(bad), y) == 1, "one missing tap at a border voxel"
    # 2. bias added twice
    assert R.mismatches(_f32(y + d["bias"]), y) > 0, "bias added twice"
    # 3. >= for > in a mask (ref holds 0 and -0.0)
    cm = K.FWD_BY_ID["expand_2_32_ref-f32.f32-bma"]
    dm = K.fwd_inputs(cm)
    ym, _ = R.fwd_f64(dm["x"], dm["w"], cm.k, dm["bias"], None, None, cm.act, dm["ref"])
    yu, _ = R.fwd_f64(dm["x"], dm["w"], cm.k, dm["bias"], None, None, cm.act, None)
    assert np.signbit(dm["ref"][dm["ref"] == 0]).any()
    assert R.mismatches(_f32(np.where(dm["ref"] >= 0, yu, 0.0)), ym) > 0, ">= for > in the mask"
    # 4. one channel pair swapped
    sw = y.copy()
    sw[..., [6, 7]] = sw[..., [7, 6]]
    assert R.mismatches(_f32(sw), y) > 0, "a channel pair swapped"
    # 5. the last voxel of a ragged row unwritten (the output starts as NaN)
    un = _f32(y)
    un[1, 4, 8, 40, :] = np.nan
    assert R.mismatches(un, y) == 32, "the last voxel of a ragged row"
    # 6. a statistic of the unrounded 16-bit value
    cr = K.FWD_BY_ID["c1r_rnd-f32.f16-rt-rnd"]
    r = K.fwd_reference(cr)
    st = R.stored(_f32(r["y"]), "f16")
    rows, scales = R.block_stats_f64(st, K.stat_tile(cr))
    e32 = R.block_stats_e32(st, K.stat_tile(cr), rows, scales)
    unr, _ = R.block_stats_f64(_f32(r["y"]), K.stat_tile(cr))
    for q in (0, 1):
        assert R.within(R.units(_f32(rows[..., q]), rows[..., q], scales[..., q]), e32[q]), "float32 sums of the stored values pass"
        assert not R.within(R.units(unr[..., q], rows[..., q], scales[..., q]), e32[q]), "sums of the unrounded values"
    # 7. dw in the wrong layout
    cw = K.WG_BY_ID["wc1_3_4_k3-f32.f32-sd0b"]
    rw = K.wg_reference(cw)
    assert R.mismatches(_f32(R.to_sd(rw["dw"], cw.k)).reshape(-1), rw["dw"].reshape(-1)) > 0, "dw in the state_dict order where tap-major is asked"
    # 8. an 8-ulp scale on one output channel: by equality on the lattice, by the units rule on random data
    s8 = _f32(y)
    s8[..., 3] = (s8[..., 3].astype(np.float32) * np.float32(1 + 8 * 2.0 ** -23)).astype(np.float64)
    assert R.mismatches(s8, y) > 0, "8 ulp on one channel (lattice)"
    cq = K.FWD_BY_ID["cout1_rnd-f32.f32-b-rnd"]
    rq = K.fwd_reference(cq)
    good = R.fwd_f32(**{k: v for k, v in K.fwd_inputs(cq).items()}, k=cq.k, act=cq.act)
    assert R.within(R.units(good, rq["y"], rq["mag"]), rq["e32"])
    ck = K.FWD_BY_ID["expand_rnd-f32.f32-bma-rnd"]
    dk = K.fwd_inputs(ck)
    rk = K.fwd_reference(ck, dk)
    gk = R.fwd_f32(dk["x"], dk["w"], ck.k, dk["bias"], None, None, ck.act, dk["ref"]).astype(np.float64)
    assert R.within(R.units(gk, rk["y"], rk["mag"]), rk["e32"])
    # On random data the units rule does NOT see 8 ulp of the value: the unit is 2^-23 x sum |terms|, which exceeds |y| wherever terms
    # cancel, and the band is MARGIN x max(e32, 1) of those.  Stated and asserted, so that the statement stays true: the equality
    # judge on the lattice (above) is what rejects this error; the units rule rejects it from 8 x MARGIN ulp of the value on.
    g8, g64 = gk.copy(), gk.copy()
    g8[..., 5] *= 1 + 8 * 2.0 ** -23
    g64[..., 5] *= 1 + 64 * 2.0 ** -23
    u8, u64 = R.units(g8, rk["y"], rk["mag"]), R.units(g64, rk["y"], rk["mag"])
    print(f"\nCONV_VALU_JUDGE a channel of {ck.id} scaled by 8 / 64 ulp: {u8:.2f} / {u64:.2f} units, e32 {rk['e32']:.2f}")
    assert R.within(u8, rk["e32"]) and u8 > R.units(gk, rk["y"], rk["mag"]), "8 ulp on random data: seen as an error, inside the band"
    assert not R.within(u64, rk["e32"]), "64 ulp on random data"
    # (a 16-bit element outside its interval)
    st16 = R.stored(rk["y"], "f16")
    assert R.outside16(st16, rk["y"], rk["mag"], rk["e32"], "f16") == 0
    st16[0, 0, 3, 3, 1] += 2 * abs(st16[0, 0, 3, 3, 1]) * 2.0 ** -10 + 2.0 ** -20
    assert R.outside16(st16, rk["y"], rk["mag"], rk["e32"], "f16") == 1
    # the amax word
    assert R.amax_ok(int(np.array([7.5], np.float32).view(np.uint32)[0]), np.array([-7.5, 2.0]), "f32")
    assert not R.amax_ok(int(np.array([7.5], np.float32).view(np.uint32)[0]), np.array([-7.0, 2.0]), "f32")
