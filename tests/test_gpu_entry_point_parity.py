"""GPU: the shorter C-ABI entry points against the `_ex` / `_st` entry points the Python binding calls.

torch_em_amd/ops.py reaches every convolution, norm, pool and upsample operation through its most general entry point
(tem_conv3d_fwd_ex, tem_conv3d_wgrad_ex, tem_*_st).  The shorter entry points of include/tem_hip.h stay for C callers; inside
the library both forms forward into the same implementation, and the kernels are deterministic
(tests/test_gpu_determinism.py).  So each test here calls one shorter entry point directly through ctypes and the ops
wrapper on the same inputs, and every output buffer -- y / gx, statistics partials, dw, db, sums, coef, the amax word --
must be bit-identical (torch.equal): no tolerance.

Shapes are the smallest that reach the code: 1x4x4x4 with 8 channels (16-byte accesses) and 3 channels (scalar accesses) for
pool / upsample, N = 2 with two groups for the norms, a 1 -> 8 first layer for the VALU convolutions, 32 -> 2 for the output
projection, and 2x32x64x64 with 32 -> 32 channels for the MFMA entries -- the smallest shape the suite pins to the z-reuse
kernel (family 3, tests/test_gpu_ops.py::test_conv_zreuse_wide_chunks_and_tile_order), which the prescaled and the
norm-epilogue data gradients require.  The precondition query of such an entry is asserted, never skipped on."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
K3 = (3, 3, 3)
F2 = (2, 2, 2)
SPLIT = 2   # Arith.BF16X3: the default split-precision mode of the MFMA kernels


def _mods():
    from torch_em_amd import _lib, ops
    return _lib, _lib.load(), ops


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def direct(name, *args):
    """call the C entry point `name` on torch's current stream"""
    _lib, lib, _ = _mods()
    _lib.check(getattr(lib, name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def rnd(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale + shift


def blank(*shape, dtype=torch.float32):
    """an output buffer with a recognisable fill: elements that neither route writes compare equal"""
    return torch.full(shape, 7, dtype=dtype, device=DEV)


def wsbuf(nbytes, always=True):
    """a workspace of its own for the direct call; always=False: no buffer for a zero size, as ops.conv_fwd passes it"""
    if not nbytes and not always:
        return None
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def same(a, b, what):
    assert bool((a != 7).any()), f"{what}: not written"   # (blank()'s fill: equal buffers that nobody wrote prove nothing)
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}: the two entry points differ"


# ---------------------------------------------------------------- pool / upsample ----
@pytest.fixture(scope="module", params=[8, 3], ids=["C8", "C3"])
def vol(request):
    """x [1, 4, 4, 4, C], a gradient of the same shape, one of the pooled shape and one of the upsampled shape, coefficients"""
    C = request.param
    return {"C": C, "x": rnd(1, 4, 4, 4, C, seed=1), "gfull": rnd(1, 4, 4, 4, C, seed=2), "gpool": rnd(1, 2, 2, 2, C, seed=3),
            "gup": rnd(1, 8, 8, 8, C, seed=4), "coef": rnd(1, C, 4, seed=5), "coef2": rnd(1, C, 4, seed=6)}


def test_maxpool_fwd(vol):
    _, _, ops = _mods()
    C, x = vol["C"], vol["x"]
    ya, yb = blank(1, 2, 2, 2, C), blank(1, 2, 2, 2, C)
    ops.maxpool_fwd(x, ya, F2)
    direct("tem_maxpool3d_fwd", P(x), C, P(yb), C, 1, 4, 4, 4, C, *F2)
    same(ya, yb, "y")


def test_maxpool_fwd_stats():
    _, lib, ops = _mods()
    C, x = 8, rnd(1, 4, 4, 4, 8, seed=1)
    nblk = lib.tem_maxpool3d_fwd_stat_blocks(4, 4, C, 2, 2)
    assert nblk == 4
    ya, yb, pb = blank(1, 2, 2, 2, C), blank(1, 2, 2, 2, C), blank(1, nblk, C, 2)
    pa, na = ops.maxpool_fwd(x, ya, F2, want_stats=True)
    direct("tem_maxpool3d_fwd_stats", P(x), C, P(yb), C, 1, 4, 4, 4, C, *F2, P(pb), nblk)
    assert na == nblk
    same(ya, yb, "y")
    same(pa, pb, "statistics partials")


@pytest.mark.parametrize("relu_mask", [False, True])
def test_maxpool_bwd(vol, relu_mask):
    _, _, ops = _mods()
    C, x, gy, gskip = vol["C"], vol["x"], vol["gpool"], vol["gfull"]
    ga, gb = blank(1, 4, 4, 4, C), blank(1, 4, 4, 4, C)
    ops.maxpool_bwd(gy, x, ga, F2, gskip=gskip, relu_mask=relu_mask)
    direct("tem_maxpool3d_bwd", P(gy), C, P(x), C, P(gskip), C, int(relu_mask), P(gb), C, 1, 4, 4, 4, C, *F2)
    same(ga, gb, "gx")


@pytest.mark.parametrize("which", ["gskip_coef", "gy_coef", "both"])
def test_maxpool_bwd_norm(vol, which):
    _, _, ops = _mods()
    C, x, gy, gskip = vol["C"], vol["x"], vol["gpool"], vol["gfull"]
    gcoef = vol["coef"] if which != "gy_coef" else None
    ycoef = vol["coef2"] if which != "gskip_coef" else None
    ga, gb = blank(1, 4, 4, 4, C), blank(1, 4, 4, 4, C)
    ops.maxpool_bwd(gy, x, ga, F2, gskip=gskip, relu_mask=True, gskip_coef=gcoef, gy_coef=ycoef)
    direct("tem_maxpool3d_bwd_norm", P(gy), C, P(x), C, P(gskip), C, 1, P(gb), C, 1, 4, 4, 4, C, *F2, P(gcoef),
           gcoef.stride(0) if gcoef is not None else 0, P(ycoef))
    same(ga, gb, "gx")


def test_upsample_fwd(vol):
    _, _, ops = _mods()
    C, x = vol["C"], vol["x"]
    ya, yb = blank(1, 8, 8, 8, C), blank(1, 8, 8, 8, C)
    ops.upsample_fwd(x, ya, F2)
    direct("tem_upsample_fwd", P(x), C, P(yb), C, 1, 4, 4, 4, C, *F2)
    same(ya, yb, "y")


def test_upsample_fwd_stats_and_upsample_stats():
    _, lib, ops = _mods()
    C, x = 8, rnd(1, 4, 4, 4, 8, seed=1)
    assert lib.tem_upsample_fwd_stats_ok(C, *F2) and ops.upsample_stats_ok(x)
    ya, yb, pb = blank(1, 8, 8, 8, C), blank(1, 8, 8, 8, C), blank(1, 16, C, 2)
    pa = ops.upsample_fwd(x, ya, F2, stats=True)
    direct("tem_upsample_fwd_stats", P(x), C, P(yb), C, 1, 4, 4, 4, C, *F2, P(pb))
    same(ya, yb, "y")
    same(pa, pb, "statistics partials")
    qb = blank(1, 16, C, 2)
    qa = ops.upsample_stats(x, F2)
    direct("tem_upsample_stats", P(x), C, 1, 4, 4, 4, C, *F2, P(qb))
    same(qa, qb, "statistics partials from the low-resolution tensor")


def test_upsample_bwd(vol):
    _, _, ops = _mods()
    C, gy = vol["C"], vol["gup"]
    ga, gb = blank(1, 4, 4, 4, C), blank(1, 4, 4, 4, C)
    ops.upsample_bwd(gy, ga, F2)
    direct("tem_upsample_bwd", P(gy), C, P(gb), C, 1, 4, 4, 4, C, *F2)
    same(ga, gb, "gx")


def test_upsample_bwd_norm(vol):
    _, _, ops = _mods()
    C, gy, u, coef = vol["C"], vol["gup"], vol["x"], vol["coef"]
    ga, gb = blank(1, 4, 4, 4, C), blank(1, 4, 4, 4, C)
    ops.upsample_bwd(gy, ga, F2, norm=(u, coef))
    direct("tem_upsample_bwd_norm", P(gy), C, P(gb), C, 1, 4, 4, 4, C, *F2, P(u), C, P(coef), coef.stride(0))
    same(ga, gb, "gx")


# ------------------------------------------------------------------------- norm ----
NN, NV, NC, NG = 2, 64, 8, 2   # N = 2, 4 x 4 x 4 voxels, C = 8, G = 2


@pytest.fixture(scope="module")
def nrm():
    _, lib, ops = _mods()
    x, gy = rnd(NN, 4, 4, 4, NC, seed=11, scale=1.5, shift=0.3), rnd(NN, 4, 4, 4, NC, seed=12)
    gamma, beta = rnd(NC, seed=13, scale=0.2, shift=1.0), rnd(NC, seed=14)
    mean, rstd, _, _ = ops.norm_stats(x, NG, gamma, beta)
    return {"x": x, "gy": gy, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "nws": lib.tem_norm_ws(NN, NV, NC),
            "sums": rnd(NN, NC, 2, seed=15), "part": rnd(NN, 3, NC, 2, seed=16)}   # hand-made first stages


def test_norm_stats(nrm):
    _, _, ops = _mods()
    x, gamma, beta = nrm["x"], nrm["gamma"], nrm["beta"]
    a = ops.norm_stats(x, NG, gamma, beta, 1e-5)
    b = (blank(NN, NG), blank(NN, NG), blank(NN, NC), blank(NN, NC))
    ws = wsbuf(nrm["nws"])
    direct("tem_norm_stats", P(x), NC, NN, NV, NC, NG, P(gamma), P(beta), 1e-5, *(P(t) for t in b), P(ws), nrm["nws"])
    for ta, tb, what in zip(a, b, ("mean", "rstd", "scale", "shift")):
        same(ta, tb, what)


@pytest.mark.parametrize("first_stage", [None, "sums", "part"])
def test_norm_bwd(nrm, first_stage):
    """tem_norm_bwd, tem_norm_bwd_from_sums and the gx form of tem_norm_bwd_from_partials"""
    _, _, ops = _mods()
    x, gy, gamma, mean, rstd = nrm["x"], nrm["gy"], nrm["gamma"], nrm["mean"], nrm["rstd"]
    sums = None if first_stage is None else nrm[first_stage]
    ga, dga, dba = blank(NN, 4, 4, 4, NC), blank(NC), blank(NC)
    gb, dgb, dbb = blank(NN, 4, 4, 4, NC), blank(NC), blank(NC)
    ops.norm_bwd(gy, x, NG, gamma, mean, rstd, True, ga, dga, dba, sums=sums)
    ws = wsbuf(nrm["nws"])
    head = (P(gy), NC, P(x), NC, NN, NV, NC, NG, P(gamma), P(mean), P(rstd), 1, P(gb), NC, P(dgb), P(dbb))
    if first_stage is None:
        direct("tem_norm_bwd", *head, P(ws), nrm["nws"])
    elif first_stage == "sums":
        direct("tem_norm_bwd_from_sums", *head, P(sums), P(ws), nrm["nws"])
    else:
        direct("tem_norm_bwd_from_partials", *head, P(sums), sums.shape[1], None, P(ws), nrm["nws"])
    same(ga, gb, "gx")
    same(dga, dgb, "dgamma")
    same(dba, dbb, "dbeta")


@pytest.mark.parametrize("first_stage", [None, "sums", "part"])
def test_norm_bwd_coef(nrm, first_stage):
    """tem_norm_bwd_coef (with and without sums) and the coef form of tem_norm_bwd_from_partials"""
    _, _, ops = _mods()
    x, gy, gamma, mean, rstd = nrm["x"], nrm["gy"], nrm["gamma"], nrm["mean"], nrm["rstd"]
    sums = None if first_stage is None else nrm[first_stage]
    dga, dba = blank(NC), blank(NC)
    cb, dgb, dbb = blank(NN, NC, 4), blank(NC), blank(NC)
    ca = ops.norm_bwd_coef(gy, x, NG, gamma, mean, rstd, dga, dba, sums=sums)
    ws = wsbuf(nrm["nws"])
    if first_stage == "part":
        direct("tem_norm_bwd_from_partials", P(gy), NC, P(x), NC, NN, NV, NC, NG, P(gamma), P(mean), P(rstd), 0, None, NC,
               P(dgb), P(dbb), P(sums), sums.shape[1], P(cb), P(ws), nrm["nws"])
    else:
        direct("tem_norm_bwd_coef", P(gy), NC, P(x), NC, NN, NV, NC, NG, P(gamma), P(mean), P(rstd), P(dgb), P(dbb), P(sums),
               P(cb), P(ws), nrm["nws"])
    same(ca, cb, "coef")
    same(dga, dgb, "dgamma")
    same(dba, dbb, "dbeta")


# ------------------------------------------------------- VALU convolutions: 1x8x8x8, 1 -> 8 ----
@pytest.fixture(scope="module")
def first():
    _, _, ops = _mods()
    w = rnd(8, 1, *K3, seed=21, scale=0.2)
    return {"x": rnd(1, 8, 8, 8, 1, seed=22), "g": rnd(1, 8, 8, 8, 8, seed=23), "y": rnd(1, 8, 8, 8, 8, seed=24), "w": w,
            "wp": ops.pack_weights(w, transpose=False, mfma=0), "bias": rnd(8, seed=25), "coef": rnd(1, 8, 4, seed=26),
            "scale": rnd(1, 1, seed=27, scale=0.1, shift=1.0), "shift": rnd(1, 1, seed=28)}


def test_conv_fwd_valu(first):
    _, _, ops = _mods()
    x, wp, bias, scale, shift = (first[n] for n in ("x", "wp", "bias", "scale", "shift"))
    ya, yb = blank(1, 8, 8, 8, 8), blank(1, 8, 8, 8, 8)
    ops.conv_fwd(x, wp, bias, ya, K3, 1, 8, scale=scale, shift=shift, act="relu", mfma=0)
    direct("tem_conv3d_fwd", P(x), 1, P(scale), P(shift), P(wp), P(bias), P(yb), 8, None, 0, None, 0, 1, 8, 8, 8, 1, 8, *K3,
           ops.ACT["relu"], 0)
    same(ya, yb, "y")


def test_conv_wgrad_valu(first):
    _, lib, ops = _mods()
    x, g, scale, shift = (first[n] for n in ("x", "g", "scale", "shift"))
    dwa, dba, dwb, dbb = blank(8 * 27), blank(8), blank(8 * 27), blank(8)
    ops.conv_wgrad(x, g, K3, 1, 8, dwa, dba, scale=scale, shift=shift, mfma=0)
    nws = lib.tem_conv3d_wgrad_ws(1, 8, 8, 8, 1, 8, *K3, 0)
    ws = wsbuf(nws)
    direct("tem_conv3d_wgrad", P(x), 1, P(scale), P(shift), P(g), 8, P(dwb), P(dbb), P(ws), nws, 1, 8, 8, 8, 1, 8, *K3, 0, 1)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")


def test_conv_wgrad_gnorm(first):
    _, lib, ops = _mods()
    x, g, y, coef, scale, shift = (first[n] for n in ("x", "g", "y", "coef", "scale", "shift"))
    assert ops.conv_wgrad_gnorm_ok(K3, 1, 8, 0)
    dwa, dba, dwb, dbb = blank(8 * 27), blank(8), blank(8 * 27), blank(8)
    ops.conv_wgrad_gnorm(x, g, y, coef, K3, 1, 8, dwa, dba, scale=scale, shift=shift)
    nws = lib.tem_conv3d_wgrad_ws(1, 8, 8, 8, 1, 8, *K3, 0)
    ws = wsbuf(nws)
    direct("tem_conv3d_wgrad_gnorm", P(x), 1, P(scale), P(shift), P(g), 8, P(y), 8, P(coef), P(dwb), P(dbb), P(ws), nws,
           1, 8, 8, 8, 1, 8, *K3, 1)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")


def test_conv1x1_out_bwd():
    _, lib, ops = _mods()
    cin, cout, nv = 32, 2, 64
    assert ops.conv1x1_out_bwd_ok(cin, cout)
    x, g, w = rnd(1, 4, 4, 4, cin, seed=31), rnd(1, 4, 4, 4, cout, seed=32), rnd(cout, cin, 1, 1, 1, seed=33, scale=0.2)
    gxa, dwa, dba = blank(1, 4, 4, 4, cin), blank(cout * cin), blank(cout)
    gxb, dwb, dbb = blank(1, 4, 4, 4, cin), blank(cout * cin), blank(cout)
    ops.conv1x1_out_bwd(x, g, w, gxa, dwa, dba)
    nws = lib.tem_conv1x1_out_bwd_ws(cin, cout)
    ws = wsbuf(nws)
    direct("tem_conv1x1_out_bwd", P(x), cin, P(g), cout, P(w), P(gxb), cin, P(dwb), P(dbb), P(ws), nws, nv, cin, cout)
    same(gxa, gxb, "gx")
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")


# ------------------------------------------------- MFMA entries: 2x32x64x64, 32 -> 32, 3x3x3 ----
MN, MD, MH, MW, MC = 2, 32, 64, 64, 32
MDIMS = (MN, MD, MH, MW, MC, MC, *K3)


@pytest.fixture(scope="module")
def big():
    _, lib, ops = _mods()
    w = rnd(MC, MC, *K3, seed=41, scale=0.1)
    x = rnd(MN, MD, MH, MW, MC, seed=42)
    g = rnd(MN, MD, MH, MW, MC, seed=43)
    mean, rstd, scale, shift = ops.norm_stats(x, MC)
    return {"x": x, "g": g, "w": w, "bias": rnd(MC, seed=44), "scale": scale, "shift": shift,
            "ref": torch.relu(rnd(MN, MD, MH, MW, MC, seed=45, shift=0.2)), "coef": rnd(MN, MC, 4, seed=46),
            "wp": ops.pack_weights(w, transpose=False, mfma=SPLIT), "wpt": ops.pack_weights(w, transpose=True, mfma=SPLIT),
            "wpt4": ops.pack_weights(w, transpose=True, mfma=4), "amax": ops.absmax(g),
            "fwd_nws": lib.tem_conv3d_fwd_ws(*MDIMS, SPLIT), "fwd_nws1": lib.tem_conv3d_fwd_ws(*MDIMS, 1),
            "wg_nws": lib.tem_conv3d_wgrad_ws(*MDIMS, SPLIT), "wg_nws8": lib.tem_conv3d_wgrad_ws(*MDIMS, 8)}


def act():
    return blank(MN, MD, MH, MW, MC)


def test_conv_fwd_mfma(big):
    _, _, ops = _mods()
    x, wp, bias, scale, shift = (big[n] for n in ("x", "wp", "bias", "scale", "shift"))
    ya, yb = act(), act()
    ops.conv_fwd(x, wp, bias, ya, K3, MC, MC, scale=scale, shift=shift, act="relu", mfma=SPLIT)
    ws = wsbuf(big["fwd_nws"], always=False)
    direct("tem_conv3d_fwd", P(x), MC, P(scale), P(shift), P(wp), P(bias), P(yb), MC, None, 0, P(ws), big["fwd_nws"], *MDIMS,
           ops.ACT["relu"], SPLIT)
    same(ya, yb, "y")


def test_conv_fwd_stats(big):
    _, _, ops = _mods()
    x, wp, bias, scale, shift = (big[n] for n in ("x", "wp", "bias", "scale", "shift"))
    nblk = ops.conv_fwd_stat_blocks(x, K3, MC, MC, SPLIT)
    assert nblk > 0
    ya, yb, pb = act(), act(), blank(MN, nblk, MC, 2)
    pa, na = ops.conv_fwd(x, wp, bias, ya, K3, MC, MC, scale=scale, shift=shift, act="relu", mfma=SPLIT, want_stats=True)
    ws = wsbuf(big["fwd_nws"], always=False)
    direct("tem_conv3d_fwd_stats", P(x), MC, P(scale), P(shift), P(wp), P(bias), P(yb), MC, None, 0, P(ws), big["fwd_nws"],
           *MDIMS, ops.ACT["relu"], SPLIT, P(pb), nblk)
    assert na == nblk
    same(ya, yb, "y")
    same(pa, pb, "statistics partials")


def test_conv_fwd_gscaled(big):
    _, _, ops = _mods()
    g, wpt4, ref, amax = (big[n] for n in ("g", "wpt4", "ref", "amax"))
    assert ops.conv_fwd_family(g, K3, MC, MC, 4, ref=ref) == 3
    ya, yb = act(), act()
    ops.conv_fwd_gscaled(g, wpt4, ya, K3, MC, MC, amax, ref=ref)
    ws = wsbuf(big["fwd_nws1"], always=False)
    direct("tem_conv3d_fwd_gscaled", P(g), MC, P(wpt4), P(yb), MC, P(ref), MC, P(amax), P(ws), big["fwd_nws1"], *MDIMS)
    same(ya, yb, "gx")


def test_conv_fwd_refnorm(big):
    _, _, ops = _mods()
    g, wpt, ref, coef = (big[n] for n in ("g", "wpt", "ref", "coef"))
    assert ops.conv_fwd_family(g, K3, MC, MC, SPLIT, ref=ref) == 3
    ya, yb = act(), act()
    ops.conv_fwd_refnorm(g, wpt, ya, K3, MC, MC, ref, coef, SPLIT)
    ws = wsbuf(big["fwd_nws1"], always=False)
    direct("tem_conv3d_fwd_refnorm", P(g), MC, P(wpt), P(yb), MC, P(ref), MC, P(coef), P(ws), big["fwd_nws1"], *MDIMS, SPLIT)
    same(ya, yb, "gx")


def test_conv_wgrad_mfma(big):
    _, _, ops = _mods()
    x, g, scale, shift = (big[n] for n in ("x", "g", "scale", "shift"))
    dwa, dba, dwb, dbb = blank(MC * MC * 27), blank(MC), blank(MC * MC * 27), blank(MC)
    ops.conv_wgrad(x, g, K3, MC, MC, dwa, dba, scale=scale, shift=shift, mfma=SPLIT)
    ws = wsbuf(big["wg_nws"])
    direct("tem_conv3d_wgrad", P(x), MC, P(scale), P(shift), P(g), MC, P(dwb), P(dbb), P(ws), big["wg_nws"], *MDIMS, SPLIT, 1)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")


def _wgrad_bufs(with_sums):
    return blank(MC * MC * 27), blank(MC), blank(MN, MC, 2) if with_sums else None


def test_conv_wgrad_sums(big):
    _, _, ops = _mods()
    x, g, w, scale, shift = (big[n] for n in ("x", "g", "w", "scale", "shift"))
    assert ops.conv_wgrad_sums_ok(x, K3, MC, MC, SPLIT)
    dwa, dba, _ = _wgrad_bufs(False)
    dwb, dbb, sb = _wgrad_bufs(True)
    sa = ops.conv_wgrad(x, g, K3, MC, MC, dwa, dba, scale=scale, shift=shift, mfma=SPLIT, sums_from=(w, None, None))
    ws = wsbuf(big["wg_nws"])
    direct("tem_conv3d_wgrad_sums", P(x), MC, P(scale), P(shift), P(g), MC, P(w), None, None, P(dwb), P(dbb), P(sb), P(ws),
           big["wg_nws"], *MDIMS, SPLIT)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")
    same(sa, sb, "sums")


@pytest.mark.parametrize("with_sums", [False, True])
def test_conv_wgrad_gmax(big, with_sums):
    _, _, ops = _mods()
    x, g, w, scale, shift = (big[n] for n in ("x", "g", "w", "scale", "shift"))
    assert ops.conv_wgrad_gmax_ok(x, K3, MC, MC, SPLIT)
    assert not with_sums or ops.conv_wgrad_sums_ok(x, K3, MC, MC, SPLIT)
    dwa, dba, _ = _wgrad_bufs(False)
    dwb, dbb, sb = _wgrad_bufs(with_sums)
    ma, mb = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    sa = ops.conv_wgrad_gmax(x, g, K3, MC, MC, dwa, dba, ma, scale=scale, shift=shift, mfma=SPLIT,
                             sums_from=(w, None, None) if with_sums else None)
    ws = wsbuf(big["wg_nws"])
    direct("tem_conv3d_wgrad_gmax", P(x), MC, P(scale), P(shift), P(g), MC, P(w) if with_sums else None, None, None, P(dwb),
           P(dbb), P(sb), P(mb), P(ws), big["wg_nws"], *MDIMS, SPLIT)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")
    same(ma, mb, "amax word")
    assert int(ma) == int(big["amax"])
    assert (sa is None) == (sb is None)
    if with_sums:
        same(sa, sb, "sums")


@pytest.mark.parametrize("with_sums", [False, True])
def test_conv_wgrad_gscaled(big, with_sums):
    _, _, ops = _mods()
    x, g, w, scale, shift, amax = (big[n] for n in ("x", "g", "w", "scale", "shift", "amax"))
    assert ops.conv_wgrad_gscaled_ok(x, K3, MC, MC)
    assert not with_sums or ops.conv_wgrad_sums_ok(x, K3, MC, MC, SPLIT)
    dwa, dba, _ = _wgrad_bufs(False)
    dwb, dbb, sb = _wgrad_bufs(with_sums)
    sa = ops.conv_wgrad_gscaled(x, g, K3, MC, MC, dwa, dba, amax, scale=scale, shift=shift,
                                sums_from=(w, None, None) if with_sums else None)
    ws = wsbuf(big["wg_nws8"])
    direct("tem_conv3d_wgrad_gscaled", P(x), MC, P(scale), P(shift), P(g), MC, P(w) if with_sums else None, None, None, P(dwb),
           P(dbb), P(sb), P(amax), P(ws), big["wg_nws8"], *MDIMS)
    same(dwa, dwb, "dw")
    same(dba, dbb, "db")
    assert (sa is None) == (sb is None)
    if with_sums:
        same(sa, sb, "sums")
