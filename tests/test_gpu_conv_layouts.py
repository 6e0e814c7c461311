"""GPU: convolution launches at the layouts the engine hands them -- dense, channel slices of wider buffers (aligned or not),
and leading dimensions on both sides of the team kernels' 32-bit plane limit (H * W * 32 * ld < 2^31) -- against a float64
CPU convolution of the same operands, and against the dispatch queries the engine plans with (conv_fwd_family,
conv_fwd_stat_blocks, the wgrad *_ok functions): a query must never promise what the launch does not deliver.

Each case either matches the reference (per-mode tolerances of test_gpu_ops.py) with every element outside the slice left
at its sentinel, or raises for a documented precondition before it writes anything."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import check_grads, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0
# per-mode tolerances of tests/test_gpu_ops.py (test_conv_fwd_dgrad_wgrad / test_conv_mixed_precision_mode)
TOL = {0: 2e-5, 1: 2e-5, 2: 1e-4, 4: 2e-5, 5: 2e-5, 7: 2e-5}
# one rounding of the STORED output relative to max |y| (16-bit storage): the unit roundoff of the format
OUT_ROUND = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
R16 = {5: torch.float16, 7: torch.bfloat16}

# (name, N, D, H, W, Cin, Cout, k, conv_fwd_variant option or None, family of a dense split-precision launch)
SHAPES = [
    ("zreuse", 2, 8, 16, 16, 32, 32, (3, 3, 3), 2, 3),
    ("splitk", 1, 16, 16, 16, 256, 256, (3, 3, 3), None, 4),
    ("pingpong", 2, 8, 16, 16, 32, 64, (3, 3, 3), 1, 2),
    ("patch", 2, 12, 24, 24, 128, 64, (3, 3, 3), None, 0),
    ("stream1x1", 1, 16, 32, 32, 64, 32, (1, 1, 1), None, 0),
]
# (name, layout of x, of y, of ref): L0 dense, L1 16-byte aligned slice with ld % 4 == 0, L2 4-byte offset with odd ld
LAYOUTS = [("L0", "L0", "L0", "L0"), ("L1x", "L1", "L0", "L0"), ("L1y", "L0", "L1", "L0"), ("L1ref", "L0", "L0", "L1"),
           ("L2x", "L2", "L0", "L0"), ("L2y", "L0", "L2", "L0"), ("L2ref", "L0", "L0", "L2")]
# (mode, storage dtype of x / y / ref)
MODES = [(0, torch.float32), (1, torch.float32), (2, torch.float32), (4, torch.float32), (5, torch.float32),
         (7, torch.float32), (5, torch.float16), (7, torch.bfloat16)]


@pytest.fixture
def variant():
    from torch_em_amd import _lib
    old = _lib.get_option("conv_fwd_variant")
    yield lambda v: _lib.set_option("conv_fwd_variant", -1 if v is None else v)
    _lib.set_option("conv_fwd_variant", old)


def place(t5, layout, ld=None):
    """t5 (dense NDHWC, cuda) copied into a sentinel-filled wider buffer -> (view, buffer, channel offset)"""
    N, D, H, W, C = t5.shape
    es = t5.element_size()
    if layout == "L0":
        return t5.clone(), None, 0
    off, ld = {"L1": (16 // es, C + 32 // es), "L2": (1, C + 3), "L3": (0, ld)}[layout]
    buf = torch.full((N, D, H, W, ld), SENT, dtype=t5.dtype, device=t5.device)
    v = buf[..., off:off + C]
    v.copy_(t5)
    return v, buf, off


def untouched(buf, off, C):
    """every element of buf outside channels [off, off + C) still holds the sentinel"""
    if buf is None:
        return True
    return all(bool((p == SENT).all()) for p in (buf[..., :off], buf[..., off + C:]) if p.numel())


_REF = {}


def ref_conv_cached(key, *args, **kw):
    """ref_conv of operands that `key` identifies (the layouts of one case share them)"""
    if key not in _REF:
        _REF.clear() if len(_REF) > 64 else None
        _REF[key] = ref_conv(*args, **kw)
    return _REF[key]


def ref_conv(x, w, b, mode, scale=None, shift=None, act=None, ref=None, rows=None):
    """float64 convolution of NCDHW cpu tensors with the operand rounding of `mode`; rows = (y0, y1): output rows only"""
    xn = x.double()
    if scale is not None:   # the kernels apply the pre-norm as one fp32 multiply-add, then round to the operand type
        xn = (xn * scale.double()[:, :, None, None, None] + shift.double()[:, :, None, None, None]).float().double()
    wn = w.double()
    if mode in R16:
        xn, wn = xn.to(R16[mode]).double(), wn.to(R16[mode]).double()
    p = tuple(v // 2 for v in w.shape[2:])
    xp = F.pad(xn, (p[2], p[2], p[1], p[1], p[0], p[0]))
    if rows is not None:
        xp = xp[:, :, :, rows[0]:rows[1] + 2 * p[1]]
    y = F.conv3d(xp, wn, None if b is None else b.double())
    if act == "relu":
        y = y.clamp_min(0)
    if ref is not None:
        r = ref if rows is None else ref[:, :, :, rows[0]:rows[1]]
        y = y * (r.double() > 0)
    return y


def nc(t5):
    return t5.permute(0, 4, 1, 2, 3).double().cpu()


def to5(x, dt=torch.float32):
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV).to(dt)


def operands(N, D, H, W, Cin, Cout, k, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(dt).float()
    w = torch.randn(Cout, Cin, *k, generator=g) * (0.5 / (Cin * k[0] * k[1] * k[2]) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    scale = torch.rand(N, Cin, generator=g) + 0.5
    shift = torch.randn(N, Cin, generator=g) * 0.5
    ref = torch.randn(N, Cout, D, H, W, generator=g).to(dt).float()
    return x, w, b, scale, shift, ref


def stats_through_cabi(x5, wp, b, y5, ref5, N, D, H, W, Cin, Cout, k, mode, nblk, scale=None, shift=None, act=None):
    """tem_conv3d_fwd_stats with a NaN-filled [N, nblk, Cout, 2] buffer -> (rc, part)"""
    from torch_em_amd import _lib, ops
    lib = _lib.load()
    part = torch.full((N, nblk, Cout, 2), float("nan"), device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    mfma = ops._mode(mode, x5, y5)
    nws = lib.tem_conv3d_fwd_ws(N, D, H, W, Cin, Cout, k[0], k[1], k[2], mfma)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
    rc = lib.tem_conv3d_fwd_stats(p(x5), ops._act5(x5)[5], p(scale), p(shift), p(wp), p(b), p(y5), ops._act5(y5)[5], p(ref5),
                                  ops._act5(ref5)[5] if ref5 is not None else 0, p(ws), nws, N, D, H, W, Cin, Cout, *k,
                                  ops.ACT[act], mfma, p(part), nblk, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, part


def check_stats(part, y5, N, C):
    """the rows finalised by norm_stats_from_partials against the float64 mean / variance of the kernel's own y"""
    from torch_em_amd import ops
    assert not torch.isnan(part).any(), f"{int(torch.isnan(part).any(-1).any(-1).sum())} statistics rows never written"
    V = y5.shape[1] * y5.shape[2] * y5.shape[3]
    mean, rstd, _, _ = ops.norm_stats_from_partials(part, N, V, C, C, eps=1e-5)
    yd = y5.double().reshape(N, V, C)
    m64, v64 = yd.mean(1), yd.var(1, unbiased=False)
    var = rstd.double() ** -2 - 1e-5
    assert float((mean.double() - m64).abs().max() / v64.sqrt().max()) < 1e-5, "mean"
    assert float(((var - v64).abs() / v64).max()) < 1e-5, "variance"


def expect_or_precondition(fn, bufs):
    """run fn(); a ValueError (TEM_EINVAL) must leave every listed output buffer as it was.  -> True when fn ran"""
    before = [b.clone() for b in bufs]
    try:
        fn()
    except ValueError:
        torch.cuda.synchronize()
        for b0, b in zip(before, bufs):
            assert bool(((b0 == b) | (b0.isnan() & b.isnan())).all()), "a launch that raised wrote to its output"
        return False
    return True


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode,dt", MODES, ids=[f"m{m}-{str(d)[6:]}" for m, d in MODES])
@pytest.mark.parametrize("lay", LAYOUTS, ids=[lay[0] for lay in LAYOUTS])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_conv_fwd_layouts(shape, lay, mode, dt, variant):
    """forward with / without pre-norm + bias + ReLU, with ref, and with statistics, at one layout per operand"""
    from torch_em_amd import ops
    name, N, D, H, W, Cin, Cout, k, var, fam = shape
    variant(var)
    mfma = mode if (mode == 0 or ops.mfma_ok(Cin, Cout, k)) else 0
    x, w, b, scale, shift, ref = operands(N, D, H, W, Cin, Cout, k, dt)
    x5, _, _ = place(to5(x, dt), lay[1])
    ref5, _, _ = place(to5(ref, dt), lay[3])
    wp = ops.pack_weights(w.to(DEV), transpose=False, mfma=mfma)
    bd, sd, hd = b.to(DEV), scale.to(DEV), shift.to(DEV)
    tol = TOL[mfma] + OUT_ROUND[dt]
    if lay[0] == "L0" and mfma >= 2 and dt == torch.float32:
        assert ops.conv_fwd_family(x5, k, Cin, Cout, mfma) == fam
    variants = [dict(), dict(ref=True)] + ([dict(norm=True, act="relu")] if (k != (1, 1, 1) or mfma in (0, 1, 2)) else [])
    for v in variants:
        if mfma == 4 and not v.get("norm"):
            continue   # mode 4 (fp16x3, scaled lo plane) is for pre-normalised operands only
        kw = dict(scale=sd, shift=hd) if v.get("norm") else {}
        r5 = ref5 if v.get("ref") else None
        y5, ybuf, yoff = place(torch.full((N, D, H, W, Cout), SENT, device=DEV, dtype=dt), lay[2])
        bufs = [ybuf if ybuf is not None else y5]
        ran = expect_or_precondition(lambda: ops.conv_fwd(x5, wp, bd, y5, k, Cin, Cout, act=v.get("act"), ref=r5,
                                                          mfma=mfma, **kw), bufs)
        if not ran:
            assert lay[1] == "L2" and mfma >= 1, f"{v}: raised without a documented precondition"   # x alignment
            continue
        exp = ref_conv_cached(("fwd", name, str(dt), mfma if mfma in R16 else 0, tuple(sorted(v))), x, w, b, mfma,
                              act=v.get("act"), ref=ref if r5 is not None else None, scale=scale if kw else None,
                              shift=shift if kw else None)
        assert rel_err(nc(y5), exp) < tol, (v, rel_err(nc(y5), exp))
        assert untouched(ybuf, yoff, Cout), v
        if r5 is not None:
            continue
        # statistics: the query the engine plans with, then the launch through the C-ABI into a NaN-filled buffer
        nblk = ops.conv_fwd_stat_blocks(x5, k, Cin, Cout, mfma, y=y5)
        y5.fill_(float("nan"))
        if nblk > 0:
            rc, part = stats_through_cabi(x5, wp, bd, y5, None, N, D, H, W, Cin, Cout, k, mfma, nblk, act=v.get("act"), **kw)
            assert rc == 0, ops._lib.load().tem_last_error()
            assert rel_err(nc(y5), exp) < tol, v
            check_stats(part, y5, N, Cout)
        got = ops.conv_fwd(x5, wp, bd, y5, k, Cin, Cout, act=v.get("act"), mfma=mfma, want_stats=True, **kw)
        assert (got is None) == (nblk <= 0), (nblk, got)
        assert rel_err(nc(y5), exp) < tol, v
        if got is not None:
            check_stats(got[0], y5, N, Cout)
        assert untouched(ybuf, yoff, Cout), v


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode,dt", [m for m in MODES if m[0] != 4], ids=[f"m{m}-{str(d)[6:]}" for m, d in MODES if m != 4])
@pytest.mark.parametrize("lay", LAYOUTS, ids=[lay[0] for lay in LAYOUTS])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_conv_dgrad_refnorm_wgrad_layouts(shape, lay, mode, dt, variant):
    """data gradient (transposed pack, with the ReLU mask of ref), its norm-backward epilogue (refnorm) where the layout
    query reports the z-reuse kernel, and the weight gradient with its gmax by-product where conv_wgrad_gmax_ok says so"""
    from torch_em_amd import _lib, ops
    name, N, D, H, W, Cin, Cout, k, var, fam = shape
    variant(var)
    # data gradient: Cout -> Cin channels
    mfma = mode if (mode == 0 or ops.mfma_ok(Cout, Cin, k)) else 0
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(N, Cout, D, H, W, generator=gen).to(dt).float()
    w = torch.randn(Cout, Cin, *k, generator=gen) * (0.5 / (Cout * k[0] * k[1] * k[2]) ** 0.5)
    a = torch.randn(N, Cin, D, H, W, generator=gen).to(dt).float()     # the ReLU output the gradient lands on
    g5, _, _ = place(to5(g, dt), lay[1])
    a5, _, _ = place(to5(a, dt), lay[3])
    wpt = ops.pack_weights(w.to(DEV), transpose=True, mfma=mfma)
    tol = TOL[mfma] + OUT_ROUND[dt]
    wt = w.transpose(0, 1).flip(2, 3, 4)   # the data gradient is the convolution with the transposed, flipped kernel
    rkey = ("dgrad", name, str(dt), mfma if mfma in R16 else 0)
    gx = ref_conv_cached(rkey + ("ref",), g, wt, None, mfma, ref=a)
    y5, ybuf, yoff = place(torch.zeros(N, D, H, W, Cin, device=DEV, dtype=dt), lay[2])
    bufs = [ybuf if ybuf is not None else y5]
    if expect_or_precondition(lambda: ops.conv_fwd(g5, wpt, None, y5, k, Cout, Cin, ref=a5, mfma=mfma), bufs):
        assert rel_err(nc(y5), gx) < tol, rel_err(nc(y5), gx)
        assert untouched(ybuf, yoff, Cin)
    else:
        assert lay[1] == "L2" and mfma >= 1
    # refnorm: y = a > 0 ? c0 * conv - c1 - (a - c3) * c2 : 0, promised by the layout query
    coef = torch.rand(N, Cin, 4, generator=gen)
    coef[..., 0] += 0.5
    y5.fill_(SENT)
    fam_ld = ops.conv_fwd_family(g5, k, Cout, Cin, mfma, y=y5, ref=a5) if mfma >= 1 else 0
    _lib.load().tem_last_error()
    try:
        ops.conv_fwd_refnorm(g5, wpt, y5, k, Cout, Cin, a5, coef.to(DEV), mfma)
        took = True
    except ValueError:
        took = False
    torch.cuda.synchronize()
    assert took == (fam_ld == 3), f"conv_fwd_family says {fam_ld}, refnorm {'ran' if took else 'raised'}"
    if took:
        c = coef.double()[:, :, :, None, None, None]
        conv = ref_conv_cached(rkey, g, wt, None, mfma)
        exp = torch.where(a > 0, c[:, :, 0] * conv - c[:, :, 1] - (a.double() - c[:, :, 3]) * c[:, :, 2], torch.zeros(()).double())
        assert rel_err(nc(y5), exp) < tol + 2e-5, rel_err(nc(y5), exp)
    else:
        assert bool((y5 == SENT).all()), "a refnorm launch that raised wrote to its output"
    assert untouched(ybuf, yoff, Cin)
    # weight gradient of the forward conv (x: Cin, gradient: Cout); x is `a` at layout lay[1], the gradient g at lay[3]
    mw = mode if mode in (0, 1, 2, 5, 7) and (mode == 0 or ops.mfma_ok(Cin, Cout, k, wgrad=True)) else 0
    if dt != torch.float32:
        return   # (16-bit weight gradients: tests/test_gpu_storage16.py)
    xw5, _, _ = place(to5(a, dt), lay[1])
    gw5, _, _ = place(to5(g, dt), lay[3] if not (dt != torch.float32 and lay[3] == "L2") else "L0")
    dw = torch.full((w.numel(),), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    if not expect_or_precondition(lambda: ops.conv_wgrad(xw5, gw5, k, Cin, Cout, dw, db, mfma=mw), [dw, db]):
        assert mw >= 1 and "L2" in (lay[1], lay[3])
        return
    r16 = mw if mw in R16 and k == (3, 3, 3) and D >= 8 else 0   # the z-sliding kernel rounds both operands
    if ("wgrad", name, r16) not in _REF:
        rnd = (lambda t: t.to(R16[r16]).double()) if r16 else (lambda t: t.double())
        _REF[("wgrad", name, r16)] = torch.nn.grad.conv3d_weight(rnd(a), w.shape, rnd(g), padding=tuple(v // 2 for v in k))
    dwe = _REF[("wgrad", name, r16)]
    assert rel_err(dw.cpu().view(w.shape), dwe) < (1e-4 if mw in (2, 5, 7) else 5e-5)
    assert rel_err(db.cpu(), g.double().sum((0, 2, 3, 4))) < 5e-5
    if mw == 2 and dt == torch.float32 and ops.conv_wgrad_gmax_ok(xw5, k, Cin, Cout, 2):
        gm = torch.zeros(1, dtype=torch.int32, device=DEV)
        dw.fill_(float("nan"))
        if not expect_or_precondition(lambda: ops.conv_wgrad_gmax(xw5, gw5, k, Cin, Cout, dw, db, gm, mfma=2), [dw, gm]):
            return
        torch.cuda.synchronize()
        assert float(gm.view(torch.float32)) == float(g.abs().max()), "gmax_ok promised max |g|"
        assert rel_err(dw.cpu().view(w.shape), dwe) < 1e-4


def test_wgrad_refusals_write_nothing():
    """Five weight-gradient calls that the launch plan (csrc/conv.hip: wgrad_plan) refuses for an argument, through the C entry
    points: each returns TEM_EINVAL with dw, db, the sums, the amax word and the workspace still at their sentinel -- a refusal
    comes before anything is enqueued.  (1, 8, 8, 8, 32 -> 32), 3x3x3 is the smallest shape of the z-sliding plan."""
    from torch_em_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    N, D, H, W, C = 1, 8, 8, 8, 32
    NV, K = N * D * H * W, (3, 3, 3)
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s, dt=torch.float32: torch.randn(*s, generator=gen).to(DEV, dt)   # noqa: E731
    F16 = 5 | (1 << 8) | (1 << 12)   # use_mfma 5 with fp16 storage of x and g
    assert lib.tem_conv3d_wgrad_sums_ok(N, D, H, W, C, C, *K, 1) == 1   # (wgrad_sums_min_mb is 0 under tests/conftest.py)
    assert lib.tem_conv3d_wgrad_gmax_ok(N, D, H, W, C, C, *K, 5) == 0 and lib.tem_conv3d_wgrad_cs_ok(N, D, H, W, C, C, *K, 0, 64) == 0

    def refused(call, shape=(N, D, H, W, C, C), mode=1):
        """call(dw, db, sums, amax, ws, ws_bytes) -> return code; the outputs it was handed must come back untouched"""
        nws = lib.tem_conv3d_wgrad_ws(*shape, *K, mode)
        outs = [torch.full((n,), SENT, device=DEV) for n in (27 * shape[4] * shape[5], shape[5], 4096, nws // 4 + 1)]
        amax = torch.full((1,), 0x07070707, dtype=torch.int32, device=DEV)
        lib.tem_last_error()
        rc = call(outs[0], outs[1], outs[2], amax, outs[3], nws)
        torch.cuda.synchronize()
        assert rc == EINVAL, (rc, lib.tem_last_error())
        assert all(bool((t == SENT).all()) for t in outs) and int(amax) == 0x07070707, "a refused weight gradient wrote to its outputs"

    x, g, w = rnd(NV, C), rnd(NV, C), rnd(C, C, 3, 3, 3)
    x35 = torch.zeros(NV, 35, device=DEV)
    # exact fp32 with the norm sums, x in rows of 35 floats: the transposing kernel that delivers the sums cannot load them
    refused(lambda dw, db, sums, amax, ws, n: lib.tem_conv3d_wgrad_sums(P(x35), 35, None, None, P(g), C, P(w), None, None, P(dw), P(db), P(sums),
                                                                         P(ws), n, N, D, H, W, C, C, *K, 1, stream))
    # a chunk stride on fp32 tensors
    refused(lambda dw, db, sums, amax, ws, n: lib.tem_conv3d_wgrad_ex(P(x), C, None, None, P(g), C, None, None, None, P(dw), P(db), None, None, None,
                                                                       P(ws), n, N, D, H, W, C, C, *K, 5, 64, None, stream), mode=5)
    # fp16 tensors on a z-sliding kernel other than the transposing one
    x16, g16 = x.half(), g.half()
    old = _lib.get_option("wgrad_zs")
    _lib.set_option("wgrad_zs", 2)
    try:
        refused(lambda dw, db, sums, amax, ws, n: lib.tem_conv3d_wgrad_ex(P(x16), C, None, None, P(g16), C, None, None, None, P(dw), P(db), None, None,
                                                                           None, P(ws), n, N, D, H, W, C, C, *K, F16, 0, None, stream), mode=F16)
    finally:
        _lib.set_option("wgrad_zs", old)
    # the first-layer weight gradient behind a norm, y in rows of 9 floats
    x1, g8, y9, coef = rnd(NV, 1), rnd(NV, 8), torch.zeros(NV, 9, device=DEV), rnd(N, 8, 4)
    refused(lambda dw, db, sums, amax, ws, n: lib.tem_conv3d_wgrad_gnorm(P(x1), 1, None, None, P(g8), 8, P(y9), 9, P(coef), P(dw), P(db), P(ws), n,
                                                                          N, D, H, W, 1, 8, *K, 1, stream), shape=(N, D, H, W, 1, 8), mode=0)
    # max |g| from a one-term mode
    refused(lambda dw, db, sums, amax, ws, n: lib.tem_conv3d_wgrad_ex(P(x), C, None, None, P(g), C, None, None, None, P(dw), P(db), None, None, P(amax),
                                                                       P(ws), n, N, D, H, W, C, C, *K, 5, 0, None, stream), mode=5)


# ---------------------------------------------------------------------------------------------------------------------
# L3: the 32-bit plane edge of the team kernels, H * W * 32 * ld = 2^31 (refused) and ld = 1016 (taken), one wide operand
# at a time.  2 x 4 x 256^2 voxels: 2 GiB per wide fp32 buffer.
# ---------------------------------------------------------------------------------------------------------------------
L3 = (2, 4, 256, 256, 32, 32, (3, 3, 3))
ROWS = [(0, 8), (248, 256)]   # output rows compared against float64 (the first and last planes' worth of byte offsets)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("ld", [1016, 1024])
@pytest.mark.parametrize("wide", ["x", "y", "ref"])
@pytest.mark.parametrize("mode,dt", MODES, ids=[f"m{m}-{str(d)[6:]}" for m, d in MODES])
def test_conv_fwd_plane_edge(mode, dt, wide, ld):
    from torch_em_amd import ops
    N, D, H, W, Cin, Cout, k = L3
    x, w, b, scale, shift, ref = operands(N, D, H, W, Cin, Cout, k, dt, seed=1)
    wp = ops.pack_weights(w.to(DEV), transpose=False, mfma=mode)
    bd, sd, hd = b.to(DEV), scale.to(DEV), shift.to(DEV)
    tol = TOL[mode] + OUT_ROUND[dt]
    x5, xbuf, _ = place(to5(x, dt), "L3" if wide == "x" else "L0", ld)
    ref5, rbuf, _ = place(to5(ref, dt), "L3" if wide == "ref" else "L0", ld)
    y5, ybuf, _ = place(torch.zeros(N, D, H, W, Cout, device=DEV, dtype=dt), "L3" if wide == "y" else "L0", ld)
    kw = dict(scale=sd, shift=hd, act="relu")
    team = 3 if (mode >= 2 or mode == 1) else 0
    if mode >= 1 and dt == torch.float32:
        fam = ops.conv_fwd_family(x5, k, Cin, Cout, mode, y=y5, ref=ref5 if wide == "ref" else None)
        assert fam == (team if ld < 1024 else 0), fam   # 2^31: the z-reuse kernel must decline the layout
    if wide == "ref":
        y5.fill_(float("nan"))
        ops.conv_fwd(x5, wp, bd, y5, k, Cin, Cout, ref=ref5, mfma=mode, **kw)
        for r in ROWS:
            exp = ref_conv(x, w, b, mode, ref=ref, rows=r, scale=scale, shift=shift, act="relu")
            assert rel_err(nc(y5[:, :, r[0]:r[1]]), exp) < tol, r
        return
    nblk = ops.conv_fwd_stat_blocks(x5, k, Cin, Cout, mode, y=y5)
    dense = ops.conv_fwd_stat_blocks(ops.Probe(N, D, H, W, Cin, dt), k, Cin, Cout, mode)
    if wide == "y" and nblk > 0:
        if nblk != dense:   # a buffer sized by the dense query: the launch refuses it before writing
            y5.fill_(SENT)
            rc, _ = stats_through_cabi(x5, wp, bd, y5, None, N, D, H, W, Cin, Cout, k, mode, dense, **kw)
            assert rc != 0 and bool((ybuf == SENT).all())
    y5.fill_(float("nan"))
    if nblk > 0:
        rc, part = stats_through_cabi(x5, wp, bd, y5, None, N, D, H, W, Cin, Cout, k, mode, nblk, **kw)
        assert rc == 0, ops._lib.load().tem_last_error()
        check_stats(part, y5, N, Cout)
    else:
        assert ops.conv_fwd(x5, wp, bd, y5, k, Cin, Cout, mfma=mode, want_stats=True, **kw) is None
    for r in ROWS:
        exp = ref_conv(x, w, b, mode, rows=r, scale=scale, shift=shift, act="relu")
        assert rel_err(nc(y5[:, :, r[0]:r[1]]), exp) < tol, r
    if ybuf is not None:
        assert bool((ybuf[..., Cout:] == SENT).all())


@pytest.mark.timeout(180)
@pytest.mark.parametrize("ld", [1016, 1024])
def test_refnorm_and_gscaled_plane_edge(ld):
    """the data-gradient epilogues at the edge: the layout query decides, and the launch honours its answer"""
    from torch_em_amd import ops
    N, D, H, W, Cin, Cout, k = L3
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(N, Cout, D, H, W, generator=gen)
    w = torch.randn(Cout, Cin, *k, generator=gen) * 0.03
    a = torch.randn(N, Cin, D, H, W, generator=gen)
    g5, a5 = to5(g), to5(a)
    y5, ybuf, _ = place(torch.zeros(N, D, H, W, Cin, device=DEV), "L3", ld)
    coef = torch.rand(N, Cin, 4, generator=gen) + 0.5
    wt = w.transpose(0, 1).flip(2, 3, 4)
    for mode in (2, 4):
        wpt = ops.pack_weights(w.to(DEV), transpose=True, mfma=mode)
        fam = ops.conv_fwd_family(g5, k, Cout, Cin, mode, y=y5, ref=a5)
        assert fam == (3 if ld < 1024 else 0)
        ybuf.fill_(SENT)
        try:
            if mode == 2:
                ops.conv_fwd_refnorm(g5, wpt, y5, k, Cout, Cin, a5, coef.to(DEV), mode)
            else:
                amax = torch.zeros(1, dtype=torch.int32, device=DEV)
                amax.view(torch.float32)[0] = float(g.abs().max())
                ops.conv_fwd_gscaled(g5, wpt, y5, k, Cout, Cin, amax, ref=a5)
            took = True
        except ValueError:
            took = False
        torch.cuda.synchronize()
        assert took == (fam == 3)
        if not took:
            assert bool((ybuf == SENT).all()), "raised after writing"
            continue
        for r in ROWS:
            conv = ref_conv(g, wt, None, mode, rows=r)
            ar = a[:, :, :, r[0]:r[1]].double()
            if mode == 2:
                c = coef.double()[:, :, :, None, None, None]
                exp = torch.where(ar > 0, c[:, :, 0] * conv - c[:, :, 1] - (ar - c[:, :, 3]) * c[:, :, 2], torch.zeros(()).double())
            else:
                exp = conv * (ar > 0)
            assert rel_err(nc(y5[:, :, r[0]:r[1]]), exp) < 1e-4, (mode, r)
        assert bool((ybuf[..., Cin:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# a whole step across the edge: the level-0 concat buffer (ld = 2 x 32 features) of a 4 x 1024 x 1024 patch crosses it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(240)
@pytest.mark.parametrize("width,precision", [(1024, None), (1008, None), (1024, "fp32")])
def test_model_step_across_the_plane_edge(width, precision):
    import contextlib

    from oracle import unet_ref
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import AnisotropicUNet, engine
    sf = [[1, 2, 2]]
    torch.manual_seed(0)
    model = AnisotropicUNet(1, 2, scale_factors=sf, initial_features=32)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 1, 4, 1024, width, generator=gen)
    y = (torch.rand(1, 2, 4, 1024, width, generator=gen) > 0.5).float()
    sd = {k: v.detach().clone().double() for k, v in model.state_dict().items()}
    pred_o, loss_o, grads_o = unet_ref.unet_loss_and_grads(sd, x.double(), y.double(), sf)
    model.to(DEV)
    with (engine.precision_scope(precision) if precision else contextlib.nullcontext()):
        pred = model(x.to(DEV))
        loss = DiceLoss()(pred, y.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert rel_err(pred.detach().cpu(), pred_o) < 1e-3
    assert abs(float(loss.detach()) - float(loss_o)) < 1e-4
    check_grads({k: p.grad.cpu() for k, p in model.named_parameters()}, grads_o, 1e-3)
