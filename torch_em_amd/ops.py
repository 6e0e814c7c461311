"""Tensor-level wrappers over the C-ABI (include/tem_hip.h).

Every function takes torch CUDA tensors only to obtain device pointers, strides and the
current HIP stream -- all arithmetic happens in libtem_hip.so.  Activations are 5-D
channels-last views `t[N, D, H, W, C]` with `t.stride(4) == 1`; `t.stride(3)` (the leading
dimension `ld`) may exceed C so that a tensor can be a channel slice of a concat buffer.
There is no CPU fallback: CPU tensors raise.
"""
import ctypes
import math
import numbers
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .arith import Arith, PackKind, pack_is_tiled

ACT = {None: 0, "none": 0, "relu": 1, "sigmoid": 2}

# Optional live kernel timing (bench.py): a list that receives (tag, flops, start_event, end_event)
# for every convolution launch; events are recorded on the stream the kernel is launched on.
PROFILER = None
# When set, only launches whose kernel tag is in this set are timed: two HIP events per launch are not free (a
# fully instrumented cfg-2 step has ~200 of them and runs 3.5-6 ms slower), so bench.py instruments everything in a
# warm-up step and only the dominant kernel inside the timed region.
PROFILER_FILTER = None


def _fwd_tag(mfma, k, cout, pp=False):
    mode = Arith(int(mfma))
    if pp in (3, 4):  # the z-reuse team kernel (csrc/conv_zr.hip); 4 = its split-K launch (16^3 / 32^3 levels)
        return f"k_conv_zr_{mode.facts.zr}<3,3,3>"
    if pp:  # the ping-pong team kernel (csrc/conv_pp.hip): the one-term modes run under the bf16x3 tag
        return f"k_conv_pp_{'f16x3' if mode is Arith.F16X3 else 'bf16x3'}<{k[0]},{k[1]},{k[2]},CT={2 if cout % 64 == 0 else 1}>"
    kind = "k_conv_fwd_" + (mode.facts.fwd or ("mfma" if mode else "valu")) + f"<{k[0]},{k[1]},{k[2]}"
    return kind + (f",NR={2 if cout % 64 == 0 else 1}>" if mode else ">")


def _wgrad_tag(mfma, k, cout):
    mode = Arith(int(mfma))
    split = mode.facts.wgrad
    nco = f",NCO={2 if cout >= 64 else 1}" if split and k[0] * k[1] * k[2] > 1 else ""
    return "k_conv_wgrad_" + (split or ("mfma" if mode else "valu")) + f"<{k[0]},{k[1]},{k[2]}{nco}>(+reduce)"


class _Timed:
    """`with _Timed(t, tag, (N, D, H, W), cin, cout, k): <launch>` -- the PROFILER bracket of one convolution launch: two events
    on the stream of `t` around the body and one (tag, flops, start, end) entry; nothing when the launch is not timed."""
    __slots__ = ("args", "ev0")

    def __init__(self, *args):
        self.args = args

    def __enter__(self):
        t, tag = self.args[:2]
        self.ev0 = None
        if PROFILER is not None and (PROFILER_FILTER is None or tag in PROFILER_FILTER):
            self.ev0 = torch.cuda.Event(enable_timing=True)
            self.ev0.record(torch.cuda.current_stream(t.device))

    def __exit__(self, exc_type, exc, tb):
        if self.ev0 is None or exc_type is not None:
            return
        t, tag, (N, D, H, W), cin, cout, k = self.args
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream(t.device))
        PROFILER.append(((tag, f"{N}x{D}x{H}x{W} {cin}->{cout}"), 2.0 * N * D * H * W * cin * cout * k[0] * k[1] * k[2], self.ev0, ev1))


def _stream(t: torch.Tensor):
    """The stream the launch goes to: torch's current stream of the TENSOR's device.  A HIP launch is issued on the
    calling thread's current device, so that device is made current for the launch and `_lib.check()` -- which wraps
    every launch -- restores the caller's (one process drives one GPU in this design; a process that touches several --
    `DefaultTrainer(device="cuda:1")`, `predict_with_halo(gpu_ids=[1])` -- gets the device of the tensors it passes,
    like a torch op would, and keeps its own current device)."""
    _lib.launch_on(t.device.index)
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# activation storage types of the C-ABI (TEM_ST_F32 / _F16 / _BF16, include/tem_hip.h): the element type of a tensor handed to
# the `_st` entry points, and -- shifted into the high bits of `use_mfma` -- to the convolution entry points
_ST = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _st(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else _ST[t.dtype]


def _mode(mfma, x, y) -> int:
    """use_mfma | TEM_MFMA_STX(storage of x) | TEM_MFMA_STY(storage of y)"""
    return int(mfma) | (_st(x) << 8) | (_st(y) << 12)


def _same_st(*ts):
    sts = {t.dtype for t in ts if t is not None}
    if len(sts) > 1:
        raise ValueError(f"tensors of one call must share their storage type, got {sorted(str(d) for d in sts)}")


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "torch_em_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback for this path"
            )


def _act5(t: torch.Tensor) -> Tuple[int, int, int, int, int, int]:
    """(N, D, H, W, C, ld) of a channels-last 5-D view; validates the stride contract:
    element (n,z,y,x,c) at (((n*D+z)*H+y)*W+x)*ld + c."""
    if isinstance(t, Planar):
        return (*t.shape, 32)
    if isinstance(t, Probe):
        return (*t.shape, t.ld)
    if t.dim() != 5:
        raise ValueError(f"expected a 5-D NDHWC tensor, got shape {tuple(t.shape)}")
    if t.dtype not in _ST:
        raise ValueError(f"expected float32 (or float16 / bfloat16 activation storage), got {t.dtype}")
    N, D, H, W, C = t.shape
    s = t.stride()
    sizes = (N, D, H, W)
    inner = [1, 1, 1, 1]  # voxels spanned by one step along each dim
    for k in (2, 1, 0):
        inner[k] = inner[k + 1] * sizes[k + 1]
    ld = None
    for k in (3, 2, 1, 0):
        if sizes[k] > 1:
            if s[k] % inner[k]:
                raise ValueError(f"tensor is not a channels-last NDHWC view: shape {tuple(t.shape)}, strides {s}")
            ld = s[k] // inner[k]
            break
    if ld is None:
        ld = C
    ok = (C == 1 or s[4] == 1) and ld >= C
    for k in range(4):
        if sizes[k] > 1 and s[k] != ld * inner[k]:
            ok = False
    if not ok:
        raise ValueError(f"tensor is not a channels-last NDHWC view: shape {tuple(t.shape)}, strides {s}")
    return N, D, H, W, C, ld


def new_act(N, D, H, W, C, device, dtype=torch.float32) -> torch.Tensor:
    return torch.empty((N, D, H, W, C), dtype=dtype, device=device)


class Planar:
    """A [N, D, H, W, 2 * 32] activation whose two 32-channel halves are two DENSE tensors of one allocation
    (buf [2, N, D, H, W, 32]): the concat buffer of a level whose halves would otherwise be 64 bytes of every 128-byte line
    in 16-bit storage (DESIGN.md 6.R5 "half lines").  The kernels that read / write all 64 channels take it through a chunk
    stride (x_cs / y_cs of tem_conv3d_fwd_ex / _wgrad_ex); everything else gets `halves[i]`, an ordinary dense tensor."""

    def __init__(self, buf: torch.Tensor):
        if buf.dim() != 6 or buf.shape[0] != 2 or buf.shape[5] != 32 or not buf.is_contiguous() or buf.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("Planar: expects a contiguous 16-bit [2, N, D, H, W, 32] buffer")
        self.buf, self.halves = buf, (buf[0], buf[1])
        self.shape = (*buf.shape[1:5], 64)
        self.dtype, self.device, self.is_cuda = buf.dtype, buf.device, buf.is_cuda
        self.cs = buf[0].numel()      # elements between the two 32-channel chunks of a voxel

    @staticmethod
    def empty(N, D, H, W, device, dtype):
        return Planar(torch.empty((2, N, D, H, W, 32), dtype=dtype, device=device))

    def empty_like(self):
        return Planar(torch.empty_like(self.buf))

    def data_ptr(self):
        return self.buf.data_ptr()

    def dim(self):
        return 5

    def record_stream(self, s):
        self.buf.record_stream(s)


def _cs(t) -> int:
    return t.cs if isinstance(t, Planar) else 0


class Probe:
    """shape + storage type (+ leading dimension: default dense) of an activation, for the query functions
    (conv_fwd_family, ..._ok) only; a Probe counts as 16-byte aligned"""

    def __init__(self, N, D, H, W, C, dtype, ld=None):
        self.shape, self.dtype, self.ld = (N, D, H, W, C), dtype, C if ld is None else int(ld)


# ---------------------------------------------------------------- layout ----
def nchw_to_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, C, *spatial] contiguous -> NDHWC (spatial may be 2-D or 3-D; 2-D gets D == 1)."""
    _req_cuda(x)
    x = x.contiguous()
    N, C = x.shape[:2]
    sp = tuple(x.shape[2:])
    D, H, W = (1,) * (3 - len(sp)) + sp
    if C == 1 and out is None:
        return x.reshape(N, D, H, W, 1)
    if out is None:
        out = new_act(N, D, H, W, C, x.device)
    _, _, _, _, _, ld = _act5(out)
    lib = _lib.load()
    _lib.check(lib.tem_nchw_to_nhwc(_p(x), _p(out), ld, N, C, D * H * W, _stream(x)), "tem_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _req_cuda(x)
    N, D, H, W, C, ld = _act5(x)
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.tem_nhwc_to_nchw(_p(x), ld, _p(out), N, C, D * H * W, _stream(x)), "tem_nhwc_to_nchw")
    return out


# ------------------------------------------------------------------ conv ----
def mfma_ok(cin: int, cout: int, k: Sequence[int], wgrad: bool = False) -> bool:
    key = tuple(int(v) for v in k)
    if key not in ((3, 3, 3), (1, 3, 3), (1, 1, 1)):
        return False
    if wgrad:
        return cin % 32 == 0 and cout % 32 == 0
    return cin % 16 == 0 and cout % 32 == 0


def pack_weights(w: torch.Tensor, transpose: bool, mfma) -> torch.Tensor:
    """state_dict layout [Cout, Cin, (kd,) kh, kw] -> kernel layout (see tem_hip.h).
    mfma: the arithmetic mode whose layout is written (arith.Arith; False / True: VALU / exact fp32) -- a TEM_WL_* layout
    IS the mode it serves."""
    _req_cuda(w)
    w = w.detach().contiguous()
    cout, cin = w.shape[:2]
    k = tuple(w.shape[2:])
    k = (1,) * (3 - len(k)) + k
    lib = _lib.load()
    dst = torch.empty(lib.tem_conv_packed_size(cout, cin, k[0], k[1], k[2]), dtype=torch.float32, device=w.device)
    _lib.check(lib.tem_conv_pack_weights(_p(w), _p(dst), cout, cin, k[0], k[1], k[2], int(transpose),
                                         int(Arith(int(mfma))), _stream(w)), "tem_conv_pack_weights")
    return dst


def pack_table(jobs):
    """Device descriptor tables for tem_conv_pack_weights_tiles (all tensors whose kernel has <= 27 taps: one workgroup per
    32 x 32 x taps tile) and tem_conv_pack_weights_batch (the rest).  jobs: (w, dst, cout, cin, k3, transpose, planes, kind)
    with (planes, kind) = Arith.pack of the layout."""
    import struct
    tiled, gather = b"", b""
    ntile = nitem = n_t = n_g = 0
    for w, dst, cout, cin, k, transpose, planes, kind in jobs:
        taps = k[0] * k[1] * k[2]
        if pack_is_tiled(planes, k, cout, cin):   # (planes 0 = generic fp32 layout: gather kernel only)
            tiled += struct.pack("<qq8iq", w.data_ptr(), dst.data_ptr(), cout, cin, k[0], k[1], k[2], int(transpose), planes,
                                 int(kind), ntile)
            ntile += ((cout + 31) // 32) * ((cin + 31) // 32)
            n_t += 1
        else:
            if kind == PackKind.FP32:
                raise ValueError(f"pack_table: the exact-fp32 layout of a {cout} x {cin} x {k} weight is not tileable and the "
                                 "gather kernel cannot write it (use pack_weights)")
            gather += struct.pack("<qq8iq", w.data_ptr(), dst.data_ptr(), cout, cin, k[0], k[1], k[2], int(transpose),
                                  planes, int(kind), nitem)
            nitem += cout * cin * taps // 8
            n_g += 1
    dev = jobs[0][0].device
    mk = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev) if blob else None  # noqa: E731
    return {"tiles": mk(tiled), "n_tiles": n_t, "total_tiles": ntile, "table": mk(gather), "n": n_g, "total": nitem,
            "keep": [(j[0], j[1]) for j in jobs]}


def pack_weights_batch(tab):
    lib = _lib.load()
    if tab["n_tiles"]:
        _lib.check(lib.tem_conv_pack_weights_tiles(_p(tab["tiles"]), tab["n_tiles"], tab["total_tiles"],
                                                   _stream(tab["tiles"])), "tem_conv_pack_weights_tiles")
    if tab["n"]:
        _lib.check(lib.tem_conv_pack_weights_batch(_p(tab["table"]), tab["n"], tab["total"], _stream(tab["table"])),
                   "tem_conv_pack_weights_batch")


def _launch_fwd(x, x_ld, w_packed, y, y_ld, ref, ref_ld, dims, cin, cout, k, mode, ws_mode, tag, scale=None, shift=None,
                bias=None, act=None, in_amax=None, ref_coef=None, part=None, x_cs=0, y_cs=0, bp=None):
    """The one tem_conv3d_fwd_ex call of the forward / data-gradient wrappers.  mode: the use_mfma word of the launch;
    ws_mode: the one the workspace is sized for (None: no workspace); tag: the profiler's kernel tag (None: not timed)."""
    N, D, H, W = dims
    lib = _lib.load()
    nws = lib.tem_conv3d_fwd_ws(N, D, H, W, cin, cout, k[0], k[1], k[2], ws_mode) if ws_mode is not None else 0
    ws = _workspace(nws, x.device) if nws else None
    with _Timed(x, tag, dims, cin, cout, k):
        _lib.check(lib.tem_conv3d_fwd_ex(_p(x), x_ld, _p(scale), _p(shift), _p(w_packed), _p(bias), _p(y), y_ld, _p(ref),
                                         ref_ld, _p(ws), nws, N, D, H, W, cin, cout, k[0], k[1], k[2], ACT[act], mode,
                                         _p(in_amax), _p(ref_coef), _p(part), part.shape[1] if part is not None else 0,
                                         x_cs, y_cs, bp.ref() if bp is not None else None, _stream(x)), "tem_conv3d_fwd_ex")


def conv_fwd(x, w_packed, bias, y, k, cin, cout, scale=None, shift=None, act=None, ref=None, mfma=False,
             want_stats=False, bp=None):
    """want_stats: also emit the first stage of the statistics of y (stat_part of tem_conv3d_fwd_ex) when this launch can;
    returns (partials [N, nblk, cout, 2], nblk) then, else y (and `None` for launches that cannot: use norm_stats).
    bp: Byproducts of this call (tem_conv3d_fwd_ex), not together with want_stats."""
    if bp is not None and want_stats:
        raise ValueError("conv_fwd: by-products and want_stats exclude each other")
    _req_cuda(x, w_packed, y)
    N, D, H, W, C, x_ld = _act5(x)
    Ny, Dy, Hy, Wy, Cy, y_ld = _act5(y)
    if C != cin or Cy != cout or (N, D, H, W) != (Ny, Dy, Hy, Wy):
        raise ValueError(f"conv_fwd: shape mismatch x{tuple(x.shape)} y{tuple(y.shape)} cin={cin} cout={cout}")
    ref_ld = 0
    if ref is not None:
        ref_ld = _act5(ref)[5]
        _same_st(y, ref)
    lib = _lib.load()
    mode = _mode(mfma, x, y)
    kind = None
    if PROFILER is not None:
        pp = lib.tem_conv3d_fwd_kernel_ld(N, D, H, W, cin, cout, k[0], k[1], k[2], mode, x_ld, y_ld, ref_ld,
                                          _misaligned(x, w_packed, bias, y, ref, scale, shift)) if mfma else 0
        kind = _fwd_tag(mfma, k, cout, pp)
    nblk = lib.tem_conv3d_fwd_stat_blocks_ld(N, D, H, W, cin, cout, k[0], k[1], k[2], mode, x_ld, y_ld, ref_ld,
                                             _misaligned(x, w_packed, bias, y, ref, scale, shift)) if want_stats else 0
    if want_stats and nblk <= 0 and (_cs(x) or _cs(y)):
        raise RuntimeError("conv_fwd: a planar tensor needs the z-reuse kernel (statistics rows expected)")
    part = torch.empty((N, nblk, cout, 2), dtype=torch.float32, device=x.device) if nblk > 0 else None
    _launch_fwd(x, x_ld, w_packed, y, y_ld, ref, ref_ld, (N, D, H, W), cin, cout, k, mode, mode if mfma else None, kind,
                scale=scale, shift=shift, bias=bias, act=act, part=part, x_cs=_cs(x), y_cs=_cs(y), bp=bp)
    if want_stats:
        return None if part is None else (part, int(nblk))
    return y


_ws_cache = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    """A per-(device, stream) scratch buffer (grown on demand, reused across calls on the same stream; kernels of
    different streams may run concurrently, so they never share one)."""
    device = torch.device(device)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def conv_wgrad_gnorm_ok(k, cin, cout, mfma) -> bool:
    return bool(_lib.load().tem_conv3d_wgrad_gnorm_ok(cin, cout, k[0], k[1], k[2], int(mfma)))


def conv_wgrad_gnorm(x, g, y, coef, k, cin, cout, dw_out, db_out=None, scale=None, shift=None):
    """First-layer weight gradient with the backward of the norm behind this conv's ReLU applied to g on load
    (tem_conv3d_wgrad_gnorm_st): g raw data gradient, y this conv's output, coef from norm_bwd_coef."""
    _req_cuda(x, g, y, coef, dw_out)
    N, D, H, W, C, x_ld = _act5(x)
    g_ld, y_ld = _act5(g)[5], _act5(y)[5]
    _same_st(g, y)
    lib = _lib.load()
    nws = lib.tem_conv3d_wgrad_ws(N, D, H, W, cin, cout, k[0], k[1], k[2], Arith.VALU)
    ws = _workspace(nws, x.device)
    kind = _wgrad_tag(Arith.VALU, k, cout) if PROFILER is not None else None
    with _Timed(x, kind, (N, D, H, W), cin, cout, k):
        _lib.check(lib.tem_conv3d_wgrad_gnorm_st(_p(x), x_ld, _p(scale), _p(shift), _p(g), g_ld, _p(y), y_ld, _p(coef), _p(dw_out),
                                                 _p(db_out), _p(ws), nws, N, D, H, W, cin, cout, k[0], k[1], k[2], 1, _st(x), _st(g),
                                                 _stream(x)), "tem_conv3d_wgrad_gnorm_st")


def conv_wgrad_sums_ok(x, k, cin, cout, mfma) -> bool:
    N, D, H, W, _, _ = _act5(x)
    return bool(_lib.load().tem_conv3d_wgrad_sums_ok(N, D, H, W, cin, cout, k[0], k[1], k[2], _mode(mfma, x, x)))


def _launch_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, arith, mode, sums_from=None, amax_in=None, amax_out=None,
                  x_cs=0, bp=None, match_channels=False):
    """The one tem_conv3d_wgrad_ex call of the weight-gradient wrappers -> sums[N, cin, 2] with sums_from, else None.
    arith: the arithmetic mode the profiler tag names; mode: the use_mfma word of the launch and of its workspace."""
    N, D, H, W, C, x_ld = _act5(x)
    Cg, g_ld = _act5(g)[4:]
    if match_channels and (C != cin or Cg != cout):
        raise ValueError("conv_wgrad: channel mismatch")
    lib = _lib.load()
    nws = lib.tem_conv3d_wgrad_ws(N, D, H, W, cin, cout, k[0], k[1], k[2], mode)
    ws = _workspace(nws, x.device)
    w = gamma = beta = sums = None
    if sums_from is not None:
        w, gamma, beta = sums_from
        w = w.detach()
        sums = torch.empty((N, cin, 2), dtype=torch.float32, device=x.device)
    kind = _wgrad_tag(arith, k, cout) if PROFILER is not None else None
    with _Timed(x, kind, (N, D, H, W), cin, cout, k):
        _lib.check(lib.tem_conv3d_wgrad_ex(_p(x), x_ld, _p(scale), _p(shift), _p(g), g_ld, _p(w), _p(gamma), _p(beta),
                                           _p(dw_out), _p(db_out), _p(sums), _p(amax_in), _p(amax_out), _p(ws), nws, N, D, H, W,
                                           cin, cout, k[0], k[1], k[2], mode, x_cs, bp.ref() if bp is not None else None,
                                           _stream(x)), "tem_conv3d_wgrad_ex")
    return sums


def conv_wgrad(x, g, k, cin, cout, dw_out, db_out=None, scale=None, shift=None, mfma=False, sums_from=None, bp=None):
    """sums_from = (weight [state_dict layout], gamma, beta): also return sums[N, cin, 2] = (sum gz, sum gz*xn) of the
    norm in front of this conv (norm_sums of tem_conv3d_wgrad_ex; check conv_wgrad_sums_ok first)."""
    if sums_from is not None:
        return _conv_wgrad_sums(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma, sums_from, bp)
    return _conv_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma)


def _conv_wgrad(x, g, k, cin, cout, dw_out, db_out=None, scale=None, shift=None, mfma=False):
    """dw_out: flat [ntaps*cin*cout] in the reference's [Cout,Cin,kd,kh,kw] order; db_out: [cout]."""
    _req_cuda(x, g, dw_out)
    _launch_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma, _mode(mfma, x, g), x_cs=_cs(x), match_channels=True)
    return dw_out


def _conv_wgrad_sums(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma, sums_from, bp=None):
    _req_cuda(x, g, dw_out, db_out)
    return _launch_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma, _mode(mfma, x, g), sums_from=sums_from,
                         x_cs=_cs(x), bp=bp)


def conv_wgrad_gmax_ok(x, k, cin, cout, mfma) -> bool:
    N, D, H, W, _, _ = _act5(x)
    return bool(_lib.load().tem_conv3d_wgrad_gmax_ok(N, D, H, W, cin, cout, k[0], k[1], k[2], int(mfma)))


def conv_wgrad_gmax(x, g, k, cin, cout, dw_out, db_out, gmax, scale=None, shift=None, mfma=Arith.BF16X3, sums_from=None, bp=None):
    """conv_wgrad that also leaves the bit pattern of max |g| in `gmax` (int32[1], cleared by the caller) -- the prescale
    of the fp16 two-term data gradient (conv_fwd_gscaled).  sums_from as in conv_wgrad -> sums[N, cin, 2] or None."""
    _req_cuda(x, g, dw_out, gmax)
    return _launch_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, mfma, int(mfma), sums_from=sums_from, amax_out=gmax, bp=bp)


def conv1x1_out_bwd_ok(cin, cout) -> bool:
    return bool(_lib.load().tem_conv1x1_out_bwd_ok(int(cin), int(cout)))


def conv1x1_out_bwd(x, g, w, gx, dw_out, db_out=None, out_amax=None):
    """Backward of the output projection in one pass over its input x (tem_conv1x1_out_bwd_st): dw [cout, cin, 1, 1, 1]-ordered, db,
    and gx = (x > 0) * (g . w).  x, gx: [N, D, H, W, cin(ld)]; g: [N, D, H, W, cout(ld)]; w: the conv's weight (state_dict)."""
    _req_cuda(x, g, w, gx, dw_out)
    N, D, H, W, cin, x_ld = _act5(x)
    cout, g_ld = _act5(g)[4], _act5(g)[5]
    gx_ld = _act5(gx)[5]
    lib = _lib.load()
    nws = lib.tem_conv1x1_out_bwd_ws(cin, cout)
    ws = _workspace(nws, x.device)
    _same_st(x, gx)
    _lib.check(lib.tem_conv1x1_out_bwd_st(_p(x), x_ld, _p(g), g_ld, _p(w.detach()), _p(gx), gx_ld, _p(dw_out), _p(db_out),
                                          _p(ws), nws, N * D * H * W, cin, cout, _p(out_amax), _st(x), _st(g), _stream(x)),
               "tem_conv1x1_out_bwd_st")
    return gx


def conv_wgrad_gscaled_ok(x, k, cin, cout) -> bool:
    N, D, H, W, _, _ = _act5(x)
    return bool(_lib.load().tem_conv3d_wgrad_gscaled_ok(N, D, H, W, cin, cout, k[0], k[1], k[2]))


def conv_wgrad_cs_ok(x, k, cin, cout, x_cs) -> bool:
    """does the weight gradient honour the chunk stride `x_cs` (elements) of a Planar input of x's size and element type?"""
    N, D, H, W, _, _ = _act5(x)
    return bool(_lib.load().tem_conv3d_wgrad_cs_ok(N, D, H, W, cin, cout, k[0], k[1], k[2], _ST[x.dtype], int(x_cs)))


def absmax(x, amax=None):
    """bit pattern of max |x| of an activation tensor [N, D, H, W, C(ld)] -> int32[1] on the device (tem_absmax);
    `amax` (cleared by the caller) accumulates when given."""
    _req_cuda(x)
    N, D, H, W, C, ld = _act5(x)
    if amax is None:
        amax = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.check(_lib.load().tem_absmax(_p(x), ld, C, N * D * H * W, _p(amax), _stream(x)), "tem_absmax")
    return amax


class Byproducts:
    """Optional by-products of ONE library call, passed explicitly (include/tem_hip.h: TemByproducts):
      out_amax  = int32[1] (cleared by the caller): bit pattern of max |output| of the tensor the call writes;
      norm_coef = (groups, mean, rstd, coef [N, C, 4]): a weight gradient that delivers the norm sums (sums_from=...) also
                  finishes them into what norm_bwd_coef(sums=...) returns for a norm without affine parameters;
      norm_sums = (x, groups, mean, rstd, part [N, nblk, C, 2]): a data gradient on the split-K z-reuse kernel also writes
                  the first stage of the backward of the norm whose input is x.
    After the call `amax` / `coef` / `sums` tell which of them it delivered (the caller runs the separate stage otherwise)."""

    def __init__(self, out_amax=None, norm_coef=None, norm_sums=None):
        c = _lib.Byproducts()
        self._keep = (out_amax, norm_coef, norm_sums)
        c.out_amax = _p(out_amax)
        if norm_coef is not None:
            groups, mean, rstd, coef = norm_coef
            c.coef_G, c.coef_mean, c.coef_rstd, c.coef = int(groups), _p(mean), _p(rstd), _p(coef)
        if norm_sums is not None:
            x, groups, mean, rstd, part = norm_sums
            c.sums_x, c.sums_x_ld, c.sums_mean, c.sums_rstd = _p(x), _act5(x)[5], _p(mean), _p(rstd)
            c.sums_G, c.sums_part, c.sums_nblk = int(groups), _p(part), part.shape[1]
        self.c = c

    def ref(self):
        return ctypes.cast(ctypes.pointer(self.c), ctypes.c_void_p)

    amax = property(lambda self: bool(self.c.delivered & _lib.BP_OUT_AMAX))
    coef = property(lambda self: bool(self.c.delivered & _lib.BP_NORM_COEF))
    sums = property(lambda self: bool(self.c.delivered & _lib.BP_NORM_SUMS))


def conv_wgrad_gscaled(x, g, k, cin, cout, dw_out, db_out, amax, scale=None, shift=None, sums_from=None, bp=None):
    """Weight gradient in the fp16 2x1 arithmetic (g_amax_in of tem_conv3d_wgrad_ex): x^ two fp16 terms, g one fp16 term prescaled
    from amax = int32[1] with the bit pattern of max |g| (absmax or a producer of g).  sums_from as in conv_wgrad."""
    _req_cuda(x, g, dw_out, amax)
    return _launch_wgrad(x, g, k, cin, cout, dw_out, db_out, scale, shift, Arith.F16X2, Arith.F16X2, sums_from=sums_from,
                         amax_in=amax, bp=bp)


def conv_fwd_gscaled(x, w_packed, y, k, cin, cout, amax, ref=None, bp=None):
    """Data gradient with fp32-class products (in_amax of tem_conv3d_fwd_ex): x an unnormalised gradient, w_packed =
    pack_weights(w, transpose=True, mfma=Arith.F16X3), amax = int32[1] holding the bit pattern of max |x| (conv_wgrad_gmax)."""
    _req_cuda(x, w_packed, y, amax)
    N, D, H, W, C, x_ld = _act5(x)
    Ny, Dy, Hy, Wy, Cy, y_ld = _act5(y)
    if C != cin or Cy != cout or (N, D, H, W) != (Ny, Dy, Hy, Wy):
        raise ValueError(f"conv_fwd_gscaled: shape mismatch x{tuple(x.shape)} y{tuple(y.shape)} cin={cin} cout={cout}")
    ref_ld = _act5(ref)[5] if ref is not None else 0
    kind = _fwd_tag(Arith.F16X3, k, cout, 3) if PROFILER is not None else None
    _launch_fwd(x, x_ld, w_packed, y, y_ld, ref, ref_ld, (N, D, H, W), cin, cout, k, Arith.F16X3, Arith.FP32, kind, in_amax=amax,
                bp=bp)
    return y


def conv_fwd_refnorm(x, w_packed, y, k, cin, cout, ref, coef, mfma, bp=None):
    """Data gradient that lands behind a ReLU + norm (ref_coef of tem_conv3d_fwd_ex): y = ref > 0 ? a*conv(x) - m1 - (ref - mean)*m2r
    : 0, coef [N, cout, 4] from norm_bwd_coef.  Only where conv_fwd_family(...) == 3."""
    _req_cuda(x, w_packed, y, ref, coef)
    N, D, H, W, C, x_ld = _act5(x)
    Ny, Dy, Hy, Wy, Cy, y_ld = _act5(y)
    if C != cin or Cy != cout or (N, D, H, W) != (Ny, Dy, Hy, Wy) or tuple(coef.shape) != (N, cout, 4) or \
            not coef.is_contiguous():
        raise ValueError(f"conv_fwd_refnorm: shape mismatch x{tuple(x.shape)} y{tuple(y.shape)} coef{tuple(coef.shape)}")
    ref_ld = _act5(ref)[5]
    _same_st(x, y, ref)
    kind = _fwd_tag(mfma, k, cout, 3) if PROFILER is not None else None
    _launch_fwd(x, x_ld, w_packed, y, y_ld, ref, ref_ld, (N, D, H, W), cin, cout, k, _mode(mfma, x, y), Arith.FP32, kind,
                ref_coef=coef, bp=bp)
    return y


def _misaligned(*ts) -> int:
    """1 when a tensor of a launch is off a 16-byte boundary (Probe / Planar / None count as aligned)"""
    return int(any(isinstance(t, torch.Tensor) and t.data_ptr() % 16 for t in ts))


def _fwd_layout(x, cout, y, ref):
    """(x_ld, y_ld, ref_ld, misaligned) of a launch that reads x and writes y (default: dense, aligned) with ref"""
    x_ld = _act5(x)[5]
    y_ld = _act5(y)[5] if y is not None else cout
    ref_ld = _act5(ref)[5] if ref is not None else 0
    return x_ld, y_ld, ref_ld, _misaligned(x, y, ref)


def conv_fwd_stat_blocks(x, k, cin, cout, mfma, y=None, ref=None) -> int:
    """tem_conv3d_fwd_stat_blocks_ld: statistics partial rows per sample the launch from x into y (None: a dense output)
    writes (0: it cannot)"""
    N, D, H, W, _, _ = _act5(x)
    return int(_lib.load().tem_conv3d_fwd_stat_blocks_ld(N, D, H, W, cin, cout, k[0], k[1], k[2], _mode(mfma, x, x),
                                                         *_fwd_layout(x, cout, y, ref)))


def conv_fwd_family(x, k, cin, cout, mfma, y=None, ref=None) -> int:
    """tem_conv3d_fwd_kernel_ld of the launch from x into y (None: a dense output) with ref: 0 patch / other kernels, 1 / 2
    ping-pong teams, 3 z-reuse teams, 4 z-reuse teams with split-K"""
    N, D, H, W, _, _ = _act5(x)
    return int(_lib.load().tem_conv3d_fwd_kernel_ld(N, D, H, W, cin, cout, k[0], k[1], k[2], _mode(mfma, x, x),
                                                    *_fwd_layout(x, cout, y, ref)))


# ------------------------------------------------------------------ norm ----
def _stats_out(rows, groups, C, dev):
    """the (mean[rows,G], rstd[rows,G], scale[rows,C], shift[rows,C]) a statistics call fills"""
    shapes = ((rows, groups), (rows, groups), (rows, C), (rows, C))
    return tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes)


def norm_stats(x, groups: int, gamma=None, beta=None, eps: float = 1e-5):
    """-> (mean[N,G], rstd[N,G], scale[N,C], shift[N,C])"""
    _req_cuda(x)
    N, D, H, W, C, ld = _act5(x)
    dev = x.device
    mean, rstd, scale, shift = _stats_out(N, groups, C, dev)
    lib = _lib.load()
    V = D * H * W
    nws = lib.tem_norm_ws(N, V, C)
    ws = _workspace(nws, dev)
    _lib.check(lib.tem_norm_stats_st(_p(x), ld, N, V, C, groups, _p(gamma), _p(beta), eps, _p(mean), _p(rstd), _p(scale),
                                     _p(shift), _p(ws), nws, _st(x), _stream(x)), "tem_norm_stats_st")
    return mean, rstd, scale, shift


def norm_stats_from_partials(part, rows: int, voxels: int, C: int, groups: int, gamma=None, beta=None,
                             eps: float = 1e-5):
    """Second stage of norm_stats on partial sums written by conv_fwd(want_stats=True).  part: [N, nblk, C, 2];
    rows = N for per-sample statistics, 1 for BatchNorm (then every sample's blocks merge into one row)."""
    _req_cuda(part)
    N, nblk = part.shape[0], part.shape[1]
    if rows == 1:
        nblk, voxels = N * nblk, N * voxels
    elif rows != N:
        raise ValueError("norm_stats_from_partials: rows must be N or 1")
    dev = part.device
    mean, rstd, scale, shift = _stats_out(rows, groups, C, dev)
    lib = _lib.load()
    _lib.check(lib.tem_norm_finalize_partials(_p(part), nblk, rows, voxels, C, groups, _p(gamma), _p(beta), eps,
                                              _p(mean), _p(rstd), _p(scale), _p(shift), _stream(part)),
               "tem_norm_finalize_partials")
    return mean, rstd, scale, shift


def _launch_norm_bwd(gy, gy_ld, x, x_ld, N, V, C, groups, gamma, mean, rstd, relu_mask, gx, gx_ld, dgamma, dbeta, sums, coef, out_amax):
    """The one tem_norm_bwd_st call.  sums: None = reduce gy and x here, [N, C, 2] from a weight gradient (one row) or partial rows
    [N, nblk, C, 2] from a data gradient (Byproducts.norm_sums); coef: reduction only -> coef [N, C, 4], gx is not written."""
    lib = _lib.load()
    nws = lib.tem_norm_ws(N, V, C)
    ws = _workspace(nws, x.device)
    nrow = 0 if sums is None else (sums.shape[1] if sums.dim() == 4 else 1)
    _lib.check(lib.tem_norm_bwd_st(_p(gy), gy_ld, _p(x), x_ld, N, V, C, groups, _p(gamma), _p(mean), _p(rstd), int(relu_mask),
                                   _p(gx), gx_ld, _p(dgamma), _p(dbeta), _p(sums), nrow, _p(coef), _p(out_amax), _p(ws), nws, _st(x),
                                   _stream(x)), "tem_norm_bwd_st")


def norm_bwd_coef(gy, x, groups, gamma, mean, rstd, dgamma=None, dbeta=None, sums=None):
    """Reduction stage of norm_bwd only -> coef[N, C, 4] = (a, m1, m2r, mean) per (sample, channel)."""
    _req_cuda(gy, x)
    if isinstance(x, Planar) and sums is None:
        # no producer delivered the sums: reduce each dense half on its own (groups never straddle the halves: 32 % (C / G) == 0)
        cg = 64 // groups
        if 32 % cg:
            raise ValueError("norm_bwd_coef: a group straddles the halves of a planar tensor")
        gh = 32 // cg
        sl = lambda t, i, n: None if t is None else t[..., i * n:(i + 1) * n]  # noqa: E731
        return torch.cat([norm_bwd_coef(gy.halves[i], x.halves[i], gh, sl(gamma, i, 32), sl(mean, i, gh).contiguous(),
                                        sl(rstd, i, gh).contiguous(), sl(dgamma, i, 32), sl(dbeta, i, 32)) for i in (0, 1)], dim=1)
    N, D, H, W, C, x_ld = _act5(x)
    gy_ld = _act5(gy)[5]
    if isinstance(x, Planar):   # with the sums given the tensors are not read: any valid leading dimension
        x_ld = gy_ld = C
    _same_st(gy, x)
    coef = torch.empty((N, C, 4), dtype=torch.float32, device=x.device)
    _launch_norm_bwd(gy, gy_ld, x, x_ld, N, D * H * W, C, groups, gamma, mean, rstd, 0, None, C, dgamma, dbeta, sums, coef, None)
    return coef


def norm_bwd(gy, x, groups, gamma, mean, rstd, relu_mask: bool, gx, dgamma=None, dbeta=None, sums=None, out_amax=None):
    """sums: [N, C, 2] from conv_wgrad(sums_from=...) -- skips the reduction pass over gy and x;
    out_amax: int32[1] (cleared by the caller) that receives the bit pattern of max |gx|"""
    _req_cuda(gy, x, gx)
    N, D, H, W, C, x_ld = _act5(x)
    gy_ld = _act5(gy)[5]
    gx_ld = _act5(gx)[5]
    _same_st(gy, x, gx)
    _launch_norm_bwd(gy, gy_ld, x, x_ld, N, D * H * W, C, groups, gamma, mean, rstd, relu_mask, gx, gx_ld, dgamma, dbeta, sums, None,
                     out_amax)
    return gx


# --------------------------------------------------------- pool / upsample ----
def _rows_vec4(x, x_ld, y, y_ld) -> bool:
    """may the launch from x into y get a statistics buffer: leading dimensions % 4 == 0 and 16-byte aligned pointers"""
    return x_ld % 4 == 0 and y_ld % 4 == 0 and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0


def maxpool_fwd(x, y, f, want_stats=False):
    """want_stats: also return (partials [N, nblk, C, 2], nblk) -- the first stage of the statistics of y (what
    conv_fwd(want_stats=True) returns for a conv output; stat_part of tem_maxpool3d_fwd_st) -- or None when this channel count
    cannot."""
    _req_cuda(x, y)
    N, D, H, W, C, x_ld = _act5(x)
    y_ld = _act5(y)[5]
    lib = _lib.load()
    nblk = int(lib.tem_maxpool3d_fwd_stat_blocks(D, H, C, f[0], f[1])) if want_stats else 0
    _same_st(x, y)
    part = None
    if nblk > 0 and _rows_vec4(x, x_ld, y, y_ld):
        part = torch.empty((N, nblk, C, 2), dtype=torch.float32, device=x.device)
    _lib.check(lib.tem_maxpool3d_fwd_st(_p(x), x_ld, _p(y), y_ld, N, D, H, W, C, f[0], f[1], f[2], _p(part),
                                        nblk if part is not None else 0, _st(x), _stream(x)), "tem_maxpool3d_fwd_st")
    if want_stats:
        return None if part is None else (part, nblk)
    return y


def maxpool_bwd(gy, x, gx, f, gskip=None, relu_mask=False, gskip_coef=None, gy_coef=None, out_amax=None):
    """gskip_coef: [N, C, 4] view (row stride = multiple of 4 floats) of norm_bwd_coef() -- gskip is then the raw data
    gradient behind that norm and the norm backward is applied on the fly (gcoef of tem_maxpool3d_bwd_st).
    gy_coef: dense [N, C, 4] coefficients of the norm whose input is the pooled tensor (gy raw as well)."""
    _req_cuda(gy, x, gx)
    N, D, H, W, C, x_ld = _act5(x)
    gy_ld = _act5(gy)[5]
    gx_ld = _act5(gx)[5]
    gs_ld = _act5(gskip)[5] if gskip is not None else 0
    lib = _lib.load()
    if gy_coef is not None and not gy_coef.is_contiguous():
        raise ValueError("maxpool_bwd: gy_coef must be contiguous")
    _same_st(gy, x, gx, gskip)
    _lib.check(lib.tem_maxpool3d_bwd_st(_p(gy), gy_ld, _p(x), x_ld, _p(gskip), gs_ld, int(relu_mask), _p(gx), gx_ld,
                                        N, D, H, W, C, f[0], f[1], f[2], _p(gskip_coef),
                                        gskip_coef.stride(0) if gskip_coef is not None else 0, _p(gy_coef), _p(out_amax), _st(x),
                                        _stream(x)), "tem_maxpool3d_bwd_st")
    return gx


def upsample_fwd(x, y, f, stats: bool = False):
    """y = interpolate(x, scale_factor=f, trilinear).  stats=True: also return the first stage of y's statistics,
    part [N, D*H, C, 2] (part of tem_upsample_fwd_st), or None when the factor-2 kernel does not take the shape -- then
    `upsample_stats` derives them from x."""
    _req_cuda(x, y)
    N, D, H, W, C, x_ld = _act5(x)
    y_ld = _act5(y)[5]
    lib = _lib.load()
    _same_st(x, y)
    part = None
    if stats and lib.tem_upsample_fwd_stats_ok(C, f[0], f[1], f[2]) and _rows_vec4(x, x_ld, y, y_ld):
        part = torch.empty((N, D * H, C, 2), dtype=torch.float32, device=x.device)
    _lib.check(lib.tem_upsample_fwd_st(_p(x), x_ld, _p(y), y_ld, N, D, H, W, C, f[0], f[1], f[2], _p(part), _st(x),
                                       _stream(x)), "tem_upsample_fwd_st")
    return part if stats else y


def upsample_stats_ok(u) -> bool:
    C = u.shape[4]
    cq = C // 4
    return C % 4 == 0 and 0 < cq <= 64 and (cq & (cq - 1)) == 0 and _act5(u)[5] % 4 == 0 and u.data_ptr() % 16 == 0


def upsample_stats(u, f):
    """First stage of the statistics of upsample(u, f), from u alone -> part [N, D*H, C, 2] (tem_upsample_stats_st)."""
    _req_cuda(u)
    N, D, H, W, C, u_ld = _act5(u)
    part = torch.empty((N, D * H, C, 2), dtype=torch.float32, device=u.device)
    _lib.check(_lib.load().tem_upsample_stats_st(_p(u), u_ld, N, D, H, W, C, f[0], f[1], f[2], _p(part), _st(u), _stream(u)),
               "tem_upsample_stats_st")
    return part


def norm_stats_from_partials2(part_a, part_b, rows: int, voxels: int, groups: int, gamma=None, beta=None,
                              eps: float = 1e-5):
    """norm_stats of a channel-concatenated tensor: channels [0, CA) summarised by part_a [N, nblkA, CA, 2], the rest by
    part_b [N, nblkB, CB, 2] (tem_norm_finalize_partials2).  rows = N, or 1 for BatchNorm."""
    _req_cuda(part_a, part_b)
    N, nba, ca = part_a.shape[0], part_a.shape[1], part_a.shape[2]
    nbb, cb = part_b.shape[1], part_b.shape[2]
    C = ca + cb
    if rows == 1:
        nba, nbb, voxels = N * nba, N * nbb, N * voxels
    elif rows != N:
        raise ValueError("norm_stats_from_partials2: rows must be N or 1")
    dev = part_a.device
    mean, rstd, scale, shift = _stats_out(rows, groups, C, dev)
    lib = _lib.load()
    _lib.check(lib.tem_norm_finalize_partials2(_p(part_a), nba, ca, _p(part_b), nbb, rows, voxels, C, groups, _p(gamma),
                                               _p(beta), eps, _p(mean), _p(rstd), _p(scale), _p(shift), _stream(part_a)),
               "tem_norm_finalize_partials2")
    return mean, rstd, scale, shift


def upsample_bwd(gy, gx, f, norm=None):
    """gx has the low-resolution shape; gy = gx's shape scaled by f.
    norm = (u, coef[N, C, 4] view): gy is the raw data gradient behind a norm whose input was upsample(u)."""
    _req_cuda(gy, gx)
    N, D, H, W, C, gx_ld = _act5(gx)
    gy_ld = _act5(gy)[5]
    u, coef = norm if norm is not None else (None, None)
    _same_st(gy, gx, u)
    _lib.check(_lib.load().tem_upsample_bwd_st(_p(gy), gy_ld, _p(gx), gx_ld, N, D, H, W, C, f[0], f[1], f[2], _p(u),
                                               _act5(u)[5] if u is not None else 0, _p(coef), coef.stride(0) if coef is not None else 0,
                                               _st(gy), _stream(gx)), "tem_upsample_bwd_st")
    return gx


def act_bwd(gy, y, act: str):
    _req_cuda(gy, y)
    gy = gy.contiguous()
    y = y.contiguous()
    gx = torch.empty_like(gy)
    lib = _lib.load()
    _lib.check(lib.tem_act_bwd(_p(gy), _p(y), _p(gx), gy.numel(), ACT[act], _stream(gy)), "tem_act_bwd")
    return gx


# ------------------------------------------------------------------ dice ----
def _ncv_strides(t: torch.Tensor):
    """(sn, sc, sv, N, C, V) for a logical [N, C, *spatial] tensor whose spatial dims are
    jointly contiguous up to a common voxel stride; returns None if not expressible."""
    N, C = t.shape[:2]
    sp = tuple(t.shape[2:])
    V = 1
    for s in sp:
        V *= s
    st = t.stride()
    sv = st[-1] if len(sp) > 0 else 1
    # check spatial dims collapse to a single stride sv
    expect = sv
    for d in range(len(sp) - 1, -1, -1):
        if sp[d] != 1 and st[2 + d] != expect:
            return None
        expect *= sp[d]
    return st[0], st[1], sv, N, C, V


def dice_sums(p, t, mask=None) -> torch.Tensor:
    """-> double[C, 3] = (sum p*t, sum p*p, sum t*t) with optional multiplicative mask."""
    _req_cuda(p, t)
    ps = _ncv_strides(p)
    if ps is None:
        p = p.contiguous()
        ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    if ts is None:
        t = t.contiguous()
        ts = _ncv_strides(t)
    if mask is not None:
        ms = _ncv_strides(mask)
        if ms is None or ms[:3] != ts[:3]:
            raise ValueError("dice: mask must share the target's strides")
    N, C, V = ps[3:]
    sums = torch.empty((C, 3), dtype=torch.float64, device=p.device)
    lib = _lib.load()
    nws = lib.tem_dice_ws(N, V, C)
    ws = _workspace(nws, p.device)
    _lib.check(lib.tem_dice_sums(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], _p(mask), N, C, V,
                                 _p(sums), _p(ws), nws, _stream(p)), "tem_dice_sums")
    return sums, p, t


REDUCE = {None: 0, "sum": 1, "mean": 2, "max": 3, "min": 4}
DICE_LOGITS, DICE_BCE = 1, 2


def dice_sums2(p, t, flags: int):
    """dice_sums for the logits / BCE members of the family (tem_dice_sums2): double[C, 3] or, with DICE_BCE, [C, 4]
    (4th column: summed binary cross entropy of the channel)."""
    _req_cuda(p, t)
    ps = _ncv_strides(p)
    if ps is None:
        p = p.contiguous()
        ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    if ts is None:
        t = t.contiguous()
        ts = _ncv_strides(t)
    N, C, V = ps[3:]
    ncol = 4 if flags & DICE_BCE else 3
    sums = torch.empty((C, ncol), dtype=torch.float64, device=p.device)
    lib = _lib.load()
    nws = lib.tem_dice_ws(N, V, C)
    ws = _workspace(nws, p.device)
    _lib.check(lib.tem_dice_sums2(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], N, C, V, _p(sums), _p(ws), nws,
                                  int(flags), _stream(p)), "tem_dice_sums2")
    return sums, p, t


def dice_finalize2(sums, eps, channelwise, invert, reduce):
    C, ncol = sums.shape
    dev = sums.device
    n_out = C if (channelwise and reduce is None) else 1
    out = torch.empty((n_out,), dtype=torch.float32, device=dev)
    ca = torch.empty((C,), dtype=torch.float32, device=dev)
    cb = torch.empty((C,), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tem_dice_finalize2(_p(sums), ncol, C, float(eps), int(channelwise), int(invert), REDUCE[reduce],
                                              _p(out), _p(ca), _p(cb), _stream(sums)), "tem_dice_finalize2")
    return out, ca, cb


def dice_grad2(p, t, ca, cb, gout, gout_per_channel, channels_last: bool, flags: int, w_dice: float, w_bce: float):
    ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    N, C, V = ps[3:]
    if channels_last:
        gp_phys = torch.empty((N,) + tuple(p.shape[2:]) + (C,), dtype=torch.float32, device=p.device)
        gp = gp_phys.permute(0, gp_phys.dim() - 1, *range(1, gp_phys.dim() - 1))
        gs = (V * C, 1, C)
    else:
        gp = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        gs = (C * V, V, 1)
    _lib.check(_lib.load().tem_dice_grad2(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], _p(ca), _p(cb), _p(gout),
                                          int(gout_per_channel), _p(gp), gs[0], gs[1], gs[2], N, C, V, int(flags),
                                          float(w_dice), float(w_bce), _stream(p)), "tem_dice_grad2")
    return gp


def dice_finalize(sums, eps, channelwise, invert, reduce):
    C = sums.shape[0]
    dev = sums.device
    n_out = C if (channelwise and reduce is None) else 1
    out = torch.empty((n_out,), dtype=torch.float32, device=dev)
    ca = torch.empty((C,), dtype=torch.float32, device=dev)
    cb = torch.empty((C,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.tem_dice_finalize(_p(sums), C, float(eps), int(channelwise), int(invert), REDUCE[reduce], _p(out),
                                     _p(ca), _p(cb), _stream(sums)), "tem_dice_finalize")
    return out, ca, cb


def dice_grad(p, t, mask, ca, cb, gout, gout_per_channel, channels_last: bool):
    """d out / d p, laid out like p (channels_last_3d memory format when p has it)."""
    ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    N, C, V = ps[3:]
    if channels_last:
        # physical [N, V, C]
        gp_phys = torch.empty((N,) + tuple(p.shape[2:]) + (C,), dtype=torch.float32, device=p.device)
        gp = gp_phys.permute(0, gp_phys.dim() - 1, *range(1, gp_phys.dim() - 1))
        gs = (V * C, 1, C)
    else:
        gp = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        gs = (C * V, V, 1)
    lib = _lib.load()
    _lib.check(lib.tem_dice_grad(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], _p(mask), _p(ca), _p(cb),
                                 _p(gout), int(gout_per_channel), _p(gp), gs[0], gs[1], gs[2], N, C, V, _stream(p)),
               "tem_dice_grad")
    return gp


def dice_sums_pair(p, t, mask):
    """-> (double[2, C, 3], p, t): `dice_sums(p, t, mask)[0]` and `dice_sums(p, t)[0]` from ONE pass over prediction, target
    and mask (tem_dice_sums_pair) -- bit for bit what the two calls give.  For passes that need no gradient."""
    _req_cuda(p, t, mask)
    ps = _ncv_strides(p)
    if ps is None:
        p = p.contiguous()
        ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    if ts is None:
        t = t.contiguous()
        ts = _ncv_strides(t)
    ms = _ncv_strides(mask)
    if ms is None or ms[:3] != ts[:3]:
        raise ValueError("dice: mask must share the target's strides")
    N, C, V = ps[3:]
    sums = torch.empty((2, C, 3), dtype=torch.float64, device=p.device)
    lib = _lib.load()
    nws = 2 * lib.tem_dice_ws(N, V, C)
    ws = _workspace(nws, p.device)
    _lib.check(lib.tem_dice_sums_pair(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], _p(mask), N, C, V,
                                      _p(sums), _p(ws), nws, _stream(p)), "tem_dice_sums_pair")
    return sums, p, t


# ---------------------------------------------------------- self-training ----
PL_MASK_NONE, PL_MASK_BOTH, PL_MASK_ONE = 0, 1, 2   # mask_mode of tem_pseudo_label_st (include/tem_hip.h)


def _is_dense(t: torch.Tensor) -> bool:
    """the elements of t fill one block of storage without gaps or overlap, in whatever order of the axes"""
    expect = 1
    for stride, size in sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def round_to(value: float, dtype: torch.dtype) -> float:
    """`value` (a Python float: a double) rounded to `dtype` the way a torch compare rounds its scalar operand"""
    return float(torch.tensor(float(value), dtype=torch.float64).to(dtype).item())


def pseudo_label(x: torch.Tensor, activation: Optional[str] = None, confidence_threshold: Optional[float] = None,
                 threshold_from_both_sides: bool = True, mask_sample: Optional[int] = None, out=None):
    """Pseudo labels and confidence mask from a teacher prediction x [N, C, *spatial] (float32 / float16 / bfloat16), one
    streaming launch (tem_pseudo_label_st; reference self_training/pseudo_labeling.py:59-72 after the forward pass).
    -> (labels, mask): labels = x itself (activation None) or sigmoid(x) in x's dtype; mask = None (no threshold),
    float32 0 / 1 for both sides, bool for one side.  Both come out in x's memory layout, so the masked Dice kernels take them
    as they are.  `mask_sample=k`: every sample gets sample k's mask (the reference's `mask_channel` slices the batch axis).
    `out=(labels, mask)` is a TEST HOOK (no library caller uses it): write into these tensors (x's shape and strides; an entry
    that is not produced is None), so a test can lay the outputs out between guard zones and poison them first."""
    _req_cuda(x)
    if x.dtype not in _ST:
        raise ValueError(f"pseudo_label: expected float32, float16 or bfloat16, got {x.dtype}")
    if activation not in (None, "sigmoid"):
        raise ValueError(f"pseudo_label: Invalid activation: {activation}")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"pseudo_label: expected a non-empty [N, C, ...] tensor, got shape {tuple(x.shape)}")
    if confidence_threshold is None:
        mask_sample = None
        if activation is None:
            return x, None
    N = x.shape[0]
    if mask_sample is not None and not 0 <= mask_sample < N:
        # the reference slices past the end of the batch axis and fails in expand()
        raise ValueError(f"pseudo_label: mask_channel {mask_sample} is out of range for a batch of {N}")
    if not _is_dense(x) or (mask_sample is not None and N > 1 and x.stride(0) != x.numel() // N):
        x = x.contiguous()
    mdtype = torch.float32 if threshold_from_both_sides else torch.bool
    if out is not None:
        for t, dtype, needed in ((out[0], x.dtype, activation is not None), (out[1], mdtype, confidence_threshold is not None)):
            if (t is not None) != needed or (needed and (t.dtype != dtype or t.shape != x.shape or t.stride() != x.stride()
                                                         or t.device != x.device)):
                raise ValueError("pseudo_label: `out` must hold exactly the tensors this call writes, laid out like x")
    labels = (out[0] if out is not None else torch.empty_like(x)) if activation is not None else None
    mode, mask, t_hi, t_lo = PL_MASK_NONE, None, 0.0, 0.0
    if confidence_threshold is not None:
        mode = PL_MASK_BOTH if threshold_from_both_sides else PL_MASK_ONE
        mask = out[1] if out is not None else torch.empty_like(x, dtype=mdtype)
        t_hi, t_lo = round_to(confidence_threshold, x.dtype), round_to(1.0 - confidence_threshold, x.dtype)
    _lib.check(_lib.load().tem_pseudo_label_st(_p(x), _p(labels), _p(mask), N, x.numel() // N, ACT[activation], mode,
                                               -1 if mask_sample is None else int(mask_sample), t_hi, t_lo, _st(x), _stream(x)),
               "tem_pseudo_label_st")
    return (x if labels is None else labels), mask


def _da_check(name: str, labels, threshold):
    """argument checks shared by label_count_partials / distribution_align: all of them before the library is touched"""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the GPU (there is no CPU path)")
    if labels.dtype not in _ST:
        raise ValueError(f"{name}: expected float32, float16 or bfloat16, got {labels.dtype}")
    if labels.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty tensor, got shape {tuple(labels.shape)}")
    if not _is_dense(labels):
        raise ValueError(f"{name}: the labels must be dense (any permutation of a contiguous tensor), got strides {labels.stride()}")
    if not math.isfinite(float(threshold)):
        raise ValueError(f"{name}: the label threshold must be finite, got {threshold}")


def source_shares(source_distribution) -> Tuple[float, float]:
    """the two class shares of a `source_distribution` (a sequence or a tensor) as Python floats; ValueError unless there are
    exactly two finite positive ones (the reference indexes [0] and [1] of the ratio).  Touches no device library."""
    src = source_distribution
    if isinstance(src, torch.Tensor):
        src = src.detach().cpu().tolist()
    try:
        src = [float(v) for v in src]
    except TypeError:
        raise ValueError(f"distribution_align: source_distribution must hold two numbers, got {source_distribution!r}") from None
    if len(src) != 2 or not all(math.isfinite(v) and v > 0 for v in src):
        raise ValueError(f"distribution_align: source_distribution must hold exactly two finite positive entries, got {src}")
    return src[0], src[1]


def _label_count(lib, labels, threshold):
    """`threshold`: already rounded to the labels' dtype"""
    n = labels.numel()
    parts = lib.tem_label_count_parts(n, _st(labels))
    if parts <= 0:
        raise ValueError(f"label_count: {n} elements are out of range")
    partials = torch.empty((parts,), dtype=torch.int64, device=labels.device)
    _lib.check(lib.tem_label_count_st(_p(labels), n, threshold, _p(partials), parts, _st(labels), _stream(labels)),
               "tem_label_count_st")
    return partials


def label_count_partials(labels: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """int64 [tem_label_count_parts(n)] on the device: per-block counts of `labels >= threshold` (tem_label_count_st; the
    compare runs in the labels' dtype against the rounded threshold, NaN counts as below).  Their sum is the size of the
    upper class; `distribution_align` hands them to its second launch without reading them."""
    _da_check("label_count_partials", labels, threshold)
    return _label_count(_lib.load(), labels, round_to(threshold, labels.dtype))


def distribution_align(labels: torch.Tensor, source_distribution, label_threshold: float = 0.5, out=None) -> torch.Tensor:
    """FixMatch's distribution alignment (reference self_training/fix_match.py:164-181) in two launches and without a host
    round trip: clip(labels * source_k / (count_k / n), 0, 1) with k the side of `label_threshold` the label is on.  -> a new
    tensor in the dtype and memory layout of `labels` (float32 / float16 / bfloat16, dense); `labels` is not written.
    `source_distribution`: two finite positive numbers (a sequence or a tensor; a device tensor is read once -- pass floats
    inside a captured region).  `out=` is a TEST HOOK (no library caller uses it): write into this tensor (the shape, strides,
    dtype and device of `labels`, other storage), so a test can lay the output out between guard zones."""
    _da_check("distribution_align", labels, label_threshold)
    s0, s1 = source_shares(source_distribution)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != labels.dtype or out.shape != labels.shape
                or out.stride() != labels.stride() or out.device != labels.device):
            raise ValueError("distribution_align: `out` must be laid out like the labels")
        nbytes = labels.numel() * labels.element_size()
        if out.data_ptr() < labels.data_ptr() + nbytes and labels.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("distribution_align: `out` must not overlap the labels")
    lib = _lib.load()
    threshold = round_to(label_threshold, labels.dtype)
    partials = _label_count(lib, labels, threshold)
    res = torch.empty_like(labels) if out is None else out
    _lib.check(lib.tem_distribution_align_st(_p(labels), _p(res), labels.numel(), threshold, s0, s1, _p(partials),
                                             partials.numel(), _st(labels), _stream(labels)), "tem_distribution_align_st")
    return res


# ---- invertible augmentations: per-sample dihedral transform of the last two axes (csrc/invaug.hip) ----
# code: bit 0 transposes, bit 1 reverses the source row, bit 2 reverses the source column (include/tem_hip.h)
DH_PATH_VEC, DH_PATH_SCALAR, DH_PATH_TILE, DH_PATH_TILE_PACKED = 0, 1, 2, 3
_DH_ROT = (0, 5, 6, 3)   # torch.rot90(x, k, (-2, -1)) for k % 4 = 0, 1, 2, 3
_DH_INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)


def dihedral_compose(first: int, then: int) -> int:
    """the code of applying `first` and then `then` (host table arithmetic; no device is touched)"""
    t_a, fr_a, fc_a = first & 1, (first >> 1) & 1, (first >> 2) & 1
    t_b, fr_b, fc_b = then & 1, (then >> 1) & 1, (then >> 2) & 1
    fr, fc = (fr_a ^ fc_b, fc_a ^ fr_b) if t_a else (fr_a ^ fr_b, fc_a ^ fc_b)
    return (t_a ^ t_b) | (fr << 1) | (fc << 2)


def _host_ints(values, what: str):
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            raise ValueError(f"{what}: expected host values (a sequence or a CPU tensor), got a device tensor")
        values = values.reshape(-1).tolist()
    elif isinstance(values, (bool, int)):
        values = [values]
    out = []
    for v in values:
        if int(v) != v:
            raise ValueError(f"{what}: expected integers, got {v!r}")
        out.append(int(v))
    return out


def dihedral_codes(h, v, k):
    """One code per sample for `x.flip(-1)` where h, then `.flip(-2)` where v, then `torch.rot90(., k, (-2, -1))`: h, v, k are
    host values, one per sample (numbers, sequences or CPU tensors of equal length) -> list of ints in 0..7."""
    h, v, k = _host_ints(h, "dihedral_codes: h"), _host_ints(v, "dihedral_codes: v"), _host_ints(k, "dihedral_codes: k")
    if not len(h) == len(v) == len(k):
        raise ValueError(f"dihedral_codes: h, v and k must have one entry per sample, got {len(h)}, {len(v)}, {len(k)}")
    return [dihedral_compose(dihedral_compose(4 if a else 0, 2 if b else 0), _DH_ROT[c % 4]) for a, b, c in zip(h, v, k)]


def _dh_codes(codes, what: str):
    codes = _host_ints(codes, what)
    bad = [c for c in codes if not 0 <= c <= 7]
    if bad:
        raise ValueError(f"{what}: codes must be within 0..7, got {bad[0]}")
    return codes


def dihedral_inverse(codes):
    """the codes that undo `codes`: 3 <-> 5, every other element of D4 is its own inverse"""
    return [_DH_INVERSE[c] for c in _dh_codes(codes, "dihedral_inverse")]


_DH_ELEM = {torch.float32, torch.float16, torch.bfloat16, torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32}


def _dh_plan(x: torch.Tensor, codes, inverse: bool):
    """every check of `dihedral` that needs no device -> (codes to launch, output shape)"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError("dihedral: expected a 4d [N,C,H,W] or 5d [N,C,D,H,W] tensor, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dtype not in _DH_ELEM:
        raise ValueError(f"dihedral: elements of 1, 2 or 4 bytes are moved (float32, float16, bfloat16, bool, ...), got {x.dtype}")
    if x.numel() == 0:
        raise ValueError(f"dihedral: expected a non-empty tensor, got shape {tuple(x.shape)}")
    codes = _dh_codes(codes, "dihedral")
    N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if len(codes) != N:
        raise ValueError(f"dihedral: expected one code per sample ({N}), got {len(codes)}")
    if inverse:
        codes = [_DH_INVERSE[c] for c in codes]
    odd = sum(c & 1 for c in codes)
    if H != W and 0 < odd < N:
        raise ValueError(f"dihedral: codes {codes} mix transposing and non-transposing elements, which needs H == W (got {H} x {W}: "
                         "the samples of one output tensor must share a shape)")
    shape = tuple(x.shape[:-2]) + ((W, H) if odd else (H, W))
    return codes, shape


def _dh_launch(x: torch.Tensor, codes, shape, out=None) -> torch.Tensor:
    _req_cuda(x)
    x = x.contiguous()
    dev = torch.tensor(codes, dtype=torch.int32).pin_memory().to(x.device, non_blocking=True)
    y = torch.empty(shape, dtype=x.dtype, device=x.device) if out is None else out
    N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    _lib.check(_lib.load().tem_dihedral2d(_p(x), _p(y), _p(dev), N, x.numel() // (N * H * W), H, W, x.element_size(), _stream(x)),
               "tem_dihedral2d")
    return y


class _Dihedral(torch.autograd.Function):
    """y = P x with P a permutation: the gradient is the inverse permutation of the incoming one, the same launch"""

    @staticmethod
    def forward(ctx, x, codes, shape):
        ctx.codes, ctx.shape = codes, tuple(x.shape)
        return _dh_launch(x, codes, shape)

    @staticmethod
    def backward(ctx, grad):
        return _dh_launch(grad, [_DH_INVERSE[c] for c in ctx.codes], ctx.shape), None, None


def dihedral(x: torch.Tensor, codes, inverse: bool = False, out=None) -> torch.Tensor:
    """Per-sample element of the dihedral group D4 on the last two axes of x [N,C,H,W] / [N,C,D,H,W], one launch at copy
    speed, exact to the bit (tem_dihedral2d).  `codes`: HOST values, one per sample (a sequence or a CPU tensor; see
    `dihedral_codes`), uploaded asynchronously; `inverse=True` applies the inverse elements instead.  -> a new tensor,
    [..., W, H] when the codes transpose.  Differentiable: the backward pass is the same launch with the inverse codes.
    ValueError for a code outside 0..7, a wrong number of codes, or transposing and non-transposing codes in one call
    when H != W.  `out=` is a TEST HOOK (no library caller uses it): write into this contiguous tensor of the output's shape
    and dtype, so a test can lay the output out between guard zones."""
    codes, shape = _dh_plan(x, codes, inverse)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != x.dtype or tuple(out.shape) != shape or not out.is_contiguous()
                or out.device != x.device):
            raise ValueError("dihedral: `out` must be a contiguous tensor of the output's shape, dtype and device")
        return _dh_launch(x, codes, shape, out)
    if torch.is_grad_enabled() and x.requires_grad:
        return _Dihedral.apply(x, codes, shape)
    return _dh_launch(x, codes, shape)


def dihedral_path(x: torch.Tensor, code: int, out=None) -> int:
    """the path a sample with `code` takes when `dihedral(x, ..., out=out)` runs (tem_dihedral2d_path; launches nothing):
    DH_PATH_VEC, DH_PATH_SCALAR, DH_PATH_TILE or DH_PATH_TILE_PACKED"""
    N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    y = torch.empty_like(x) if out is None else out
    rc = _lib.load().tem_dihedral2d_path(_p(x), _p(y), int(code), N, x.numel() // (N * H * W), H, W, x.element_size())
    if rc < 0:
        _lib.check(-1, "tem_dihedral2d_path")
    return rc


# ---------------------------------------------------------------- clDice ----
# modes of tem_cldice_step (include/tem_hip.h)
CLD_ROUND0, CLD_ROUND, CLD_ERODE, CLD_OPEN, CLD_DILATE, CLD_BWD_POINT0, CLD_BWD_POINT = range(7)


def _cld_geo(x: torch.Tensor):
    """x [N, C, (D,) H, W] -> (x, (sn, sc, sv), (N, C, D, H, W, ndim)); read in place when its spatial dims collapse to
    one voxel stride (NCDHW, NDHWC, channel-sliced views), copied otherwise"""
    if x.dim() not in (4, 5):
        raise ValueError(f"cldice: expected a 4d [N,C,H,W] or 5d [N,C,D,H,W] tensor, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"cldice: expected float32, got {x.dtype}")
    _req_cuda(x)
    st = _ncv_strides(x)
    if st is None:
        x = x.contiguous()
        st = _ncv_strides(x)
    N, C = x.shape[:2]
    D = x.shape[2] if x.dim() == 5 else 1
    H, W = x.shape[-2:]
    if min(N, C, D, H, W) < 1:
        raise ValueError(f"cldice: empty tensor {tuple(x.shape)}")
    return x, st[:3], (N, C, D, H, W, x.dim() - 2)


def _cld_scratch(count: int, like_shape, device, numel: int):
    """`count` planar fp32 tensors carved from the stream's static workspace"""
    ws = _workspace(count * numel * 4, device)
    return [ws[i * numel * 4:(i + 1) * numel * 4].view(torch.float32).view(like_shape) for i in range(count)]


def _cld_step(lib, e, st, geo, a_in, b_in, e_next, out, out2, mode):
    _lib.check(lib.tem_cldice_step(_p(e), st[0], st[1], st[2], _p(a_in), _p(b_in), _p(e_next), _p(out), _p(out2), *geo,
                                   mode, _stream(e)), "tem_cldice_step")


def _planar_st(geo):
    N, C, D, H, W, _ = geo
    V = D * H * W
    return (C * V, V, 1)


def cldice_morph(x: torch.Tensor, mode: int):
    """soft_erode / soft_open / soft_dilate of x (one fused launch); -> (out, e1) with e1 = erode(x), kept for the
    backward of the opening (None otherwise)"""
    x, st, geo = _cld_geo(x)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    e1 = None
    if mode == CLD_ERODE:
        _cld_step(lib, x, st, geo, None, None, out, None, None, CLD_ERODE)
    elif mode == CLD_OPEN:
        e1 = torch.empty_like(out)
        _cld_step(lib, x, st, geo, None, None, e1, None, None, CLD_ERODE)
        _cld_step(lib, x, st, geo, None, None, None, out, None, CLD_OPEN)
    elif mode == CLD_DILATE:
        _cld_step(lib, x, st, geo, None, None, None, out, None, CLD_DILATE)
    else:
        raise ValueError(f"cldice_morph: mode {mode}")
    return out, e1


def _cld_out(x, channels_last: bool):
    """an empty gradient laid out like the prediction: channels-last memory when it is, planar otherwise"""
    N, C = x.shape[:2]
    V = x[0, 0].numel()
    if channels_last:
        phys = torch.empty((N,) + tuple(x.shape[2:]) + (C,), dtype=torch.float32, device=x.device)
        return phys.permute(0, phys.dim() - 1, *range(1, phys.dim() - 1)), (V * C, 1, C)
    return torch.empty(x.shape, dtype=torch.float32, device=x.device), (C * V, V, 1)


def cldice_morph_bwd(x: torch.Tensor, e1, g: torch.Tensor, mode: int, channels_last: bool = False) -> torch.Tensor:
    """gradient of cldice_morph's output w.r.t. x for the upstream g (gather form, PyTorch's tie rules)"""
    x, st, geo = _cld_geo(x)
    g = g.to(torch.float32).contiguous()
    lib = _lib.load()
    out, os_ = _cld_out(x, channels_last)
    if mode == CLD_DILATE:
        if os_[2] != 1:   # the dilation backward writes planar
            out, os_ = _cld_out(x, False)
        _lib.check(lib.tem_cldice_dilate_bwd(_p(x), st[0], st[1], st[2], _p(g), None, _p(out), *geo, _stream(x)),
                   "tem_cldice_dilate_bwd")
        return out
    if mode == CLD_OPEN:
        g1 = torch.empty_like(g)
        pst = _planar_st(geo)
        _lib.check(lib.tem_cldice_dilate_bwd(_p(e1), pst[0], pst[1], pst[2], _p(g), None, _p(g1), *geo, _stream(x)),
                   "tem_cldice_dilate_bwd")
        g = g1
    _lib.check(lib.tem_cldice_erode_bwd(_p(x), st[0], st[1], st[2], _p(g), None, None, None, None, _p(out), os_[0], os_[1],
                                        os_[2], *geo, _stream(x)), "tem_cldice_erode_bwd")
    return out


def cldice_skel_fwd(x: torch.Tensor, num_iter: int, save: bool):
    """soft skeleton of x: num_iter + 1 fused rounds (tem_cldice_step).  -> (skel planar [N, C, ...], saved) with
    saved = (x as read, estack [K+1, ...] = e_1..e_{K+1}, sstack [K, ...] = skel_0..skel_{K-1}) from torch's allocator
    when `save`, else None (the erosions then ping-pong in the stream's workspace)"""
    K = int(num_iter)
    if K < 0:
        raise ValueError("cldice: num_iter must not be negative")
    x, st, geo = _cld_geo(x)
    lib = _lib.load()
    pst = _planar_st(geo)
    skel = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if save:
        estack = torch.empty((K + 1,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        sstack = torch.empty((K,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        enext = [estack[j] for j in range(K + 1)]
        souts = [sstack[j] for j in range(K)] + [skel]
    else:
        pp = _cld_scratch(2, x.shape, x.device, x.numel())
        enext = [pp[j % 2] for j in range(K)] + [None]   # the last erosion is not kept
        souts = [skel] * (K + 1)                          # updated in place
    e, est = x, st
    for j in range(K + 1):
        _cld_step(lib, e, est, geo, souts[j - 1] if j else None, None, enext[j], souts[j], None, CLD_ROUND if j else CLD_ROUND0)
        e, est = enext[j], pst
    return skel, ((x, estack, sstack) if save else None)


def cldice_skel_bwd(saved, gs: torch.Tensor, channels_last: bool, direct=None, coef=None, gout=None,
                    gs_is_scratch: bool = False) -> torch.Tensor:
    """d / d x of the soft skeleton for the upstream gs (planar), rounds in reverse: point, dilate, erode (gather
    form).  direct / coef / gout: the clDice term coef[2] * gout * direct added in the last launch.  The gradient is
    laid out like the prediction (channels-last memory when `channels_last`)."""
    x, estack, sstack = saved
    x, st, geo = _cld_geo(x)
    lib = _lib.load()
    K = sstack.shape[0]
    pst = _planar_st(geo)
    n = x.numel()
    bufs = _cld_scratch(4, x.shape, x.device, n)
    h, b0, b1 = bufs[0], bufs[1], bufs[2]
    if gs_is_scratch:
        gsb = gs                      # already ours to overwrite
    else:
        gsb = bufs[3]
        gsb.copy_(gs.to(torch.float32))
    out, os_ = _cld_out(x, channels_last)
    stream = _stream(x)
    for j in range(K, -1, -1):
        e, est = (estack[j - 1], pst) if j else (x, st)
        if j:
            _cld_step(lib, e, est, geo, sstack[j - 1], gsb, None, h, gsb, CLD_BWD_POINT)
        else:
            _cld_step(lib, e, est, geo, None, gsb, None, h, None, CLD_BWD_POINT0)
        _lib.check(lib.tem_cldice_dilate_bwd(_p(estack[j]), pst[0], pst[1], pst[2], _p(h), _p(b0) if j < K else None,
                                             _p(b1), *geo, stream), "tem_cldice_dilate_bwd")
        if j:
            _lib.check(lib.tem_cldice_erode_bwd(_p(e), est[0], est[1], est[2], _p(b1), _p(h), None, None, None, _p(b0),
                                                pst[0], pst[1], pst[2], *geo, stream), "tem_cldice_erode_bwd")
        else:
            _lib.check(lib.tem_cldice_erode_bwd(_p(e), est[0], est[1], est[2], _p(b1), _p(h), _p(direct), _p(coef), _p(gout),
                                                _p(out), os_[0], os_[1], os_[2], *geo, stream), "tem_cldice_erode_bwd")
    return out


def cldice_score_fwd(x, t, skel_x, skel_t, eps: float, invert: bool):
    """-> (out float[1], coef float[4], sums double[4]) of the clDice score (tem_cldice_sums + tem_cldice_finalize)"""
    x, xs, geo = _cld_geo(x)
    t, ts, _ = _cld_geo(t)
    N, C, D, H, W, _ = geo
    V = D * H * W
    lib = _lib.load()
    nws = lib.tem_cldice_ws(N, C, V, 0, 0)
    ws = _workspace(nws, x.device)
    sums = torch.empty((4,), dtype=torch.float64, device=x.device)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    coef = torch.empty((4,), dtype=torch.float32, device=x.device)
    _lib.check(lib.tem_cldice_sums(_p(skel_x), _p(skel_t), _p(x), xs[0], xs[1], xs[2], _p(t), ts[0], ts[1], ts[2], N, C, V,
                                   _p(ws), nws, _stream(x)), "tem_cldice_sums")
    _lib.check(lib.tem_cldice_finalize(_p(ws), float(eps), int(invert), _p(sums), _p(out), _p(coef), _stream(x)),
               "tem_cldice_finalize")
    return out, coef, sums


def cldice_score_bwd(saved, t, skel_t, coef, gout, channels_last: bool) -> torch.Tensor:
    """d score / d x: the seed gout * (coef[0] t + coef[1]) (tem_cldice_grad) through the skeleton backward, plus the
    direct part coef[2] * gout * skel_t"""
    x = saved[0]
    t, ts, geo = _cld_geo(t)
    N, C, D, H, W, _ = geo
    V = D * H * W
    gs = _cld_scratch(4, x.shape, x.device, x.numel())[3]
    _lib.check(_lib.load().tem_cldice_grad(_p(t), ts[0], ts[1], ts[2], _p(coef), _p(gout), _p(gs), N, C, V, _stream(t)),
               "tem_cldice_grad")
    return cldice_skel_bwd(saved, gs, channels_last, direct=skel_t, coef=coef, gout=gout, gs_is_scratch=True)


# ------------------------------------------------------------- optimizer ----
def bump_versions(tensors):
    """The kernels below write parameters through raw pointers, which autograd's version counters do not see;
    consumers that cache derived data per `tensor._version` (the engine's packed weight fragments) must be
    told.  ONE host call for all of them, no device work.  (`_increment_version` takes an iterable of tensors: handing
    it a single tensor makes it iterate over the tensor's ROWS -- 512 view objects for a [512, 512, 3, 3, 3] weight;
    46 such calls were 6.5 ms of host time per optimizer step.)"""
    tensors = list(tensors)
    inc = getattr(torch._C, "_increment_version", None)
    if inc is not None:
        inc(tensors)
        return
    for t in tensors:  # pragma: no cover -- very old torch: a no-op in-place op bumps the counter
        t.add_(0)


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _req_cuda(param, grad, exp_avg, exp_avg_sq)
    lib = _lib.load()
    _lib.check(lib.tem_adamw_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1, beta2,
                                  eps, weight_decay, int(step), grad_scale, _stream(param)), "tem_adamw_step")


def adamw_hyper(host_buf, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """Fill the 12-float HOST tensor that `adamw_step_dev` reads (after a copy to the device): tem_adamw_hyper."""
    assert not host_buf.is_cuda and host_buf.dtype == torch.float32 and host_buf.numel() >= 12
    lib = _lib.load()
    _lib.check(lib.tem_adamw_hyper(ctypes.c_void_p(host_buf.data_ptr()), lr, beta1, beta2, eps, weight_decay, int(step),
                                   grad_scale), "tem_adamw_hyper")


def adamw_step_dev(param, grad, exp_avg, exp_avg_sq, hyper):
    """adamw_step with lr / bias corrections read from the device tensor `hyper` (HIP-graph capture)."""
    _req_cuda(param, grad, exp_avg, exp_avg_sq, hyper)
    lib = _lib.load()
    _lib.check(lib.tem_adamw_step_dev(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(hyper),
                                      _stream(param)), "tem_adamw_step_dev")


def adamw_step_tab(param, grad, exp_avg, exp_avg_sq, table, sstate):
    """adamw_step with its scalars from the row of `table` that the device-side step count in `sstate` selects; skipped
    when sstate's overflow flag is up (tem_adamw_step_tab)."""
    _req_cuda(param, grad, exp_avg, exp_avg_sq, table, sstate)
    lib = _lib.load()
    _lib.check(lib.tem_adamw_step_tab(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(table),
                                      _p(sstate), _stream(param)), "tem_adamw_step_tab")


def amp_unscale_dev(grad, sstate):
    _req_cuda(grad, sstate)
    lib = _lib.load()
    _lib.check(lib.tem_amp_unscale_dev(_p(grad), grad.numel(), _p(sstate), _stream(grad)), "tem_amp_unscale_dev")


def amp_update_dev(sstate, growth, backoff, interval):
    _req_cuda(sstate)
    lib = _lib.load()
    _lib.check(lib.tem_amp_update_dev(_p(sstate), float(growth), float(backoff), int(interval), _stream(sstate)),
               "tem_amp_update_dev")


def amp_unscale(grad, inv_scale, found_inf):
    """grad *= inv_scale in place; found_inf[0] = 1 if any element is not finite (GradScaler.unscale_)."""
    _req_cuda(grad, found_inf)
    lib = _lib.load()
    _lib.check(lib.tem_amp_unscale(_p(grad), grad.numel(), float(inv_scale), _p(found_inf), _stream(grad)),
               "tem_amp_unscale")


def ema_update(theta_k, theta_q, momentum):
    _req_cuda(theta_k, theta_q)
    lib = _lib.load()
    _lib.check(lib.tem_ema_update(_p(theta_k), _p(theta_q), theta_k.numel(), momentum, _stream(theta_k)),
               "tem_ema_update")


# ---------------------------------------------------------------- labels ----
BOUNDARY_MODES = {"thick": 0, "inner": 1, "outer": 2}


def boundary_target(labels: torch.Tensor, add_binary_target: bool, mode: str = "thick") -> torch.Tensor:
    _req_cuda(labels)
    if mode not in BOUNDARY_MODES:
        raise NotImplementedError(f"find_boundaries mode '{mode}': the MI355X kernel has {sorted(BOUNDARY_MODES)} "
                                  "('subpixel' returns a 2n-1 grid, which cannot be a training target)")
    labels = labels.to(torch.int64).contiguous()
    sp = tuple(labels.shape)
    D, H, W = (1,) * (3 - len(sp)) + sp
    nch = 2 if add_binary_target else 1
    out = torch.empty((nch,) + sp, dtype=torch.float32, device=labels.device)
    lib = _lib.load()
    _lib.check(lib.tem_boundary_target_mode(_p(labels), _p(out), D, H, W, int(add_binary_target),
                                            BOUNDARY_MODES[mode], _stream(labels)), "tem_boundary_target_mode")
    return out


def affinity_target(labels, offsets, ignore_label=None, add_binary_target=False, add_mask=False,
                    include_ignore_transitions=False) -> torch.Tensor:
    _req_cuda(labels)
    labels = labels.to(torch.int64).contiguous()
    sp = tuple(labels.shape)
    nd = len(sp)
    D, H, W = (1,) * (3 - nd) + sp
    offs = []
    for o in offsets:
        o = [int(v) for v in o]
        if len(o) != nd:
            raise ValueError("offset dimensionality does not match the labels")
        offs.extend([0] * (3 - nd) + o)
    n_off = len(offsets)
    arr = (ctypes.c_int * len(offs))(*offs)
    cb = 1 if add_binary_target else 0
    nch = (n_off + cb) * (2 if add_mask else 1)
    out = torch.empty((nch,) + sp, dtype=torch.float32, device=labels.device)
    lib = _lib.load()
    _lib.check(lib.tem_affinity_target(_p(labels), _p(out), D, H, W, arr, n_off, int(ignore_label is not None),
                                       int(ignore_label or 0), int(add_binary_target), int(add_mask),
                                       int(include_ignore_transitions), _stream(labels)), "tem_affinity_target")
    return out


def standardize(x: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """Per-sample (first axis) standardisation of a contiguous tensor."""
    _req_cuda(x)
    x = x.contiguous()
    N = x.shape[0]
    L = x.numel() // N
    y = torch.empty_like(x)
    lib = _lib.load()
    nws = N * 256 * 16
    ws = _workspace(nws, x.device)
    _lib.check(lib.tem_standardize(_p(x), _p(y), N, L, eps, _p(ws), nws, _stream(x)), "tem_standardize")
    return y


# ---- min-max / percentile normalisation and contrast of raw data (csrc/rawnorm.hip) ----
def _rows(x: torch.Tensor):
    """-> (x as contiguous float32, N, L): rows are the entries of the first axis"""
    _req_cuda(x)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"expected a non-empty tensor of rows, got shape {tuple(x.shape)}")
    x = x.float().contiguous()
    N = x.shape[0]
    return x, N, x.numel() // N


def _host_floats(values, n: int, what: str):
    """a python number or a sequence of n of them -> ctypes float[n] (HOST values, carried in kernel arguments)"""
    vals = [float(v) for v in values] if isinstance(values, (list, tuple)) or hasattr(values, "__len__") else [float(values)] * n
    if len(vals) != n:
        raise ValueError(f"{what}: expected one value or {n} (one per row), got {len(vals)}")
    return (ctypes.c_float * n)(*vals)


def _fill(values, n: int, device, what: str) -> torch.Tensor:
    """host values -> a device float32 [n] without a copy or a synchronisation (tem_rawnorm_fill)"""
    out = torch.empty((n,), dtype=torch.float32, device=device)
    _lib.check(_lib.load().tem_rawnorm_fill(_p(out), _host_floats(values, n, what), n, _stream(out)), "tem_rawnorm_fill")
    return out


def _clip(clip):
    """None | (lo, hi) with None for an open side -> (flag, lo, hi)"""
    if clip is None:
        return 0, 0.0, 0.0
    lo, hi = clip
    return 1, float("-inf") if lo is None else float(lo), float("inf") if hi is None else float(hi)


def row_minmax(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(min, max) per entry of the first axis, float32 [N] on the device (tem_row_minmax; exact, bitwise reproducible)"""
    x, N, L = _rows(x)
    mn = torch.empty((N,), dtype=torch.float32, device=x.device)
    mx = torch.empty_like(mn)
    lib = _lib.load()
    nws = lib.tem_rawnorm_ws(N, L, 0)
    ws = _workspace(nws, x.device)
    _lib.check(lib.tem_row_minmax(_p(x), N, L, _p(mn), _p(mx), _p(ws), nws, _stream(x)), "tem_row_minmax")
    return mn, mx


_SELECT_KMAX = 8  # ranks per row and call of tem_row_select


def row_order_statistics(x: torch.Tensor, ranks) -> torch.Tensor:
    """out[n, k] = sorted(row n)[ranks[n][k]] exactly (0-based ranks, HOST integers: one list for every row or one list per
    row), float32 [N, K] on the device; radix select, no sort, no read-back (tem_row_select).  NaN input is undefined."""
    x, N, L = _rows(x)
    ranks = [list(r) for r in ranks] if len(ranks) and hasattr(ranks[0], "__len__") else [list(ranks)] * N
    K = len(ranks[0]) if ranks else 0
    if len(ranks) != N or K == 0 or any(len(r) != K for r in ranks):
        raise ValueError(f"row_order_statistics: expected {N} equally long, non-empty rank lists")
    out = torch.empty((N, K), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    for k0 in range(0, K, _SELECT_KMAX):
        kk = min(K - k0, _SELECT_KMAX)
        part = out if kk == K else torch.empty((N, kk), dtype=torch.float32, device=x.device)
        flat = (ctypes.c_int64 * (N * kk))(*[int(v) for r in ranks for v in r[k0:k0 + kk]])
        nws = lib.tem_rawnorm_ws(N, L, kk)
        ws = _workspace(nws, x.device)
        _lib.check(lib.tem_row_select(_p(x), N, L, flat, kk, _p(part), _p(ws), nws, _stream(x)), "tem_row_select")
        if part is not out:
            out[:, k0:k0 + kk] = part
    return out


def _apply(x, N, L, sub, div, clip) -> torch.Tensor:
    y = torch.empty_like(x)
    flag, lo, hi = _clip(clip)
    _lib.check(_lib.load().tem_rawnorm_apply(_p(x), _p(y), N, L, _p(sub), _p(div), flag, lo, hi, _stream(x)), "tem_rawnorm_apply")
    return y


def normalize(x: torch.Tensor, eps: float = 1e-7, clip=None, minval=None, maxval=None) -> torch.Tensor:
    """(x - min) / (fl32(max - min) + eps) per entry of the first axis, every step one float32 operation in the reference's
    order (`normalize`, transform/raw.py:88-116).  `minval` / `maxval` (HOST numbers) replace the row's own: with `minval`
    alone the divisor is fl32(fl32(max - minval) + eps), with `maxval` it is fl32(maxval + eps), the sum formed in double as
    the reference forms it; with both the apply kernel runs alone."""
    x, N, L = _rows(x)
    mn = mx = None
    if minval is None or maxval is None:
        mn, mx = row_minmax(x)
    if minval is not None:
        mn = _fill(minval, N, x.device, "minval")
    if maxval is not None:
        return _apply(x, N, L, mn, _fill(float(maxval) + float(eps), N, x.device, "maxval"), clip)
    sub, div = torch.empty_like(mn), torch.empty_like(mn)
    _lib.check(_lib.load().tem_rawnorm_minmax_coef(_p(mn), _p(mx), N, eps, _p(sub), _p(div), _stream(x)), "tem_rawnorm_minmax_coef")
    return _apply(x, N, L, sub, div, clip)


def percentile_plan(L: int, q: float):
    """(lower rank, upper rank, weight) of numpy's linear-interpolation percentile q of L float32 values, computed as the
    installed numpy computes them for float32 data: q / 100, the virtual index (L - 1) * q and the weight are FLOAT32
    (`np.percentile` divides by `a.dtype.type(100)`), and an index at or past the end takes the last element twice."""
    import numpy as np
    quant = np.asanyarray(np.true_divide(float(q), np.float32(100)))
    if not (0.0 <= quant <= 1.0):
        raise ValueError("Percentiles must be in the range [0, 100]")
    virt = np.asanyarray((L - 1) * quant)
    prev = np.floor(virt)
    if virt >= L - 1:
        lo = hi = L - 1
        t = virt - np.float32(-1)   # numpy indexes the last element as -1 before it forms the weight
    else:
        lo, hi, t = int(prev), int(prev) + 1, virt - prev
    return lo, hi, float(np.float32(t))


def normalize_percentile(x: torch.Tensor, lower=1.0, upper=99.0, eps: float = 1e-7, clip=None, return_percentiles: bool = False):
    """(x - v_lower) / (fl32(v_upper - v_lower) + eps) per entry of the first axis, v = np.percentile of the row (`normalize_percentile`,
    transform/raw.py:119-140): four exact order statistics per row from the radix select, numpy's float32 interpolation
    and the apply kernel; nothing leaves the device.  `lower` / `upper`: numbers, or one per row.  return_percentiles: also
    the device tensor [N, 2] of (v_lower, v_upper)."""
    x, N, L = _rows(x)
    lows = [float(v) for v in lower] if hasattr(lower, "__len__") else [float(lower)] * N
    ups = [float(v) for v in upper] if hasattr(upper, "__len__") else [float(upper)] * N
    if len(lows) != N or len(ups) != N:
        raise ValueError(f"normalize_percentile: expected one percentile or {N} (one per row)")
    ranks, weights = [], []
    for ql, qu in zip(lows, ups):
        a = percentile_plan(L, ql)
        b = percentile_plan(L, qu)
        ranks.append([a[0], a[1], b[0], b[1]])
        weights += [a[2], b[2]]
    os_ = row_order_statistics(x, ranks)
    sub = torch.empty((N,), dtype=torch.float32, device=x.device)
    div = torch.empty_like(sub)
    v = torch.empty((N, 2), dtype=torch.float32, device=x.device) if return_percentiles else None
    t = (ctypes.c_float * (2 * N))(*weights)
    _lib.check(_lib.load().tem_rawnorm_percentile_coef(_p(os_), t, N, eps, _p(sub), _p(div), _p(v), _stream(x)),
               "tem_rawnorm_percentile_coef")
    y = _apply(x, N, L, sub, div, clip)
    return (y, v) if return_percentiles else y


def contrast(x: torch.Tensor, alpha, mean: float, clip=None) -> torch.Tensor:
    """fl32(mean + fl32(alpha[n] * fl32(x - mean))) per entry of the first axis, then the clip (`RandomContrast`,
    transform/raw.py:305-334); alpha: a number or one per row (HOST values)."""
    x, N, L = _rows(x)
    a = _fill(alpha, N, x.device, "alpha")
    y = torch.empty_like(x)
    flag, lo, hi = _clip(clip)
    _lib.check(_lib.load().tem_rawnorm_contrast(_p(x), _p(y), N, L, _p(a), float(mean), flag, lo, hi, _stream(x)),
               "tem_rawnorm_contrast")
    return y


# ---- noise and blur raw augmentations (csrc/rawaug.hip; the stream: transform/_philox.py) ----
def _seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be within [0, 2^64), got {seed}")
    return seed


def philox_words(seed: int, row: int, i0: int, rnd: int, n: int, device="cuda") -> torch.Tensor:
    """The words w0..w3 of elements i0 .. i0+n-1 of stream row `row` at redraw `rnd`, [n, 4] on the device (int32 storage of
    the uint32 bit patterns): the stream itself, for tests (tem_rawaug_philox_words)."""
    if n <= 0 or not (0 <= row < 2 ** 32 and 0 <= rnd < 2 ** 32 and 0 <= i0 and i0 + n <= 2 ** 64):
        raise ValueError("philox_words: n > 0, row and round within [0, 2^32), elements within [0, 2^64)")
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    _req_cuda(out)
    _lib.check(_lib.load().tem_rawaug_philox_words(_p(out), _seed(seed), row, i0, rnd, n, _stream(out)), "tem_rawaug_philox_words")
    return out


def gauss_noise(x: torch.Tensor, std, seed: int, clip=None, row0: int = 0) -> torch.Tensor:
    """fl32(x + fl32(std[n] * z)) per entry of the first axis, z standard normal from the stream (seed, row0 + n, i), then
    the clip (`AdditiveGaussianNoise`, transform/raw.py:337-363); std: a number or one per row (HOST values)."""
    x, N, L = _rows(x)
    s = _fill(std, N, x.device, "std")
    y = torch.empty_like(x)
    flag, lo, hi = _clip(clip)
    _lib.check(_lib.load().tem_rawaug_gauss_noise(_p(x), _p(y), N, L, _p(s), _seed(seed), int(row0), flag, lo, hi, _stream(x)),
               "tem_rawaug_gauss_noise")
    return y


def poisson_add(x: torch.Tensor, lam, seed: int, clip=None, row0: int = 0) -> torch.Tensor:
    """fl32(x + fl32(k / lam[n])) with k ~ Poisson(lam[n]) from the stream, then the clip (`AdditivePoissonNoise`,
    transform/raw.py:366-391); lam: a positive number or one per row (HOST values; below 2^24)."""
    x, N, L = _rows(x)
    lm = _fill(lam, N, x.device, "lam")
    y = torch.empty_like(x)
    flag, lo, hi = _clip(clip)
    _lib.check(_lib.load().tem_rawaug_poisson_add(_p(x), _p(y), N, L, _p(lm), _seed(seed), int(row0), flag, lo, hi, _stream(x)),
               "tem_rawaug_poisson_add")
    return y


def poisson_scaled(x: torch.Tensor, mult, seed: int, clip=None, row0: int = 0, offset=None) -> torch.Tensor:
    """fl32(fl32(k / mult[n]) + offset[n]) with k ~ Poisson(fl32(fl32(x - offset[n]) * mult[n])), then the clip
    (`PoissonNoise`, transform/raw.py:394-425).  offset: None -> the row minimum (tem_row_minmax, composed here), or a
    device float32 [N]; mult: a number or one per row (HOST values)."""
    x, N, L = _rows(x)
    if offset is None:
        offset, _ = row_minmax(x)
    elif not (torch.is_tensor(offset) and offset.is_cuda and offset.dtype == torch.float32 and offset.numel() == N):
        raise ValueError(f"poisson_scaled: offset must be a device float32 tensor of {N} entries (one per row) or None")
    offset = offset.contiguous()
    m = _fill(mult, N, x.device, "mult")
    y = torch.empty_like(x)
    flag, lo, hi = _clip(clip)
    _lib.check(_lib.load().tem_rawaug_poisson_scaled(_p(x), _p(y), N, L, _p(offset), _p(m), _seed(seed), int(row0), flag, lo, hi,
                                                     _stream(x)), "tem_rawaug_poisson_scaled")
    return y


def blur2d(x: torch.Tensor, wy, wx=None) -> torch.Tensor:
    """The last two axes of x convolved with the 1-D weights wy (along H) and wx (along W; None: wy), reflect border without
    edge repeat; all other axes are independent planes (`GaussianBlur`, transform/raw.py:428-454).  Weights: HOST sequences
    of odd length <= 63 with len // 2 < the axis' size."""
    _req_cuda(x)
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"blur2d: expected a non-empty tensor of at least two axes, got shape {tuple(x.shape)}")
    x = x.float().contiguous()
    H, W = int(x.shape[-2]), int(x.shape[-1])
    wy = [float(v) for v in wy]
    wx = wy if wx is None else [float(v) for v in wx]
    dy = _fill(wy, len(wy), x.device, "wy")
    dx = dy if wx is wy else _fill(wx, len(wx), x.device, "wx")
    y = torch.empty_like(x)
    _lib.check(_lib.load().tem_rawaug_blur2d(_p(x), _p(y), x.numel() // (H * W), H, W, _p(dy), _p(dx), len(wy), len(wx), _stream(x)),
               "tem_rawaug_blur2d")
    return y


def blur3d(x: torch.Tensor, wz, wy, wx) -> torch.Tensor:
    """The last three axes of x convolved with the 1-D weights wz (along D), wy (along H) and wx (along W): `blur2d` of
    every plane, then a pass that streams along the plane and takes its taps along z (tem_rawaug_blur_z), the same reflect
    border without edge repeat on all three axes.  Weights: HOST sequences of odd length <= 63 with len // 2 < the axis'
    size; the one tap [1.0] along z (all a volume of D = 1 admits) leaves `blur2d`."""
    _req_cuda(x)
    if x.dim() < 3 or x.numel() == 0:
        raise ValueError(f"blur3d: expected a non-empty tensor of at least three axes, got shape {tuple(x.shape)}")
    wz = [float(v) for v in wz]
    D = int(x.shape[-3])
    if len(wz) % 2 == 0 or len(wz) > 63:
        raise ValueError(f"blur3d: the tap count along z must be odd and within 1..63 (got {len(wz)})")
    if len(wz) // 2 >= D:
        raise ValueError(f"blur3d: the reflect border needs k/2 < size ({len(wz)} taps along z on {D} planes)")
    y = blur2d(x, wy, wx)
    if wz == [1.0]:
        return y
    HW = int(x.shape[-2]) * int(x.shape[-1])
    dz = _fill(wz, len(wz), x.device, "wz")
    out = torch.empty_like(y)
    _lib.check(_lib.load().tem_rawaug_blur_z(_p(y), _p(out), y.numel() // (D * HW), D, HW, _p(dz), len(wz), _stream(y)),
               "tem_rawaug_blur_z")
    return out


# ---- EM defect augmentation (csrc/defect.hip; the tables: include/tem_hip.h, host side: transform/defect.py) ----
DEFECT_KEEP, DEFECT_DROP, DEFECT_LOW, DEFECT_PASTE, DEFECT_DEFORM = range(5)
DEFECT_KMAX = 33   # taps of the separable filter


def _to_device(host, device) -> torch.Tensor:
    """a small host numpy array -> the device, through pinned memory, on the current stream, without a synchronisation"""
    return torch.from_numpy(host).pin_memory().to(device, non_blocking=True)


def _slices(x: torch.Tensor, what: str):
    _req_cuda(x)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"{what}: expected a contiguous float32 tensor [S, H, W], got {x.dtype} {tuple(x.shape)}")
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[2])


class DefectTables:
    """The device tables of one defect call (include/tem_hip.h), checked on the host before they are copied: the kernels
    index with what they hold.  plan int32 [S, 4], rec int32 [D, 8] (None if D == 0), tables int32."""

    def __init__(self, plan, rec, tables, S, H, W, planes, device):
        import numpy as np
        plan = np.ascontiguousarray(plan, dtype=np.int32).reshape(-1, 4)
        rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 8)
        tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1)
        self.S, self.H, self.W, self.D, self.planes = int(S), int(H), int(W), int(rec.shape[0]), int(planes)
        if self.H < 4 or self.W < 4 or self.H > 65535 or self.W > 65535 or not 0 < self.S <= 65535:
            raise ValueError(f"defect: slices of 4 x 4 to 65535 x 65535 pixels, at most 65535 of them (got {S} of {H} x {W})")
        code = plan[:, 0]
        if plan.shape[0] != self.S or code.min() < DEFECT_KEEP or code.max() > DEFECT_DEFORM:
            raise ValueError("defect: the plan holds one record with a code of 0..4 per slice")
        paste = plan[code == DEFECT_PASTE, 1]
        if paste.size and (paste.min() < 0 or paste.max() >= self.planes):
            raise ValueError(f"defect: a pasted slice names an artifact plane outside [0, {self.planes})")
        if sorted(rec[:, 0].tolist()) != np.nonzero(code == DEFECT_DEFORM)[0].tolist():
            raise ValueError("defect: the records must name exactly the slices the plan marks deformed, each once")
        for r in rec:
            mode, off = int(r[1]), int(r[2])
            if mode not in (0, 1, 2) or not 0 <= int(r[3]) + 1 < 2 ** 31:
                raise ValueError("defect: a record's mode is 0, 1 or 2 and its stream rows lie within [0, 2^31)")
            if mode:
                n, other = (self.H, self.W) if mode == 1 else (self.W, self.H)
                if off < 0 or off + n > tables.size:
                    raise ValueError("defect: an interval table does not lie within `tables`")
                lo, hi = tables[off:off + n] & 0xffff, (tables[off:off + n] >> 16) & 0xffff
                if (lo > hi).any() or hi.max() >= other:
                    raise ValueError("defect: an interval of a line leaves the slice")
        self.plan = _to_device(plan, device)
        self.rec = _to_device(rec, device) if self.D else None
        self.tables = _to_device(tables if tables.size else np.zeros(1, np.int32), device)

    def _geom(self, x, what):
        if _slices(x, what) != (self.S, self.H, self.W) or x.device != self.plan.device:
            raise ValueError(f"{what}: the tables were made for [{self.S}, {self.H}, {self.W}] on {self.plan.device}")


def defect_mean(x: torch.Tensor, tab: DefectTables) -> torch.Tensor:
    """float32 [S]: the mean of every slice the plan marks low contrast (summed in float64 in a fixed order), 0 elsewhere"""
    tab._geom(x, "defect_mean")
    mean = torch.empty((tab.S,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tem_defect_mean(_p(x), tab.S, tab.H * tab.W, _p(tab.plan), _p(mean), _stream(x)), "tem_defect_mean")
    return mean


def defect_apply(x: torch.Tensor, tab: DefectTables, mean: torch.Tensor, art=None, alpha=None) -> torch.Tensor:
    """The streaming pass over all slices: keep, drop, low contrast with `mean`, paste of plane plan[n, 1] of `art` / `alpha`
    (float32 [planes, H, W]).  Deformed slices of the result are left unwritten: `defect_warp` fills them."""
    tab._geom(x, "defect_apply")
    if (art is None) != (alpha is None) or (art is None and tab.planes) or mean.dtype != torch.float32 or mean.numel() != tab.S \
            or mean.device != x.device:
        raise ValueError("defect_apply: art and alpha come together (the planes the tables were made for), mean is float32 [S]")
    for t in (art, alpha):
        if t is not None and (_slices(t, "defect_apply: art / alpha") != (tab.planes, tab.H, tab.W) or t.device != x.device):
            raise ValueError(f"defect_apply: artifact and alpha planes must be [{tab.planes}, {tab.H}, {tab.W}] on {x.device}")
    y = torch.empty_like(x)
    _lib.check(_lib.load().tem_defect_apply(_p(x), _p(y), tab.S, tab.H * tab.W, _p(tab.plan), _p(mean), _p(art), _p(alpha), _stream(x)),
               "tem_defect_apply")
    return y


def _defect_weights(w, device):
    w = [float(v) for v in w]
    if not (1 <= len(w) <= DEFECT_KMAX and len(w) % 2 == 1):
        raise ValueError(f"defect: the filter takes an odd number of at most {DEFECT_KMAX} weights, got {len(w)}")
    return _fill(w, len(w), device, "weights"), len(w)


def _defect_out(out, shape, device, what):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: `out` must be a contiguous float32 tensor {tuple(shape)} on {device}")
    return out


def defect_flow(tab: DefectTables, seed: int, strength: float, weights, out=None) -> torch.Tensor:
    """float32 [D, 2, H, W]: for every record of mode 0 the two noise planes (stream rows rec[d, 3], + 1) times `strength`,
    filtered along W then H with the HOST `weights`, edge repeat; plane 0 displaces columns, plane 1 rows.  The planes of
    compress records are not written."""
    if not tab.D:
        raise ValueError("defect_flow: no slice is deformed")
    flow = _defect_out(out, (tab.D, 2, tab.H, tab.W), tab.plan.device, "defect_flow")
    w, k = _defect_weights(weights, flow.device)
    _lib.check(_lib.load().tem_defect_flow(_p(flow), tab.D, tab.H, tab.W, _p(tab.rec), _seed(seed), float(strength), _p(w), k,
                                           _stream(flow)), "tem_defect_flow")
    return flow


def defect_prefilter(x: torch.Tensor, tab: DefectTables, weights, out=None) -> torch.Tensor:
    """float32 [D, H, W]: slice rec[d, 0] of x filtered along W then H with the HOST `weights`, whole-sample mirror border
    (`transform.defect.spline_fir_weights()`: the cubic B-spline coefficients)."""
    tab._geom(x, "defect_prefilter")
    if not tab.D:
        raise ValueError("defect_prefilter: no slice is deformed")
    coef = _defect_out(out, (tab.D, tab.H, tab.W), x.device, "defect_prefilter")
    w, k = _defect_weights(weights, x.device)
    _lib.check(_lib.load().tem_defect_prefilter(_p(x), _p(coef), tab.D, tab.H, tab.W, _p(tab.rec), _p(w), k, _stream(x)),
               "tem_defect_prefilter")
    return coef


def defect_warp(coef: torch.Tensor, flow: torch.Tensor, y: torch.Tensor, tab: DefectTables, seed: int, noise_scale: float) -> torch.Tensor:
    """Writes slice rec[d, 0] of y [S, H, W]: the cubic interpolant of coef[d] at the identity plus the flow (flow[d], or the
    compress flow of the record and its interval table), cval outside the slice, 0 in the band of a compress line."""
    tab._geom(y, "defect_warp")
    if not tab.D:
        raise ValueError("defect_warp: no slice is deformed")
    _defect_out(coef, (tab.D, tab.H, tab.W), y.device, "defect_warp: coef")
    _defect_out(flow, (tab.D, 2, tab.H, tab.W), y.device, "defect_warp: flow")
    _lib.check(_lib.load().tem_defect_warp(_p(coef), _p(flow), _p(y), tab.D, tab.H, tab.W, _p(tab.rec), _p(tab.tables), _seed(seed),
                                           float(noise_scale), _stream(y)), "tem_defect_warp")
    return y


# ---- distance-based instance segmentation (csrc/distance.hip) ----
POD_DIST, POD_BOUNDARY, POD_DIRECTED, POD_FOREGROUND, POD_INSTANCES = 1, 2, 4, 8, 16


def _flat_cumsum(flag: torch.Tensor) -> torch.Tensor:
    """inclusive prefix sum of int32 flags over the whole batch, on the device (no host synchronisation); the kernels
    that read it subtract the previous sample's total.  One flat scan: torch's per-row scan of [N, V] is ~50x slower."""
    return torch.cumsum(flag, dim=0, dtype=torch.int32)


def pod_ids(labels: torch.Tensor, apply_label: bool, min_size: int) -> torch.Tensor:
    """int64 [N, D, H, W] labels -> int32 object ids 1..n per sample (0 background): connected components in
    first-occurrence order (apply_label) or ascending original ids; objects below min_size voxels dropped, the rest
    renumbered in order (tem_pod_cc_* / tem_pod_seq_* / tem_pod_size_*)."""
    _req_cuda(labels)
    labels = labels.to(torch.int64).contiguous()
    N, D, H, W = labels.shape
    V = D * H * W
    lib = _lib.load()
    ids = torch.empty((N * V,), dtype=torch.int32, device=labels.device)
    flag = torch.empty((N * V,), dtype=torch.int32, device=labels.device)
    if apply_label:
        parent = torch.empty((N * V,), dtype=torch.int32, device=labels.device)
        _lib.check(lib.tem_pod_cc_roots(_p(labels), _p(parent), _p(flag), N, D, H, W, _stream(labels)), "tem_pod_cc_roots")
        rank = _flat_cumsum(flag)
        _lib.check(lib.tem_pod_cc_assign(_p(labels), _p(parent), _p(rank), _p(ids), N, V, _stream(labels)),
                   "tem_pod_cc_assign")
    else:
        srt, order = torch.sort(labels.view(N, V), dim=1)
        _lib.check(lib.tem_pod_seq_flag(_p(srt), _p(flag), N, V, _stream(labels)), "tem_pod_seq_flag")
        rank = _flat_cumsum(flag)
        _lib.check(lib.tem_pod_seq_assign(_p(srt), _p(order), _p(rank), _p(ids), N, V, _stream(labels)),
                   "tem_pod_seq_assign")
    ids = ids.view(N, D, H, W)
    if min_size > 0:
        size_filter_(ids, min_size)
    return ids


def size_filter_(ids: torch.Tensor, min_size: int) -> torch.Tensor:
    """in place on contiguous int32 ids [N, D, H, W]: positive ids with fewer than min_size voxels become 0, the surviving
    ones are renumbered 1..n in ascending order, per sample (tem_pod_size_keep / tem_pod_size_apply); id 0 stays 0."""
    _req_cuda(ids)
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    N = ids.shape[0]
    V = ids.numel() // N
    lib = _lib.load()
    cnt = torch.empty((N * (V + 1),), dtype=torch.int32, device=ids.device)
    keep = torch.empty_like(cnt)
    _lib.check(lib.tem_pod_size_keep(_p(ids), _p(cnt), _p(keep), N, V, int(min_size), _stream(ids)), "tem_pod_size_keep")
    newid = _flat_cumsum(keep)
    _lib.check(lib.tem_pod_size_apply(_p(ids), _p(keep), _p(newid), N, V, _stream(ids)), "tem_pod_size_apply")
    return ids


# ---- seeded watershed (csrc/watershed.hip) ----
_WS_MARKERS = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def watershed_rounds(V: int) -> int:
    """ceil(log2(V)) + 1: the Boruvka rounds `seeded_watershed` enqueues for samples of V voxels, the bound of `rounds_out`"""
    return max(int(V) - 1, 0).bit_length() + 1


def voxel_ranks(height: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """float32 heights [N, ...] -> (rank, order), int32 [N, V]: the voxels of each sample ranked by (height, linear index),
    by a stable ascending sort (`np.argsort(kind="stable")` of the flattened sample): order[n, rank[n, v]] = v.  -0.0 and
    0.0 tie.  The heights are not read back: NaNs are not rejected and where they are ranked is not promised."""
    if height.dtype != torch.float32 or height.dim() < 2 or height.numel() == 0:
        raise ValueError(f"voxel_ranks: expected non-empty float32 heights [N, ...], got {height.dtype} {tuple(height.shape)}")
    _req_cuda(height)
    N = int(height.shape[0])
    V = height.numel() // N
    if V >= 2 ** 31 - 1:
        raise ValueError(f"voxel_ranks: {V} voxels per sample, at most 2^31 - 2 supported")
    # x + 0.0 turns -0.0 into 0.0 and nothing else: a sort that compares bit patterns ties the two as well
    order = torch.sort(height.reshape(N, V) + 0.0, dim=1, stable=True).indices
    rank = torch.empty((N, V), dtype=torch.int32, device=height.device)
    rank.scatter_(1, order, torch.arange(V, dtype=torch.int32, device=height.device).expand(N, V))
    return rank, order.to(torch.int32)


def _ws_args(height, markers, mask, rounds_out):
    """the host-side checks of `seeded_watershed` (dtypes, shapes; the values of tensors that are still on the host)"""
    if height.dim() != 4 or height.dtype != torch.float32 or height.numel() == 0:
        raise ValueError(f"seeded_watershed: expected non-empty float32 heights [N, D, H, W], got {height.dtype} {tuple(height.shape)}")
    if markers.dtype not in _WS_MARKERS:
        raise ValueError(f"seeded_watershed: markers must be of an integer type, got {markers.dtype}")
    if markers.shape != height.shape:
        raise ValueError(f"seeded_watershed: markers {tuple(markers.shape)} do not match the heights {tuple(height.shape)}")
    if mask is not None and (mask.dtype != torch.bool or mask.shape != height.shape):
        raise ValueError(f"seeded_watershed: expected a bool mask {tuple(height.shape)}, got {mask.dtype} {tuple(mask.shape)}")
    if rounds_out is not None and (rounds_out.dtype != torch.int32 or rounds_out.numel() != 1):
        raise ValueError(f"seeded_watershed: rounds_out is one int32, got {rounds_out.dtype} {tuple(rounds_out.shape)}")
    V = height.numel() // int(height.shape[0])
    if V >= 2 ** 31 - 1:
        raise ValueError(f"seeded_watershed: {V} voxels per sample, at most 2^31 - 2 supported")
    if not markers.is_cuda and markers.dtype != torch.bool and int(markers.min()) < 0:
        raise ValueError("seeded_watershed: markers must be >= 0")
    if not height.is_cuda and not bool(torch.isfinite(height).all()):
        raise ValueError("seeded_watershed: heights must be finite")


def seeded_watershed(height: torch.Tensor, markers: torch.Tensor, mask: Optional[torch.Tensor] = None,
                     rounds_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Seeded watershed of float32 heights [N, D, H, W] (2-D: D = 1) from integer markers >= 0 inside a bool mask (None:
    everything) -> int32 [N, D, H, W]: the minimum spanning forest rooted in the markers (tem_watershed; the definition:
    DESIGN.md "Seeded watershed").  Voxels are ranked by (height, linear index) (`voxel_ranks`), an edge between masked
    face neighbours is as high as its higher end, ties go to the lower other end; every masked voxel takes the marker of
    its tree, a masked voxel without a path to a marker and every voxel outside the mask get 0; markers outside the mask
    are ignored, marker voxels keep their value.  On heights without ties this is a priority flood's segmentation up to the
    voxels on a pass; a PLATEAU goes to the marker that reaches it first in raster order, it is not split half-way.
    Deterministic, stream-ordered, nothing is read back: the values of device tensors are not checked -- a negative marker
    (or one above 2^31 - 1) counts as no marker, and heights must be finite (tensors still on the host are checked and then
    refused like any host tensor).  rounds_out: a device int32 that receives the rounds that did work, at most
    `watershed_rounds(D * H * W)`."""
    _ws_args(height, markers, mask, rounds_out)
    _req_cuda(height, markers, mask, rounds_out)
    N, D, H, W = (int(s) for s in height.shape)
    V = D * H * W
    height = height.contiguous()
    if markers.dtype not in (torch.int32, torch.int64):
        markers = markers.to(torch.int32)
    markers = markers.contiguous()
    mask = None if mask is None else mask.contiguous()
    rank, order = voxel_ranks(height)
    lib = _lib.load()
    nbytes = int(lib.tem_watershed_ws(N, V))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=height.device)
    out = torch.empty((N, D, H, W), dtype=torch.int32, device=height.device)
    _lib.check(lib.tem_watershed(_p(rank), _p(order), _p(markers), markers.element_size(), _p(mask), _p(out), _p(rounds_out),
                                 N, D, H, W, _p(ws), nbytes, _stream(height)), "tem_watershed")
    return out


# ---- mutex watershed (csrc/mws.hip) ----
MWS_MAX_CHANNELS = 32          # TEM_MWS_MAX_CHANNELS
MWS_MAX_BATCH = 64             # TEM_MWS_MAX_BATCH
MWS_ROUNDS_PER_BATCH = 16      # the default: profiles/mws_bench.txt


def mws_table_slots(n_repulsive: int) -> int:
    """the slots of the mutex set for `n_repulsive` existing repulsive edges: a power of two, at least twice their count"""
    return int(_lib.load().tem_mws_table_slots(int(n_repulsive)))


def _mws_args(aff, offsets, n_attractive, mask, edge_valid, rounds_per_batch):
    """the host-side checks of `mutex_watershed` (dtypes, shapes, offsets) -> offsets as a list of C (dz, dy, dx)"""
    if not torch.is_tensor(aff) or aff.dim() != 5 or aff.dtype != torch.float32 or aff.numel() == 0:
        raise ValueError("mutex_watershed: expected non-empty float32 affinities [N, C, D, H, W], got "
                         f"{getattr(aff, 'dtype', type(aff))} {tuple(getattr(aff, 'shape', ()))}")
    N, C, D, H, W = (int(s) for s in aff.shape)
    V = D * H * W
    try:
        offs = [[int(x) for x in o] for o in offsets]
    except (TypeError, ValueError):
        raise ValueError("mutex_watershed: offsets must be integer vectors of length 2 or 3") from None
    if len(offs) != C:
        raise ValueError(f"mutex_watershed: {len(offs)} offsets do not match the {C} affinity channels")
    if C > MWS_MAX_CHANNELS:
        raise ValueError(f"mutex_watershed: {C} channels, at most {MWS_MAX_CHANNELS} supported")
    if any(len(o) not in (2, 3) or len(o) != len(offs[0]) for o in offs):
        raise ValueError("mutex_watershed: offsets must be integer vectors of one length, 2 or 3")
    if len(offs[0]) == 2 and D != 1:
        raise ValueError(f"mutex_watershed: offsets of length 2 need D = 1, got D = {D}")
    if any(abs(x) >= 2 ** 30 for o in offs for x in o):
        raise ValueError("mutex_watershed: offsets must be below 2^30 in magnitude")
    if isinstance(n_attractive, bool) or not isinstance(n_attractive, numbers.Integral) or not 0 <= n_attractive <= C:
        raise ValueError(f"mutex_watershed: n_attractive must be an integer within 0..{C}, got {n_attractive}")
    if mask is not None and (mask.dtype != torch.bool or tuple(mask.shape) != (N, D, H, W)):
        raise ValueError(f"mutex_watershed: expected a bool mask {(N, D, H, W)}, got {mask.dtype} {tuple(mask.shape)}")
    if edge_valid is not None and (edge_valid.dtype != torch.bool or edge_valid.shape != aff.shape):
        raise ValueError(f"mutex_watershed: expected bool edge_valid {tuple(aff.shape)}, got {edge_valid.dtype} {tuple(edge_valid.shape)}")
    if V >= 2 ** 31 - 1 or C * V >= 2 ** 32 - 1 or N * V >= 2 ** 33 - 1:
        raise ValueError(f"mutex_watershed: {N} samples of {C} x {V} edges; V below 2^31 - 1, C * V below 2^32 - 1 and "
                         "N * V below 2^33 - 1 supported")
    if isinstance(rounds_per_batch, bool) or not isinstance(rounds_per_batch, numbers.Integral) or not 1 <= rounds_per_batch <= MWS_MAX_BATCH:
        raise ValueError(f"mutex_watershed: rounds_per_batch must be an integer within 1..{MWS_MAX_BATCH}, got {rounds_per_batch}")
    return [[0] * (3 - len(o)) + o for o in offs]


def mutex_watershed(aff: torch.Tensor, offsets, n_attractive: int, mask: Optional[torch.Tensor] = None,
                    edge_valid: Optional[torch.Tensor] = None, rounds_per_batch: int = MWS_ROUNDS_PER_BATCH,
                    return_rounds: bool = False):
    """Mutex watershed of float32 affinities [N, C, D, H, W] (2-D: D = 1) -> int32 ids [N, D, H, W] (tem_mws_*; the
    definition: DESIGN.md "Mutex watershed").  Edge (c, v) joins voxel v and v + offsets[c] (C integer vectors of length 2
    or 3) when that voxel is inside the sample, both are inside the bool `mask` [N, D, H, W] (None: everything) and the
    bool `edge_valid` [N, C, D, H, W] (None: every edge) is set; edges never cross samples.  The `n_attractive` leading
    channels are attractive with priority 1 - aff, the others repulsive with priority aff (float32; -0.0 ties with 0.0);
    edges are taken by priority descending, ties by the lower id c * V + v: an attractive edge merges its two clusters
    unless they are one or mutually exclusive (the union inherits the mutexes), a repulsive edge between two clusters makes
    them mutually exclusive.  Ids: 0 outside the mask, else 1..n per sample in raster order of each cluster's first voxel;
    a masked voxel without edges is a segment of its own.  The result is that of the sequential algorithm, bit for bit;
    where NaN affinities are placed is not promised, and parity with affogato / elf is not pinned (their sort leaves the
    order of ties open).
    The number of rounds depends on the data: rounds are enqueued `rounds_per_batch` (1..64) at a time and two ints are
    read back after each batch, plus the edge counts once at the start (they size the mutex set).  `return_rounds`: also
    the number of rounds that did work."""
    offs = _mws_args(aff, offsets, n_attractive, mask, edge_valid, rounds_per_batch)
    _req_cuda(aff, mask, edge_valid)
    N, C, D, H, W = (int(s) for s in aff.shape)
    aff = aff.contiguous()
    mask = None if mask is None else mask.contiguous()
    edge_valid = None if edge_valid is None else edge_valid.contiguous()
    dev = aff.device
    lib = _lib.load()
    coffs = (ctypes.c_int * (3 * C))(*[x for o in offs for x in o])
    geom = (int(n_attractive), N, C, D, H, W)
    nbytes = int(lib.tem_mws_ws(N, C, D, H, W))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.check(lib.tem_mws_init(_p(mask), _p(edge_valid), coffs, *geom, _p(ws), nbytes, _stream(aff)), "tem_mws_init")
    n_edges, n_rep = ws[:16].view(torch.int64).tolist()
    slots = mws_table_slots(n_rep)
    table = torch.empty((slots,), dtype=torch.int64, device=dev)
    first, work = 1, 0
    while True:
        _lib.check(lib.tem_mws_run(_p(aff), coffs, *geom, _p(ws), nbytes, _p(table), slots, first, int(rounds_per_batch),
                                   _stream(aff)), "tem_mws_run")
        work, alive = ws[16:24].view(torch.int32).tolist()
        first = 0
        if work > n_edges + 1:
            raise RuntimeError(f"mutex_watershed: {work} working rounds for {n_edges} edges: every working round commits an edge")
        if not alive:
            break
    first_voxel = torch.empty((N, D, H, W), dtype=torch.int32, device=dev)
    _lib.check(lib.tem_mws_labels(_p(first_voxel), N, C, D, H, W, _p(ws), nbytes, _stream(aff)), "tem_mws_labels")
    ids = pod_ids(first_voxel, False, 0)       # 1 + first voxel, ascending -> 1..n in raster order of the first voxel
    return (ids, work) if return_rounds else ids


# ---- label overlaps and instance-segmentation scores (csrc/overlap.hip) ----
_OV_LABELS = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


class LabelOverlaps(NamedTuple):
    """The contingency table of two label batches of V voxels per sample, all on the device (`label_overlaps`): the
    distinct (seg id, target id) pairs in ascending order with their voxel counts -- rows below `npairs[n]` are valid,
    the rest is unspecified -- and both marginals, indexed by the DENSE ids (0 stays 0, the other values 1..n in
    ascending order, per sample)."""
    pa: torch.Tensor       # int32 [N, V]
    pb: torch.Tensor       # int32 [N, V]
    n_ab: torch.Tensor     # int32 [N, V]
    npairs: torch.Tensor   # int32 [N]
    n_a: torch.Tensor      # int32 [N, V + 1]
    n_b: torch.Tensor      # int32 [N, V + 1]
    ws: torch.Tensor       # uint8 [tem_overlap_ws(N, V)], scratch of both calls


class OverlapScores(NamedTuple):
    """Per-sample sums over a contingency table (`overlap_scores`; include/tem_hip.h: TemOverlapRecord), on the device"""
    sum_ab: torch.Tensor      # int64 [N]    sum n_ab^2 (exact; below 2^62)
    sum_a: torch.Tensor       # int64 [N]    sum n_a^2
    sum_b: torch.Tensor       # int64 [N]    sum n_b^2
    s_ab: torch.Tensor        # float64 [N]  sum n_ab log2 n_ab
    s_a: torch.Tensor         # float64 [N]
    s_b: torch.Tensor         # float64 [N]
    dice_pred: torch.Tensor   # float64 [N]  mean best Dice of the seg objects against the target's
    dice_true: torch.Tensor   # float64 [N]  mean best Dice of the target objects against the seg's
    n_pred: torch.Tensor      # int32 [N]    distinct non-zero ids of seg
    n_true: torch.Tensor      # int32 [N]    distinct non-zero ids of target
    tp: torch.Tensor          # int32 [N]    matches at the threshold
    best_pred: torch.Tensor   # float64 [N, V + 1]  best Dice per dense seg id (0 for id 0 and absent ids)
    best_true: torch.Tensor   # float64 [N, V + 1]
    n: int                    # voxels per sample


def _ov_args(seg, target):
    """the host-side checks of `label_overlaps` (dtypes and shapes; values are not looked at)"""
    for name, t in (("seg", seg), ("target", target)):
        if not torch.is_tensor(t) or t.dtype not in _OV_LABELS:
            raise ValueError(f"label_overlaps: {name} must be a tensor of an integer type, got {getattr(t, 'dtype', type(t))}")
    if seg.shape != target.shape:
        raise ValueError(f"label_overlaps: seg {tuple(seg.shape)} and target {tuple(target.shape)} must have one shape")
    if seg.dim() != 4 or seg.numel() == 0:
        raise ValueError(f"label_overlaps: expected non-empty labels [N, D, H, W], got {tuple(seg.shape)}")
    N = int(seg.shape[0])
    V = seg.numel() // N
    if V >= 2 ** 31 - 1 or N * V >= 2 ** 31 - 1 or N > 65535:
        raise ValueError(f"label_overlaps: {N} samples of {V} voxels; at most 2^31 - 2 voxels in all and 65535 samples supported")
    return N, V


def label_overlaps(seg: torch.Tensor, target: torch.Tensor) -> LabelOverlaps:
    """The contingency table of two integer label batches [N, D, H, W] (2-D: D = 1) of one shape, any integer dtype, values
    >= 0, built per sample on the device (tem_overlap_flag / tem_overlap_table; DESIGN.md "Instance segmentation scores").
    Both sides are made dense first (`pod_ids(x, False, 0)`: 0 stays 0, the other values become 1..n ascending), so pa,
    pb and the marginals speak of dense ids.  Deterministic, stream-ordered, nothing is read back: the values of device
    tensors are not inspected -- a negative id is not refused, it is numbered like any other non-zero value; host tensors
    are refused like any host tensor."""
    N, V = _ov_args(seg, target)
    _req_cuda(seg, target)
    a = pod_ids(seg, False, 0).view(N, V)
    b = pod_ids(target, False, 0).view(N, V)
    key = a.to(torch.int64).mul_(V + 1).add_(b)
    srt = torch.sort(key, dim=1).values
    dev = seg.device
    lib = _lib.load()
    flag = torch.empty((N * V,), dtype=torch.int32, device=dev)
    _lib.check(lib.tem_overlap_flag(_p(srt), _p(flag), N, V, _stream(seg)), "tem_overlap_flag")
    rank = _flat_cumsum(flag)
    nbytes = int(lib.tem_overlap_ws(N, V))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    pa, pb, n_ab = (torch.empty((N, V), dtype=torch.int32, device=dev) for _ in range(3))
    n_a, n_b = (torch.empty((N, V + 1), dtype=torch.int32, device=dev) for _ in range(2))
    npairs = torch.empty((N,), dtype=torch.int32, device=dev)
    _lib.check(lib.tem_overlap_table(_p(srt), _p(rank), _p(pa), _p(pb), _p(n_ab), _p(npairs), _p(n_a), _p(n_b), N, V, _p(ws),
                                     nbytes, _stream(seg)), "tem_overlap_table")
    return LabelOverlaps(pa, pb, n_ab, npairs, n_a, n_b, ws)


def _ov_threshold(threshold) -> float:
    threshold = float(threshold)
    if not 0.5 <= threshold <= 1.0:
        raise ValueError(f"overlap_scores: threshold {threshold}: a threshold below 0.5 needs an assignment solver and is not "
                         "provided (0.5 <= threshold <= 1)")
    return threshold


def overlap_scores(ov: LabelOverlaps, threshold: float = 0.5) -> OverlapScores:
    """The sums every instance score is a fixed expression of, per sample, from a contingency table (tem_overlap_scores;
    the fields: `OverlapScores`).  Label 0 counts in the sums of squares and of n log2 n; it is ignored in n_pred, n_true,
    tp and the best Dice.  tp counts the pairs with n_ab >= threshold * (n_a + n_b - n_ab) minus the objects of either
    side with two of them: the size of the maximum matching for 0.5 <= threshold <= 1; a threshold below
    0.5 is refused.  Integer fields are exact, the float64 sums are reduced in a fixed order: bit-identical from run to
    run.  Nothing is read back."""
    threshold = _ov_threshold(threshold)
    _req_cuda(*ov[:7])
    N, V = (int(s) for s in ov.pa.shape)
    dev = ov.pa.device
    lib = _lib.load()
    rec = torch.empty((N, 10), dtype=torch.int64, device=dev)
    best = torch.empty((2, N, V + 1), dtype=torch.float64, device=dev)
    _lib.check(lib.tem_overlap_scores(_p(ov.pa), _p(ov.pb), _p(ov.n_ab), _p(ov.npairs), _p(ov.n_a), _p(ov.n_b), threshold,
                                      _p(rec), _p(best[0]), _p(best[1]), N, V, _p(ov.ws), ov.ws.numel(), _stream(ov.pa)),
               "tem_overlap_scores")
    real = rec[:, 3:8].view(torch.float64)
    ints = rec[:, 8:10].view(torch.int32)
    return OverlapScores(rec[:, 0], rec[:, 1], rec[:, 2], real[:, 0], real[:, 1], real[:, 2], real[:, 3], real[:, 4],
                         ints[:, 0], ints[:, 1], ints[:, 2], best[0], best[1], V)


def pod_targets(ids: torch.Tensor, ndim: int, sampling, flags: int, fill: float) -> torch.Tensor:
    """int32 ids [N, D, H, W] -> float32 [N, C, D, H, W] per-object distance targets (tem_pod_targets)."""
    _req_cuda(ids)
    N, D, H, W = ids.shape
    V = D * H * W
    nch = (1 if flags & POD_DIST else 0) + (ndim if flags & POD_DIRECTED else 0) + (1 if flags & POD_BOUNDARY else 0)
    nc = nch + (1 if flags & POD_INSTANCES else 0) + (1 if flags & POD_FOREGROUND else 0)
    out = torch.empty((N, nc, D, H, W), dtype=torch.float32, device=ids.device)
    lib = _lib.load()
    nws = lib.tem_pod_ws(N, V, ndim, flags)
    ws = torch.empty((nws,), dtype=torch.uint8, device=ids.device)
    samp = (ctypes.c_float * 3)(*[float(s) for s in sampling])
    _lib.check(lib.tem_pod_targets(_p(ids), _p(out), N, D, H, W, ndim, samp, int(flags), float(fill), _p(ws), nws,
                                   _stream(ids)), "tem_pod_targets")
    return out


VDT_NONE = 0x3fffffff   # include/tem_hip.h: TEM_VDT_NONE, the squared distance of a sample without target voxels
DT_DIST, DT_DIRECTED, DT_NORMALIZE, DT_INVERT, DT_CLIP = 1, 2, 4, 8, 16


def vector_edt(labels: torch.Tensor, foreground_id: int):
    """int64 labels [N, D, H, W] (2-D: D == 1) -> (offsets int32 [N, 3, D, H, W] in (z, y, x) order, pointing from each
    voxel to a nearest voxel equal to foreground_id; their exact squared length int32 [N, D, H, W]; empty int32 [N], 1
    where a sample has no such voxel -- its offsets are 0 and its squared distances VDT_NONE).  tem_vector_edt."""
    _req_cuda(labels)
    labels = labels.to(torch.int64).contiguous()
    N, D, H, W = labels.shape
    dev = labels.device
    vec = torch.empty((N, 3, D, H, W), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, D, H, W), dtype=torch.int32, device=dev)
    empty = torch.empty((N,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tem_vector_edt(_p(labels), int(foreground_id), _p(vec), _p(d2), _p(empty), N, D, H, W,
                                          _stream(labels)), "tem_vector_edt")
    return vec, d2, empty


def distance_targets(labels: torch.Tensor, ndim: int, foreground_id: int = 1, distances: bool = True,
                     directed_distances: bool = False, normalize: bool = True, max_distance: Optional[float] = None,
                     invert: bool = False) -> torch.Tensor:
    """int64 labels [N, D, H, W] -> float32 [N, C, D, H, W], channels [distances?][directed x ndim?] of the reference's
    DistanceTransform before `func` (tem_vector_edt, tem_distance_targets); no host synchronisation."""
    vec, d2, empty = vector_edt(labels, foreground_id)
    N, D, H, W = d2.shape
    flags = ((DT_DIST if distances else 0) | (DT_DIRECTED if directed_distances else 0) | (DT_NORMALIZE if normalize else 0)
             | (DT_INVERT if invert else 0) | (DT_CLIP if max_distance is not None else 0))
    nc = (1 if distances else 0) + (ndim if directed_distances else 0)
    out = torch.empty((N, nc, D, H, W), dtype=torch.float32, device=d2.device)
    lib = _lib.load()
    nws = lib.tem_distance_targets_ws(N, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=d2.device)
    _lib.check(lib.tem_distance_targets(_p(vec), _p(d2), _p(empty), _p(out), N, D, H, W, ndim, flags,
                                        float(max_distance or 0.0), _p(ws), nws, _stream(d2)), "tem_distance_targets")
    return out


def onehot_target(labels: torch.Tensor, class_ids) -> torch.Tensor:
    """int64 labels [N, *spatial] and a list of ids -> float32 [N, C, *spatial] (tem_onehot_target)."""
    _req_cuda(labels)
    labels = labels.to(torch.int64).contiguous()
    ids = (ctypes.c_int64 * len(class_ids))(*[int(c) for c in class_ids])
    N, C = labels.shape[0], len(class_ids)
    V = labels.numel() // N
    out = torch.empty((N, C) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    _lib.check(_lib.load().tem_onehot_target(_p(labels), ids, C, _p(out), N, V, _stream(labels)), "tem_onehot_target")
    return out


def boundary_target_masked(labels: torch.Tensor, mode: str, kind: int, key_label: int, mask_label: int,
                           add_binary_target: bool) -> torch.Tensor:
    """int64 labels [N, D, H, W] -> int8 [N, 1(+1), D, H, W]: boundaries with the boundaries of (labels != key_label)
    (kind 0) or (labels == key_label) (kind 1) set to mask_label (tem_boundary_target_masked)."""
    _req_cuda(labels)
    if mode not in BOUNDARY_MODES:
        raise NotImplementedError(f"find_boundaries mode '{mode}': the MI355X kernel has {sorted(BOUNDARY_MODES)} "
                                  "('subpixel' returns a 2n-1 grid, which cannot be a training target)")
    labels = labels.to(torch.int64).contiguous()
    N, D, H, W = labels.shape
    out = torch.empty((N, 2 if add_binary_target else 1, D, H, W), dtype=torch.int8, device=labels.device)
    _lib.check(_lib.load().tem_boundary_target_masked(_p(labels), _p(out), N, D, H, W, BOUNDARY_MODES[mode], int(kind),
                                                      int(key_label), int(mask_label), int(add_binary_target),
                                                      _stream(labels)), "tem_boundary_target_masked")
    return out


def _ncv_or_contiguous(t):
    s = _ncv_strides(t)
    if s is None:
        t = t.contiguous()
        s = _ncv_strides(t)
    return t, s


def dist_loss_fwd(p, t, mask_bg: bool, mse: bool, eps_fg: float, eps_dist: float):
    """-> (loss float[], coef float[6], p, t) of DistanceLoss / DiceBasedDistanceLoss on [N, 3, *spatial]
    (tem_dist_loss_fwd: one pass over both tensors, fixed-order double sums)."""
    _req_cuda(p, t)
    p, ps = _ncv_or_contiguous(p)
    t, ts = _ncv_or_contiguous(t)
    N, C, V = ps[3:]
    dev = p.device
    sums = torch.empty((12,), dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty((6,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    nws = lib.tem_dist_loss_ws()
    ws = _workspace(nws, dev)
    _lib.check(lib.tem_dist_loss_fwd(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], N, V, int(mask_bg), int(mse),
                                     float(eps_fg), float(eps_dist), _p(sums), _p(loss), _p(coef), _p(ws), nws,
                                     _stream(p)), "tem_dist_loss_fwd")
    return loss, coef, p, t


def dist_loss_grad(p, t, coef, gout, mask_bg: bool) -> torch.Tensor:
    """d loss / d p with p's strides (tem_dist_loss_grad); gout: device scalar"""
    ps = _ncv_strides(p)
    ts = _ncv_strides(t)
    gp = torch.empty_like(p)
    if _ncv_strides(gp)[:3] != ps[:3]:
        raise RuntimeError("dist_loss_grad: the gradient does not share the prediction's strides")
    N, C, V = ps[3:]
    _lib.check(_lib.load().tem_dist_loss_grad(_p(p), ps[0], ps[1], ps[2], _p(t), ts[0], ts[1], ts[2], _p(coef), _p(gout),
                                              _p(gp), N, V, int(mask_bg), _stream(p)), "tem_dist_loss_grad")
    return gp


# ---- patch supply from device-resident volumes (csrc/patch.hip; the tables: include/tem_hip.h; data/device_dataset.py) ----
PT_DTYPE = {torch.uint8: 0, torch.uint16: 1, torch.int16: 2, torch.int32: 3, torch.int64: 4, torch.float32: 5}
_PT_LABELS = (torch.uint8, torch.uint16, torch.int32, torch.int64)


class PatchBoxes:
    """Boxes checked against their volumes and copied to the device: int32 [M, 8] (volume, z0, y0, x0, dz, dy, dx, 0)."""
    __slots__ = ("dev", "host", "M", "max_vox")

    def __init__(self, dev, host):
        self.dev, self.host, self.M = dev, host, int(host.shape[0])
        self.max_vox = int((host[:, 4].astype("int64") * host[:, 5] * host[:, 6]).max())


class PatchVolumes:
    """Volumes [C, D, H, W] of one dtype that stay on the device, and their descriptor table (int64 [V, 6]: pointer, dtype code,
    C, D, H, W).  The kernels index with what the tables hold, so `boxes()` checks every box on the host before it is copied."""

    def __init__(self, volumes):
        volumes = list(volumes)
        _req_cuda(*volumes)
        if not volumes or any(v.dim() != 4 or v.numel() == 0 or not v.is_contiguous() for v in volumes):
            raise ValueError("PatchVolumes: expected non-empty contiguous tensors [C, D, H, W]")
        if len({v.dtype for v in volumes}) != 1 or volumes[0].dtype not in PT_DTYPE or len({v.device for v in volumes}) != 1:
            raise ValueError(f"PatchVolumes: one device and one dtype of {sorted(str(d) for d in PT_DTYPE)} for all volumes")
        self.volumes, self.dtype, self.device = volumes, volumes[0].dtype, volumes[0].device
        self.shapes = [tuple(int(s) for s in v.shape) for v in volumes]
        import numpy as np
        self.table = _to_device(np.array([[v.data_ptr(), PT_DTYPE[v.dtype], *v.shape] for v in volumes], dtype=np.int64), self.device)

    def boxes(self, boxes) -> PatchBoxes:
        """host integers [M, 7] (volume, z0, y0, x0, dz, dy, dx) -> PatchBoxes; raises for a box that leaves its volume"""
        if isinstance(boxes, PatchBoxes):
            return boxes
        import numpy as np
        b = np.asarray(boxes, dtype=np.int64).reshape(-1, 7)
        if not 0 < b.shape[0] <= 65535:
            raise ValueError(f"patch: 1..65535 boxes per call, got {b.shape[0]}")
        if b[:, 0].min() < 0 or b[:, 0].max() >= len(self.volumes):
            raise ValueError(f"patch: a box names a volume outside [0, {len(self.volumes)})")
        dims = np.array([s[1:] for s in self.shapes], dtype=np.int64)[b[:, 0]]
        if (b[:, 1:4] < 0).any() or (b[:, 4:7] < 1).any() or (b[:, 1:4] + b[:, 4:7] > dims).any():
            bad = int(np.nonzero((b[:, 1:4] < 0).any(1) | (b[:, 4:7] < 1).any(1) | (b[:, 1:4] + b[:, 4:7] > dims).any(1))[0][0])
            raise ValueError(f"patch: box {bad} {b[bad, 1:].tolist()} is empty or leaves its volume {self.shapes[int(b[bad, 0])][1:]}")
        if (b[:, 4] * b[:, 5] * b[:, 6]).max() >= 2 ** 31:
            raise ValueError("patch: a box holds 2^31 voxels or more")
        host = np.zeros((b.shape[0], 8), dtype=np.int32)
        host[:, :7] = b
        return PatchBoxes(_to_device(host, self.device), host)


def patch_count(vols: PatchVolumes, boxes, value: int) -> torch.Tensor:
    """int32 [M, 2] on the device: per box of channel 0 of a label volume (uint8 / uint16 / int32 / int64) the voxels != value
    and the voxels != the box's first voxel (tem_patch_count; one streaming pass, bitwise reproducible)"""
    if vols.dtype not in _PT_LABELS:
        raise ValueError(f"patch_count: label volumes are uint8, uint16, int32 or int64, got {vols.dtype}")
    bx = vols.boxes(boxes)
    out = torch.empty((bx.M, 2), dtype=torch.int32, device=vols.device)
    _lib.check(_lib.load().tem_patch_count(_p(vols.table), _p(bx.dev), bx.M, PT_DTYPE[vols.dtype], bx.max_vox, int(value), _p(out),
                                           _stream(out)), "tem_patch_count")
    return out


def patch_hist_path(n_ids: int) -> int:
    """which kernel `patch_hist` runs for this many ids: 0 the workgroup's LDS table, 1 global adds (-1: refused)"""
    return int(_lib.load().tem_patch_hist_path(int(n_ids)))


def patch_hist(vols: PatchVolumes, boxes, n_ids: int) -> torch.Tensor:
    """int32 [M, n_ids] on the device: voxels per dense id (int32 volumes, channel 0; `pod_ids` makes them) in every box
    (tem_patch_hist; runs of equal ids along x are added once)"""
    if vols.dtype != torch.int32:
        raise ValueError(f"patch_hist: the volumes hold dense int32 ids, got {vols.dtype}")
    if patch_hist_path(n_ids) < 0:
        raise ValueError(f"patch_hist: n_ids >= 1, got {n_ids}")
    bx = vols.boxes(boxes)
    hist = torch.empty((bx.M, int(n_ids)), dtype=torch.int32, device=vols.device)
    _lib.check(_lib.load().tem_patch_hist(_p(vols.table), _p(bx.dev), bx.M, bx.max_vox, int(n_ids), _p(hist), _stream(hist)),
               "tem_patch_hist")
    return hist


def _pt_sel(sel, n, hist, what):
    if sel.dtype != torch.int32 or sel.dim() != 1 or (n is not None and sel.numel() != n) or sel.numel() == 0 or sel.device != hist.device \
            or not sel.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous int32 vector{'' if n is None else f' of {n} entries'} on {hist.device}")


def patch_hist_instances(hist: torch.Tensor, excluded: torch.Tensor, min_size: int = 1) -> torch.Tensor:
    """int32 [M]: ids with at least max(min_size, 1) voxels in the box whose entry of `excluded` (int32 [n_ids]) is 0"""
    _req_cuda(hist, excluded)
    if hist.dim() != 2 or hist.dtype != torch.int32 or not hist.is_contiguous():
        raise ValueError("patch_hist_instances: expected the contiguous int32 [M, n_ids] of patch_hist")
    _pt_sel(excluded, hist.shape[1], hist, "patch_hist_instances: excluded")
    out = torch.empty((hist.shape[0],), dtype=torch.int32, device=hist.device)
    _lib.check(_lib.load().tem_patch_hist_reduce(_p(hist), hist.shape[0], hist.shape[1], 0, _p(excluded), 0, int(min_size), _p(out),
                                                 _stream(out)), "tem_patch_hist_reduce")
    return out


def patch_hist_listed(hist: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """int32 [M, K]: the box's voxels of every dense id in `ids` (int32 [K]; an id outside the histogram counts 0)"""
    _req_cuda(hist, ids)
    if hist.dim() != 2 or hist.dtype != torch.int32 or not hist.is_contiguous():
        raise ValueError("patch_hist_listed: expected the contiguous int32 [M, n_ids] of patch_hist")
    _pt_sel(ids, None, hist, "patch_hist_listed: ids")
    out = torch.empty((hist.shape[0], ids.numel()), dtype=torch.int32, device=hist.device)
    _lib.check(_lib.load().tem_patch_hist_reduce(_p(hist), hist.shape[0], hist.shape[1], 1, _p(ids), ids.numel(), 1, _p(out),
                                                 _stream(out)), "tem_patch_hist_reduce")
    return out


def patch_gather(vols: PatchVolumes, boxes, patch_shape, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[B, C, pd, ph, pw] of `dtype` (float32 / int32 / int64) on the device: every box cast to dtype, with ZEROS where the box
    is smaller than the patch -- `np.pad(mode="constant")`, what the reference's `ensure_patch_shape` does for its
    SegmentationDataset; NOT the reflect padding of `TensorDataset`.  One launch (tem_patch_gather)."""
    if dtype not in (torch.float32, torch.int32, torch.int64) or (vols.dtype == torch.float32 and dtype != torch.float32):
        raise ValueError(f"patch_gather: {vols.dtype} volumes do not gather to {dtype} (float32, int32, int64; float32 stays float32)")
    bx = vols.boxes(boxes)
    pd, ph, pw = (int(p) for p in patch_shape)
    C = {s[0] for s in (vols.shapes[int(i)] for i in set(bx.host[:, 0].tolist()))}
    if len(C) != 1:
        raise ValueError("patch_gather: the volumes of one call have the same number of channels")
    C = C.pop()
    if min(pd, ph, pw) < 1 or (bx.host[:, 4:7] > (pd, ph, pw)).any() or bx.M * C > 65535 or pd * ph * pw >= 2 ** 31:
        raise ValueError(f"patch_gather: boxes must fit the patch {(pd, ph, pw)}; at most 65535 planes of < 2^31 voxels")
    out = torch.empty((bx.M, C, pd, ph, pw), dtype=dtype, device=vols.device)
    _lib.check(_lib.load().tem_patch_gather(_p(vols.table), _p(bx.dev), bx.M, C, PT_DTYPE[vols.dtype], pd, ph, pw, _p(out),
                                            PT_DTYPE[dtype], _stream(out)), "tem_patch_gather")
    return out
