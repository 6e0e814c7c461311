"""Forward/backward engine of the MI355X U-Net path.

One `torch.autograd.Function` (`UNetFunction`) spans the whole network.  Its forward mirrors
the data flow of the reference (`UNetBase._apply_default`, model/unet.py:194-209; `Encoder.forward`
:311-321; `Decoder.forward` :375-388; `ConvBlock` :429-438; `Upsampler.forward` :455-458) and its
hand-written backward replaces what autograd derives for those modules -- but both are
sequenced MI355X-first:

* activations are channels-last (NDHWC) fp32 in HBM, allocated once per step; torch is used
  for memory, streams and the autograd hook only, every FLOP runs in libtem_hip.so;
* pre-norm is never materialised: `norm_stats` emits per-(n,c) scale/shift and the conv kernel
  applies them while staging its input tile (zero padding AFTER the norm, as in the reference);
* bias + ReLU live in the conv epilogue; ReLU-backward masks live in the dgrad epilogue, the
  norm-backward apply kernel or the max-pool-backward kernel (never a pass of their own);
* skip concatenation is free: the encoder block writes its output into the upper channel half of
  a [.., Cup+Cskip] buffer, the decoder's upsampler writes the lower half (leading dimension `ld`);
* Upsampler = interpolate -> 1x1 conv in the reference; both are linear and the interpolation
  weights sum to one, so the engine runs the 1x1 conv first (1/8 of the voxels) and interpolates
  its output.  Results differ from the reference order only by fp32 rounding (tests: 1e-4);
* parameter gradients are written into ONE flat fp32 arena per step (views are returned to
  autograd), so the optimizer step and the data-parallel all-reduce are single launches.
"""
import os
import threading
from dataclasses import dataclass
from typing import Any, List, NamedTuple, Optional

import torch
import torch.nn as nn

from .. import ops
from ..arith import Arith
from . import pack

_FORCE_GENERIC = os.environ.get("TEM_DISABLE_MFMA", "0") == "1"

# Arithmetic of the MFMA convolutions:
#   "fp32"   everything exact fp32 on v_mfma_f32_32x32x2_f32 (157 TFLOP/s peak).
#   "mixed"  forward convolutions exact fp32; gradient-side convolutions (dgrad, wgrad) split-bf16
#            "bf16x3": x = hi + lo in bf16, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32
#            accumulation (~1e-5 relative per product, 833 TFLOP/s effective peak).
#   "split"  as "mixed", but the forward convolutions use "bf16x6": three bf16 terms per operand (all
#            24 mantissa bits) and the six products of order <= 2^-16 -- per-product error ~2^-23,
#            the fp32 class, at 16/6 of the exact-fp32 MFMA rate (417 TFLOP/s effective peak).
#   "split16" (DEFAULT) as "split", except that forward convolutions whose input is PRE-NORMALISED (fused InstanceNorm /
#            GroupNorm / BatchNorm in front, i.e. every 3x3x3 conv of a ConvBlock) use "fp16x3": x = hi + lo' * 2^-12 with
#            two fp16 terms (22 mantissa bits; the lo plane is stored scaled by 2^12 so that it stays out of fp16's
#            subnormal range), hi*hi in one fp32 accumulator and hi*lo' + lo'*hi in a second one that the epilogue adds
#            back times 2^-12 -- per-product error ~2^-22, still the fp32 class, at HALF the MFMAs of bf16x6 (833
#            TFLOP/s effective peak).  Gradient error against float64 equals the fp32 reference path's own
#            (tests/test_gpu_unet.py: 3.5e-4 / 5.9e-6 / 1.3e-3 vs 3.8e-4 / 8.6e-5 / 1.3e-3).  Raw-activation inputs
#            (norm=None nets, 1x1x1 convs) keep bf16x6: no range assumption there.
#   "bf16x3" forward in bf16x3 too (forward noise 1e-5: NOT parity-grade, see below).
#   "amp"    mixed precision, the counterpart of the reference's torch.autocast(float16) default on GPUs: conv operands
#            rounded to fp16, ONE v_mfma_f32_32x32x16_f16 per product, fp32 accumulation, fp32 storage; needs loss
#            scaling (optim.GradScaler).  2^-11 per operand: NOT parity-grade; the trainers select it only when asked
#            (mixed_precision=True with an explicit mixed_precision_dtype="float16", or TEM_MIXED_PRECISION=1).
#   "amp_bf16" the same with operands rounded to bf16 (ONE v_mfma_f32_32x32x16_bf16 per product): the counterpart of
#            torch.autocast(bfloat16), mixed_precision_dtype="bfloat16"; fp32 exponent range, so no loss scaling (the
#            reference creates a GradScaler for float16 only, trainer/default_trainer.py:134-142); 2^-8 per operand.
# Why the forward keeps fp32-class products ("split" is the default; "mixed"/"fp32" use the exact MFMA): the U-Net's gradient is ill-conditioned w.r.t. the FORWARD values -- a
# 1e-7 relative forward perturbation flips ReLU masks / pooling arg-maxes of near-ties and moves
# gradient entries by ~1e-4..1e-3 (that is the fp32 reference's own distance from the float64
# gradient; tests/test_gpu_unet.py) -- so 1e-5 forward noise would cost ~5e-3 in the gradients.
# The backward convolutions are LINEAR in the incoming gradient with masks fixed by the forward
# pass, so their 1e-5 error is not amplified.
PRECISION = os.environ.get("TEM_PRECISION", "split16")
# Activation STORAGE of the two mixed modes (round 5): every tensor between two kernels of the step -- activations, saved
# tensors, data gradients -- is fp16 ("amp") / bf16 ("amp_bf16") in HBM, as under torch.autocast in the reference trainer
# (trainer/default_trainer.py:134-142, 781-794); the network input, the prediction, statistics, coefficients, parameters and
# the gradient arena stay fp32, all arithmetic stays fp32 with one rounding per stored value.  TEM_AMP_STORAGE=32 keeps fp32
# tensors (the mixed modes of rounds 1-4: 16-bit operands only).  The fp32-class modes always store fp32.
_AMP_STORAGE16 = os.environ.get("TEM_AMP_STORAGE", "16") != "32"


def act_dtype():
    """element type of the activation tensors the engine allocates in the current precision mode"""
    if _AMP_STORAGE16 and not _FORCE_GENERIC:
        if PRECISION == "amp":
            return torch.float16
        if PRECISION == "amp_bf16":
            return torch.bfloat16
    return torch.float32


def set_precision(mode: str):
    global PRECISION
    if mode not in ("fp32", "mixed", "split", "split16", "bf16x3", "amp", "amp_bf16"):
        raise ValueError(f"unknown precision mode {mode}")
    PRECISION = mode


class precision_scope:
    """`with precision_scope("amp"):` -- the arithmetic of every engine call inside (the role torch.autocast plays
    in the reference trainer, trainer/default_trainer.py:800-803).  Forward AND backward of a step must run in the
    same scope: the packed weights are keyed on the mode."""

    def __init__(self, mode: str):
        self.mode, self.prev = mode, None

    def __enter__(self):
        self.prev = PRECISION
        set_precision(self.mode)
        return self

    def __exit__(self, *exc):
        set_precision(self.prev)
        return False


def _f3(f, dim):
    if isinstance(f, int):
        f = (f,) * dim
    f = tuple(int(v) for v in f)
    return (1,) * (3 - len(f)) + f


class ConvSpec:
    """A conv layer of the reference model plus the norm that precedes it (both parameter holders)."""

    def __init__(self, conv: nn.Module, norm: Optional[nn.Module]):
        self.conv, self.norm = conv, norm
        self.k = pack.k3(conv.kernel_size)
        self.cin, self.cout = conv.in_channels, conv.out_channels

    # --- norm description -------------------------------------------------------
    def norm_args(self):
        """(groups, gamma, beta, eps) or None"""
        n = self.norm
        if n is None:
            return None
        if isinstance(n, nn.GroupNorm):
            return n.num_groups, n.weight, n.bias, n.eps
        # InstanceNorm == one group per channel; affine=False by default in the reference
        return self.cin, getattr(n, "weight", None), getattr(n, "bias", None), n.eps

    # --- packed weights (cached until the parameter changes) -----------------------
    def _modes(self):
        mode_f = {"bf16x3": Arith.BF16X3, "split": Arith.BF16X6, "split16": Arith.BF16X6, "amp": Arith.F16,
                  "amp_bf16": Arith.BF16}.get(PRECISION, Arith.FP32)
        if PRECISION == "split16" and self.norm is not None and self.k != (1, 1, 1):
            # fp16x3: the conv reads pre-normalised activations (|x^| of order 1..100 << 65504; clamped at 6e4)
            mode_f = Arith.F16X3
        mode_d = Arith.F16 if PRECISION == "amp" else Arith.BF16 if PRECISION == "amp_bf16" else \
            Arith.BF16X3 if PRECISION in ("bf16x3", "mixed", "split", "split16") else Arith.FP32
        mf = mode_f if (not _FORCE_GENERIC) and ops.mfma_ok(self.cin, self.cout, self.k) else Arith.VALU
        md = mode_d if (not _FORCE_GENERIC) and ops.mfma_ok(self.cout, self.cin, self.k) else Arith.VALU
        mw = mode_d if (not _FORCE_GENERIC) and ops.mfma_ok(self.cin, self.cout, self.k, wgrad=True) else Arith.VALU
        return mf, md, mw

    def packed(self) -> pack.PackEntry:
        return pack.packed(self.conv, PRECISION, self._modes)


class NormStats(NamedTuple):
    """Statistics of the norm in front of a conv (_stats).  mode "sample": InstanceNorm / GroupNorm per sample; "batch":
    BatchNorm in training mode; "frozen": a norm with running statistics in eval mode (mean / rstd are None)."""
    mean: Optional[torch.Tensor]
    rstd: Optional[torch.Tensor]
    scale: torch.Tensor   # [N, C]: the conv applies x * scale + shift while it stages its input
    shift: torch.Tensor
    mode: str

    @property
    def per_sample(self) -> bool:
        return self.mode == "sample"


@dataclass(slots=True)
class BlockState:
    """What the backward of a ConvBlock needs from its forward (_block_fwd)."""
    xin: Any            # block input (a tensor or an ops.Planar concat)
    a1: torch.Tensor    # ReLU output of conv1
    out: torch.Tensor   # ReLU output of conv2
    s1: Optional[NormStats]
    s2: Optional[NormStats]
    c1: ConvSpec
    c2: ConvSpec
    out_part: Any       # first-stage statistics of `out` (partials, nblk) when asked for and delivered


@dataclass(slots=True)
class Level:
    """One encoder level: its block and the concat buffer it shares with the decoder stage of the same resolution."""
    cat: Any            # [.., c_up + Cskip] concat buffer (tensor or ops.Planar)
    skip: torch.Tensor  # its skip half = the block's output
    bs: BlockState
    f: tuple            # pooling factor
    c_up: int
    floor_sub: Optional[torch.Tensor] = None   # dense copy of the sub-volume whole pooling windows cover (check_shape = False)
    cat_c: Optional[torch.Tensor] = None       # concat buffer of the decoder stage when the skip is centre-cropped
    crop: Optional[list] = None                # ... and the crop offsets


@dataclass(slots=True)
class DecStage:
    """One decoder stage: 1x1 conv at low resolution (low -> t), upsampling into the concat buffer, block (-> out)."""
    low: torch.Tensor
    sspec: ConvSpec
    bs: BlockState
    f: tuple
    out: torch.Tensor
    t: torch.Tensor


class SideOut(NamedTuple):
    ospec: ConvSpec
    y: torch.Tensor


@dataclass(slots=True)
class Step:
    """Everything a forward pass keeps for its backward (_forward_impl(keep=True))."""
    levels: List[Level]
    dec: List[DecStage]
    base: BlockState
    last: torch.Tensor            # output of the last decoder block
    act: Optional[str]            # final activation fused into the output conv(s)
    y: torch.Tensor               # prediction (NDHWC)
    dim: int
    x_shape: tuple
    ospec: Optional[ConvSpec] = None        # output conv of a plain network
    side: Optional[List[SideOut]] = None    # return_side_outputs: one per decoder stage, coarse .. fine


# Weight gradients of the pre-normalised 3x3x3 convolutions in the "fp16 2x1" arithmetic (round 4, VERDICT r3 item 2:
# "measure whether the backward needs three MFMAs per product at all"): x^ = hi + lo in two fp16 terms, g ONE fp16 term
# after a power-of-two prescale from max |g| -- two MFMAs per product instead of the three of bf16x3.  A weight gradient
# is a LEAF of the backward pass (nothing reads dw downstream), so its rounding does not propagate; with the forward
# pass held fixed (scripts/backward_arith_sim.py, profiles/r04_backward_arith_sim.txt) every dw tensor picks up ~2e-4
# of unbiased noise (an 11-bit g), against 1e-3 tolerance and 1.4e-3 .. 3.9e-3 for the fp32 reference path itself.  What
# does NOT work, measured there: one term for x^ (the ReLU zeros of the previous layer all normalise to the SAME value,
# whose rounding error is coherent over the volume: 1.2e-3 on the last decoder conv), any bf16 single term (8 bits),
# and fewer products in the DATA gradients (their error is handed down the whole backward pass: 5e-4 .. 8e-4).
# TEM_WGRAD_ARITH=bf16x3 restores the three-product weight gradients.
_WGRAD_F16X2 = os.environ.get("TEM_WGRAD_ARITH", "f16x2") == "f16x2"


_FUSE_OUT_BWD = os.environ.get("TEM_FUSE_OUT_BWD", "1") != "0"   # out_conv: weight gradient + masked data gradient in one kernel
_FUSE_AMAX = os.environ.get("TEM_FUSE_AMAX", "1") != "0"   # 0: every fp16 2x1 weight gradient runs its own absmax pass
# the weight gradient that delivers the norm sums also finishes them into the norm-backward coefficients; 0: ops.norm_bwd_coef
_FUSE_COEF = os.environ.get("TEM_FUSE_NORM_COEF", "1") != "0"
_FUSE_POOL_STATS = os.environ.get("TEM_FUSE_POOL_STATS", "1") != "0"   # max-pool forward writes the statistics partials of its output


def _coef_request(spec, stats, x):
    """-> (coef [N, Cin, 4], bp): a weight gradient that delivers the norm sums (sums_from=...) also finishes them into the
    coefficients of the norm backward when given bp (ops.Byproducts.norm_coef) and the layer allows it, else (None, None).
    Norms with affine parameters keep the separate stage: their dgamma / dbeta come from it."""
    groups, gamma, beta, _ = spec.norm_args()
    if _FUSE_COEF and gamma is None and beta is None and stats is not None and stats.per_sample:
        coef = torch.empty((x.shape[0], spec.cin, 4), dtype=torch.float32, device=x.device)
        return coef, ops.Byproducts(norm_coef=(groups, stats.mean, stats.rstd, coef))
    return None, None


def _amax_slot(grads):
    """A cleared word for `out_amax=` of the launch that writes a data gradient: the launch also delivers max |out| for the
    fp16 2x1 weight gradient that reads `out` next (_wgrad(amax=)); None when no such weight gradient runs.  The word
    describes `out` as written: it travels next to it and is dropped where `out` is modified."""
    on = grads is not None and _FUSE_AMAX and _WGRAD_F16X2 and PRECISION == "split16" and not _FORCE_GENERIC
    return grads.amax_slot() if on else None


def _wgrad_f16x2_ok(spec, x, stats) -> bool:
    return _WGRAD_F16X2 and PRECISION == "split16" and stats is not None and not _FORCE_GENERIC and \
        spec.k == (3, 3, 3) and spec.cin % 32 == 0 and spec.cout % 32 == 0 and \
        ops.conv_wgrad_gscaled_ok(x, spec.k, spec.cin, spec.cout)


def fused_activation(act: nn.Module) -> Optional[str]:
    """Final activations that run inside the out_conv epilogue."""
    if isinstance(act, nn.Sigmoid):
        return "sigmoid"
    if isinstance(act, nn.ReLU):
        return "relu"
    return None


# -----------------------------------------------------------------------------------
# building blocks
# -----------------------------------------------------------------------------------
# No-grad forward passes (validation, tiled inference, the SPOCO teacher) do not feed a backward pass, so the
# ill-conditioning argument for 24-bit forward products (top of this file) does not apply: they run the bf16x3 kernels
# (outputs ~1e-5 from fp32, inside the 1e-3 tolerance; 1.6x faster convolutions).  TEM_INFER_BF16X3=0 keeps bf16x6.
_INFER_BF16X3 = os.environ.get("TEM_INFER_BF16X3", "1") != "0"
class _ThreadFlags(threading.local):
    no_grad_forward = False   # per thread: predict_with_halo drives one thread per device


_TLS = _ThreadFlags()


# Forward statistics of a conv output that feeds the next norm directly (conv1 -> norm2 of every ConvBlock) come out of
# the conv's epilogue instead of a separate pass over the tensor (ops.conv_fwd(want_stats=True)); TEM_FUSE_STATS=0 disables.
_FUSE_STATS = os.environ.get("TEM_FUSE_STATS", "1") != "0"
_FUSE_CONCAT_STATS = os.environ.get("TEM_FUSE_CONCAT_STATS", "1") != "0"


def _conv(spec: ConvSpec, x, y, stats=None, act=None, want_stats=False):
    ent = spec.packed()
    scale, shift = (stats.scale, stats.shift) if stats is not None else (None, None)
    wp = ent.get("fwd_inf" if _TLS.no_grad_forward and _INFER_BF16X3 and ent.fwd.mode == Arith.BF16X6 else "fwd")
    return ops.conv_fwd(x, wp.buf, spec.conv.bias, y, spec.k, spec.cin, spec.cout, scale=scale, shift=shift, act=act,
                        mfma=wp.mode, want_stats=want_stats)


class _Grads:
    """Flat fp32 gradient arena (layout: torch_em_amd.arena.arena_layout, `model.parameters()` order).
    Tracks which element ranges backward has produced so that a data-parallel `GradSync` can
    all-reduce them while the rest of backward is still running."""

    def __init__(self, params: List[torch.Tensor]):
        from ..arena import arena_layout
        self.offsets, total = arena_layout(params)
        self.shapes = {id(p): p.shape for p in params}
        self.flat = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        self.written = set()
        self._new = []
        self._amax = None     # int32 words for max |g| of data gradients (_amax_slot, ops.absmax)
        self._amax_used = 0

    def amax_slot(self) -> torch.Tensor:
        """one cleared 32-bit word (a view of a pool that one memset per backward pass clears)"""
        if self._amax is None or self._amax_used >= self._amax.numel():
            self._amax = torch.zeros(64, dtype=torch.int32, device=self.flat.device)
            self._amax_used = 0
        i = self._amax_used
        self._amax_used += 1
        return self._amax[i:i + 1]

    def view(self, p: torch.Tensor, track: bool = True) -> torch.Tensor:
        o, n = self.offsets[id(p)]
        if track:
            self.written.add(id(p))
            self._new.append((o, o + (n + 3) // 4 * 4))
        return self.flat[o:o + n].view(self.shapes[id(p)])

    def take_new_ranges(self):
        """Coalesced element ranges written since the last call."""
        if not self._new:
            return []
        rs = sorted(self._new)
        self._new = []
        out = [list(rs[0])]
        for lo, hi in rs[1:]:
            if lo <= out[-1][1]:
                out[-1][1] = max(out[-1][1], hi)
            else:
                out.append([lo, hi])
        return [tuple(r) for r in out]


# the split-K epilogue of a data gradient also writes the first stage of the backward of the norm in front of the conv
# (TEM_BP_NORM_SUMS of tem_conv3d_fwd_ex: k_norm_partial<.,1> disappears for the 16^3 / 8^3 levels); 0: the pass over gx and x
_FUSE_DGRAD_SUMS = os.environ.get("TEM_FUSE_DGRAD_SUMS", "1") != "0"


def _dgrad(spec: ConvSpec, g, gx, ref=None, refnorm=None, grads=None, sums_for=None):
    """-> (sums, amax), each None when not asked for or not delivered.
    refnorm: coef [N, C, 4] of the norm behind `ref` -- its backward (and ref's ReLU mask) run in the kernel's epilogue.
    grads: gx is FINAL after this call (nothing rewrites it): ask the kernel for max |gx| as a by-product (_amax_slot).
    sums_for = (x, stats): gx lands behind the norm whose input is x -> partial rows [N, nblk, C, 2] of its backward's first
    stage when this launch can deliver them (plain launch on the split-K z-reuse kernel).  Not together with grads."""
    assert grads is None or sums_for is None
    ent = spec.packed()
    part = slot = bp = None
    if sums_for is not None and _FUSE_DGRAD_SUMS and ref is None and refnorm is None and not _FORCE_GENERIC:
        x, stats = sums_for
        mode = ent.dgrad.mode
        if stats is not None and stats.per_sample and ops.conv_fwd_family(g, spec.k, spec.cout, spec.cin, mode, y=gx) == 4:
            nblk = ops.conv_fwd_stat_blocks(g, spec.k, spec.cout, spec.cin, mode, y=gx)
            if nblk > 0:
                part = torch.empty((x.shape[0], nblk, spec.cin, 2), dtype=torch.float32, device=x.device)
                bp = ops.Byproducts(norm_sums=(x, spec.norm_args()[0], stats.mean, stats.rstd, part))
    else:
        slot = _amax_slot(grads)
        if slot is not None:
            bp = ops.Byproducts(out_amax=slot)
    wp = ent.get("dgrad")
    if refnorm is not None:
        ops.conv_fwd_refnorm(g, wp.buf, gx, spec.k, spec.cout, spec.cin, ref, refnorm, wp.mode, bp=bp)
    else:
        ops.conv_fwd(g, wp.buf, None, gx, spec.k, spec.cout, spec.cin, ref=ref, mfma=wp.mode, bp=bp)
    return (part if part is not None and bp.sums else None), (slot if slot is not None and bp.amax else None)


# Norm-backward sums from the weight gradient (csrc/wgrad_sums.hip, ops.conv_wgrad(sums_from=...)): the reduction pass over the
# data gradient and the norm input disappears for the layers that qualify.  tem_set_option("wgrad_sums", 0) disables.
def _wgrad(spec: ConvSpec, x, g, grads: _Grads, stats=None, want_sums=False, amax=None):
    """-> (sums [N, Cin, 2], coef [N, Cin, 4]) for _norm_bwd_inplace: the sums when want_sums and the layer qualifies, the
    finished coefficients when the launch delivered them too (_coef_request); each None otherwise.
    amax: int32[1] that HOLDS max |g| (a producer of g delivered it, _amax_slot) for the fp16 2x1 arithmetic, else None."""
    ent = spec.packed()
    scale, shift = (stats.scale, stats.shift) if stats is not None else (None, None)
    dw = grads.view(spec.conv.weight)
    db = grads.view(spec.conv.bias) if spec.conv.bias is not None else None
    f16x2 = ent.wgrad == Arith.BF16X3 and _wgrad_f16x2_ok(spec, x, stats)
    sums_from = coef = bp = None
    if want_sums and stats is not None and stats.per_sample and db is not None and \
            ops.conv_wgrad_sums_ok(x, spec.k, spec.cin, spec.cout, ent.wgrad):
        _, gamma, beta, _ = spec.norm_args()
        sums_from = spec.conv.weight, gamma, beta
    if f16x2 and amax is None:   # no producer of g delivered max |g|: one pass over g
        amax = ops.absmax(g, grads.amax_slot())
    if sums_from is not None:
        coef, bp = _coef_request(spec, stats, x)
    if f16x2:
        sums = ops.conv_wgrad_gscaled(x, g, spec.k, spec.cin, spec.cout, dw, db, amax, scale=scale, shift=shift,
                                      sums_from=sums_from, bp=bp)
    else:
        sums = ops.conv_wgrad(x, g, spec.k, spec.cin, spec.cout, dw, db, scale=scale, shift=shift, mfma=ent.wgrad,
                              sums_from=sums_from, bp=bp)
    if sums_from is None:
        return None, None
    return sums, (coef if bp is not None and bp.coef else None)


def _is_batchnorm(n) -> bool:
    return isinstance(n, nn.modules.batchnorm._BatchNorm)


def _flat_batch(t):
    """[N, D, H, W, C(ld)] -> [1, N*D, H, W, C] view: BatchNorm statistics run over the batch and the volume."""
    N, D, H, W, C = t.shape
    return t.as_strided((1, N * D, H, W, C), (N * D * t.stride(1), t.stride(1), t.stride(2), t.stride(3), t.stride(4)))


def _update_running(n, mean, var_biased, count):
    """running statistics of BatchNorm / InstanceNorm(track_running_stats=True), torch semantics: unbiased variance,
    momentum None = cumulative average.  mean / var: [rows, C], averaged over rows (instances)."""
    with torch.no_grad():
        if _is_batchnorm(n):  # nn.InstanceNorm never touches the counter (torch/nn/modules/instancenorm.py)
            n.num_batches_tracked += 1
        m = n.momentum if n.momentum is not None else 1.0 / float(n.num_batches_tracked)
        unbiased = var_biased * (count / max(count - 1, 1))
        n.running_mean.mul_(1.0 - m).add_(mean.mean(0), alpha=m)
        n.running_var.mul_(1.0 - m).add_(unbiased.mean(0), alpha=m)


# 16-bit storage: the concat buffer of a level with 2 x 32 channels as two dense planes (ops.Planar) -- a 32-channel slice of
# an interleaved 16-bit buffer is 64 bytes of every 128-byte line, and the kernels that read one half (max-pool forward /
# backward, upsample backward) pay for the whole line (profiles/r05_halfline.txt).  TEM_PLANAR_CONCAT=0: interleaved as in fp32.
_PLANAR_CONCAT = os.environ.get("TEM_PLANAR_CONCAT", "1") != "0"


def _planar_concat_ok(adt, c_up, enc_blk, dec_blk, shape, dev, floor) -> bool:
    if not _PLANAR_CONCAT or adt == torch.float32 or c_up != 32 or enc_blk.out_channels != 32 or floor or _FORCE_GENERIC or \
            not _DEFER_CONCAT_NORM:
        return False
    c1 = dec_blk.conv_specs()[0]
    n = c1.norm
    if c1.k != (3, 3, 3) or c1.cin != 64 or c1.cout % 32 or (n is not None and (_is_batchnorm(n) or not _norm_is_live(n))):
        return False
    N, D, H, W = shape
    ent = c1.packed()
    x64, g = ops.Probe(N, D, H, W, 64, adt), ops.Probe(N, D, H, W, c1.cout, adt)
    return ops.conv_fwd_family(x64, c1.k, 64, c1.cout, ent.fwd.mode, y=g) == 3 and \
        ops.conv_fwd_family(g, c1.k, c1.cout, 64, ent.dgrad.mode, y=x64) == 3 and \
        ops.conv_wgrad_cs_ok(x64, c1.k, 64, c1.cout, N * D * H * W * 32)   # the stride ops.Planar gives its two planes


def _half(t, c_up, i):
    """channels [:c_up] (i = 0: the upsampled half) or [c_up:] (i = 1: the skip half) of a concat buffer"""
    if isinstance(t, ops.Planar):
        return t.halves[i]
    return t[..., :c_up] if i == 0 else t[..., c_up:]


def _like(t):
    return t.empty_like() if isinstance(t, ops.Planar) else torch.empty_like(t)


def _planar_stats(x, groups, gamma, beta, eps):
    """ops.norm_stats of a planar concat without first-stage rows from its producers: each dense half on its own"""
    cg = 64 // groups
    if 32 % cg:
        raise ValueError("a norm group straddles the halves of a planar concat buffer")
    sl = lambda t, i: None if t is None else t[i * 32:(i + 1) * 32]  # noqa: E731
    parts = [ops.norm_stats(x.halves[i], 32 // cg, sl(gamma, i), sl(beta, i), eps) for i in (0, 1)]
    return tuple(torch.cat([parts[0][j], parts[1][j]], dim=1) for j in range(4))


def _stats(spec: ConvSpec, x, partials=None, partials2=None):
    """Statistics of the norm in front of a conv -> NormStats, or None without a norm (reference `get_norm_layer`,
    model/unet.py:391-406).
    partials: (part, nblk) from the producing conv's epilogue (ops.conv_fwd(want_stats=True)) or None."""
    na = spec.norm_args()
    if na is None:
        return None
    groups, gamma, beta, eps = na
    n = spec.norm
    N = x.shape[0]
    tracked = getattr(n, "track_running_stats", False) and getattr(n, "running_mean", None) is not None
    if tracked and not n.training:
        scale = torch.rsqrt(n.running_var.float() + eps)
        if gamma is not None:
            scale = scale * gamma.detach().float()
        shift = -n.running_mean.float() * scale
        if beta is not None:
            shift = shift + beta.detach().float()
        return NormStats(None, None, scale.expand(N, -1).contiguous(), shift.expand(N, -1).contiguous(), "frozen")
    vox = x.shape[1] * x.shape[2] * x.shape[3]
    if _is_batchnorm(n):
        xb = _flat_batch(x)
        if partials2 is not None:
            mean, rstd, scale, shift = ops.norm_stats_from_partials2(partials2[0], partials2[1], 1, vox, groups, gamma, beta, eps)
        elif partials is not None:
            mean, rstd, scale, shift = ops.norm_stats_from_partials(partials[0], 1, vox, x.shape[4], groups, gamma, beta, eps)
        else:
            mean, rstd, scale, shift = ops.norm_stats(xb, groups, gamma, beta, eps)
        if tracked:
            _update_running(n, mean, 1.0 / (rstd * rstd) - eps, xb.shape[1] * xb.shape[2] * xb.shape[3])
        return NormStats(mean, rstd, scale.expand(N, -1).contiguous(), shift.expand(N, -1).contiguous(), "batch")
    if partials2 is not None:
        mean, rstd, scale, shift = ops.norm_stats_from_partials2(partials2[0], partials2[1], N, vox, groups, gamma, beta, eps)
    elif partials is not None:
        mean, rstd, scale, shift = ops.norm_stats_from_partials(partials[0], N, vox, x.shape[4], groups, gamma, beta, eps)
    elif isinstance(x, ops.Planar):
        mean, rstd, scale, shift = _planar_stats(x, groups, gamma, beta, eps)
    else:
        mean, rstd, scale, shift = ops.norm_stats(x, groups, gamma, beta, eps)
    if tracked:  # InstanceNormTrackStats: per-instance statistics, running averages of their batch means
        _update_running(n, mean, 1.0 / (rstd * rstd) - eps, x.shape[1] * x.shape[2] * x.shape[3])
    return NormStats(mean, rstd, scale, shift, "sample")


def _norm_is_live(n) -> bool:
    """does this norm compute statistics of its input in the current mode?"""
    return n is not None and not (getattr(n, "track_running_stats", False) and
                                  getattr(n, "running_mean", None) is not None and not n.training)


def _block_fwd(blk, xin, out, in_partials2=None, out_stats=False, in_partials=None):
    """ConvBlock (reference model/unet.py:429-438): [norm->conv->ReLU] x 2.  Returns what backward needs.
    in_partials2: first-stage statistics of the two channel halves of xin (decoder concat) or None.
    in_partials: first-stage statistics of xin from its producer (the max-pool kernel) or None.
    out_stats: also return the first-stage statistics of `out` (out_part; None when conv2 cannot provide them)."""
    c1, c2 = blk.conv_specs()
    N, D, H, W, _ = xin.shape
    s1 = _stats(c1, xin, partials=in_partials, partials2=in_partials2)
    a1 = ops.new_act(N, D, H, W, c1.cout, xin.device, out.dtype)
    live = _norm_is_live(c2.norm)
    part = _conv(c1, xin, a1, s1, act="relu", want_stats=_FUSE_STATS and live)
    s2 = _stats(c2, a1, partials=part if (_FUSE_STATS and live) else None)
    out_part = _conv(c2, a1, out, s2, act="relu", want_stats=bool(out_stats))
    return BlockState(xin, a1, out, s1, s2, c1, c2, out_part if out_stats else None)


# The norm in front of a decoder block reads concat(upsample(u), skip).  Its backward needs no elementwise pass over that
# (largest) tensor: the two kernels that consume the gradient next -- upsample backward and the encoder's max-pool
# backward -- apply gx = a*g - m1 - (x - mean)*m2r on the fly (ops.norm_bwd_coef / ops.upsample_bwd(norm=...) /
# ops.maxpool_bwd(gskip_coef=...)).  TEM_DEFER_CONCAT_NORM=0 restores the in-place pass.
_DEFER_CONCAT_NORM = os.environ.get("TEM_DEFER_CONCAT_NORM", "1") != "0"
# norm backward + ReLU mask in the epilogue of the data-gradient kernel (ops.conv_fwd_refnorm); TEM_FUSE_NORM_BWD_DGRAD=0:
# the elementwise pass of ops.norm_bwd(sums=...)
_FUSE_NORM_BWD_DGRAD = os.environ.get("TEM_FUSE_NORM_BWD_DGRAD", "1") != "0"


def _norm_bwd_inplace(spec: ConvSpec, g, x, stats, relu_mask, grads: _Grads, sums=None, coef=None, coef_only=False, amax=False):
    """coef_only: return the [N, C, 4] coefficients instead of applying them (g stays the raw data gradient); `coef`: the
    weight gradient behind `sums` finished them already (_wgrad)
    amax: a weight gradient reads the rewritten g next -- the elementwise pass delivers max |g| (_amax_slot): returned"""
    groups, gamma, beta, _ = spec.norm_args()
    dgamma = grads.view(gamma) if gamma is not None else None
    dbeta = grads.view(beta) if beta is not None else None
    if coef_only:
        assert stats.per_sample
        if coef is not None:
            return coef
        return ops.norm_bwd_coef(g, x, groups, gamma, stats.mean, stats.rstd, dgamma, dbeta, sums=sums)
    if stats.mode == "frozen":
        raise NotImplementedError("backward through a norm with frozen running statistics (model.eval()) is not "
                                  "supported; call model.train() for training")
    if stats.mode == "batch":
        gb = _flat_batch(g)
        ops.norm_bwd(gb, _flat_batch(x), groups, gamma, stats.mean, stats.rstd, relu_mask, gb, dgamma, dbeta)
        return None
    slot = _amax_slot(grads if amax else None)
    ops.norm_bwd(g, x, groups, gamma, stats.mean, stats.rstd, relu_mask, g, dgamma, dbeta, sums=sums, out_amax=slot)
    return slot


def _norm2_in_dgrad_ok(bs: BlockState, gout, ga1, need_ga1: bool) -> bool:
    """weight gradient of conv2 first (it delivers the sums of norm2's backward), norm2's backward in the data-gradient epilogue"""
    c2, a1 = bs.c2, bs.a1
    return bs.s2 is not None and _FUSE_NORM_BWD_DGRAD and bs.s2.per_sample and need_ga1 and c2.conv.bias is not None and \
        ops.conv_wgrad_sums_ok(a1, c2.k, c2.cin, c2.cout, c2.packed().wgrad) and \
        ops.conv_fwd_family(gout, c2.k, c2.cout, c2.cin, c2.packed().dgrad.mode, y=ga1, ref=a1) == 3


def _norm2_in_wgrad1_ok(bs: BlockState) -> bool:
    """first block of the net (nothing but conv1's weight gradient reads ga1): that kernel applies norm2's backward on load"""
    c1 = bs.c1
    return _DEFER_CONCAT_NORM and bs.s2.per_sample and c1.conv.bias is not None and \
        ops.conv_wgrad_gnorm_ok(c1.k, c1.cin, c1.cout, c1.packed().wgrad)


def _block_bwd(bs: BlockState, gout, gout_amax, gin, grads: _Grads, defer_input_norm=False):
    """gout: gradient w.r.t. the block's pre-ReLU conv2 output (i.e. already ReLU-masked); gout_amax: max |gout| from the
    kernel that wrote it (_amax_slot) or None.
    gin: buffer for the gradient w.r.t. the block input, or None when not needed.
    defer_input_norm: leave the backward of the block's FIRST norm to the consumers of gin: returns its coefficients
    ([N, C, 4], see _DEFER_CONCAT_NORM) and gin holds the raw data gradient; returns None when it was applied here."""
    c1, c2, xin, a1, s1, s2 = bs.c1, bs.c2, bs.xin, bs.a1, bs.s1, bs.s2
    ga1 = torch.empty_like(a1)
    ga1_amax = None
    affine1 = s1 is not None and c1.norm_args()[1] is not None
    only_dw1 = gin is None and not affine1    # nothing but conv1's weight gradient reads ga1
    if _norm2_in_dgrad_ok(bs, gout, ga1, not only_dw1):
        # The weight gradient runs FIRST and delivers the sums of norm2's backward (ops.conv_wgrad(sums_from=...)) without the data
        # gradient existing yet; with the coefficients known, the data-gradient kernel applies norm2's backward and the
        # ReLU mask of a1 in its epilogue: no elementwise pass over ga1 and a1 (0.28 ms at 2 x 128^3 x 32)
        sums, coef = _wgrad(c2, a1, gout, grads, s2, want_sums=True, amax=gout_amax)
        coef = _norm_bwd_inplace(c2, gout, a1, s2, True, grads, sums=sums, coef=coef, coef_only=True)
        _, ga1_amax = _dgrad(c2, gout, ga1, ref=a1, refnorm=coef, grads=grads)
    elif s2 is not None:
        dsums, _ = _dgrad(c2, gout, ga1, sums_for=(a1, s2))
        sums, coef = _wgrad(c2, a1, gout, grads, s2, want_sums=True, amax=gout_amax)
        if sums is None:
            sums = dsums
        if only_dw1 and _norm2_in_wgrad1_ok(bs):
            # no pass that rewrites ga1: conv1's weight gradient applies norm2's backward (+ the ReLU mask of a1) while it loads g
            coef = _norm_bwd_inplace(c2, ga1, a1, s2, True, grads, sums=sums, coef=coef, coef_only=True)
            ops.conv_wgrad_gnorm(xin, ga1, a1, coef, c1.k, c1.cin, c1.cout, grads.view(c1.conv.weight),
                                 grads.view(c1.conv.bias), scale=None if s1 is None else s1.scale,
                                 shift=None if s1 is None else s1.shift)
            return None
        ga1_amax = _norm_bwd_inplace(c2, ga1, a1, s2, True, grads, sums=sums, amax=True)  # a1 is a ReLU output: mask fused
    else:
        _dgrad(c2, gout, ga1, ref=a1)
        _wgrad(c2, a1, gout, grads, s2, amax=gout_amax)
    if only_dw1:
        _wgrad(c1, xin, ga1, grads, s1, amax=ga1_amax)
        return None
    if gin is None:
        N, D, H, W, _ = xin.shape
        gin = ops.new_act(N, D, H, W, c1.cin, xin.device, xin.dtype)
    dsums, _ = _dgrad(c1, ga1, gin, sums_for=(xin, s1) if s1 is not None else None)
    sums, coef = _wgrad(c1, xin, ga1, grads, s1, want_sums=s1 is not None, amax=ga1_amax)
    if sums is None:
        sums = dsums
    if s1 is not None:
        if defer_input_norm and _DEFER_CONCAT_NORM and s1.per_sample:
            return _norm_bwd_inplace(c1, gin, xin, s1, False, grads, sums=sums, coef=coef, coef_only=True)
        _norm_bwd_inplace(c1, gin, xin, s1, False, grads, sums=sums)
    return None


# -----------------------------------------------------------------------------------
# whole network
# -----------------------------------------------------------------------------------
def _dim_of(model) -> int:
    conv = model.encoder.blocks[0].block[1] if model.encoder.blocks[0].norm is not None else \
        model.encoder.blocks[0].block[0]
    return 2 if isinstance(conv, nn.Conv2d) else 3


def _forward_impl(model, x: torch.Tensor, keep: bool):
    prev, _TLS.no_grad_forward = _TLS.no_grad_forward, not keep
    try:
        return _forward_impl_body(model, x, keep)
    finally:
        _TLS.no_grad_forward = prev


def _forward_impl_body(model, x: torch.Tensor, keep: bool):
    dim = _dim_of(model)
    if x.dim() != dim + 2:
        raise ValueError(f"expected a {dim + 2}-D input [N, C, *spatial], got shape {tuple(x.shape)}")
    if x.shape[1] != model.in_channels:
        raise ValueError(f"expected {model.in_channels} input channels, got {x.shape[1]}")
    enc, dec = model.encoder, model.decoder
    depth = len(enc)
    xin = ops.nchw_to_nhwc(x.float())
    N = xin.shape[0]
    dev = xin.device
    adt = act_dtype()   # fp32, or the 16-bit storage type of the mixed modes (the network input and the prediction stay fp32)
    levels, stages = [], []
    cur = xin
    cur_part = None   # first-stage statistics of `cur` from the kernel that produced it (the max-pool), if any
    for l in range(depth):
        blk = enc.blocks[l]
        f = _f3(enc.scale_factors[l], dim)
        c_up = dec.samplers[depth - 1 - l].conv.out_channels
        _, D, H, W, _ = cur.shape
        floor = bool(D % f[0] or H % f[1] or W % f[2])
        if floor and getattr(model, "check_shape", True):
            raise ValueError(f"Invalid shape for U-Net: {(D, H, W)[3 - dim:]} is not divisible by {f[3 - dim:]}")
        if _planar_concat_ok(adt, c_up, blk, dec.blocks[depth - 1 - l], (N, D, H, W), dev, floor):
            cat = ops.Planar.empty(N, D, H, W, dev, adt)   # two dense 32-channel planes (16-bit storage: whole lines per half)
            skip = cat.halves[1]
        else:
            cat = ops.new_act(N, D, H, W, c_up + blk.out_channels, dev, adt)
            skip = cat[..., c_up:]
        # the skip tensor feeds the norm in front of the decoder block of this level: its statistics come out of the
        # epilogue of this block's second conv (with the upsampled half's from the low-resolution tensor, see below)
        dnorm = dec.blocks[depth - 1 - l].conv_specs()[0].norm
        bs = _block_fwd(blk, cur, skip, out_stats=_FUSE_STATS and _FUSE_CONCAT_STATS and _norm_is_live(dnorm), in_partials=cur_part)
        pooled = ops.new_act(N, D // f[0], H // f[1], W // f[2], blk.out_channels, dev, adt)
        lv = Level(cat, skip, bs, f, c_up)
        if floor:
            # model.check_shape = False and a size the factor does not divide: nn.MaxPool3d drops the remainder.  The pooling
            # kernels take whole windows, so they get a dense copy of the covered sub-volume (not the fast path; the
            # decoder then crops this level's skip tensor, reference Decoder._crop)
            lv.floor_sub = skip[:, :D // f[0] * f[0], :H // f[1] * f[1], :W // f[2] * f[2]].contiguous()
            ops.maxpool_fwd(lv.floor_sub, pooled, f)
            cur_part = None
        else:
            # the statistics of the pooled tensor (norm of the next block's first conv) as a by-product of the pooling pass
            nxt = (enc.blocks[l + 1] if l + 1 < depth else model.base).conv_specs()[0].norm
            if _FUSE_STATS and _FUSE_POOL_STATS and _norm_is_live(nxt):
                cur_part = ops.maxpool_fwd(skip, pooled, f, want_stats=True)   # (partials, nblk) or None
            else:
                ops.maxpool_fwd(skip, pooled, f)
                cur_part = None
        levels.append(lv)
        cur = pooled
    _, D, H, W, _ = cur.shape
    base_out = ops.new_act(N, D, H, W, model.base.out_channels, dev, adt)
    base = _block_fwd(model.base, cur, base_out, in_partials=cur_part)
    cur = base_out
    for i in range(depth):
        lv = levels[depth - 1 - i]
        sampler, blk = dec.samplers[i], dec.blocks[i]
        f = _f3(dec.scale_factors[i], dim)
        if f != lv.f:
            raise ValueError("decoder scale factors must mirror the encoder's")
        sspec = ConvSpec(sampler.conv, None)
        _, d, h, w, _ = cur.shape
        t = ops.new_act(N, d, h, w, sspec.cout, dev, adt)
        _conv(sspec, cur, t)                       # 1x1 conv at low resolution ...
        cat = lv.cat
        up_sp, sk_sp = (d * f[0], h * f[1], w * f[2]), tuple(cat.shape[1:4])
        cropped = up_sp != sk_sp
        if cropped:
            # reference Decoder._crop (model/unet.py:363-373; reachable with model.check_shape = False only): the skip tensor
            # is centre-cropped by (difference // 2) per side.  Not the fast path: the concat buffer the encoder wrote into
            # has the skip's shape, so a second one with the upsampled shape receives a copy of the cropped skip half, and
            # its statistics / the backward of its norm take the plain (unfused) route.
            diff = [a - b_ for a, b_ in zip(sk_sp, up_sp)]
            if any(v < 0 or v % 2 for v in diff):
                raise RuntimeError(f"Sizes of tensors must match except in dimension 1: the upsampled tensor is {up_sp}, the "
                                   f"skip connection {sk_sp} (Decoder._crop removes (difference // 2) per side, which only "
                                   "fits even differences; the reference fails in torch.cat the same way)")
            off = [v // 2 for v in diff]
            cat = ops.new_act(N, up_sp[0], up_sp[1], up_sp[2], lv.cat.shape[4], dev, adt)
            cat[..., lv.c_up:] = lv.skip[:, off[0]:off[0] + up_sp[0], off[1]:off[1] + up_sp[1], off[2]:off[2] + up_sp[2]]
            lv.cat_c, lv.crop = cat, off
        # statistics of the concat for the block's first norm without reading it: the skip half's partial sums were
        # written by the encoder conv that produced it, the upsampled half's come out of the upsampling kernel (factor 2:
        # ops.upsample_fwd(stats=True)) or follow from the low-resolution t (sum y = sum (U^T 1) t, sum y^2 = sum t (U^T U t):
        # ops.upsample_stats)
        p2 = None
        skip_part = None if cropped else lv.bs.out_part
        want_stats = False
        if skip_part is not None:
            na = blk.conv_specs()[0].norm_args()
            cpg = cat.shape[4] // na[0]
            want_stats = lv.c_up % cpg == 0 and ops.upsample_stats_ok(t)
        up_part = ops.upsample_fwd(t, _half(cat, lv.c_up, 0), f, stats=want_stats)  # ... interpolated straight into the concat buffer
        out = ops.new_act(N, cat.shape[1], cat.shape[2], cat.shape[3], blk.out_channels, dev, adt)
        if want_stats:
            p2 = (up_part if up_part is not None else ops.upsample_stats(t, f), skip_part[0])
        bs = _block_fwd(blk, cat, out, in_partials2=p2)
        stages.append(DecStage(cur, sspec, bs, f, out, t))
        cur = out
    act = fused_activation(model.final_activation) if model.final_activation is not None else None

    def step(y, ospec=None, side=None):
        return Step(levels, stages, base, cur, act, y, dim, tuple(x.shape), ospec, side) if keep else None

    if isinstance(model.out_conv, nn.ModuleList):
        # return_side_outputs (reference model/unet.py:211-228): a 1x1 conv (+ activation) on every decoder level
        if act == "sigmoid" and any(c is None for c in model.out_conv):
            raise NotImplementedError("final Sigmoid without out_conv is not supported")
        side = []
        for i, conv in enumerate(model.out_conv):
            if conv is None:
                raise NotImplementedError("side outputs without an output convolution are not supported")
            feat = stages[i].out
            ospec = ConvSpec(conv, None)
            yi = ops.new_act(N, feat.shape[1], feat.shape[2], feat.shape[3], ospec.cout, dev)
            _conv(ospec, feat, yi, act=act)
            side.append(SideOut(ospec, yi))
        return [sd.y for sd in side][::-1], step(side[-1].y, side=side)  # full resolution first
    ospec = None
    if model.out_conv is not None:
        ospec = ConvSpec(model.out_conv, None)
        y = ops.new_act(N, cur.shape[1], cur.shape[2], cur.shape[3], ospec.cout, dev)
        _conv(ospec, cur, y, act=act)
    else:
        y = cur if cur.dtype == torch.float32 else cur.float()   # the prediction is fp32 in every mode
        if act == "sigmoid":
            raise NotImplementedError("final Sigmoid without out_conv is not supported")
    return y, step(y, ospec)


def _to_logical(y5: torch.Tensor, dim: int) -> torch.Tensor:
    """NDHWC buffer -> logical [N, C, *spatial] view (channels_last memory format, no copy)."""
    y = y5.permute(0, 4, 1, 2, 3)
    return y[:, :, 0] if dim == 2 else y


def _from_logical(g: torch.Tensor, dim: int) -> torch.Tensor:
    """logical [N, C, *spatial] gradient -> contiguous NDHWC buffer (free if it already is one)."""
    if dim == 2:
        g = g.unsqueeze(2)
    g5 = g.permute(0, 2, 3, 4, 1)
    if g5.is_contiguous():
        return g5
    return ops.nchw_to_nhwc(g.contiguous())


def _backward_impl(model, st: Step, gy: torch.Tensor, params: List[torch.Tensor], need_input_grad: bool):
    dim = st.dim
    depth = len(st.levels)
    grads = _Grads(params)
    sync = getattr(model, "_tem_grad_sync", None)  # data-parallel gradient exchange (multi_gpu_training.DDP)

    def stage_done():
        if sync is not None:
            for lo, hi in grads.take_new_ranges():
                sync.ready(grads.flat, lo, hi)

    side, ospec = st.side, st.ospec
    side_g = None
    if side is not None:
        # gy: gradients of the side outputs, full resolution first -> decoder order (coarse .. fine)
        side_g = list(gy)[::-1]
        gy = side_g[-1]
        ospec = side[-1].ospec
        if gy is None:
            gy = torch.zeros_like(_to_logical(side[-1].y, dim))

    def side_grad(i, feat):
        """dL/d(decoder level i output) through its side conv (ReLU-masked like every gradient of a block output)."""
        gi = side_g[i]
        if gi is None:
            return None
        gs = _from_logical(gi.float(), dim)
        if st.act is not None:
            gs = ops.act_bwd(gs, side[i].y, st.act)
        out = torch.empty_like(feat)
        _dgrad(side[i].ospec, gs, out, ref=feat)
        _wgrad(side[i].ospec, feat, gs, grads)
        return out

    g = _from_logical(gy.float(), dim)
    if st.act is not None:
        g = ops.act_bwd(g, st.y, st.act)
    last = st.last
    g_cur = torch.empty_like(last)
    g_amax = None    # max |g_cur| from the kernel that wrote g_cur (_amax_slot), None once g_cur is modified
    if ospec is not None:
        if _FUSE_OUT_BWD and not _FORCE_GENERIC and ospec.k == (1, 1, 1) and ospec.conv.weight.is_contiguous() and \
                ops.conv1x1_out_bwd_ok(ospec.cin, ospec.cout):
            # weight / bias gradient of out_conv and its masked data gradient in one pass over `last`
            g_amax = _amax_slot(grads)
            ops.conv1x1_out_bwd(last, g, ospec.conv.weight, g_cur, grads.view(ospec.conv.weight),
                                grads.view(ospec.conv.bias) if ospec.conv.bias is not None else None, out_amax=g_amax)
        else:
            _, g_amax = _dgrad(ospec, g, g_cur, ref=last, grads=grads)
            _wgrad(ospec, last, g, grads)
    else:
        ops.maxpool_bwd(g.to(last.dtype), last, g_cur, (1, 1, 1), relu_mask=True)
    g_skip, g_skip_coef = [None] * depth, [None] * depth   # per level: the decoder's gradient of the skip tensor
    for i in reversed(range(depth)):
        d = st.dec[i]
        l = depth - 1 - i
        lv = st.levels[l]
        g_cat = _like(lv.cat if lv.crop is None else lv.cat_c)
        coef = _block_bwd(d.bs, g_cur, g_amax, g_cat, grads, defer_input_norm=lv.crop is None)
        low, sspec = d.low, d.sspec
        g_t = ops.new_act(low.shape[0], low.shape[1], low.shape[2], low.shape[3], sspec.cout, low.device, low.dtype)
        ops.upsample_bwd(_half(g_cat, lv.c_up, 0), g_t, d.f,
                         norm=None if coef is None else (d.t, coef[:, :lv.c_up]))
        g_skip_coef[l] = None if coef is None else coef[:, lv.c_up:]
        g_low = torch.empty_like(low)
        _, g_amax = _dgrad(sspec, g_t, g_low, ref=low, grads=grads)  # `low` is the ReLU output of the previous block
        _wgrad(sspec, low, g_t, grads)
        if side is not None and i > 0:
            extra = side_grad(i - 1, low)  # `low` is decoder level i-1's output
            if extra is not None:
                g_low.add_(extra)
                g_amax = None
        g_skip[l] = _half(g_cat, lv.c_up, 1)
        if lv.crop is not None:   # the adjoint of the centre crop: zeros around the gradient of the cropped window
            o, sk = lv.crop, lv.skip
            gs = torch.zeros(sk.shape, dtype=sk.dtype, device=sk.device)
            gs[:, o[0]:o[0] + g_cat.shape[1], o[1]:o[1] + g_cat.shape[2], o[2]:o[2] + g_cat.shape[3]] = g_skip[l]
            g_skip[l] = gs
        g_cur = g_low
        stage_done()
    g_pooled = torch.empty_like(st.base.xin)
    # the input of this block (and of every encoder block below level 0) is a max-pooled tensor: the backward of its
    # first norm is applied by the max-pool backward that consumes the gradient (it recomputes the pooled value anyway)
    pool_coef = _block_bwd(st.base, g_cur, g_amax, g_pooled, grads, defer_input_norm=True)
    g_cur = g_pooled
    stage_done()
    for l in reversed(range(depth)):
        lv = st.levels[l]
        skip = lv.skip
        g_skip_full = ops.new_act(skip.shape[0], skip.shape[1], skip.shape[2], skip.shape[3], skip.shape[4],
                                  skip.device, skip.dtype)
        if lv.floor_sub is not None:
            # remainder voxels outside every pooling window only receive the (zero-padded, cropped) decoder gradient
            sub = lv.floor_sub
            g_sub = torch.empty_like(sub)
            ops.maxpool_bwd(g_cur, sub, g_sub, lv.f, gy_coef=pool_coef)
            g_skip_full.copy_(g_skip[l])
            g_skip_full[:, :sub.shape[1], :sub.shape[2], :sub.shape[3]] += g_sub
            g_skip_full.mul_(skip > 0)
            g_amax = None
        else:
            g_amax = _amax_slot(grads)
            ops.maxpool_bwd(g_cur, skip, g_skip_full, lv.f, gskip=g_skip[l], relu_mask=True,
                            gskip_coef=g_skip_coef[l], gy_coef=pool_coef, out_amax=g_amax)
        need_in = (l > 0) or need_input_grad
        g_in = torch.empty_like(lv.bs.xin) if need_in else None
        pool_coef = _block_bwd(lv.bs, g_skip_full, g_amax, g_in, grads, defer_input_norm=l > 0)
        g_cur = g_in
        stage_done()
    if sync is not None:
        sync.finish(grads.flat)
    gx = None
    if need_input_grad:
        gx = ops.nhwc_to_nchw(g_cur)
        if dim == 2:
            gx = gx[:, :, 0]
    return gx, grads


class UNetFunction(torch.autograd.Function):
    """y = UNet(x; params) as a single autograd node (see the module docstring)."""

    @staticmethod
    def forward(ctx, model, x, *params):
        need_grad = any(ctx.needs_input_grad[1:])
        y5, st = _forward_impl(model, x, keep=need_grad)
        ctx.model, ctx.st, ctx.nparams = model, st, len(params)
        # `params` are the autograd inputs -- the module's parameters, or fresh leaves that alias them (fresh_leaves());
        # the engine itself always works on the module's own parameter objects (gradient arena keyed by their identity)
        ctx.params = list(model.parameters())
        assert len(ctx.params) == len(params)
        if isinstance(y5, list):
            return tuple(_to_logical(y, _dim_of(model)) for y in y5)
        return _to_logical(y5, _dim_of(model))

    @staticmethod
    def backward(ctx, *gys):
        gy = gys if len(gys) > 1 or isinstance(ctx.model.out_conv, nn.ModuleList) else gys[0]
        st = ctx.st
        if st is None:
            raise RuntimeError("UNetFunction.backward called twice (activations were released)")
        gx, grads = _backward_impl(ctx.model, st, gy, ctx.params, ctx.needs_input_grad[1])
        ctx.st = None  # release activations
        if ctx.params:
            ctx.params[0]._tem_grad_flat = grads.flat  # lets FusedAdamW / GradSync find the arena (arena.py)
        out = [None, gx]
        for i, p in enumerate(ctx.params):
            if ctx.needs_input_grad[2 + i]:
                out.append(grads.view(p, track=False))
            else:
                out.append(None)
        return tuple(out)


_LEAF_SINK = None


class fresh_leaves:
    """`with fresh_leaves() as pairs:` -- every U-Net forward inside takes its parameters through NEW leaf tensors that
    alias them (`p.detach().requires_grad_()`), and appends (parameters, leaves) to `pairs`; the caller obtains the
    gradients with `torch.autograd.grad(loss, leaves)` and assigns them.  For HIP-graph capture (torch_em_amd/graph.py):
    a parameter's own AccumulateGrad node lives on the stream it was created on for as long as ANY autograd graph that
    used the parameter is alive (a loss tensor the caller kept from an eager step is enough); delivering a gradient to it
    from the capturing stream is an unjoined cross-stream dependency, and hipStreamEndCapture crashes the process.  New
    leaves get new nodes on the capturing stream."""

    def __enter__(self):
        global _LEAF_SINK
        self.prev, self.pairs = _LEAF_SINK, []
        _LEAF_SINK = self.pairs
        return self.pairs

    def __exit__(self, *exc):
        global _LEAF_SINK
        _LEAF_SINK = self.prev
        return False


def unet_forward(model, x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError(
            "torch_em_amd.model runs on MI355X only (input is a CPU tensor). There is no CPU fallback for this "
            "path; move model and data to 'cuda' or use the reference torch_em on CPU."
        )
    params = [p for p in model.parameters()]
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        inputs = params
        if _LEAF_SINK is not None:
            inputs = [p.detach().requires_grad_(True) if p.requires_grad else p for p in params]
            _LEAF_SINK.append((params, inputs))
        out = UNetFunction.apply(model, x, *inputs)
        return list(out) if isinstance(out, tuple) else out
    y5, _ = _forward_impl(model, x, keep=False)
    if isinstance(y5, list):
        return [_to_logical(y, _dim_of(model)) for y in y5]
    return _to_logical(y5, _dim_of(model))


def run_single_block(block, x):
    raise NotImplementedError(
        "ConvBlock modules of torch_em_amd are parameter containers driven by the U-Net engine; "
        "stand-alone calls are not supported"
    )
