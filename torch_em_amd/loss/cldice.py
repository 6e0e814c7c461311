"""clDice losses for the MI355X path (reference loss/cldice.py; https://arxiv.org/abs/2003.07311).

Drop-in for `torch_em.loss.cldice`: `SoftSkeletonize` (:11-70), `cldice_score` (:73-108), `SoftclDiceLoss` (:111-161),
`CombinedclDiceLoss` (:166-216) -- same signatures, defaults, `init_kwargs` and `ValueError`s.  The soft skeleton is an
iterated 3-D (or 2-D) stencil; here every round is one fused launch of libtem_hip.so (csrc/cldice.hip) and the
backward is written in gather form with PyTorch's tie rules (first extremum for the pools, half / half for
`torch.min(a, b)` on equality, strict `> 0` for the ReLUs), so it is bitwise reproducible.  Prediction and target are
read in place through their strides (NDHWC, NCDHW, channel-sliced views).  Inputs are assumed finite.
"""
import torch
import torch.nn as nn

from .. import ops
from .dice import _is_channels_last, dice_score


def _prepare(input_: torch.Tensor) -> torch.Tensor:
    if input_.dim() not in (4, 5):
        raise ValueError(f"Expect a 4d [N,C,H,W] or 5d [N,C,D,H,W] tensor, got: {input_.shape}.")
    if not input_.is_cuda:
        raise RuntimeError("torch_em_amd.loss runs on MI355X only (got CPU tensors); there is no CPU fallback")
    return input_.to(torch.float32)


class _MorphFunction(torch.autograd.Function):
    """soft_erode / soft_dilate / soft_open: one fused launch forward, gather-form backward"""

    @staticmethod
    def forward(ctx, input_, mode):
        out, e1 = ops.cldice_morph(input_, mode)
        ctx.save_for_backward(input_, e1)
        ctx.mode, ctx.cl = mode, _is_channels_last(input_)
        return out

    @staticmethod
    def backward(ctx, gout):
        input_, e1 = ctx.saved_tensors
        return ops.cldice_morph_bwd(input_, e1, gout, ctx.mode, ctx.cl), None


class _SkelFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_, num_iter):
        need = ctx.needs_input_grad[0]
        skel, saved = ops.cldice_skel_fwd(input_, num_iter, need)
        if need:
            ctx.save_for_backward(*saved)
        ctx.cl = _is_channels_last(input_)
        return skel

    @staticmethod
    def backward(ctx, gout):
        return ops.cldice_skel_bwd(ctx.saved_tensors, gout.contiguous(), ctx.cl), None


class SoftSkeletonize(nn.Module):
    """Differentiable approximation of skeletonisation by iterated min- and max-pooling (reference :11-70).

    Args:
        num_iter: Number of iterations; should be at least the largest radius in the data.
    """

    def __init__(self, num_iter: int = 5):
        super().__init__()
        self.num_iter = num_iter

    def soft_erode(self, input_: torch.Tensor) -> torch.Tensor:
        return _MorphFunction.apply(_prepare(input_), ops.CLD_ERODE)

    def soft_dilate(self, input_: torch.Tensor) -> torch.Tensor:
        return _MorphFunction.apply(_prepare(input_), ops.CLD_DILATE)

    def soft_open(self, input_: torch.Tensor) -> torch.Tensor:
        return _MorphFunction.apply(_prepare(input_), ops.CLD_OPEN)

    def soft_skel(self, input_: torch.Tensor) -> torch.Tensor:
        return _SkelFunction.apply(_prepare(input_), self.num_iter)

    def forward(self, input_: torch.Tensor) -> torch.Tensor:
        return self.soft_skel(input_)


class _ClDiceFunction(torch.autograd.Function):
    """The whole score as one autograd node: two skeletons, one pass for the four sums, a device-side finalise; the
    backward seeds the skeleton backward with coef_a * t + coef_b and adds the direct part coef * skel_t."""

    @staticmethod
    def forward(ctx, input_, target, num_iter, invert, eps):
        need = ctx.needs_input_grad[0]
        skel_t, _ = ops.cldice_skel_fwd(target, num_iter, False)
        skel_x, saved = ops.cldice_skel_fwd(input_, num_iter, need)
        out, coef, _ = ops.cldice_score_fwd(input_, target, skel_x, skel_t, eps, invert)
        if need:
            ctx.save_for_backward(*saved, target, skel_t, coef)
        ctx.cl = _is_channels_last(input_)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        x, estack, sstack, target, skel_t, coef = ctx.saved_tensors
        gp = ops.cldice_score_bwd((x, estack, sstack), target, skel_t, coef, gout.contiguous().float().reshape(1), ctx.cl)
        return gp, None, None, None, None


def cldice_score(input_: torch.Tensor, target: torch.Tensor, num_iter: int = 5, invert: bool = False,
                 eps: float = 1e-7) -> torch.Tensor:
    """Soft clDice score between input and target (reference :73-108): the harmonic mean of the topology precision
    <skel(input), target> / |skel(input)| and the topology sensitivity <skel(target), input> / |skel(target)|."""
    if input_.shape != target.shape:
        raise ValueError(f"Expect input and target of same shape, got: {input_.shape}, {target.shape}.")
    return _ClDiceFunction.apply(_prepare(input_), _prepare(target), int(num_iter), bool(invert), float(eps))


class SoftclDiceLoss(nn.Module):
    """1 - clDice score (reference :111-161).

    Args:
        num_iter: Number of iterations for soft-skeletonization.
        eps: The epsilon value added to the denominators for numerical stability.
        exclude_background: Whether to exclude channel 0 from the loss computation.
    """

    def __init__(self, num_iter: int = 5, eps: float = 1e-7, exclude_background: bool = False):
        super().__init__()
        self.num_iter = num_iter
        self.eps = eps
        self.exclude_background = exclude_background
        self.init_kwargs = {"num_iter": num_iter, "eps": eps, "exclude_background": exclude_background}

    def _slice(self, input_, target):
        if input_.shape != target.shape:
            raise ValueError(f"Expect input and target of same shape, got: {input_.shape}, {target.shape}.")
        if self.exclude_background:   # channel-strided views, read in place
            target = target[:, 1:, :, :]
            input_ = input_[:, 1:, :, :]
        return input_, target

    def forward(self, input_: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        input_, target = self._slice(input_, target)
        return cldice_score(input_, target, num_iter=self.num_iter, invert=True, eps=self.eps)


class CombinedclDiceLoss(SoftclDiceLoss):
    """(1 - alpha) * soft Dice loss + alpha * soft clDice loss (reference :166-216).

    Args:
        num_iter: Number of iterations for soft-skeletonization.
        alpha: The weight of the clDice term.
        eps: The epsilon value added to the denominators for numerical stability.
        exclude_background: Whether to exclude channel 0 from the loss computation.
    """

    def __init__(self, num_iter: int = 5, alpha: float = 0.5, eps: float = 1e-7, exclude_background: bool = False):
        super().__init__(num_iter=num_iter, eps=eps, exclude_background=exclude_background)
        self.alpha = alpha
        self.init_kwargs = {"num_iter": num_iter, "alpha": alpha, "eps": eps, "exclude_background": exclude_background}

    def forward(self, input_: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        input_, target = self._slice(input_, target)
        dice = dice_score(input_, target, invert=True, channelwise=False, eps=self.eps)
        cldice = cldice_score(input_, target, num_iter=self.num_iter, invert=True, eps=self.eps)
        return (1.0 - self.alpha) * dice + self.alpha * cldice
