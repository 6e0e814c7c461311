"""Losses for distance-based instance segmentation (reference loss/distance_based.py).

`DistanceLoss` and `DiceBasedDistanceLoss` keep the reference's constructor signatures, `init_kwargs` and shape asserts:
a 3-channel prediction (foreground, center distance, boundary distance) against the targets of
`transform.PerObjectDistanceTransform(instances=False, directed_distances=False)`.  The arithmetic runs in
libtem_hip.so: one pass reads the six channels once for every sum (tem_dist_loss_fwd, fixed-order double reduction,
bitwise reproducible), one launch writes the whole input gradient (tem_dist_loss_grad), one autograd node.

Supported compositions -- the two the reference uses: `foreground_loss` a DiceLoss, `distance_loss` a DiceLoss or
`nn.MSELoss(reduction="mean")`.  Anything else raises `NotImplementedError`.
"""
import torch
import torch.nn as nn

from .. import ops
from .dice import DiceLoss


def _dice_eps(loss: nn.Module, role: str) -> float:
    """eps of a DiceLoss term (ours, or torch-em's with the same attributes); on a one-channel slice every channel
    reduction gives the same value, only the per-channel tensor of reduce_channel=None differs"""
    if type(loss).__name__ == "DiceLoss" and hasattr(loss, "eps") and getattr(loss, "reduce_channel", None) is not None:
        return float(loss.eps)
    raise NotImplementedError(f"DistanceLoss: {role} {loss!r} is not supported on the MI355X path: use DiceLoss() (a "
                              "channel reduction other than None)" + (" or nn.MSELoss(reduction='mean')"
                                                                      if role == "distance_loss" else ""))


class _DistanceLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_, target, mask_bg, mse, eps_fg, eps_dist):
        loss, coef, p, t = ops.dist_loss_fwd(input_, target, mask_bg, mse, eps_fg, eps_dist)
        ctx.save_for_backward(p, t, coef)
        ctx.mask_bg = mask_bg
        return loss

    @staticmethod
    def backward(ctx, gout):
        p, t, coef = ctx.saved_tensors
        gp = ops.dist_loss_grad(p, t, coef, gout.contiguous().float().reshape(1), ctx.mask_bg)
        return gp, None, None, None, None, None


class DistanceLoss(nn.Module):
    """foreground loss + center-distance loss + boundary-distance loss (reference loss/distance_based.py:7-62)."""

    def __init__(self, mask_distances_in_bg: bool = True, foreground_loss: nn.Module = DiceLoss(),
                 distance_loss: nn.Module = nn.MSELoss(reduction="mean")) -> None:
        super().__init__()
        self.foreground_loss = foreground_loss
        self.distance_loss = distance_loss
        self.mask_distances_in_bg = mask_distances_in_bg
        self.init_kwargs = {"mask_distances_in_bg": mask_distances_in_bg}
        self._eps_fg = _dice_eps(foreground_loss, "foreground_loss")
        if isinstance(distance_loss, nn.MSELoss):
            if distance_loss.reduction != "mean":
                raise NotImplementedError("DistanceLoss: nn.MSELoss supported with reduction='mean' only")
            self._mse, self._eps_dist = True, 0.0
        else:
            self._mse, self._eps_dist = False, _dice_eps(distance_loss, "distance_loss")

    def forward(self, input_: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        assert input_.shape == target.shape, input_.shape
        assert input_.shape[1] == 3, input_.shape
        if not input_.is_cuda:
            raise RuntimeError("torch_em_amd.loss runs on MI355X only (got CPU tensors); there is no CPU fallback")
        return _DistanceLossFunction.apply(input_.to(torch.float32), target.to(torch.float32),
                                           bool(self.mask_distances_in_bg), self._mse, self._eps_fg, self._eps_dist)


class DiceBasedDistanceLoss(DistanceLoss):
    """DistanceLoss with the Dice loss for all three terms (reference loss/distance_based.py:65-75)."""

    def __init__(self, mask_distances_in_bg: bool) -> None:
        super().__init__(mask_distances_in_bg, foreground_loss=DiceLoss(), distance_loss=DiceLoss())
