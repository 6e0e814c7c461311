"""Weighted sum of several losses (reference loss/combined_loss.py); host-side composition only."""
from typing import List

import torch


class CombinedLoss(torch.nn.Module):
    """Combination of multiple losses.

    Args:
        losses: The loss functions to combine.
        loss_weights: The weights for the loss functions; equal weights summing to one by default.
    """

    def __init__(self, *losses: torch.nn.Module, loss_weights: List[float] = None):
        super().__init__()
        self.losses = torch.nn.ModuleList(losses)
        n_losses = len(self.losses)
        if loss_weights is None:
            self.loss_weights = [1.0 / n_losses] * n_losses if n_losses else None
        else:
            assert len(loss_weights) == n_losses
            self.loss_weights = loss_weights

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        assert self.loss_weights is not None
        return sum([loss(x, y) * weight for loss, weight in zip(self.losses, self.loss_weights)])
