"""Loss and metric wrappers of self-training (reference torch_em/self_training/loss.py:9-85).

Both take `(model, input_, labels, label_filter=None)`, run the model and compare its prediction with the (pseudo) labels
through an inner loss.  The reference applies a label filter as two products, `loss(prediction * filter, labels * filter)`.
When the inner loss is this package's `DiceLoss` the filter goes to the Dice kernels as their multiplicative mask instead --
the same value and gradient, and the two products never exist in HBM.  Any other inner loss gets the reference's products.

`DefaultSelfTrainingLossAndMetric` under `torch.no_grad()` (validation), with loss and metric both `DiceLoss` of equal
settings: masked loss and unmasked metric come from ONE pass over the prediction (`dice_loss_pair`, tem_dice_sums_pair).
"""
from typing import Optional

import torch
import torch.nn as nn

from ..loss.dice import DiceLoss, dice_loss_pair


def _as_mask(label_filter: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """float32 filter with the strides the Dice kernels will see for `labels` (they require mask and target to share them)"""
    m = label_filter.to(torch.float32)
    if m.shape != labels.shape or m.stride() != labels.stride():   # a dense tensor keeps its strides through .to(float32)
        m = torch.empty_like(labels, dtype=torch.float32).copy_(m.expand_as(labels))
    return m


def _filtered(loss, prediction, labels, label_filter):
    if label_filter is None:
        return loss(prediction, labels)
    if type(loss) is DiceLoss:
        return loss(prediction, labels, mask=_as_mask(label_filter, labels))
    return loss(prediction * label_filter, labels * label_filter)


class DefaultSelfTrainingLoss(nn.Module):
    """loss(model(input_), labels), both multiplied by `label_filter` if given (reference `:9-49`).

    Args:
        loss: the inner loss between the student's prediction and the (pseudo) labels.
        activation: applied to the prediction first.
    """

    def __init__(self, loss: Optional[nn.Module] = None, activation: Optional[nn.Module] = None):
        super().__init__()
        self.activation = activation
        self.loss = DiceLoss() if loss is None else loss
        self.init_kwargs = {}   # as in the reference: inner loss and activation are not serialised by name

    def __call__(self, model: nn.Module, input_: torch.Tensor, labels: torch.Tensor,
                 label_filter: Optional[torch.Tensor] = None) -> torch.Tensor:
        prediction = model(input_)
        if self.activation is not None:
            prediction = self.activation(prediction)
        return _filtered(self.loss, prediction, labels, label_filter)


class DefaultSelfTrainingLossAndMetric(nn.Module):
    """(filtered loss, unfiltered metric) from one run of the model (reference `:52-85`)."""

    def __init__(self, loss: Optional[nn.Module] = None, metric: Optional[nn.Module] = None,
                 activation: Optional[nn.Module] = None):
        super().__init__()
        self.activation = activation
        self.loss = DiceLoss() if loss is None else loss
        self.metric = DiceLoss() if metric is None else metric
        self.init_kwargs = {}

    def _one_pass(self, prediction, label_filter) -> bool:
        return label_filter is not None and type(self.loss) is DiceLoss and type(self.metric) is DiceLoss and \
            self.loss.init_kwargs == self.metric.init_kwargs and not (torch.is_grad_enabled() and prediction.requires_grad)

    def __call__(self, model, input_, labels, label_filter=None):
        prediction = model(input_)
        if self.activation is not None:
            prediction = self.activation(prediction)
        if self._one_pass(prediction, label_filter):
            return dice_loss_pair(prediction, labels, _as_mask(label_filter, labels), **self.loss.init_kwargs)
        return _filtered(self.loss, prediction, labels, label_filter), self.metric(prediction, labels)
