"""Loss and metric wrappers of self-training (reference torch_em/self_training/loss.py:9-85).

Both take `(model, input_, labels, label_filter=None)`, run the model and compare its prediction with the (pseudo) labels
through an inner loss.  The reference applies a label filter as two products, `loss(prediction * filter, labels * filter)`.
When the inner loss is this package's `DiceLoss` the filter goes to the Dice kernels as their multiplicative mask instead --
the same value and gradient, and the two products never exist in HBM.  Any other inner loss gets the reference's products.

`DefaultSelfTrainingLossAndMetric` under `torch.no_grad()` (validation), with loss and metric both `DiceLoss` of equal
settings: masked loss and unmasked metric come from ONE pass over the prediction (`dice_loss_pair`, tem_dice_sums_pair).

Below them, the four classes of the trainers with invertible augmentations (reference `:171-406`), which take the prediction
instead of (model, input): `SelfTrainingLossWithInvertibleAugmentations`, `SelfTrainingLossAndMetricWithInvertibleAugmentations`,
`UniMatchv2Loss`, `UniMatchv2LossAndMetric`.
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

    def _pair(self, prediction, labels, label_filter):
        """(filtered loss, unfiltered metric) of an activated prediction"""
        if self._one_pass(prediction, label_filter):
            return dice_loss_pair(prediction, labels, _as_mask(label_filter, labels), **self.loss.init_kwargs)
        return _filtered(self.loss, prediction, labels, label_filter), self.metric(prediction, labels)

    def __call__(self, model, input_, labels, label_filter=None):
        prediction = model(input_)
        if self.activation is not None:
            prediction = self.activation(prediction)
        return self._pair(prediction, labels, label_filter)


# ---- the variants of the trainers with invertible augmentations (reference `:171-406`) -------------------------------------
# They take the PREDICTION, already mapped back into the common frame by the trainer, not (model, input).  The label filter
# goes to the Dice kernels as their mask, as above.  `pred_dim=2`: the prediction is the stack [2, B, C, ...] of the two
# strong views of UniMatch v2, and loss and metric are the means over the two (two Dice reductions; a fused two-view
# reduction is not built).
class SelfTrainingLossWithInvertibleAugmentations(nn.Module):
    """loss(prediction, labels), both multiplied by `label_filter` if given (reference `:171-215`)."""

    def __init__(self, loss: Optional[nn.Module] = None, activation: Optional[nn.Module] = None):
        super().__init__()
        self.activation = activation
        self.loss = DiceLoss() if loss is None else loss
        self.init_kwargs = {}

    def __call__(self, prediction: torch.Tensor, labels: torch.Tensor, label_filter: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.activation is not None:
            prediction = self.activation(prediction)
        return _filtered(self.loss, prediction, labels, label_filter)


class SelfTrainingLossAndMetricWithInvertibleAugmentations(DefaultSelfTrainingLossAndMetric):
    """(filtered loss, unfiltered metric) of a prediction (reference `:218-269`); one pass over it under `no_grad` when loss
    and metric are `DiceLoss` of equal settings, as in `DefaultSelfTrainingLossAndMetric`."""

    def __call__(self, prediction: torch.Tensor, labels: torch.Tensor, label_filter: Optional[torch.Tensor] = None):
        if self.activation is not None:
            prediction = self.activation(prediction)
        return self._pair(prediction, labels, label_filter)


def _check_pred_dim(prediction, pred_dim):
    assert pred_dim in (1, 2), "pred_dim must be either 1 or 2"
    if pred_dim == 2:
        assert len(prediction) == 2, "only implemented for list of len 2"


class UniMatchv2Loss(SelfTrainingLossWithInvertibleAugmentations):
    """`pred_dim=1`: as `SelfTrainingLossWithInvertibleAugmentations`; `pred_dim=2`: the mean of the loss of the two stacked
    student predictions against the shared pseudo labels (reference `:272-332`)."""

    def __call__(self, prediction, labels, label_filter=None, pred_dim: int = 1) -> torch.Tensor:
        _check_pred_dim(prediction, pred_dim)
        if self.activation is not None:
            prediction = self.activation(prediction)
        if pred_dim == 1:
            return _filtered(self.loss, prediction, labels, label_filter)
        return (_filtered(self.loss, prediction[0], labels, label_filter) + _filtered(self.loss, prediction[1], labels, label_filter)) / 2


class UniMatchv2LossAndMetric(SelfTrainingLossAndMetricWithInvertibleAugmentations):
    """(loss, metric) as `UniMatchv2Loss`, the metric unfiltered and averaged over the views too (reference `:335-406`)."""

    def __call__(self, prediction, labels, label_filter=None, pred_dim: int = 1):
        if self.activation is not None:
            prediction = self.activation(prediction)
        _check_pred_dim(prediction, pred_dim)
        if pred_dim == 1:
            return self._pair(prediction, labels, label_filter)
        (l0, m0), (l1, m1) = self._pair(prediction[0], labels, label_filter), self._pair(prediction[1], labels, label_filter)
        return (l0 + l1) / 2, (m0 + m1) / 2
