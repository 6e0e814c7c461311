"""Pseudo labelers for self-training on the MI355X path (reference torch_em/self_training/pseudo_labeling.py).

`DefaultPseudoLabeler` (`:7-75`) and `ScheduledPseudoLabeler` (`:160-397`) with the reference's signatures, `init_kwargs`,
`confidence_threshold` attribute and `step()`.  What follows the teacher's forward pass -- activation, the threshold compares,
the cast, the expansion of a shared mask -- is ONE streaming launch (`ops.pseudo_label`, csrc/selftrain.hip): labels and mask
come out in the memory layout of the teacher's prediction, which is what the masked Dice kernels read in place.

`activation` may be None, `nn.Sigmoid()` or `torch.sigmoid`: these run inside the kernel.  Any other callable is applied with
torch first and the kernel computes the mask only.

The reference's `mask_channel` slices the BATCH axis (`pseudo_labels[mask_channel:mask_channel + 1]`, `:65-71`): with
`mask_channel=k` every sample gets sample k's mask in all channels.  Reproduced as it is, like the SPOCO quirks.

The threshold schedule of `ScheduledPseudoLabeler` is host arithmetic on Python floats; it performs the reference's operations
in the reference's order, so the thresholds are the same doubles (tests/golden/g17_selftrain.npz).
"""
from typing import Callable, Literal, Optional, Union

import numpy as np
import torch

from .. import ops


def _kernel_activation(activation):
    """-> (name for ops.pseudo_label, callable to apply with torch first)"""
    if activation is None:
        return None, None
    if isinstance(activation, torch.nn.Sigmoid) or activation is torch.sigmoid or activation is torch.Tensor.sigmoid:
        return "sigmoid", None
    return None, activation


def _label(labeler, teacher, input_, mask_sample):
    prediction = teacher(input_)
    name, pre = _kernel_activation(labeler.activation)
    if pre is not None:
        prediction = pre(prediction)
    return ops.pseudo_label(prediction, name, labeler.confidence_threshold, labeler.threshold_from_both_sides, mask_sample)


class DefaultPseudoLabeler:
    """Pseudo labels from a (teacher) model's prediction, with an optional confidence mask (reference `:7-75`).

    confidence_threshold None: no mask.  threshold_from_both_sides: the mask keeps values >= threshold and values
    <= 1 - threshold (float32 0 / 1, for binary labels); otherwise only values >= threshold (bool, for multi-class labels).
    """

    def __init__(self, activation: Optional[torch.nn.Module] = None, confidence_threshold: Optional[float] = None,
                 threshold_from_both_sides: bool = True, mask_channel: Optional[int] = None):
        self.activation = activation
        self.confidence_threshold = confidence_threshold
        self.threshold_from_both_sides = threshold_from_both_sides
        self.mask_channel = mask_channel
        # the activation is not serialised, as in the reference
        self.init_kwargs = {"activation": None, "confidence_threshold": confidence_threshold,
                            "threshold_from_both_sides": threshold_from_both_sides, "mask_channel": mask_channel}

    def __call__(self, teacher: torch.nn.Module, input_: torch.Tensor):
        """-> (pseudo_labels, label_mask or None)"""
        return _label(self, teacher, input_, self.mask_channel)

    def step(self, metric, epoch):
        pass


class ScheduledPseudoLabeler:
    """Pseudo labeler whose confidence threshold follows a schedule (reference `:160-397`): lowered when a monitored metric
    stops improving (`increase=False`; every `patience` epochs when the metric is None), or raised every `step_epoch` epochs
    until `last_step_epoch` (`increase=True`).  `factor` is an additive step (`threshold_mode="abs"`) or a relative one
    ("rel"); the threshold stays inside [min_ct, max_ct].  With `warm_up_epochs > 0` (decreasing schedule only) nothing
    happens before that epoch, at which the threshold is set to `max_ct`."""

    def __init__(self, activation: Optional[Union[torch.nn.Module, Callable]] = None,
                 confidence_threshold: Optional[float] = None, increase: bool = False, last_step_epoch: int = None,
                 threshold_from_both_sides: bool = True, mode: Literal["min", "max"] = "min", factor: float = 0.05,
                 patience: int = 10, threshold: float = 1e-4, threshold_mode: Literal["rel", "abs"] = "abs",
                 min_ct: float = 0.5, max_ct: float = 0.95, eps: float = 1e-8, warm_up_epochs: int = 0,
                 mask_channel: Optional[int] = None, verbose: bool = True):
        self.activation = activation
        self.confidence_threshold = confidence_threshold
        self.increase = increase
        self.threshold_from_both_sides = threshold_from_both_sides
        self.init_kwargs = {"activation": None, "confidence_threshold": confidence_threshold,
                            "threshold_from_both_sides": threshold_from_both_sides, "mask_channel": mask_channel}
        if mode not in ("min", "max"):
            raise ValueError(f"Invalid mode: {mode}. Mode should be 'min' or 'max'.")
        assert factor < 1, f"Factor must be smaller than 1, got {factor}"
        if threshold_mode not in ("rel", "abs"):
            # the reference's message names `mode` here
            raise ValueError(f"Invalid threshold mode: {mode}. Threshold mode should be 'rel' or 'abs'.")
        self.mode, self.factor, self.patience = mode, factor, patience
        self.threshold, self.threshold_mode = threshold, threshold_mode
        self.min_ct, self.max_ct, self.eps, self.warm_up_epochs = min_ct, max_ct, eps, warm_up_epochs
        if increase and warm_up_epochs > 0:
            raise ValueError("warm_up_epochs > 0 is only supported when increase=False.")
        if mask_channel is not None:
            raise NotImplementedError("mask_channel is not implemented yet; only None is supported.")
        self.mask_channel, self.verbose = mask_channel, verbose
        self.best = float("inf") if mode == "min" else float("-inf")
        self.num_bad_epochs: int = 0
        self.last_epoch = 0
        if increase:
            self._plan_increase(last_step_epoch)

    def _plan_increase(self, last_step_epoch):
        """epochs between two increments so that max_ct is reached by last_step_epoch (at least one epoch apart)"""
        self.last_step_epoch = last_step_epoch
        n_increments = len(np.arange(self.min_ct, self.max_ct + self.factor / 2, self.factor)) - 1
        if n_increments <= 0:
            self.step_epoch = 0
        else:
            self.step_epoch = max(1, int(np.floor(self.last_step_epoch / n_increments)))
            self.last_step_epoch = max(self.last_step_epoch, self.step_epoch * n_increments)
        print(f"ScheduledPseudoLabeler: Increasing confidence_threshold every {self.step_epoch} epochs;",
              f"until epoch {self.last_step_epoch}")

    def __call__(self, teacher, input_):
        return _label(self, teacher, input_, None)

    # ---- schedule (host) ----------------------------------------------------------------------
    def end_warm_up(self):
        self.confidence_threshold = self.max_ct
        print(f"End of warm-up phase reached: setting confidence threshold to {self.confidence_threshold}")

    def _is_better(self, a, best):
        if self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold) if self.mode == "min" else a > best * (self.threshold + 1.0)
        return a < best - self.threshold if self.mode == "min" else a > best + self.threshold

    def _move_ct(self, new_ct, epoch, verb):
        old_ct = self.confidence_threshold
        if abs(old_ct - new_ct) > self.eps:
            self.confidence_threshold = new_ct
        if self.verbose:
            print(f"Epoch {epoch}: {verb} confidence threshold from {old_ct} to {self.confidence_threshold}")

    def _reduce_ct(self, epoch):
        ct = self.confidence_threshold
        self._move_ct(max(ct * (1 - self.factor) if self.threshold_mode == "rel" else ct - self.factor, self.min_ct),
                      epoch, "reducing")

    def _increase_ct(self, epoch):
        ct = self.confidence_threshold
        self._move_ct(min(ct * (1 + self.factor) if self.threshold_mode == "rel" else ct + self.factor, self.max_ct),
                      epoch, "increase")

    def decrease_step(self, metric, epoch=None):
        if epoch is None:
            epoch = self.last_epoch = self.last_epoch + 1
        if metric is None:   # no metric: lower the threshold every `patience` epochs
            if epoch != 0 and epoch % self.patience == 0:
                self._reduce_ct(epoch)
            return
        current = float(metric)
        if self._is_better(current, self.best):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            self._reduce_ct(epoch)
            self.num_bad_epochs = 0

    def increase_step(self, epoch):
        if epoch <= self.last_step_epoch and epoch != 0 and epoch % self.step_epoch == 0:
            self._increase_ct(epoch)

    def step(self, metric=None, epoch=None):
        if self.warm_up_epochs > 0 and epoch == self.warm_up_epochs:
            self.end_warm_up()
        elif epoch > self.warm_up_epochs:
            if self.increase:
                self.increase_step(epoch)
            else:
                self.decrease_step(metric, epoch)
