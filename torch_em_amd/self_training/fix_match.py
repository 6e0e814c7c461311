"""FixMatchTrainer for the MI355X path (reference torch_em/self_training/fix_match.py:13-368).

Semi-supervised learning / domain adaptation after Sohn et al. (https://arxiv.org/abs/2001.07685): the "teacher" is the
student itself (weight sharing) -- it predicts pseudo labels on a weakly augmented view under `no_grad`, and is trained on the
strongly augmented view of the same input against them, alone or together with labelled data (one backward pass over the mean
of the two losses).  Constructor arguments, loader / loss selection, the order of the operations in a step, the checkpoint
contents and the logger calls are the reference's; `logger` defaults to None as in `MeanTeacherTrainer`, with which this
trainer shares everything but the steps (`mean_teacher.SelfTrainingTrainer`).

Where it differs from the mean teacher, as the reference does:
  * `val_loader` is the unsupervised VALIDATION loader when there is one;
  * the pseudo labeler runs the student in train mode; there is no second model, no momentum update and no sampler;
  * `pseudo_labeler.step` is not called after validation (only the reference's invertible-augmentation variant does);
  * the checkpoint has no `teacher_state`.

Distribution alignment (`source_distribution=[share below the label threshold, share above]`, reference `:164-181`): in
training, every label is scaled by source share / predicted share of its class and clipped to [0, 1].  The reference runs a
compare, a `torch.unique` (a sort and a device-to-host synchronisation) and five element-wise passes; here it is two launches
without a host round trip (`ops.distribution_align`, csrc/selftrain.hip).

The semi-supervised step runs the labeler's `no_grad` forward of the model BETWEEN its supervised gradient forward and the
backward pass: every forward of the engine owns its activations and by-products, so the first node is not disturbed
(tests/test_gpu_fixmatch.py pins this).  `view_transforms` and `hip_graph` as in `MeanTeacherTrainer`.
"""
from typing import Callable, Optional, Sequence

import torch

from .. import ops
from .mean_teacher import _PARTS, Dummy, InvertibleAugmentationsMixin, SelfTrainingTrainer

__all__ = ["FixMatchTrainer", "FixMatchTrainerWithInvertibleAugmentations"]


class FixMatchTrainer(SelfTrainingTrainer):
    """See the module docstring.  Loaders: `unsupervised_train_loader` (a weakly and a strongly augmented view of the same
    input per batch, or one raw batch with `view_transforms`), optional `supervised_train_loader` (input, labels), and at
    least one of `unsupervised_val_loader` / `supervised_val_loader`.  Callables: `pseudo_labeler(model, input) -> (labels,
    filter)`, `unsupervised_loss(model, input, labels, filter)`, `supervised_loss(model, input, labels)`, and at least one of
    the `*_loss_and_metric` variants returning (loss, metric).  `source_distribution`: None, or the two class shares the
    pseudo labels are aligned to."""
    _PARTS = tuple(k for k in _PARTS if k != "sampler")
    _STEP_DESCRIPTION = "this step runs a pseudo labeler on the model and up to two gradient passes of it"

    def __init__(self, model: torch.nn.Module, unsupervised_train_loader, unsupervised_loss: Callable,
                 pseudo_labeler: Callable, supervised_train_loader=None, unsupervised_val_loader=None,
                 supervised_val_loader=None, supervised_loss: Optional[Callable] = None,
                 unsupervised_loss_and_metric: Optional[Callable] = None,
                 supervised_loss_and_metric: Optional[Callable] = None, logger=None,
                 source_distribution: Optional[Sequence[float]] = None, view_transforms=None, **kwargs):
        # ValueError unless there are exactly two finite positive shares: the reference indexes [0] and [1] of the ratio
        source = None if source_distribution is None else list(ops.source_shares(source_distribution))
        train_loader, val_loader = self._select(unsupervised_train_loader, supervised_train_loader, unsupervised_val_loader,
                                                supervised_val_loader, supervised_loss, unsupervised_loss_and_metric,
                                                supervised_loss_and_metric, kwargs)
        super().__init__(model=model, train_loader=train_loader, val_loader=val_loader, loss=Dummy(), metric=Dummy(),
                         logger=logger, **kwargs)
        self.unsupervised_loss, self.supervised_loss = unsupervised_loss, supervised_loss
        self.pseudo_labeler = pseudo_labeler
        self._set_view_transforms(view_transforms)
        # the reference keeps a float32 tensor on the device; the kernel takes the two shares as launch arguments, so they
        # stay on the host (float32-rounded there) and no step reads them back
        self.source_distribution = source

    def _labeling_model(self):
        return self.model   # weight sharing: the student labels its own weakly augmented view

    # ---- checkpoints --------------------------------------------------------------------------
    def _record_extra(self):
        return {"source_distribution": self.source_distribution}

    @classmethod
    def _ctor_extra(cls, record):
        return {"source_distribution": record["source_distribution"]}

    # ---- distribution alignment -------------------------------------------------------------------
    def get_distribution_alignment(self, pseudo_labels, label_threshold=0.5):
        """the labels themselves without a `source_distribution` (the very tensor, as the reference), else a new tensor with
        every label scaled by source share / predicted share of its class and clipped to [0, 1]"""
        if self.source_distribution is None:
            return pseudo_labels
        if not ops._is_dense(pseudo_labels):
            pseudo_labels = pseudo_labels.contiguous()
        return ops.distribution_align(pseudo_labels, self.source_distribution, label_threshold)

    def _aligned_labels(self, teacher_input):
        pseudo_labels, label_filter = self._pseudo_labels(teacher_input)   # no_grad, the precision context, train mode
        pseudo_labels = pseudo_labels.detach()
        if label_filter is not None:
            label_filter = label_filter.detach()
        return self.get_distribution_alignment(pseudo_labels), label_filter

    # ---- steps (training only: validation does not align) -------------------------------------------
    def _unsupervised_step(self, xu1, xu2):
        """labels from the model itself, alignment, then zero_grad / loss / backward / optimizer step (reference `:194-215`)
        -> (loss, pseudo_labels, label_filter)"""
        pseudo_labels, label_filter = self._aligned_labels(xu1)
        self.optimizer.zero_grad()
        with self._precision():
            loss = self.unsupervised_loss(self.model, xu2, pseudo_labels, label_filter)
            self._backprop(loss)
        return loss, pseudo_labels, label_filter

    def _semisupervised_step(self, xs, ys, xu1, xu2):
        """zero_grad, supervised forward, the labeler's no_grad forward of the SAME model, alignment, unsupervised forward,
        ONE backward pass over the mean of the two losses (reference `:244-273`)
        -> (supervised loss, unsupervised loss, combined loss, pseudo_labels, label_filter)"""
        self.optimizer.zero_grad()
        with self._precision():
            supervised_loss = self.supervised_loss(self.model, xs, ys)
        pseudo_labels, label_filter = self._aligned_labels(xu1)
        with self._precision():
            unsupervised_loss = self.unsupervised_loss(self.model, xu2, pseudo_labels, label_filter)
            loss = (supervised_loss + unsupervised_loss) / 2
            self._backprop(loss)
        return supervised_loss, unsupervised_loss, loss, pseudo_labels, label_filter


class FixMatchTrainerWithInvertibleAugmentations(InvertibleAugmentationsMixin, FixMatchTrainer):
    """`FixMatchTrainer` whose views come from `augmenter` (a `FixMatchAugmenters`: weak teacher view, strong student view)
    and whose losses take predictions in the common frame: the loops and their order of operations are
    `mean_teacher.InvertibleAugmentationsMixin`'s (reference `fix_match.py:371-689`).  Its own: the labels are detached and
    aligned to `source_distribution` BEFORE they are mapped back (training only), and -- unlike the plain `FixMatchTrainer` --
    `pseudo_labeler.step` follows every unsupervised validation."""
    _PARTS = tuple(k for k in FixMatchTrainer._PARTS if k != "view_transforms") + ("augmenter",)

    def __init__(self, model: torch.nn.Module, unsupervised_train_loader, unsupervised_loss: Callable, pseudo_labeler: Callable,
                 augmenter, **kwargs):
        if kwargs.get("view_transforms") is not None:
            raise ValueError(f"{type(self).__name__}: the views come from `augmenter`; view_transforms must be None")
        self._set_augmenter(augmenter)
        super().__init__(model=model, unsupervised_train_loader=unsupervised_train_loader, unsupervised_loss=unsupervised_loss,
                         pseudo_labeler=pseudo_labeler, **kwargs)

    def _prepare_labels(self, pseudo_labels, label_filter):
        pseudo_labels = pseudo_labels.detach()
        if label_filter is not None:
            label_filter = label_filter.detach()
        return self.get_distribution_alignment(pseudo_labels), label_filter
