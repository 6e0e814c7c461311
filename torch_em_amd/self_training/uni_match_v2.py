"""UniMatchv2Trainer for the MI355X path (reference torch_em/self_training/uni_match_v2.py:9-435).

Semi-supervised learning / domain adaptation after Yang et al. (https://arxiv.org/abs/2410.10777): an EMA teacher labels a
weakly augmented view, the student is trained on TWO strongly augmented views of the same input against those labels, and the
loss is the mean over the two.  The trainer is a `MeanTeacherTrainerWithInvertibleAugmentations` (teacher, momentum ramp,
checkpoint contents, loader selection) with an `UniMatchv2Augmenters` (`.weak`, `.strong1`, `.strong2`) and losses that take
`pred_dim` (self_training/loss.py: `UniMatchv2Loss`, `UniMatchv2LossAndMetric`).

The order of operations is the reference's; where it differs from the other self-training trainers of this package:
  * `augmenter.reset_all()` per batch; the three views are formed first: weak, strong1, strong2;
  * the teacher is in eval mode (set once in the constructor; the student's `train()` / `eval()` do not touch it);
  * the student runs ONCE per unsupervised step, on `cat(x_s1, x_s2)`, and its output is split in two;
  * both halves are mapped back by ONE `ops.dihedral` launch over the 2B batch with the two code vectors concatenated (the
    reference inverts them one after the other and stacks); the loss gets the [2, B, C, ...] view of that tensor, `pred_dim=2`;
  * the semi-supervised loop backpropagates the supervised and the unsupervised loss SEPARATELY: zero_grad, supervised
    forward / backward / optimizer step, labels, zero_grad, unsupervised forward / backward / optimizer step -- two optimizer
    steps per iteration, and no combined loss is logged;
  * there is no sampler call (the reference accepts one and never asks it);
  * validation uses `pred_dim=2` as well, and `pseudo_labeler.step` follows the unsupervised validation;
  * logger calls: `log_train_unsupervised(it, loss, x, pred_s1_inv, pred_s2_inv, labels_inv, filter_inv)` and
    `log_train_augmentations(it, x_w, x_s1, x_s2, labels, pred_s1, pred_s2)` (the latter, and `log_validation_augmentations`,
    when the logger object has them).
Two deliberate differences: the unsupervised loop clears the gradients before every step (the reference's never does, so
its gradients add up over the whole run -- an oversight; its semi-supervised loop clears them), and the supervised forward
runs inside the trainer's precision context like every other forward (the reference leaves it outside autocast).  `complementary_dropout=True` raises NotImplementedError: it drops encoder features of the reference's UNETR
and runs that model's decoder by hand; this package has no UNETR.  `hip_graph=True` is refused as by the base class.
"""
import time

import torch

from .. import ops
from .mean_teacher import MeanTeacherTrainerWithInvertibleAugmentations, _to

__all__ = ["UniMatchv2Trainer"]


class UniMatchv2Trainer(MeanTeacherTrainerWithInvertibleAugmentations):
    """See the module docstring.  Arguments as `MeanTeacherTrainerWithInvertibleAugmentations`, all by keyword, plus
    `complementary_dropout` (must be False)."""
    _AUGMENTER_VIEWS = ("weak", "strong1", "strong2")
    _STEP_DESCRIPTION = "this step runs a teacher, a pseudo labeler and the student on two views"

    def __init__(self, complementary_dropout=False, **kwargs):
        if complementary_dropout:
            raise NotImplementedError("UniMatchv2Trainer: complementary_dropout=True needs the decoder of the reference's UNETR, "
                                      "which this package does not have")
        super().__init__(**kwargs)
        self.complementary_dropout = False
        self.teacher.eval()

    def _record_extra(self):
        return dict(super()._record_extra(), complementary_dropout=False)

    @classmethod
    def _ctor_extra(cls, record):
        return dict(super()._ctor_extra(record), complementary_dropout=record.get("complementary_dropout", False))

    def load_checkpoint(self, checkpoint="best"):
        save_dict = super().load_checkpoint(checkpoint)
        self.teacher.eval()
        return save_dict

    # ---- pieces of a step -------------------------------------------------------------------------
    def _three_views(self, batch):
        """-> (raw batch, weak view, strong view 1, strong view 2), after `reset_all`"""
        self.augmenter.reset_all()
        x = self._raw_batch(batch)
        return x, self.augmenter.weak.transform(x), self.augmenter.strong1.transform(x), self.augmenter.strong2.transform(x)

    def _inverted_labels(self, teacher_input, train: bool):
        with self._precision(), torch.no_grad():
            pseudo_labels, label_filter = self.pseudo_labeler(self.teacher, teacher_input)
            inverse = self.augmenter.weak.reverse_transform
            return pseudo_labels, label_filter, inverse(pseudo_labels), None if label_filter is None else inverse(label_filter)

    def _invert_both(self, pred):
        """the student's output on cat(x_s1, x_s2) -> [2, B, C, ...] in the common frame, in one launch when the augmenters'
        geometric chains give their codes (transform/invertible_augmentations.py: `AugmentationSequential.codes`)"""
        s1, s2 = self.augmenter.strong1, self.augmenter.strong2
        B = pred.shape[0] // 2
        chains = [getattr(s, "geometrical_transforms", None) for s in (s1, s2)]
        if all(hasattr(c, "codes") for c in chains):
            codes = chains[0].codes(s1.params, B) + chains[1].codes(s2.params, B)
            inv = ops.dihedral(pred, codes, inverse=True)
            return inv.view((2, B) + tuple(inv.shape[1:]))
        p1, p2 = pred.chunk(2)
        return torch.stack((s1.reverse_transform(p1), s2.reverse_transform(p2)))

    def _student(self, x_s1, x_s2):
        """-> (pred_s1, pred_s2, their stack in the common frame)"""
        pred = self.model(torch.cat((x_s1, x_s2)))
        pred_s1, pred_s2 = pred.chunk(2)
        return pred_s1, pred_s2, self._invert_both(pred)

    def _log_unsupervised_step(self, loss, x, views, preds, stack, pseudo_labels, labels_inv, filter_inv):
        self.logger.log_train_unsupervised(self._iteration, loss, x, stack[0], stack[1], labels_inv, filter_inv)
        self._log_if_present("log_train_augmentations", self._iteration, *views, pseudo_labels, *preds)
        self._log_common()

    # ---- loops ------------------------------------------------------------------------------------
    def _train_epoch_unsupervised(self, progress):
        self.model.train()
        n_iter, t0 = 0, time.time()
        for batch in self.unsupervised_train_loader:
            x, x_w, x_s1, x_s2 = self._three_views(batch)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(x_w, train=True)
            # NOT in the reference, whose unsupervised loop never clears the gradients, so that every step applies the sum of
            # all gradients since the start of training -- an oversight there (its semi-supervised loop clears them)
            self.optimizer.zero_grad()
            with self._precision():
                pred_s1, pred_s2, stack = self._student(x_s1, x_s2)
                loss = self.unsupervised_loss(stack, labels_inv, filter_inv, pred_dim=2)
                self._backprop(loss)
            if self.logger is not None:
                self._log_unsupervised_step(loss, x, (x_w, x_s1, x_s2), (pred_s1, pred_s2), stack, pseudo_labels, labels_inv, filter_inv)
            self._after_step()
            self._iteration += 1
            n_iter += 1
            if self._iteration >= self.max_iteration:
                break
            progress.update(1)
        return (time.time() - t0) / max(n_iter, 1)

    def _train_epoch_semisupervised(self, progress):
        self.model.train()
        n_iter, t0 = 0, time.time()
        prepass = self._prepass(train=True)
        for (xs, ys), batch in zip(self.supervised_train_loader, self.unsupervised_train_loader):
            xs, ys = prepass(_to(xs, self.device), _to(ys, self.device))
            x, x_w, x_s1, x_s2 = self._three_views(batch)
            self.optimizer.zero_grad()
            with self._precision():
                pred_s = self.model(xs)
                supervised_loss = self.supervised_loss(pred_s, ys)
                self._backprop(supervised_loss)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(x_w, train=True)
            self.optimizer.zero_grad()
            with self._precision():
                pred_s1, pred_s2, stack = self._student(x_s1, x_s2)
                unsupervised_loss = self.unsupervised_loss(stack, labels_inv, filter_inv, pred_dim=2)
                self._backprop(unsupervised_loss)
            if self.logger is not None:
                self.logger.log_train_supervised(self._iteration, supervised_loss, xs, ys, pred_s)
                self._log_unsupervised_step(unsupervised_loss, x, (x_w, x_s1, x_s2), (pred_s1, pred_s2), stack, pseudo_labels,
                                            labels_inv, filter_inv)
            self._after_step()
            self._iteration += 1
            n_iter += 1
            if self._iteration >= self.max_iteration:
                break
            progress.update(1)
        return (time.time() - t0) / max(n_iter, 1)

    def _validate_unsupervised(self):
        metric_val = loss_val = None
        for batch in self.unsupervised_val_loader:
            x, x_w, x_s1, x_s2 = self._three_views(batch)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(x_w, train=False)
            with self._precision():
                pred_s1, pred_s2, stack = self._student(x_s1, x_s2)
                loss, metric = self.unsupervised_loss_and_metric(stack, labels_inv, filter_inv, pred_dim=2)
            loss_val = loss.detach() if loss_val is None else loss_val + loss.detach()
            metric_val = metric.detach() if metric_val is None else metric_val + metric.detach()
        n = len(self.unsupervised_val_loader)
        metric_val, loss_val = float(metric_val) / n, float(loss_val) / n
        if self.logger is not None:
            self.logger.log_validation_unsupervised(self._iteration, metric_val, loss_val, x, stack[0], stack[1], labels_inv, filter_inv)
            self._log_if_present("log_validation_augmentations", self._iteration, x_w, x_s1, x_s2, pseudo_labels, pred_s1, pred_s2)
        self.pseudo_labeler.step(metric_val, self._epoch)
        return metric_val
