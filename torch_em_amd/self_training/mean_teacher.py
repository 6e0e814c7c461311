"""MeanTeacherTrainer for the MI355X path (reference torch_em/self_training/mean_teacher.py:17-399).

Semi-supervised learning / domain adaptation after Tarvainen & Valpola (https://arxiv.org/abs/1703.01780): a teacher that is
the exponential moving average of the student predicts pseudo labels on unlabelled data; the student is trained on them,
alone (unsupervised loop) or together with labelled data (semi-supervised loop, one backward pass over the mean of the two
losses).  Constructor arguments, loader / loss selection, the teacher's (re)initialisation, the momentum ramp, the checkpoint
contents and the logger calls are the reference's; `logger` defaults to None here (the tensorboard logger classes are not
part of this package -- any object with the reference's method names is called).

What runs differently:
  * the step between the teacher's forward pass and the student's loss is one streaming launch (`ops.pseudo_label`) and the
    label filter is the Dice kernels' mask (self_training/loss.py);
  * the teacher update is one launch over the flat parameter arenas (`tem_ema_update`), shared with `SPOCOTrainer`;
  * `view_transforms=(teacher_aug, student_aug)` (not in the reference; the counterpart of `DefaultTrainer`'s on-device
    `raw_transform` / `augmentation`): the unsupervised loaders yield ONE raw batch x and the trainer forms
    `(teacher_aug(x), student_aug(x))` on the device -- e.g. two `transform.raw.get_default_mean_teacher_augmentations()`.
    With `view_transforms=None` the loaders yield pairs, as in the reference;
  * `hip_graph=True` raises NotImplementedError: the captured step (graph.py) knows one model and one loss.

The semi-supervised step runs the student twice with gradients before one `backward()`: two `UNetFunction` nodes, each with
its own gradient arena, which autograd adds.  `FusedAdamW` then takes its per-tensor path for that step; the unsupervised
step has one node and stays on the one-launch path.

`SelfTrainingTrainer` holds what this trainer shares with `FixMatchTrainer` (fix_match.py).

At the end of the file: `MeanTeacherTrainerWithInvertibleAugmentations` (reference `:402-723`) and the
`InvertibleAugmentationsMixin` it shares with `FixMatchTrainerWithInvertibleAugmentations` -- one raw batch from the loader,
views formed and inverted on the device (transform/invertible_augmentations.py), losses that take predictions.  The places
where their order of operations differs from the trainers above are listed in the mixin's docstring.
"""
import os
import pickle
import time
import warnings
from copy import deepcopy
from typing import Callable, Optional

import torch

from ..arena import ema_teacher_update
from ..trainer.default_trainer import _FROM_CHECKPOINT, DefaultTrainer, _import_class

_LOADERS = ("unsupervised_train_loader", "supervised_train_loader", "unsupervised_val_loader", "supervised_val_loader")
_PARTS = ("pseudo_labeler", "unsupervised_loss", "supervised_loss", "unsupervised_loss_and_metric",
          "supervised_loss_and_metric", "sampler", "view_transforms")


class Dummy(torch.nn.Module):
    """Stands in for `loss` and `metric` of DefaultTrainer, which this trainer does not use (reference `:13-14`)."""
    init_kwargs = {}


def _to(batch, device):
    return batch.to(device, non_blocking=True)


class SelfTrainingTrainer(DefaultTrainer):
    """What `MeanTeacherTrainer` and `FixMatchTrainer` share: loader and loss selection, the checkpoint record and
    `from_checkpoint`, the batches (`_raw`, `_views`), the logger calls, the training loops around `_unsupervised_step` /
    `_semisupervised_step` and the validation loops.  A subclass provides the two steps and says through the hooks below which
    model labels, what follows a step and what its record holds."""
    _PARTS = _PARTS                  # callables of the constructor that go into the checkpoint record
    _VAL_LOADER_FROM_TRAIN = False   # `val_loader` when there is an unsupervised validation loader: that loader, or the TRAIN loader
    _STEP_DESCRIPTION = ""           # what the step runs, for the refusal of hip_graph=True

    def _select(self, unsupervised_train_loader, supervised_train_loader, unsupervised_val_loader, supervised_val_loader,
                supervised_loss, unsupervised_loss_and_metric, supervised_loss_and_metric, kwargs):
        """The constructor logic of both references -> (train_loader, val_loader).  `kwargs` loses what a deserialised
        `init` may carry."""
        if kwargs.get("hip_graph"):
            raise NotImplementedError(f"{type(self).__name__}: hip_graph=True is not supported -- the captured training step "
                                      f"(torch_em_amd/graph.py) knows one model and one loss; {self._STEP_DESCRIPTION}")
        if supervised_train_loader is None:
            train_loader = unsupervised_train_loader
            self._train_epoch_impl = self._train_epoch_unsupervised
        else:
            assert supervised_loss is not None
            # the shorter loader bounds the epoch: zip() stops there
            train_loader = supervised_train_loader if len(supervised_train_loader) < len(unsupervised_train_loader) \
                else unsupervised_train_loader
            self._train_epoch_impl = self._train_epoch_semisupervised
        self.unsupervised_train_loader, self.supervised_train_loader = unsupervised_train_loader, supervised_train_loader
        assert supervised_val_loader is not None or unsupervised_val_loader is not None
        self.supervised_val_loader, self.unsupervised_val_loader = supervised_val_loader, unsupervised_val_loader
        if unsupervised_val_loader is None:
            val_loader = supervised_val_loader
        else:
            val_loader = unsupervised_train_loader if self._VAL_LOADER_FROM_TRAIN else unsupervised_val_loader
        assert supervised_loss_and_metric is not None or unsupervised_loss_and_metric is not None
        self.supervised_loss_and_metric = supervised_loss_and_metric
        self.unsupervised_loss_and_metric = unsupervised_loss_and_metric
        for key in ("train_loader", "val_loader", "metric", "loss"):   # may come back from a deserialised `init`
            kwargs.pop(key, None)
        kwargs["hip_graph"] = False
        return train_loader, val_loader

    def _set_view_transforms(self, view_transforms):
        if view_transforms is not None and len(view_transforms) != 2:
            raise ValueError("view_transforms: expected (teacher_augmentation, student_augmentation)")
        self.view_transforms = view_transforms

    # ---- hooks ----------------------------------------------------------------------------------
    def _labeling_model(self):
        """the model the pseudo labeler runs"""
        raise NotImplementedError

    def _after_step(self):
        """between a training step (and its logger calls) and the iteration counter"""

    def _after_unsupervised_validation(self, metric_val):
        pass

    def _record_extra(self) -> dict:
        """the subclass's own constructor arguments, for the checkpoint's `self_training` record"""
        return {}

    @classmethod
    def _ctor_extra(cls, record) -> dict:
        """... and back: record -> constructor keywords"""
        return {}

    def _extra_state(self) -> dict:
        """top-level checkpoint entries next to `init`"""
        return {}

    # ---- checkpoints --------------------------------------------------------------------------
    def _self_training_record(self):
        """What `from_checkpoint` needs beyond DefaultTrainer's record: the callables (pickled when they can be) and the
        datasets / batch sizes of the four loaders."""
        rec, lost = self._record_extra(), []
        for key in self._PARTS:
            obj = getattr(self, key)
            try:
                pickle.dumps(obj)
            except Exception:   # a lambda / local function
                obj = None
                lost.append(key)
            rec[key] = obj
        for key in _LOADERS:
            loader = getattr(self, key)
            rec[key + "_dataset"] = getattr(loader, "dataset", None)
            rec[key + "_kwargs"] = {"batch_size": getattr(loader, "batch_size", None)}
        rec["unpicklable"] = lost
        if lost:
            warnings.warn(f"{type(self).__name__}: {lost} cannot be pickled into the checkpoint; from_checkpoint() will ask for them")
        return rec

    def save_checkpoint(self, name, current_metric, best_metric, **extra_save_dict):
        dummy = f"{Dummy.__module__}.{Dummy.__name__}"
        extra_state = self._extra_state()
        extra_state["init"] = {
            "train_loader_kwargs": {"batch_size": getattr(self.train_loader, "batch_size", None)},
            "train_dataset": getattr(self.train_loader, "dataset", None),
            "val_loader_kwargs": {"batch_size": getattr(self.val_loader, "batch_size", None)},
            "val_dataset": getattr(self.val_loader, "dataset", None),
            "loss_class": dummy, "loss_kwargs": {}, "metric_class": dummy, "metric_kwargs": {},
            "trainer_class": f"{type(self).__module__}.{type(self).__name__}",
            "self_training": self._self_training_record(),
        }
        extra_state.update(**extra_save_dict)
        super().save_checkpoint(name, current_metric, best_metric, **extra_state)

    @classmethod
    def from_checkpoint(cls, checkpoint_folder, name="best", device=None, raw_transform=_FROM_CHECKPOINT,
                        target_transform=_FROM_CHECKPOINT, augmentation=_FROM_CHECKPOINT, save_dict=None, **given):
        """Rebuild the trainer from `<checkpoint_folder>/<name>.pt`.  Loaders are rebuilt from the pickled datasets and the
        callables come back from the checkpoint unless passed in `given` (same names as the constructor's).  The on-device
        `raw_transform` / `target_transform` / `augmentation` and `prefetch` of the saved trainer come back as in
        `DefaultTrainer.from_checkpoint`.  Anything that could not be pickled must be passed (RuntimeError otherwise: a
        resumed run must not train on un-standardised inputs or without its labeler silently)."""
        if save_dict is None:
            save_dict = torch.load(os.path.join(checkpoint_folder, f"{name}.pt"), weights_only=False)
        init = save_dict["init"]
        st = init["self_training"]
        transforms = cls._device_transforms_from(init, raw_transform, target_transform, augmentation)
        missing = [k for k in st["unpicklable"] if k not in given]
        if missing:
            raise RuntimeError(f"from_checkpoint: the saved trainer used {missing}, which could not be stored in the "
                               "checkpoint; pass them to from_checkpoint()")
        model = _import_class(init["model_class"])(**init["model_kwargs"])
        optimizer = _import_class(init["optimizer_class"])(model.parameters(), **init["optimizer_kwargs"])
        sched = None
        if init.get("lr_scheduler_class"):
            sched = _import_class(init["lr_scheduler_class"])(optimizer, **init["lr_scheduler_kwargs"])
        parts = {k: given.pop(k, st[k]) for k in cls._PARTS}
        for key in _LOADERS:
            loader = given.pop(key, None)
            if loader is None and st[key + "_dataset"] is not None:
                loader = torch.utils.data.DataLoader(st[key + "_dataset"], **st[key + "_kwargs"])
            parts[key] = loader
        if given:
            raise TypeError(f"from_checkpoint: unexpected arguments {sorted(given)}")
        trainer = cls(model=model, name=init["name"],
                      optimizer=optimizer, device=device or init["device"], lr_scheduler=sched,
                      log_image_interval=init["log_image_interval"], mixed_precision=init["mixed_precision"],
                      early_stopping=init["early_stopping"], logger=None, id_=init["id_"], save_root=init["save_root"],
                      rank=init.get("rank"), mixed_precision_dtype=init["mixed_precision_dtype"]
                      if init.get("mixed_precision_explicit", False) else None, prefetch=init.get("prefetch", True),
                      **cls._ctor_extra(st), **transforms, **parts)
        trainer._initialize(0, save_dict)
        trainer._is_initialized = True
        return trainer

    # ---- batches --------------------------------------------------------------------------------
    def _raw(self, x):
        """the trainer's on-device `raw_transform` (e.g. per-sample standardisation), as every supervised batch gets it"""
        rt = getattr(self, "raw_transform", None)
        return _to(x, self.device) if rt is None else rt(_to(x, self.device))

    def _views(self, batch):
        """-> (teacher_input, student_input) on the device: the loader's pair, or the two `view_transforms` of its one batch.
        `raw_transform` is applied to what the loader yields -- both views of a pair, or the one batch before it is augmented --
        so supervised and unsupervised inputs reach the student on the same scale."""
        if self.view_transforms is None:
            xu1, xu2 = batch
            return self._raw(xu1), self._raw(xu2)
        if isinstance(batch, (list, tuple)):
            if len(batch) != 1:
                raise ValueError(f"{type(self).__name__}: with view_transforms the unsupervised loaders yield one raw batch")
            batch = batch[0]
        x = self._raw(batch)
        teacher_aug, student_aug = self.view_transforms
        return teacher_aug(x), student_aug(x)

    def _pseudo_labels(self, teacher_input):
        with self._precision(), torch.no_grad():
            return self.pseudo_labeler(self._labeling_model(), teacher_input)

    def _log_common(self):
        self.logger.log_lr(self._iteration, [pm["lr"] for pm in self.optimizer.param_groups][0])
        if self.pseudo_labeler.confidence_threshold is not None:
            self.logger.log_ct(self._iteration, self.pseudo_labeler.confidence_threshold)

    def _log_pred(self, x):
        if self._iteration % self.log_image_interval != 0:
            return None
        with torch.no_grad(), self._precision():
            return self.model(x)

    # ---- loops ------------------------------------------------------------------------------------
    def _train_epoch(self, progress):
        return self._train_epoch_impl(progress)

    def _train_epoch_unsupervised(self, progress):
        self.model.train()
        n_iter, t0 = 0, time.time()
        for batch in self.unsupervised_train_loader:
            xu1, xu2 = self._views(batch)
            done = self._unsupervised_step(xu1, xu2)
            if done is None:
                continue   # the batch does not meet the sampler's condition
            loss, pseudo_labels, label_filter = done
            if self.logger is not None:
                self.logger.log_train_unsupervised(self._iteration, loss, xu1, xu2, self._log_pred(xu2), pseudo_labels,
                                                   label_filter)
                self._log_common()
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
            xu1, xu2 = self._views(batch)
            supervised_loss, unsupervised_loss, loss, pseudo_labels, label_filter = self._semisupervised_step(xs, ys, xu1, xu2)
            if self.logger is not None:
                unsup_pred, sup_pred = self._log_pred(xu2), self._log_pred(xs)
                self.logger.log_train_supervised(self._iteration, supervised_loss, xs, ys, sup_pred)
                self.logger.log_train_unsupervised(self._iteration, unsupervised_loss, xu1, xu2, unsup_pred, pseudo_labels,
                                                   label_filter)
                self.logger.log_combined_loss(self._iteration, loss)
                self._log_common()
            self._after_step()
            self._iteration += 1
            n_iter += 1
            if self._iteration >= self.max_iteration:
                break
            progress.update(1)
        return (time.time() - t0) / max(n_iter, 1)

    def _validate_supervised(self):
        metric_val = loss_val = None
        prepass = self._prepass(train=False)
        for x, y in self.supervised_val_loader:
            x, y = prepass(_to(x, self.device), _to(y, self.device))
            with self._precision():
                loss, metric = self.supervised_loss_and_metric(self.model, x, y)
            loss_val = loss.detach() if loss_val is None else loss_val + loss.detach()
            metric_val = metric.detach() if metric_val is None else metric_val + metric.detach()
        n = len(self.supervised_val_loader)
        metric_val, loss_val = float(metric_val) / n, float(loss_val) / n
        if self.logger is not None:
            with self._precision():
                pred = self.model(x)
            self.logger.log_validation_supervised(self._iteration, metric_val, loss_val, x, y, pred)
        return metric_val

    def _validate_unsupervised(self):
        metric_val = loss_val = None
        for batch in self.unsupervised_val_loader:
            x1, x2 = self._views(batch)
            with self._precision():
                pseudo_labels, label_filter = self.pseudo_labeler(self._labeling_model(), x1)
                loss, metric = self.unsupervised_loss_and_metric(self.model, x2, pseudo_labels, label_filter)
            loss_val = loss.detach() if loss_val is None else loss_val + loss.detach()
            metric_val = metric.detach() if metric_val is None else metric_val + metric.detach()
        n = len(self.unsupervised_val_loader)
        metric_val, loss_val = float(metric_val) / n, float(loss_val) / n
        if self.logger is not None:
            with self._precision():
                pred = self.model(x2)
            self.logger.log_validation_unsupervised(self._iteration, metric_val, loss_val, x1, x2, pred, pseudo_labels,
                                                    label_filter)
        self._after_unsupervised_validation(metric_val)
        return metric_val

    def _validate(self):
        self.model.eval()
        with torch.no_grad():
            sup = None if self.supervised_val_loader is None else self._validate_supervised()
            unsup = None if self.unsupervised_val_loader is None else self._validate_unsupervised()
        if unsup is None:
            return sup
        if sup is None:
            return unsup
        return (sup + unsup) / 2


class MeanTeacherTrainer(SelfTrainingTrainer):
    """See the module docstring.  Loaders: `unsupervised_train_loader` (two views of the same input per batch, or one raw
    batch with `view_transforms`), optional `supervised_train_loader` (input, labels), and at least one of
    `unsupervised_val_loader` / `supervised_val_loader`.  Callables: `pseudo_labeler(teacher, input) -> (labels, filter)`,
    `unsupervised_loss(model, input, labels, filter)`, `supervised_loss(model, input, labels)`, and at least one of the
    `*_loss_and_metric` variants returning (loss, metric).  `reinit_teacher=None`: reinitialise iff there is supervised data.
    `sampler(pseudo_labels, filter) -> bool` may reject a batch."""
    # as the reference (`:117-120`): with an unsupervised validation loader, `val_loader` is the unsupervised TRAIN loader
    _VAL_LOADER_FROM_TRAIN = True
    _STEP_DESCRIPTION = "this step runs a teacher, a pseudo labeler and up to two student passes"

    def __init__(self, model: torch.nn.Module, unsupervised_train_loader, unsupervised_loss: Callable,
                 pseudo_labeler: Callable, supervised_train_loader=None, unsupervised_val_loader=None,
                 supervised_val_loader=None, supervised_loss: Optional[Callable] = None,
                 unsupervised_loss_and_metric: Optional[Callable] = None,
                 supervised_loss_and_metric: Optional[Callable] = None, logger=None, momentum: float = 0.999,
                 reinit_teacher: Optional[bool] = None, sampler: Optional[Callable] = None, view_transforms=None, **kwargs):
        self.sampler = sampler
        train_loader, val_loader = self._select(unsupervised_train_loader, supervised_train_loader, unsupervised_val_loader,
                                                supervised_val_loader, supervised_loss, unsupervised_loss_and_metric,
                                                supervised_loss_and_metric, kwargs)
        super().__init__(model=model, train_loader=train_loader, val_loader=val_loader, loss=Dummy(), metric=Dummy(),
                         logger=logger, **kwargs)
        self.unsupervised_loss, self.supervised_loss = unsupervised_loss, supervised_loss
        self.pseudo_labeler, self.momentum = pseudo_labeler, momentum
        self._set_view_transforms(view_transforms)
        self.reinit_teacher = (supervised_train_loader is not None) if reinit_teacher is None else reinit_teacher
        with torch.no_grad():
            self.teacher = deepcopy(self.model)
            if self.reinit_teacher:
                for layer in self.teacher.children():   # direct children only (for the U-Nets: out_conv), as the reference
                    if hasattr(layer, "reset_parameters"):
                        layer.reset_parameters()
            for param in self.teacher.parameters():
                param.requires_grad = False
        self._arena1 = self._arena2 = None

    # ---- EMA teacher ------------------------------------------------------------------------
    def _current_momentum(self) -> float:
        """A reinitialised teacher follows the student quickly at first: min(1 - 1 / (iteration + 1), momentum)."""
        if self.reinit_teacher:
            return min(1 - 1 / (self._iteration + 1), self.momentum)
        return self.momentum

    def _momentum_update(self):
        ema_teacher_update(self, self.teacher, float(self._current_momentum()))

    def _labeling_model(self):
        return self.teacher

    def _after_step(self):
        with torch.no_grad():
            self._momentum_update()

    def _after_unsupervised_validation(self, metric_val):
        self.pseudo_labeler.step(metric_val, self._epoch)   # the threshold schedule advances with the validation metric

    # ---- checkpoints --------------------------------------------------------------------------
    def _record_extra(self):
        return {"momentum": self.momentum, "reinit_teacher": self.reinit_teacher}

    @classmethod
    def _ctor_extra(cls, record):
        return {"momentum": record["momentum"], "reinit_teacher": record["reinit_teacher"]}

    def _extra_state(self):
        return {"teacher_state": self.teacher.state_dict()}

    def load_checkpoint(self, checkpoint="best"):
        save_dict = super().load_checkpoint(checkpoint)
        if save_dict is not None:
            self.teacher.load_state_dict(save_dict["teacher_state"])
            self.teacher.to(self.device)
            self._arena2 = None
        return save_dict

    def _initialize(self, iterations, load_from_checkpoint, epochs=None):
        best_metric = super()._initialize(iterations, load_from_checkpoint, epochs)
        self.teacher.to(self.device)
        return best_metric

    # ---- steps ------------------------------------------------------------------------------------
    def _unsupervised_step(self, xu1, xu2):
        """teacher forward + labeler, student forward / backward on the pseudo labels, optimizer step (the caller updates the
        teacher) -> (loss, pseudo_labels, label_filter), or None when the sampler rejects the batch (nothing ran but the teacher)"""
        pseudo_labels, label_filter = self._pseudo_labels(xu1)
        if self.sampler is not None and not self.sampler(pseudo_labels, label_filter):
            return None
        self.optimizer.zero_grad()
        with self._precision():
            loss = self.unsupervised_loss(self.model, xu2, pseudo_labels, label_filter)
            self._backprop(loss)
        return loss, pseudo_labels, label_filter

    def _semisupervised_step(self, xs, ys, xu1, xu2):
        """supervised and unsupervised student passes, ONE backward pass over the mean of the two losses
        -> (supervised loss, unsupervised loss, combined loss, pseudo_labels, label_filter)"""
        self.optimizer.zero_grad()
        with self._precision():
            supervised_loss = self.supervised_loss(self.model, xs, ys)
        pseudo_labels, label_filter = self._pseudo_labels(xu1)
        with self._precision():
            unsupervised_loss = self.unsupervised_loss(self.model, xu2, pseudo_labels, label_filter)
            loss = (supervised_loss + unsupervised_loss) / 2
            self._backprop(loss)
        return supervised_loss, unsupervised_loss, loss, pseudo_labels, label_filter


class InvertibleAugmentationsMixin:
    """The loops of the reference's `MeanTeacherTrainerWithInvertibleAugmentations` (`mean_teacher.py:402-723`) and
    `FixMatchTrainerWithInvertibleAugmentations` (`fix_match.py:371-689`), which differ only in what the hooks of
    `SelfTrainingTrainer` say: the unsupervised loaders yield ONE raw batch, `augmenter.teacher` / `augmenter.student`
    (transform/invertible_augmentations.py) form the two views on the device, and pseudo labels, label filter and student
    prediction are mapped back into the common frame (one `ops.dihedral` launch each) before the loss.  The losses take
    PREDICTIONS: `unsupervised_loss(pred, labels, filter)`, `supervised_loss(pred, labels)` and the `*_loss_and_metric`
    variants alike (self_training/loss.py: `SelfTrainingLossWithInvertibleAugmentations`, ...).

    Where the order of operations differs from the base trainers, it is the reference's:
      * `augmenter.reset_all()` at the start of every batch, training and validation;
      * the views are formed before `zero_grad` and before any model runs, teacher first, then student;
      * the sampler sees the UN-inverted pseudo labels and filter;
      * the student runs once per step -- its prediction is inverted and handed to the loss, and the logger gets that same
        prediction (the base trainers run the model again for the logger);
      * `pseudo_labeler.step` follows the unsupervised validation in BOTH variants (the plain FixMatchTrainer never steps);
      * logger calls: `log_train_unsupervised(it, loss, x, x, pred_inv, labels_inv, filter_inv)` with the raw batch twice,
        then `log_train_augmentations(it, view1, view2, labels, pred)` -- and `log_validation_augmentations` -- when the
        logger object has them.
    `raw_transform` is applied to the raw batch before the augmenter; supervised batches take the trainer's usual pre-pass.
    `hip_graph=True` is refused as by the base class; `augmenter` joins the checkpoint record."""
    _AUGMENTER_VIEWS = ("teacher", "student")

    def _set_augmenter(self, augmenter):
        missing = [v for v in self._AUGMENTER_VIEWS + ("reset_all",) if not hasattr(augmenter, v)]
        if missing:
            raise ValueError(f"{type(self).__name__}: the augmenter lacks {missing} (see transform/invertible_augmentations.py)")
        self.augmenter = augmenter

    def _raw_batch(self, batch):
        if isinstance(batch, (list, tuple)):
            if len(batch) != 1:
                raise ValueError(f"{type(self).__name__}: the unsupervised loaders yield one raw batch")
            batch = batch[0]
        return self._raw(batch)

    def _two_views(self, batch):
        """-> (raw batch, teacher view, student view), after `reset_all`"""
        self.augmenter.reset_all()
        xu = self._raw_batch(batch)
        return xu, self.augmenter.teacher.transform(xu), self.augmenter.student.transform(xu)

    def _prepare_labels(self, pseudo_labels, label_filter):
        """between the labeler and the inversion, in training (FixMatch: detach and align)"""
        return pseudo_labels, label_filter

    def _inverted_labels(self, teacher_input, train: bool):
        """-> (labels, filter, labels in the common frame, filter in the common frame)"""
        with self._precision(), torch.no_grad():
            pseudo_labels, label_filter = self.pseudo_labeler(self._labeling_model(), teacher_input)
            if train:
                pseudo_labels, label_filter = self._prepare_labels(pseudo_labels, label_filter)
            inverse = self.augmenter.teacher.reverse_transform
            return pseudo_labels, label_filter, inverse(pseudo_labels), None if label_filter is None else inverse(label_filter)

    def _log_if_present(self, name, *args):
        log = getattr(self.logger, name, None)
        if log is not None:
            log(*args)

    def _shown(self, pred):
        return pred if self._iteration % self.log_image_interval == 0 else None

    # ---- loops ------------------------------------------------------------------------------------
    def _train_epoch_unsupervised(self, progress):
        self.model.train()
        n_iter, t0 = 0, time.time()
        for batch in self.unsupervised_train_loader:
            xu, xu1, xu2 = self._two_views(batch)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(xu1, train=True)
            sampler = getattr(self, "sampler", None)
            if sampler is not None and not sampler(pseudo_labels, label_filter):
                continue
            self.optimizer.zero_grad()
            with self._precision():
                pred = self.model(xu2)
                pred_inv = self.augmenter.student.reverse_transform(pred)
                loss = self.unsupervised_loss(pred_inv, labels_inv, filter_inv)
                self._backprop(loss)
            if self.logger is not None:
                self.logger.log_train_unsupervised(self._iteration, loss, xu, xu, pred_inv, labels_inv, filter_inv)
                self._log_if_present("log_train_augmentations", self._iteration, xu1, xu2, pseudo_labels, self._shown(pred))
                self._log_common()
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
            xu, xu1, xu2 = self._two_views(batch)
            self.optimizer.zero_grad()
            with self._precision():
                supervised_pred = self.model(xs)
                supervised_loss = self.supervised_loss(supervised_pred, ys)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(xu1, train=True)
            with self._precision():
                unsup_pred = self.model(xu2)
                unsup_pred_inv = self.augmenter.student.reverse_transform(unsup_pred)
                unsupervised_loss = self.unsupervised_loss(unsup_pred_inv, labels_inv, filter_inv)
                loss = (supervised_loss + unsupervised_loss) / 2
                self._backprop(loss)
            if self.logger is not None:
                self.logger.log_train_supervised(self._iteration, supervised_loss, xs, ys, self._shown(supervised_pred))
                self.logger.log_train_unsupervised(self._iteration, unsupervised_loss, xu, xu, unsup_pred_inv, labels_inv, filter_inv)
                self._log_if_present("log_train_augmentations", self._iteration, xu1, xu2, pseudo_labels, self._shown(unsup_pred))
                self.logger.log_combined_loss(self._iteration, loss)
                self._log_common()
            self._after_step()
            self._iteration += 1
            n_iter += 1
            if self._iteration >= self.max_iteration:
                break
            progress.update(1)
        return (time.time() - t0) / max(n_iter, 1)

    def _validate_supervised(self):
        metric_val = loss_val = None
        prepass = self._prepass(train=False)
        for x, y in self.supervised_val_loader:
            x, y = prepass(_to(x, self.device), _to(y, self.device))
            with self._precision():
                pred = self.model(x)
                loss, metric = self.supervised_loss_and_metric(pred, y)
            loss_val = loss.detach() if loss_val is None else loss_val + loss.detach()
            metric_val = metric.detach() if metric_val is None else metric_val + metric.detach()
        n = len(self.supervised_val_loader)
        metric_val, loss_val = float(metric_val) / n, float(loss_val) / n
        if self.logger is not None:
            self.logger.log_validation_supervised(self._iteration, metric_val, loss_val, x, y, pred)
        return metric_val

    def _validate_unsupervised(self):
        metric_val = loss_val = None
        for batch in self.unsupervised_val_loader:
            x, x1, x2 = self._two_views(batch)
            pseudo_labels, label_filter, labels_inv, filter_inv = self._inverted_labels(x1, train=False)
            with self._precision():
                pred = self.model(x2)
                pred_inv = self.augmenter.student.reverse_transform(pred)
                loss, metric = self.unsupervised_loss_and_metric(pred_inv, labels_inv, filter_inv)
            loss_val = loss.detach() if loss_val is None else loss_val + loss.detach()
            metric_val = metric.detach() if metric_val is None else metric_val + metric.detach()
        n = len(self.unsupervised_val_loader)
        metric_val, loss_val = float(metric_val) / n, float(loss_val) / n
        if self.logger is not None:
            self.logger.log_validation_unsupervised(self._iteration, metric_val, loss_val, x, x, pred_inv, labels_inv, filter_inv)
            self._log_if_present("log_validation_augmentations", self._iteration, x1, x2, pseudo_labels, pred)
        self.pseudo_labeler.step(metric_val, self._epoch)
        return metric_val


class MeanTeacherTrainerWithInvertibleAugmentations(InvertibleAugmentationsMixin, MeanTeacherTrainer):
    """`MeanTeacherTrainer` whose views come from `augmenter` (a `MeanTeacherAugmenters`) and whose losses take predictions
    in the common frame: see `InvertibleAugmentationsMixin`.  Constructor as the reference (`mean_teacher.py:466-502`)."""
    _PARTS = tuple(k for k in _PARTS if k != "view_transforms") + ("augmenter",)

    def __init__(self, model: torch.nn.Module, unsupervised_train_loader, unsupervised_loss: Callable, pseudo_labeler: Callable,
                 augmenter, **kwargs):
        if kwargs.get("view_transforms") is not None:
            raise ValueError(f"{type(self).__name__}: the views come from `augmenter`; view_transforms must be None")
        self._set_augmenter(augmenter)
        super().__init__(model=model, unsupervised_train_loader=unsupervised_train_loader, unsupervised_loss=unsupervised_loss,
                         pseudo_labeler=pseudo_labeler, **kwargs)
