"""Flat fp32 arenas for parameters, gradients and optimizer state.

MI355X-first memory layout for the training step: the 46 parameter tensors of the U-Net live
in ONE contiguous HBM buffer (each tensor a 16-byte-aligned view), and so do their gradients and
AdamW moments.  The optimizer step is then a single launch over 85 MB and the data-parallel
gradient exchange is an RCCL all-reduce over contiguous ranges of the gradient arena -- no
per-tensor launches, no bucket copies (the reference relies on torch's for-each AdamW over 46
tensors and on DDP's bucket flatten/unflatten copies, multi_gpu_training.py:79).
"""
from typing import Dict, List, Tuple

import torch


def arena_layout(params: List[torch.Tensor]) -> Tuple[Dict[int, Tuple[int, int]], int]:
    """id(param) -> (offset, numel) with every offset a multiple of 4 floats; total length."""
    total, offsets = 0, {}
    for p in params:
        offsets[id(p)] = (total, p.numel())
        total += (p.numel() + 3) // 4 * 4
    return offsets, total


def _student_flat(trainer, params):
    """The student's flat parameter buffer WITHOUT re-homing its parameters a second time: FusedAdamW already keeps
    them in one arena (optim.py); building another ParamArena over the same tensors would invalidate that one, and
    the two would rebuild each other (and every packed weight) on every step."""
    ar = getattr(trainer.optimizer, "_arena", None)
    if ar is not None and ar.is_current() and len(ar.params) == len(params) and \
            all(a is b for a, b in zip(ar.params, params)):
        return ar.flat
    if hasattr(trainer.optimizer, "_ensure_arena"):
        return None  # a FusedAdamW over a different parameter list: leave its arena alone
    if trainer._arena1 is None or not trainer._arena1.is_current():
        trainer._arena1 = ParamArena(trainer.model)
    return trainer._arena1.flat


def ema_teacher_update(trainer, teacher: torch.nn.Module, momentum: float):
    """teacher <- m * teacher + (1 - m) * trainer.model as ONE launch over the flat arenas of both models (tem_ema_update):
    the momentum update of SPOCOTrainer and MeanTeacherTrainer.  The trainer keeps `_arena1` (the student's arena when the
    optimizer has none) and `_arena2` (the teacher's), both None at first."""
    from . import ops
    p1 = [p for p in trainer.model.parameters()]
    if not p1 or not p1[0].is_cuda:
        raise RuntimeError(f"{type(trainer).__name__}._momentum_update runs on MI355X only (parameters are on the CPU)")
    if trainer._arena2 is None or not trainer._arena2.is_current():
        trainer._arena2 = ParamArena(teacher)
    src = _student_flat(trainer, p1)
    if src is not None:
        ops.ema_update(trainer._arena2.flat, src, float(momentum))
    else:  # no shared flat buffer (foreign optimizer layout): one launch per tensor, nothing is re-homed
        for q, p in zip(trainer._arena2.params, p1):
            ops.ema_update(q.data.view(-1), p.data.contiguous().view(-1), float(momentum))
    ops.bump_versions(trainer._arena2.params)


class ParamArena:
    """Re-homes the parameters of a module into one flat buffer (p.data becomes a view)."""

    def __init__(self, module: torch.nn.Module):
        self.params = [p for p in module.parameters()]
        self.offsets, self.total = arena_layout(self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        for p in self.params:
            o, n = self.offsets[id(p)]
            view = self.flat[o:o + n].view(p.shape)
            view.copy_(p.data)
            p.data = view

    def is_current(self) -> bool:
        """False once something (e.g. module.to(device)) replaced the parameter storages."""
        base = self.flat.data_ptr()
        return all(p.data_ptr() == base + 4 * self.offsets[id(p)][0] for p in self.params)

    def grads_flat(self):
        """The flat gradient arena if every p.grad is the engine's view of one buffer in arena order, else None.
        The engine leaves a reference to its arena on the first parameter (`_tem_grad_flat`); autograd may have
        detached the views it was handed, so membership is verified by address."""
        flat = getattr(self.params[0], "_tem_grad_flat", None)
        if flat is None or flat.numel() < self.total or self.params[0].grad is None:
            return None
        base = flat.data_ptr()
        for p in self.params:
            g = p.grad
            if g is None or g.data_ptr() != base + 4 * self.offsets[id(p)][0] or not g.is_contiguous():
                return None
        return flat[:self.total]
