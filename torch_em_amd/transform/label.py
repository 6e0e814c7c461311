"""Label-to-target transforms on device (reference torch_em/transform/label.py).

`BoundaryTransform` (`:100-129`) and `AffinityTransform` (`:248-327`) keep the reference's constructor
arguments and output conventions (channel order, float 0/1 values, "disaffinity" = 1 - affinity, mask channels
appended), but run as integer-compare HIP kernels (`tem_boundary_target`, `tem_affinity_target`), bit-exact
with the reference semantics (scikit-image `find_boundaries(mode="thick")`; the brute-force affinity
definitions of the reference's test/transform/test_label_transforms.py:5-55).

MI355X-first placement: in the reference these run on the CPU inside `Dataset.__getitem__`
(`data/segmentation_dataset.py:233-245`); here they are meant to run on the training device on the label
batch right after the H2D copy (`DefaultTrainer(target_transform=...)`), so the loader ships int labels
(8 B/voxel) instead of float targets (up to 96 B/voxel for 12 affinity channels + masks).  CUDA tensors in ->
CUDA tensors out; numpy in -> numpy out (via the device; main process only).
"""
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import ops


def labels_to_binary(labels, background_label: int = 0):
    """(labels != background) in the labels' dtype (reference `:34-44`)."""
    if torch.is_tensor(labels):
        return (labels != background_label).to(labels.dtype)
    return (labels != background_label).astype(labels.dtype)


def _to_device(labels, ndim):
    is_np = not torch.is_tensor(labels)
    t = torch.as_tensor(np.ascontiguousarray(labels)) if is_np else labels
    if t.dtype in (torch.uint64,):
        t = t.to(torch.int64)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("torch_em_amd.transform.label runs on MI355X only; there is no CPU fallback")
        t = t.cuda()
    while ndim is not None and t.dim() > ndim and t.shape[0] == 1:  # ensure_spatial_array: drop singleton axes
        t = t[0]
    return t.to(torch.int64).contiguous(), is_np


class BoundaryTransform:
    """Instance labels -> boundary map [1(+1), *spatial] (reference `:100-129`)."""

    def __init__(self, mode: str = "thick", add_binary_target: bool = False, ndim: Optional[int] = None):
        if mode not in ops.BOUNDARY_MODES:
            raise NotImplementedError(f"BoundaryTransform mode '{mode}': the MI355X kernel has "
                                      f"{sorted(ops.BOUNDARY_MODES)}; 'subpixel' returns a 2n-1 grid, which cannot "
                                      "be a training target")
        self.mode, self.add_binary_target, self.ndim = mode, add_binary_target, ndim

    def __call__(self, labels):
        t, is_np = _to_device(labels, self.ndim)
        if t.dim() not in (2, 3):
            raise ValueError(f"expected 2-D or 3-D labels, got shape {tuple(t.shape)}")
        out = ops.boundary_target(t, self.add_binary_target, self.mode)
        return out.cpu().numpy() if is_np else out


class AffinityTransform:
    """Instance labels -> (dis)affinities [+binary] [+masks] (reference `:248-327`)."""

    def __init__(self, offsets: List[List[int]], ignore_label: Optional[int] = None, add_binary_target: bool = False,
                 add_mask: bool = False, include_ignore_transitions: bool = False):
        self.offsets = offsets
        self.ndim = len(self.offsets[0])
        assert self.ndim in (2, 3)
        self.ignore_label = ignore_label
        self.add_binary_target = add_binary_target
        self.add_mask = add_mask
        self.include_ignore_transitions = include_ignore_transitions

    def __call__(self, labels):
        t, is_np = _to_device(labels, self.ndim)
        if t.dim() != self.ndim:
            raise ValueError(f"expected {self.ndim}-D labels, got shape {tuple(t.shape)}")
        out = ops.affinity_target(t, self.offsets, ignore_label=self.ignore_label,
                                  add_binary_target=self.add_binary_target, add_mask=self.add_mask,
                                  include_ignore_transitions=self.include_ignore_transitions)
        return out.cpu().numpy() if is_np else out


class PerObjectDistanceTransform:
    """Instance labels -> normalised per-object distance targets (reference `:454-633`), in HIP (csrc/distance.hip).

    Same constructor arguments, defaults and `ValueError` as the reference, and its channel order
    `[instances?] [foreground?] [distance?] [directed x ndim?] [boundary?]`.  Per object: the center is the rounded
    centroid (round half to even), or -- where that voxel lies outside the object -- the arg-max of the distance to the
    object's inner boundary (first in C order on ties); the reference ignores `correct_centers` and always corrects,
    and so does this.  distance = |center - x| and directed = (center - x) per axis, both scaled by `sampling`;
    boundary = b(center candidate) - b(x) with b the distance to the nearest inner-boundary voxel.  Each channel is
    divided by its maximum |value| over the object + 1e-7; background gets `distance_fill_value`.

    Inputs: 2-D or 3-D labels (numpy or torch), or a batch `[N, 1, *spatial]` (4-D: 2-D samples, 5-D: 3-D samples),
    which returns `[N, C, *spatial]` from one launch per phase with samples independent -- the form to hand to
    `DefaultTrainer(target_transform=...)`.  CUDA in -> CUDA out, float32 (the `instances` channel holds the ids as
    float32: exact below 2^24 objects).  numpy in -> numpy out, float32, or float64 with `instances=True` (the
    reference's concatenation of uint32 ids and float32 distances).  No host synchronisation: every buffer is sized
    from the voxel count.

    Conventions the reference takes from bioimage_cpp, which no fixture pins yet (assumptions, like row T1):
    `apply_label` numbers face-connected components of equal nonzero labels in first-occurrence (raster) order; the
    directed distances point from the voxel to the center (center - x, vigra's vector-distance sign); a sample that
    one object fills entirely has no boundary voxel, and its boundary channel is 0.  Degenerate samples: no objects ->
    fill value everywhere and foreground 0; a one-voxel object -> all distances 0.
    """
    eps = 1e-7

    def __init__(self, distances: bool = True, boundary_distances: bool = True, directed_distances: bool = False,
                 foreground: bool = True, instances: bool = False, apply_label: bool = True, correct_centers: bool = True,
                 min_size: int = 0, distance_fill_value: float = 1.0, sampling: Optional[Tuple[float, ...]] = None):
        if sum([distances, directed_distances, boundary_distances]) == 0:
            raise ValueError("At least one of distances or directed distances has to be passed.")
        self.distances = distances
        self.boundary_distances = boundary_distances
        self.directed_distances = directed_distances
        self.foreground = foreground
        self.instances = instances
        self.apply_label = apply_label
        self.correct_centers = correct_centers
        self.min_size = min_size
        self.distance_fill_value = distance_fill_value
        self.sampling = sampling

    def _flags(self) -> int:
        return ((ops.POD_DIST if self.distances else 0) | (ops.POD_BOUNDARY if self.boundary_distances else 0)
                | (ops.POD_DIRECTED if self.directed_distances else 0) | (ops.POD_FOREGROUND if self.foreground else 0)
                | (ops.POD_INSTANCES if self.instances else 0))

    def __call__(self, labels):
        t, is_np = _to_device(labels, None)
        if t.dim() in (2, 3):
            batched, ndim, sp = False, t.dim(), tuple(t.shape)
            t = t[None]
        elif t.dim() in (4, 5) and t.shape[1] == 1:
            batched, ndim, sp = True, t.dim() - 2, tuple(t.shape[2:])
            t = t[:, 0]
        else:
            raise ValueError(f"expected 2-D or 3-D labels or a batch [N, 1, *spatial], got shape {tuple(t.shape)}")
        N = t.shape[0]
        t = t.reshape((N,) + (1,) * (3 - ndim) + sp)
        sampling = (1.0,) * ndim if self.sampling is None else tuple(float(s) for s in self.sampling)
        if len(sampling) != ndim:
            raise ValueError(f"sampling {self.sampling} does not match the {ndim}-D labels")
        ids = ops.pod_ids(t, self.apply_label, self.min_size)
        out = ops.pod_targets(ids, ndim, (1.0,) * (3 - ndim) + sampling, self._flags(), self.distance_fill_value)
        out = out.reshape((N, out.shape[1]) + sp)
        if not batched:
            out = out[0]
        if is_np:
            out = out.cpu().numpy()
            return out.astype("float64") if self.instances else out
        return out


class BatchTargets:
    """Apply a label transform to every sample of an int label batch [N, 1, *spatial] on device."""

    def __init__(self, transform):
        self.transform = transform

    def __call__(self, y: torch.Tensor) -> torch.Tensor:
        return torch.stack([self.transform(s) for s in y])
