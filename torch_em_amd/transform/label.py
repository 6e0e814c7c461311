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

The rest of the reference module rides on the kernels of csrc/distance.hip and csrc/label.hip: `connected_components`,
`label_consecutive` and `MinSizeLabelTransform` (union-find components, sequential relabelling, the size filter; int32
ids), `NoToBackgroundBoundaryTransform` and `BoundaryTransformWithIgnoreLabel` (one fused int8 kernel), `OneHotTransform`
and `DistanceTransform` (an exact integer vector EDT plus one finishing pass).  All of them take 2-D or 3-D labels or a
batch `[N, 1, *spatial]` (-> `[N, C, *spatial]`, samples independent).
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


def _as_batch(labels, ndim=None):
    """-> (int64 labels [N, D, H, W] on the device, is_np, batched, spatial shape).  2-D or 3-D labels are one sample;
    [N, 1, *spatial] (4-D: 2-D samples, 5-D: 3-D samples) is a batch.  With `ndim` given, an input of ndim + 2 axes whose
    second axis is 1 is a batch; anything else has its leading singleton axes dropped down to ndim axes, as the
    reference's ensure_spatial_array does."""
    t, is_np = _to_device(labels, None)
    if (t.dim() in (4, 5) if ndim is None else t.dim() == ndim + 2) and t.shape[1] == 1:
        batched, sp = True, tuple(t.shape[2:])
        t = t[:, 0]
    else:
        while ndim is not None and t.dim() > ndim and t.shape[0] == 1:
            t = t[0]
        batched, sp = False, tuple(t.shape)
        t = t[None]
    if len(sp) not in (2, 3) or (ndim is not None and len(sp) != ndim):
        raise ValueError(f"expected 2-D or 3-D labels or a batch [N, 1, *spatial], got shape {tuple(labels.shape)}")
    return t.reshape((t.shape[0],) + (1,) * (3 - len(sp)) + sp).contiguous(), is_np, batched, sp


def _from_batch(out, is_np, batched, sp, channels=True):
    """[N, (C,) D, H, W] -> the caller's form: [N, C, *spatial] for a batch, [C, *spatial] or [*spatial] for one sample"""
    out = out.reshape(tuple(out.shape[:2 if channels else 1]) + sp)
    if batched and not channels:
        out = out[:, None]
    if not batched:
        out = out[0]
    return out.cpu().numpy() if is_np else out


def _components(t, ensure_zero):
    ids = ops.pod_ids(t, True, 0)
    if ensure_zero:   # reference :29-30: `if 0 not in labels: labels -= 1`, per sample, decided on the device
        ids -= (ids.amin(dim=(1, 2, 3), keepdim=True) > 0).to(ids.dtype)
    return ids


def connected_components(labels, ndim: Optional[int] = None, ensure_zero: bool = False):
    """Face-connected components of equal nonzero labels, numbered 1..n in first-occurrence (raster) order with 0 kept as
    background (reference `:16-31`; the numbering is the unpinned bioimage_cpp assumption `PerObjectDistanceTransform`
    documents).  `ensure_zero`: a sample without any 0 has 1 subtracted.  int32 ids in the labels' shape; a batch
    `[N, 1, *spatial]` is numbered per sample.  No host synchronisation."""
    t, is_np, batched, sp = _as_batch(labels, ndim)
    return _from_batch(_components(t, ensure_zero), is_np, batched, sp, channels=False)


def label_consecutive(labels, with_background: bool = True):
    """Distinct values -> consecutive ids in ascending order (reference `:47-65`): 0 stays 0 and the other values become
    1..n; `with_background=False` follows the reference's `+1 ... -1`: labels holding a 0 are shifted up by one first,
    and 1 is subtracted after the relabelling, so the ids are 0..n-1.  int32 ids, per sample for a batch
    `[N, 1, *spatial]`.  No host synchronisation."""
    t, is_np, batched, sp = _as_batch(labels, None)
    if not with_background:
        t = t + (t == 0).flatten(1).any(dim=1).to(t.dtype).view(-1, 1, 1, 1)
    ids = ops.pod_ids(t, False, 0)
    if not with_background:
        ids -= 1
    return _from_batch(ids, is_np, batched, sp, channels=False)


class MinSizeLabelTransform:
    """Connected components, then objects below `min_size` voxels set to 0 and the rest renumbered in order (reference
    `:68-96`); `min_size=None` returns the components.  int32 ids; batches `[N, 1, *spatial]` per sample."""

    def __init__(self, min_size: Optional[int] = None, ndim: Optional[int] = None, ensure_zero: bool = False):
        self.min_size, self.ndim, self.ensure_zero = min_size, ndim, ensure_zero

    def __call__(self, labels):
        t, is_np, batched, sp = _as_batch(labels, self.ndim)
        ids = _components(t, self.ensure_zero)
        if self.min_size is not None and self.min_size > 0:
            ops.size_filter_(ids, self.min_size)
        return _from_batch(ids, is_np, batched, sp, channels=False)


class _MaskedBoundaryTransform:
    def _call(self, labels, kind, key_label, mask_label):
        t, is_np, batched, sp = _as_batch(labels, self.ndim)
        out = ops.boundary_target_masked(t, self.mode, kind, key_label, mask_label, self.add_binary_target)
        return _from_batch(out, is_np, batched, sp)


class NoToBackgroundBoundaryTransform(_MaskedBoundaryTransform):
    """Boundaries [1(+1), *spatial] as int8, with the boundaries between `bg_label` and everything else set to
    `mask_label` (reference `:133-188`); the optional binary channel is `labels != bg_label` with voxels labelled
    `mask_label` set to it.  One fused kernel (`tem_boundary_target_masked`); modes thick, inner, outer."""

    def __init__(self, bg_label: int = 0, mask_label: int = -1, mode: str = "thick", add_binary_target: bool = False,
                 ndim: Optional[int] = None):
        if mode not in ops.BOUNDARY_MODES:
            raise NotImplementedError(f"mode '{mode}': the MI355X kernel has {sorted(ops.BOUNDARY_MODES)}")
        self.bg_label, self.mask_label, self.mode, self.ndim = bg_label, mask_label, mode, ndim
        self.add_binary_target = add_binary_target

    def __call__(self, labels):
        return self._call(labels, 0, self.bg_label, self.mask_label)


class BoundaryTransformWithIgnoreLabel(_MaskedBoundaryTransform):
    """Boundaries [1(+1), *spatial] as int8, with the boundaries of the `ignore_label` region set to `ignore_label`
    (reference `:192-244`); the optional binary channel is `labels != 0` with ignored voxels set to `ignore_label`."""

    def __init__(self, ignore_label: int = -1, mode: str = "thick", add_binary_target: bool = False,
                 ndim: Optional[int] = None):
        if mode not in ops.BOUNDARY_MODES:
            raise NotImplementedError(f"mode '{mode}': the MI355X kernel has {sorted(ops.BOUNDARY_MODES)}")
        self.ignore_label, self.mode, self.ndim, self.add_binary_target = ignore_label, mode, ndim, add_binary_target

    def __call__(self, labels):
        return self._call(labels, 1, self.ignore_label, self.ignore_label)


class OneHotTransform:
    """Semantic labels -> one-hot float32 [C, *spatial] (reference `:330-353`), one streaming kernel.

    `class_ids=None` takes the ids from `torch.unique(labels)`: the channel count then depends on the data, so this is
    the one host synchronisation in this module, and a batch `[N, 1, *spatial]` -- whose samples could disagree on the
    count -- raises `ValueError`; pass `class_ids` for batches."""

    def __init__(self, class_ids=None):
        self.class_ids = list(range(class_ids)) if isinstance(class_ids, int) else class_ids

    def __call__(self, labels):
        t, is_np, batched, sp = _as_batch(labels, None)
        class_ids = self.class_ids
        if class_ids is None:
            if batched:
                raise ValueError("OneHotTransform(class_ids=None) cannot take a batch: the channel count depends on the "
                                 "data; pass class_ids")
            class_ids = torch.unique(t).tolist()
        return _from_batch(ops.onehot_target(t, class_ids), is_np, batched, sp)


class DistanceTransform:
    """Labels -> distances to the voxels equal to `foreground_id` (reference `:356-451`), in HIP (csrc/distance.hip:
    an exact integer vector EDT, then one finishing pass).

    Same constructor arguments, defaults, `ValueError` and `eps` as the reference; channel order
    `[distances?] [directed x ndim?]`, float32.  With only `distances` one sample's result has no channel axis (its shape
    is the labels' shape), as in the reference; a batch `[N, 1, *spatial]` always returns `[N, C, *spatial]`, samples
    independent.  `func` is applied to each part before concatenation and receives device tensors (also for numpy input, which goes
    through the device): pass `torch.sqrt`, not `np.sqrt`.  A sample without foreground takes the
    reference's fill vector (0 if `invert`, else sqrt(sum(shape_i^2) / 2), in every component) through the same steps.
    No host synchronisation: the empty-sample decision and all maxima stay on the device.

    Mirrored quirk: the reference normalises and inverts the directed distances with maxima over axes `(1, 2)` of the
    `[ndim, *spatial]` array.  For 2-D labels that is one maximum per channel; for 3-D labels it leaves the last axis, so
    every (channel, x column) has its own maximum.  The parity definition is the reference's arithmetic, so this does
    the same.  `invert` uses the maximum after normalisation, as the reference does.

    Unpinned assumptions (bioimage_cpp's vector_difference_transform, which no fixture pins): the vectors point from the
    voxel to its nearest foreground voxel (t - x, the sign `PerObjectDistanceTransform` also assumes), in (z, y, x)
    order; among equally near foreground voxels the kernel's separable passes (x, y, z) each keep the candidate with the
    smallest index along their axis -- the distance channel does not depend on that choice, the directed channels do."""
    eps = 1e-7

    def __init__(self, distances: bool = True, directed_distances: bool = False, normalize: bool = True,
                 max_distance: Optional[float] = None, foreground_id: int = 1, invert: bool = False, func=None):
        if sum((distances, directed_distances)) == 0:
            raise ValueError("At least one of 'distances' or 'directed_distances' must be set to 'True'")
        self.directed_distances = directed_distances
        self.distances = distances
        self.normalize = normalize
        self.max_distance = max_distance
        self.foreground_id = foreground_id
        self.invert = invert
        self.func = func

    def __call__(self, labels):
        t, is_np, batched, sp = _as_batch(labels, None)
        out = ops.distance_targets(t, len(sp), self.foreground_id, self.distances, self.directed_distances, self.normalize,
                                   self.max_distance, self.invert)
        if self.func is not None:
            nd = 1 if self.distances else 0
            out = torch.cat([self.func(p) for p in (out[:, :nd], out[:, nd:]) if p.shape[1] > 0], dim=1)
        only_dist = self.distances and not self.directed_distances
        return _from_batch(out[:, 0] if only_dist else out, is_np, batched, sp, channels=not only_dist)


class BatchTargets:
    """Apply a label transform to every sample of an int label batch [N, 1, *spatial] on device."""

    def __init__(self, transform):
        self.transform = transform

    def __call__(self, y: torch.Tensor) -> torch.Tensor:
        return torch.stack([self.transform(s) for s in y])
