"""Instance segmentation from network predictions, on the device (reference torch_em/util/segmentation.py): thresholds,
connected components, a seeded watershed and a size filter, composed without a copy to the host.

Names, argument names and defaults are the reference's.  Inputs are numpy arrays or device tensors -- 2-D or 3-D arrays are
one sample, `[N, 1, *spatial]` is a batch segmented per sample (the convention of transform/label.py); the result is int32
ids, numpy for numpy inputs and a device tensor for device tensors (the reference returns uint / uint64).

The watershed is `ops.seeded_watershed`: the minimum spanning forest rooted in the seeds (DESIGN.md "Seeded watershed"), a
unique object a parallel kernel can reproduce bit for bit.  On heights without ties it is the segmentation of the
reference's priority flood up to the voxels on a pass; a plateau goes to the seed that reaches it first in raster order, it
is not split half-way.  Parity with `bioimage_cpp.segmentation.watershed` itself is not pinned (it is not installed where
this was written), nor is the numbering of `bioimage_cpp.segmentation.label`: seeds are numbered in raster order, as
`transform.label.connected_components` documents.

The mutex watershed, `mutex_watershed_segmentation`, lives in `torch_em_amd.util.mutex_watershed` and is exported by
`torch_em_amd.util`: a test of this module pins that it does not carry that name.

Not provided: `watershed_from_maxima` (needs `peak_local_max` with greedy spacing)."""
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..transform.defect import gaussian_weights
from ..transform.label import _as_batch, _from_batch


def _spatial(x, what: str):
    """(batched, spatial shape) of a 2-D / 3-D sample or a batch [N, 1, *spatial], from the shape alone"""
    shape = tuple(x.shape)
    if len(shape) in (4, 5) and shape[1] == 1:
        return True, shape[2:]
    if len(shape) in (2, 3):
        return False, shape
    raise ValueError(f"{what}: expected a 2-D or 3-D array or a batch [N, 1, *spatial], got shape {shape}")


def _same_shape(what: str, **arrays):
    shapes = {k: tuple(v.shape) for k, v in arrays.items()}
    if len(set(shapes.values())) != 1:
        raise ValueError(f"{what}: the inputs must have one shape, got {shapes}")
    return _spatial(next(iter(arrays.values())), what)


def _as_float_batch(x):
    """-> (float32 [N, D, H, W] on the device, is_np): `_as_batch` of transform/label.py for a prediction"""
    is_np = not torch.is_tensor(x)
    t = torch.as_tensor(np.ascontiguousarray(x)) if is_np else x
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("torch_em_amd.util.segmentation runs on MI355X only; there is no CPU fallback")
        t = t.cuda()
    batched, sp = _spatial(t, "segmentation")
    N = t.shape[0] if batched else 1
    return t.to(torch.float32).reshape((N,) + (1,) * (3 - len(sp)) + tuple(sp)).contiguous(), is_np


def _thr(value) -> float:
    """a threshold as the float32 the comparison uses (numpy's and torch's scalar rule, made explicit)"""
    return float(np.float32(value))


def _seeds(flag: torch.Tensor) -> torch.Tensor:
    """bool [N, D, H, W] -> its face-connected components, int32 ids 1..n per sample in raster order"""
    return ops.pod_ids(flag.to(torch.int64), True, 0)


def _filtered(ids: torch.Tensor, min_size: int) -> torch.Tensor:
    """the size filter on DENSE int32 ids (values <= the voxel count, as seeds and their watershed are); a new tensor"""
    return ops.size_filter_(ids.clone(), int(min_size)) if min_size > 0 else ids


def size_filter(seg, min_size: int, hmap=None, with_background: bool = False):
    """Remove the segments with fewer than `min_size` voxels (reference `:19-49`).  `min_size == 0` returns `seg` untouched.
    Without `hmap` the small segments become 0 and the survivors are renumbered 1..n in ascending order of their ids.  With
    `hmap` (a height map in seg's shape, or with a channel axis in front, of which the maximum over the first `seg.ndim`
    channels is taken) the small segments are set to 0 and EVERY voxel is refilled from the remaining segments by
    `ops.seeded_watershed` over `hmap`, then the ids are renumbered 1..n ascending; `with_background`: the background
    competes as a segment of its own and is never removed (the reference's `seg + 1 ... exclude=[1]`).  The reference's
    `hmap` path is `elf.segmentation.watershed.apply_size_filter`; elf is not installed where this was written, so this
    path is not pinned against it.  Ids must be >= 0 (checked for numpy input; device tensors are not read back)."""
    if min_size == 0:
        return seg
    batched, sp = _spatial(seg, "size_filter")
    if hmap is not None:
        hs = tuple(hmap.shape)
        ok = hs == tuple(seg.shape) or (hs[2:] == tuple(sp) and hs[0] == seg.shape[0] if batched
                                        else len(hs) == len(sp) + 1 and hs[1:] == tuple(sp))
        if not ok:
            raise ValueError(f"size_filter: hmap {hs} does not match the segmentation {tuple(seg.shape)} "
                             "(the same shape, or with a channel axis)")
    if not torch.is_tensor(seg) and np.asarray(seg).size and np.asarray(seg).min() < 0:
        raise ValueError("size_filter: segment ids must be >= 0")
    t, is_np, batched, sp = _as_batch(seg)
    if hmap is None:
        return _from_batch(ops.pod_ids(t, False, int(min_size)), is_np, batched, sp, channels=False)
    h = torch.as_tensor(np.ascontiguousarray(hmap)) if not torch.is_tensor(hmap) else hmap
    h = h.to(t.device).to(torch.float32)
    if tuple(h.shape) != tuple(seg.shape):
        h = h[:, :len(sp)].amax(dim=1) if batched else h[:len(sp)].amax(dim=0)
    h = h.reshape(t.shape).contiguous()
    ids = ops.pod_ids(t, False, 0)
    kept = ops.size_filter_(ids.clone(), int(min_size))
    if with_background:
        markers = torch.where((ids > 0) & (kept == 0), 0, kept + 1)
        out = (ops.seeded_watershed(h, markers) - 1).clamp_(min=0)   # nothing left to grow from: all background
    else:
        out = ops.seeded_watershed(h, kept)
    return _from_batch(out, is_np, batched, sp, channels=False)


def connected_components_with_boundaries(foreground, boundaries, threshold: float = 0.5):
    """Seeds: the connected components of `clip(foreground - boundaries, 0, 1) > threshold`; grown by a seeded watershed
    over `boundaries` inside `foreground > threshold` (reference `:83-100`)."""
    _same_shape("connected_components_with_boundaries", foreground=foreground, boundaries=boundaries)
    batched, sp = _spatial(foreground, "connected_components_with_boundaries")
    fg, is_np = _as_float_batch(foreground)
    bd, _ = _as_float_batch(boundaries)
    thr = _thr(threshold)
    seeds = _seeds(torch.clip(fg - bd, 0, 1) > thr)
    seg = ops.seeded_watershed(bd, seeds, fg > thr)
    return _from_batch(seg, is_np, batched, tuple(sp), channels=False)


def watershed_from_components(boundaries, foreground, min_size: int = 50, threshold1: float = 0.5, threshold2: float = 0.5):
    """Seeds: the connected components of `foreground - boundaries > threshold1`; grown by a seeded watershed over
    `boundaries` inside `foreground > threshold2`; segments below `min_size` removed and the rest renumbered (reference
    `:103-132`)."""
    _same_shape("watershed_from_components", boundaries=boundaries, foreground=foreground)
    batched, sp = _spatial(foreground, "watershed_from_components")
    fg, is_np = _as_float_batch(foreground)
    bd, _ = _as_float_batch(boundaries)
    seeds = _seeds((fg - bd) > _thr(threshold1))
    seg = ops.seeded_watershed(bd, seeds, fg > _thr(threshold2))
    return _from_batch(_filtered(seg, min_size), is_np, batched, tuple(sp), channels=False)


def _smooth(x: torch.Tensor, sigma: float, ndim: int) -> torch.Tensor:
    w = gaussian_weights(sigma, truncate=4.0).astype(np.float32).tolist()
    return ops.blur2d(x, w, w) if ndim == 2 else ops.blur3d(x, w, w, w)


def watershed_from_center_and_boundary_distances(center_distances, boundary_distances, foreground_map,
                                                 center_distance_threshold: float = 0.5,
                                                 boundary_distance_threshold: float = 0.5, foreground_threshold: float = 0.5,
                                                 distance_smoothing: float = 1.6, min_size: int = 0, debug: bool = False):
    """Seeded watershed on the distances to object centers and boundaries (reference `:175-233`): both distance maps are
    smoothed, the seeds are the connected components where both are below their thresholds inside
    `foreground_map > foreground_threshold`, they grow over the smoothed boundary distances inside that foreground, and
    segments below `min_size` are removed.  `debug`: also the dictionary of intermediates (`center_distances`,
    `boundary_distances`, `foreground_mask`, `markers`), in the caller's form.
    Smoothing is `ops.blur3d` (2-D: `ops.blur2d`) with `gaussian_weights(distance_smoothing, truncate=4.0)` rounded to
    float32: scipy's `gaussian_filter(mode="mirror")`.  Where `bioimage_cpp.filters.gaussian_smoothing` truncates and what
    it does at the border is not known here, so the smoothed maps are not pinned against it."""
    what = "watershed_from_center_and_boundary_distances"
    _same_shape(what, center_distances=center_distances, boundary_distances=boundary_distances, foreground_map=foreground_map)
    batched, sp = _spatial(foreground_map, what)
    sp = tuple(sp)
    cd, is_np = _as_float_batch(center_distances)
    bd, _ = _as_float_batch(boundary_distances)
    fg, _ = _as_float_batch(foreground_map)
    if distance_smoothing > 0:
        cd = _smooth(cd, distance_smoothing, len(sp))
        bd = _smooth(bd, distance_smoothing, len(sp))
    fg_mask = fg > _thr(foreground_threshold)
    marker_map = (cd < _thr(center_distance_threshold)) & (bd < _thr(boundary_distance_threshold)) & fg_mask
    markers = _seeds(marker_map)
    seg = _filtered(ops.seeded_watershed(bd, markers, fg_mask), min_size)
    seg = _from_batch(seg, is_np, batched, sp, channels=False)
    if debug:
        inter = {"center_distances": cd, "boundary_distances": bd, "foreground_mask": fg_mask, "markers": markers}
        return seg, {k: _from_batch(v, is_np, batched, sp, channels=False) for k, v in inter.items()}
    return seg
