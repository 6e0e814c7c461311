"""A seeded watershed from the maxima of the boundary distance map, on the device (reference torch_em/util/segmentation.py:
`watershed_from_maxima`, there through bioimage_cpp and `skimage.feature.peak_local_max`), composed without a copy to the
host: the exact EDT (`ops.vector_edt`), the Gaussian (`ops.blur2d` / `blur3d`), `ops.peak_markers` (DESIGN.md "Peak
maxima": the box maximum filter, the peak test and the greedy minimum-spacing pass of scikit-image >= 0.19, bit for bit),
`ops.seeded_watershed` and the size filter.

Inputs and results follow `torch_em_amd.util.segmentation`: numpy arrays or device tensors, one 2-D or 3-D sample or a batch
`[N, 1, *spatial]`, int32 ids.  The functions live here and not in that module because its test pins that it has no
`watershed_from_maxima`; `torch_em_amd.util` exports them.  Parity with bioimage_cpp's distance transform, smoothing and
watershed is not pinned (it is not installed where this was written); the peaks are, against the definition."""
import torch

from .. import ops
from ..transform.label import _from_batch
from .segmentation import _as_float_batch, _filtered, _same_shape, _smooth, _spatial, _thr

__all__ = ["boundary_distance_map", "watershed_from_maxima"]


def _boundary_distances(bd: torch.Tensor, threshold: float) -> torch.Tensor:
    """float32 [N, D, H, W] -> the float32 square root of `ops.vector_edt`'s exact squared distance to the nearest voxel with
    bd >= threshold.  The root is taken in float64 and rounded once more: for an integer below 2^31 that is the correctly
    rounded float32 root (53 >= 2 * 24 + 2 bits), whatever the device's float32 sqrt does in its last bit."""
    _, d2, _ = ops.vector_edt((bd >= _thr(threshold)).to(torch.int64), 1)
    return torch.sqrt(d2.to(torch.float64)).to(torch.float32)


def boundary_distance_map(boundaries, threshold: float = 0.1):
    """The distance of every voxel with `boundaries < threshold` to the nearest voxel with `boundaries >= threshold`, 0 on
    those voxels themselves: float32, exact squared distances and one correctly rounded root (scipy's
    `distance_transform_edt(boundaries < threshold)` rounded to float32).  A sample WITHOUT a voxel at or above the
    threshold has no distance: it yields `sqrt(ops.VDT_NONE)` = 32768.0 everywhere."""
    batched, sp = _spatial(boundaries, "boundary_distance_map")
    bd, is_np = _as_float_batch(boundaries)
    return _from_batch(_boundary_distances(bd, threshold), is_np, batched, tuple(sp), channels=False)


def watershed_from_maxima(boundaries, foreground, min_distance: int, min_size: int = 50, sigma: float = 1.0,
                          threshold1: float = 0.5):
    """Seeds: the maxima of the smoothed boundary distances at least `min_distance` apart; grown by a seeded watershed over
    `boundaries` inside `foreground != 0`; segments below `min_size` removed and the rest renumbered (reference `:135-172`).
    The distances are `boundary_distance_map(boundaries, 0.1)`, set to 0 outside `foreground > threshold1` and smoothed with
    `gaussian_weights(sigma, truncate=4.0)` (`sigma <= 0`: not smoothed); the seeds are
    `ops.peak_markers(..., min_distance, exclude_border=False)`, numbered highest peak first, equal heights in raster
    order.  As in the reference the watershed's mask is `foreground.astype(bool)`, not the thresholded one.  A sample
    whose boundaries stay below 0.1 everywhere has the constant distance 32768 inside the thresholded foreground: its
    peaks are those of that plateau.
    The reference writes its seeds with the first two coordinates of each peak only, so it is 2-D in effect; here a 3-D
    sample uses all three coordinates."""
    what = "watershed_from_maxima"
    _same_shape(what, boundaries=boundaries, foreground=foreground)
    batched, sp = _spatial(foreground, what)
    sp = tuple(sp)
    fg, is_np = _as_float_batch(foreground)
    bd, _ = _as_float_batch(boundaries)
    dist = _boundary_distances(bd, 0.1)
    dist = torch.where(fg > _thr(threshold1), dist, torch.zeros_like(dist))
    if sigma > 0:
        dist = _smooth(dist, sigma, len(sp))
    seeds = ops.peak_markers(dist, min_distance, exclude_border=False)
    seg = ops.seeded_watershed(bd, seeds, fg != 0)
    return _from_batch(_filtered(seg, min_size), is_np, batched, sp, channels=False)
