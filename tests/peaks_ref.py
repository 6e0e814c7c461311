"""The numpy / scipy oracle of peak_local_max and watershed_from_maxima (TEST INFRASTRUCTURE; shares no code with the
package).  The definition is scikit-image's (>= 0.19), restated in DESIGN.md "Peak maxima"; one sample (2-D or 3-D) a call."""
import numpy as np
from scipy import ndimage

import watershed_ref as R


def peak_local_max(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, num_peaks=None):
    """-> int64 [n, 3], the (z, y, x) of the peaks: highest first, equal heights in raster order, greedily spaced"""
    a = np.asarray(image, np.float32)
    a = a.reshape((1,) * (3 - a.ndim) + a.shape)
    d = int(min_distance)
    cand = a == ndimage.maximum_filter(a, size=2 * d + 1, mode="nearest")
    if cand.all():
        cand[:] = False
    thr = a.min() if threshold_abs is None else np.float32(threshold_abs)
    if threshold_rel is not None:
        thr = max(thr, np.float32(threshold_rel) * a.max())
    cand &= a > thr
    b = d if exclude_border is True else int(exclude_border)
    for ax in range(3):
        if a.shape[ax] > 1 and b > 0:
            edge = [slice(None)] * 3
            for edge[ax] in (slice(None, b), slice(-b, None)):
                cand[tuple(edge)] = False
    coords = np.argwhere(cand)
    coords = coords[np.argsort(-(a[cand] + np.float32(0)), kind="stable")]
    kept = np.zeros((0, 3), np.int64)
    for c in coords:
        if not len(kept) or ((kept - c) ** 2).sum(1).min() >= d * d:
            kept = np.vstack([kept, c])
    return kept[:num_peaks]


def markers(peaks, shape):
    out = np.zeros((1,) * (3 - len(shape)) + tuple(shape), np.int64)
    out[tuple(peaks.T)] = np.arange(1, len(peaks) + 1)
    return out.reshape(shape)


def boundary_distances(boundaries, threshold=0.1):
    """float32: the correctly rounded root of scipy's EDT, squared back to the exact integer"""
    d2 = np.rint(ndimage.distance_transform_edt(np.asarray(boundaries, np.float32) < np.float32(threshold)) ** 2)
    return np.sqrt(d2.astype(np.float32))


def watershed_from_smoothed(boundaries, foreground, smoothed, min_distance, min_size):
    """watershed_from_maxima behind its smoothing: `smoothed` is the smoothed, masked distance map"""
    seeds = markers(peak_local_max(smoothed, min_distance, exclude_border=False), np.shape(boundaries))
    return R.np_size_filter(R.kruskal(boundaries, seeds, np.asarray(foreground) != 0), min_size)
