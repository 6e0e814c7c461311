"""GPU: peak_local_max on the device (csrc/peaks.hip, ops.peak_local_max / peak_markers) and
torch_em_amd.util.watershed_from_maxima against the numpy / scipy oracle tests/peaks_ref.py.  Coordinates, their order and
labels are compared with array_equal: everything compared is an integer, there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

import peaks_ref as P
from oracle.gpu_kit import DEV

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def misaligned(a):
    """the array in a device buffer whose base is one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 4
    return view


def smooth_noise(rs, shape, sigma=1.5):
    a = gaussian_filter(rs.rand(*shape).astype(np.float32), sigma).astype(np.float32)
    return (a - a.min()) / (a.max() - a.min())


def ridge(shape, axis):
    a = np.zeros(shape, np.float32)
    sl = [s // 2 for s in shape]
    sl[axis] = slice(5, shape[axis] - 5)
    a[tuple(sl)] = 1
    return a


def spikes(*at):
    a = np.zeros((8, 16, 16), np.float32)
    for p in at:
        a[p] = 1
    return a


def build_cases():
    """name -> (image [D, H, W], the arguments of peak_local_max)"""
    C = {}
    rs = np.random.RandomState(5)
    C["single_voxel"] = (np.float32([[[0.5]]]), dict(min_distance=1, exclude_border=False))
    for name, shape in (("line_w", (1, 1, 37)), ("line_h", (1, 37, 1)), ("line_d", (37, 1, 1))):
        C[name] = (rs.rand(*shape).astype(np.float32), dict(min_distance=2))
    for shape in ((3, 5, 257), (2, 17, 130), (8, 16, 16), (1, 70, 131)):       # no multiple of a tile; axes shorter than d
        for d in (1, 2, 7, 20, 31):
            C["noise_%dx%dx%d_d%d" % (shape + (d,))] = (smooth_noise(rs, shape), dict(min_distance=d, exclude_border=False))
    for shape in ((2, 17, 130), (1, 70, 131)):                                  # ties everywhere
        base = smooth_noise(rs, shape)
        for levels, d in ((4, 2), (4, 7), (8, 2), (8, 20)):
            C["quantised%d_%dx%dx%d_d%d" % ((levels,) + shape + (d,))] = (np.floor(base * levels).clip(0, levels - 1).astype(np.float32),
                                                                       dict(min_distance=d, exclude_border=False))
    for name, shape, ax in (("ridge_x", (1, 3, 1000), 2), ("ridge_y", (1, 1000, 3), 1), ("ridge_z", (1000, 3, 1), 0), ("ridge_line", (1, 1, 1000), 2)):
        C[name] = (ridge(shape, ax), dict(min_distance=3, exclude_border=False))         # a chain across many workgroups
    plateau = np.zeros((1, 64, 70), np.float32)
    plateau[0, 10:50, 20:60] = 2
    for d in (1, 5, 31):
        C[f"plateau_d{d}"] = (plateau, dict(min_distance=d, exclude_border=False))
    block = np.zeros((12, 20, 70), np.float32)
    block[1:11, 3:19, 2:68] = 1
    C["plateau_3d"] = (block, dict(min_distance=4, exclude_border=False))
    zeros = np.where(rs.rand(2, 9, 33) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[rs.rand(2, 9, 33) < 0.1] = -1
    C["signed_zeros"] = (zeros, dict(min_distance=2, exclude_border=False))
    C["at_distance"] = (spikes((2, 4, 4), (2, 7, 8)), dict(min_distance=5, exclude_border=False))       # 25 is not below 25: both
    C["below_distance"] = (spikes((2, 4, 4), (4, 7, 7)), dict(min_distance=5, exclude_border=False))    # 22: the later one goes
    q = (4, 12, 33)
    C["constant"] = (np.full(q, 0.25, np.float32), dict(min_distance=2, exclude_border=False))
    C["constant_low_threshold"] = (np.full(q, 0.25, np.float32), dict(min_distance=2, threshold_abs=-1.0, exclude_border=False))
    C["nothing_above"] = (smooth_noise(rs, q), dict(min_distance=2, threshold_abs=10.0, exclude_border=False))
    img = smooth_noise(rs, (6, 30, 40), 1.0)
    C["threshold_abs"] = (img, dict(min_distance=2, threshold_abs=0.6, exclude_border=False))
    C["threshold_rel"] = (img, dict(min_distance=2, threshold_rel=0.7, exclude_border=False))
    C["threshold_both"] = (img, dict(min_distance=2, threshold_abs=0.5, threshold_rel=0.3))
    C["border_true"] = (img, dict(min_distance=2, exclude_border=True))
    C["border_2"] = (img, dict(min_distance=1, exclude_border=2))
    C["border_2d"] = (img[:1], dict(min_distance=3, exclude_border=True))
    return C


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    image, kw = CASES[name]
    return P.peak_local_max(image, **kw)


def run(image, put=dev, **kw):
    """one sample [D, H, W] -> (peaks int64 [n, 3], the marker volume, rounds)"""
    from torch_em_amd import ops
    (peaks,), rounds = ops.peak_local_max(put(image[None]), return_rounds=True, **kw)
    mk = ops.peak_markers(put(image[None]), **kw)
    assert peaks.dtype == mk.dtype == torch.int32 and tuple(mk.shape) == (1,) + image.shape and peaks.shape[1] == 3
    return peaks.cpu().numpy().astype(np.int64), mk[0].cpu().numpy(), rounds


@pytest.mark.parametrize("name", sorted(CASES))
def test_peaks_are_the_sequential_ones(name):
    image, kw = CASES[name]
    want = reference(name)
    got, mk, rounds = run(image, **kw)
    assert np.array_equal(got, want), (name, len(got), len(want))
    assert np.array_equal(mk, P.markers(want, image.shape)), "peak_markers is the scatter of the list"
    assert rounds >= 1
    got_m, mk_m, _ = run(image, put=misaligned, rounds_per_batch=1, **kw)
    assert np.array_equal(got_m, want) and np.array_equal(mk_m, mk), "4 bytes past a 16-byte boundary, one round a batch"


def test_the_cases_cover_what_they_are_for():
    n = {name: len(reference(name)) for name in CASES}
    assert not n["constant"] and not n["constant_low_threshold"] and not n["nothing_above"] and not n["single_voxel"]
    assert n["at_distance"] == 2 and n["below_distance"] == 1 and n["ridge_x"] == n["ridge_line"] == 330
    assert n["plateau_d1"] == 1600 and n["signed_zeros"] > 50 and 0 < n["threshold_rel"] < n["threshold_abs"]
    assert 0 < n["border_true"] < n["border_2"] and 0 < n["threshold_both"] < n["threshold_rel"]


@pytest.mark.parametrize("name", ["threshold_abs", "quantised4_2x17x130_d2"])
def test_num_peaks_cuts_the_list(name):
    image, kw = CASES[name]
    want = reference(name)
    for k in (1, len(want) - 1, len(want), len(want) + 5):
        got, mk, _ = run(image, num_peaks=k, **kw)
        assert np.array_equal(got, want[:k]) and np.array_equal(mk, P.markers(want[:k], image.shape)), k


def test_batch_equals_single_calls():
    from torch_em_amd import ops
    rs = np.random.RandomState(3)
    shape = (5, 20, 70)
    batch = np.stack([smooth_noise(rs, shape), np.floor(smooth_noise(rs, shape) * 4).astype(np.float32), np.full(shape, 1, np.float32)])
    got = ops.peak_local_max(dev(batch), 3, exclude_border=False)
    mk = ops.peak_markers(dev(batch), 3, exclude_border=False).cpu().numpy()
    for n in range(3):
        want = P.peak_local_max(batch[n], 3, exclude_border=False)
        assert np.array_equal(got[n].cpu().numpy(), want) and np.array_equal(mk[n], P.markers(want, shape)), n
    assert len(got[0]) and len(got[1]) and not len(got[2])


@functools.lru_cache(maxsize=None)
def touching(ndim):
    """(foreground, boundaries) of a few touching discs / balls plus noise"""
    rs = np.random.RandomState(60 + ndim)
    shape = (48, 56) if ndim == 2 else (12, 28, 32)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1)
    centers = [(14, 14), (14, 30), (32, 22), (34, 42)] if ndim == 2 else [(6, 8, 8), (6, 8, 20), (6, 19, 14)]
    dist = np.min([np.sqrt(((grid - c) ** 2).sum(-1)) for c in centers], axis=0)
    r = 9.5 if ndim == 2 else 7.5
    fg = (dist < r).astype(np.float32)
    bd = ((dist >= r - 1.5) & (dist < r + 1)).astype(np.float32)
    noise = 0.04 * rs.rand(*shape).astype(np.float32)
    return np.clip(fg * 0.9 + noise, 0, 1).astype(np.float32), np.clip(bd * 0.8 + noise, 0, 1).astype(np.float32)


@pytest.mark.parametrize("where", ["numpy", "device"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_watershed_from_maxima(ndim, where):
    """the oracle starts from the DEVICE's smoothed map (ops.blur2d / blur3d, tested elsewhere), so no peak moves on a last
    bit of the Gaussian; the distance map in front of it is compared bit for bit"""
    from torch_em_amd import ops
    from torch_em_amd import util as U
    from torch_em_amd.transform.defect import gaussian_weights
    fg, bd = touching(ndim)
    give = (lambda a: a) if where == "numpy" else dev
    dist = U.boundary_distance_map(give(bd))
    dist = dist if where == "numpy" else dist.cpu().numpy()
    assert dist.dtype == np.float32 and np.array_equal(dist, P.boundary_distances(bd))
    w = gaussian_weights(1.0, truncate=4.0).astype(np.float32).tolist()
    masked = dev(np.where(fg > np.float32(0.5), dist, np.float32(0))[None])
    smoothed = (ops.blur2d(masked, w, w) if ndim == 2 else ops.blur3d(masked, w, w, w))[0].cpu().numpy()
    for d, min_size in ((4, 0), (4, 30), (2, 10)):
        want = P.watershed_from_smoothed(bd, fg, smoothed, d, min_size)
        got = U.watershed_from_maxima(give(bd), give(fg), d, min_size=min_size)
        got = got if where == "numpy" else got.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want) and want.max() >= 3, (d, min_size, int(want.max()))
