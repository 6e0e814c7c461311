"""CPU: numpy / scipy oracles and fixtures for the label transforms that ride on csrc/distance.hip and csrc/label.hip
(`connected_components`, `label_consecutive`, `MinSizeLabelTransform`, `NoToBackgroundBoundaryTransform`,
`BoundaryTransformWithIgnoreLabel`, `OneHotTransform`, `DistanceTransform`), their known answers, and the host-side
surface of those names (no GPU needed).  tests/test_gpu_label_targets.py compares the kernels with these oracles.

Each oracle restates the reference's transform/label.py on numpy / scipy.  Where the reference calls bioimage_cpp (not a
test dependency) it uses the conventions the transforms document as unpinned assumptions: face-connected components
numbered in first-occurrence order, relabel_sequential = ascending values -> 1..n with 0 kept, vector distances pointing
from the voxel to its nearest foreground voxel (t - x) in (z, y, x) order."""
import itertools

import numpy as np
import pytest
from scipy import ndimage

from oracle.label_ref import boundaries_mode
from test_distance_cpu import blobs_2d, oracle_ids, voronoi_3d


# ---- oracles -------------------------------------------------------------------------------------------------------
def vdt_oracle(labels, foreground_id):
    """-> (exact squared distance to the nearest voxel equal to foreground_id, int64; one valid offset field
    [ndim, *shape], int64, t - x from scipy's feature transform), or (None, None) when no voxel has that id"""
    labels = np.asarray(labels)
    target = labels == foreground_id
    if not target.any():
        return None, None
    dist, idx = ndimage.distance_transform_edt(~target, return_indices=True)
    grid = np.indices(labels.shape)
    return np.rint(dist ** 2).astype("int64"), idx.astype("int64") - grid


def vdt_brute_force(labels, foreground_id):
    """squared distance by a loop over all voxel pairs (small arrays only)"""
    labels = np.asarray(labels)
    targets = np.argwhere(labels == foreground_id)
    out = np.zeros(labels.shape, "int64")
    for x in np.ndindex(*labels.shape):
        out[x] = min(int(((t - np.array(x)) ** 2).sum()) for t in targets)
    return out


def distance_transform_oracle(labels, vectors=None, distances=True, directed_distances=False, normalize=True,
                              max_distance=None, foreground_id=1, invert=False, func=None):
    """the reference's DistanceTransform.__call__ / _compute_distances / _compute_directed_distances /
    _get_distances_for_empty_labels (transform/label.py:390-451) in float64, axes (1, 2) included.  `vectors`: an
    offset field [ndim, *shape] to use in place of scipy's, so that a tie choice can be shared."""
    eps = 1e-7
    labels = np.asarray(labels)
    if (labels == foreground_id).sum() == 0:
        fill_value = 0.0 if invert else np.sqrt(np.linalg.norm(list(labels.shape)) ** 2 / 2)
        dd = np.full((labels.ndim,) + labels.shape, fill_value)
    else:
        dd = np.array(vdt_oracle(labels, foreground_id)[1] if vectors is None else vectors, dtype="float64")
    assert dd.shape == (labels.ndim,) + labels.shape
    parts = []
    if distances:
        d = np.linalg.norm(dd, axis=0)
        if max_distance is not None:
            d = np.clip(d, 0, max_distance)
        if normalize:
            d = d / (d.max() + eps)
        if invert:
            d = d.max() - d
        if func is not None:
            d = func(d)
        parts.append(d)
    if directed_distances:
        v = dd.copy()
        if max_distance is not None:
            v = np.clip(v, -max_distance, max_distance)
        if normalize:
            v = v / (np.abs(v).max(axis=(1, 2), keepdims=True) + eps)
        if invert:
            v = v.max(axis=(1, 2), keepdims=True) - v
        if func is not None:
            v = func(v)
        parts.append(v)
    if distances and directed_distances:
        return np.concatenate((parts[0][None], parts[1]), axis=0)
    return parts[0]


def _relabel_sequential(x):
    """0 stays 0, the other values become 1..n in ascending order"""
    u, inv = np.unique(x, return_inverse=True)
    return (inv.reshape(x.shape) + (0 if u[0] == 0 else 1)).astype("int64")


def connected_components_oracle(labels, ensure_zero=False):
    ids = oracle_ids(labels, apply_label=True).astype("int64")
    if ensure_zero and 0 not in ids:
        ids -= 1
    return ids


def label_consecutive_oracle(labels, with_background=True):
    labels = np.array(labels, dtype="int64")
    if with_background:
        return _relabel_sequential(labels)
    if 0 in labels:
        labels += 1
    seg = _relabel_sequential(labels)
    assert seg.min() == 1
    return seg - 1


def min_size_oracle(labels, min_size=None, ensure_zero=False):
    comp = connected_components_oracle(labels, ensure_zero)
    if min_size is not None:
        ids, sizes = np.unique(comp, return_counts=True)
        comp[np.isin(comp, ids[sizes < min_size])] = 0
        comp = _relabel_sequential(comp)
    return comp


def one_hot_oracle(labels, class_ids=None):
    labels = np.asarray(labels)
    class_ids = np.unique(labels).tolist() if class_ids is None else (list(range(class_ids)) if isinstance(class_ids, int)
                                                                        else class_ids)
    out = np.zeros((len(class_ids),) + labels.shape, "float32")
    for i, c in enumerate(class_ids):
        out[i][labels == c] = 1.0
    return out


def _masked_boundaries(labels, second, mask_value, binary, mode, add_binary_target):
    labels = np.asarray(labels).astype("int64")
    b = boundaries_mode(labels, mode)[0].astype("int8")
    b[boundaries_mode(second.astype("int64"), mode)[0].astype(bool)] = mask_value
    if not add_binary_target:
        return b[None]
    binary = binary.astype("int8")
    binary[labels == mask_value] = mask_value
    return np.stack([binary, b])


def no_to_background_oracle(labels, bg_label=0, mask_label=-1, mode="thick", add_binary_target=False):
    labels = np.asarray(labels)
    return _masked_boundaries(labels, labels != bg_label, mask_label, labels != bg_label, mode, add_binary_target)


def ignore_label_oracle(labels, ignore_label=-1, mode="thick", add_binary_target=False):
    labels = np.asarray(labels)
    return _masked_boundaries(labels, labels == ignore_label, ignore_label, labels != 0, mode, add_binary_target)


# ---- fixtures ------------------------------------------------------------------------------------------------------
def _sparse(shape, seed, n):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, "int64")
    lab.reshape(-1)[rng.choice(lab.size, n, replace=False)] = 1
    return lab


def vdt_fixtures():
    """name -> (labels, foreground_id).  Target voxels are dense enough that no distance reaches 32: there half a float32
    ulp is 2^-21 > 1e-6 / 2, and the inverted un-normalised distance channel (an irrational number of that size stored
    as float32) could not meet the 1e-6 absolute bound whatever the kernel did."""
    f = {}
    lab = np.zeros((7, 9), "int64")
    lab[3, 4] = 1
    f["single_7x9"] = (lab, 1)
    lab = _sparse((5, 300), 0, 40)
    lab[2, ::25] = 1
    f["line_5x300"] = (lab, 1)
    f["line_300x5"] = (np.ascontiguousarray(lab.T), 1)
    f["blobs_33x47"] = (blobs_2d(3, shape=(33, 47), sigma=2.0, frac=0.3) * 4, 4)
    f["vol_6x7x8"] = (_sparse((6, 7, 8), 1, 5), 1)
    lab = _sparse((3, 5, 260), 2, 30)
    lab[1, 2, ::20] = 1
    f["vol_3x5x260"] = (lab, 1)
    vor = voronoi_3d(3, shape=(12, 20, 18), n=12)
    cell = int(vor[6, 10, 9]) or int(vor.max())
    f["voronoi_cell"] = (vor, cell)
    f["voronoi_absent"] = (vor, 999)
    yy, xx = np.mgrid[:9, :9]
    f["checker_9x9"] = (((yy + xx) % 2).astype("int64"), 1)
    lab = np.zeros((9, 9), "int64")
    lab[4, 1] = lab[4, 7] = 1
    f["two_symmetric"] = (lab, 1)
    lab = np.zeros((10, 11), "int64")
    lab[0, :] = lab[-1, :] = lab[:, 0] = lab[:, -1] = 2
    f["border_10x11"] = (lab, 2)
    f["all_target_5x6"] = (np.ones((5, 6), "int64"), 1)
    f["all_target_3x4x5"] = (np.full((3, 4, 5), 7, "int64"), 7)
    lab = np.zeros((7, 9), "int64")
    lab[:, 4] = 1
    f["hyperplane_7x9"] = (lab, 1)
    lab = np.zeros((6, 7, 8), "int64")
    lab[:, 3, :] = 1
    f["hyperplane_6x7x8"] = (lab, 1)
    f["empty_6x7"] = (np.zeros((6, 7), "int64"), 1)
    f["empty_4x5x6"] = (np.zeros((4, 5, 6), "int64"), 1)
    return f


TIE_FREE = ("single_7x9", "hyperplane_7x9", "hyperplane_6x7x8")


def merged_voronoi():
    """12x20x18 Voronoi labels with cells merged so that one id has more than one component"""
    vor = voronoi_3d(3, shape=(12, 20, 18), n=12)
    ids = [int(i) for i in np.unique(vor) if i != 0]
    out = vor.copy()
    for a, b in itertools.combinations(ids, 2):   # the first pair of cells that do not touch
        grown = ndimage.binary_dilation(vor == a, structure=ndimage.generate_binary_structure(3, 3))
        if not (grown & (vor == b)).any():
            out[vor == b] = a
            return out
    raise AssertionError("every pair of cells touches")


def small_fixtures():
    """labels for the six small transforms: blobs with several ids, merged Voronoi cells, a volume without any 0"""
    blobs = blobs_2d(3, shape=(33, 47), sigma=2.0, frac=0.4)
    blobs[:, 24:] *= 3                                     # two ids, so that objects of different ids touch
    blobs[20:, :10] = np.where(blobs[20:, :10] > 0, 5, 0)
    nozero = np.ones((9, 11, 10), "int64")
    nozero[3:6, 4:8, 2:5] = 4
    nozero[0, 0, :3] = 2
    nozero[8, 10, 9] = 2
    return {"blobs_33x47": blobs, "voronoi_merged": merged_voronoi(), "nozero_9x11x10": nozero}


def with_ignore(labels):
    """the same labels with two regions set to -1: one inside the volume, one on the border"""
    out = labels.copy()
    out[tuple(slice(s // 3, s // 3 + 3) for s in out.shape)] = -1
    out[(0,) * (out.ndim - 1)] = -1
    return out


# ---- CPU tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, (lab, fg) in vdt_fixtures().items() if lab.size <= 6 * 7 * 8))
def test_vdt_oracle_equals_brute_force(name):
    lab, fg = vdt_fixtures()[name]
    d2, vec = vdt_oracle(lab, fg)
    if d2 is None:
        assert not (lab == fg).any()
        return
    np.testing.assert_array_equal(d2, vdt_brute_force(lab, fg))
    np.testing.assert_array_equal((vec ** 2).sum(0), d2)          # the offset field realises the distance ...
    tgt = tuple(np.indices(lab.shape) + vec)
    assert (lab[tgt] == fg).all()                                  # ... and ends on target voxels


def test_fixtures_keep_distances_below_32():
    for name, (lab, fg) in vdt_fixtures().items():
        d2 = vdt_oracle(lab, fg)[0]
        assert d2 is None or d2.max() < 32 ** 2, name


def test_known_answers_single_voxel():
    lab = np.zeros((3, 5), "int64")
    lab[1, 2] = 1
    d2, vec = vdt_oracle(lab, 1)
    np.testing.assert_array_equal(d2, [[5, 2, 1, 2, 5], [4, 1, 0, 1, 4], [5, 2, 1, 2, 5]])
    np.testing.assert_array_equal(vec[0], [[1] * 5, [0] * 5, [-1] * 5])
    np.testing.assert_array_equal(vec[1], [[2, 1, 0, -1, -2]] * 3)
    s5 = np.sqrt(5.0)
    raw = distance_transform_oracle(lab, normalize=False)
    np.testing.assert_allclose(raw, np.sqrt(d2), rtol=0, atol=1e-15)
    norm = distance_transform_oracle(lab)
    assert norm.shape == lab.shape and abs(norm[0, 0] - s5 / (s5 + 1e-7)) < 1e-15 and norm[1, 2] == 0
    inv = distance_transform_oracle(lab, invert=True)
    assert inv[0, 0] == 0 and abs(inv[1, 2] - s5 / (s5 + 1e-7)) < 1e-15
    both = distance_transform_oracle(lab, directed_distances=True, normalize=False, max_distance=1)
    assert both.shape == (3, 3, 5)
    np.testing.assert_array_equal(both[0], np.clip(np.sqrt(d2), 0, 1))
    np.testing.assert_array_equal(both[2], [[1, 1, 0, -1, -1]] * 3)
    dinv = distance_transform_oracle(lab, distances=False, directed_distances=True, normalize=False, invert=True)
    np.testing.assert_array_equal(dinv[1], [[0, 1, 2, 3, 4]] * 3)  # max over axes (1, 2) = 2, minus the offset


def test_known_answers_hyperplane():
    lab = np.zeros((2, 3, 4), "int64")
    lab[:, 1, :] = 1
    d2, vec = vdt_oracle(lab, 1)
    np.testing.assert_array_equal(d2[:, :, 0], [[1, 0, 1]] * 2)
    assert (vec[0] == 0).all() and (vec[2] == 0).all()
    np.testing.assert_array_equal(vec[1][:, :, 0], [[1, 0, -1]] * 2)
    out = distance_transform_oracle(lab, directed_distances=True)
    assert out.shape == (4, 2, 3, 4)
    np.testing.assert_allclose(out[0][:, :, 0], [[1 / (1 + 1e-7), 0, 1 / (1 + 1e-7)]] * 2, atol=1e-15)
    # axes (1, 2) of [3, 2, 3, 4] are z and y: one maximum per (channel, x column); the all-zero channels divide by eps
    assert (out[1] == 0).all() and (out[3] == 0).all()
    np.testing.assert_allclose(out[2][:, :, 3], [[1 / (1 + 1e-7), 0, -1 / (1 + 1e-7)]] * 2, atol=1e-15)


@pytest.mark.parametrize("invert", [False, True])
def test_known_answers_no_foreground(invert):
    lab = np.zeros((3, 4), "int64")
    fill = 0.0 if invert else np.sqrt((9 + 16) / 2)
    raw = distance_transform_oracle(lab, directed_distances=True, normalize=False, invert=invert)
    assert raw.shape == (3, 3, 4)
    if invert:
        assert (raw == 0).all()
        assert (distance_transform_oracle(lab, directed_distances=True, invert=True) == 0).all()
    else:
        np.testing.assert_allclose(raw[0], np.sqrt(2) * fill, atol=1e-12)
        np.testing.assert_allclose(raw[1:], fill, atol=1e-12)
        norm = distance_transform_oracle(lab, directed_distances=True)
        np.testing.assert_allclose(norm, 1.0, atol=1e-7)
    assert vdt_oracle(lab, 1) == (None, None)


def test_small_oracles_known_answers():
    lab = np.array([[0, 7, 7, 0, 3], [0, 0, 0, 0, 3], [7, 7, 0, 9, 0]])
    np.testing.assert_array_equal(connected_components_oracle(lab), [[0, 1, 1, 0, 2], [0, 0, 0, 0, 2], [3, 3, 0, 4, 0]])
    np.testing.assert_array_equal(label_consecutive_oracle(lab), [[0, 2, 2, 0, 1], [0, 0, 0, 0, 1], [2, 2, 0, 3, 0]])
    np.testing.assert_array_equal(label_consecutive_oracle(lab, False), [[0, 2, 2, 0, 1], [0, 0, 0, 0, 1], [2, 2, 0, 3, 0]])
    np.testing.assert_array_equal(label_consecutive_oracle(lab + 2, False), [[0, 2, 2, 0, 1], [0, 0, 0, 0, 1], [2, 2, 0, 3, 0]])
    np.testing.assert_array_equal(min_size_oracle(lab, 2), [[0, 1, 1, 0, 2], [0, 0, 0, 0, 2], [3, 3, 0, 0, 0]])
    np.testing.assert_array_equal(min_size_oracle(lab, None), connected_components_oracle(lab))
    full = np.array([[5, 5, 2], [5, 2, 2]])
    np.testing.assert_array_equal(connected_components_oracle(full, ensure_zero=True), [[0, 0, 1], [0, 1, 1]])
    np.testing.assert_array_equal(connected_components_oracle(full), [[1, 1, 2], [1, 2, 2]])
    np.testing.assert_array_equal(one_hot_oracle(full, [2, 9, 5]), [[[0, 0, 1], [0, 1, 1]], [[0] * 3] * 2, [[1, 1, 0], [1, 0, 0]]])
    assert one_hot_oracle(full).shape == (2, 2, 3) and one_hot_oracle(full, 3).shape == (3, 2, 3)
    row = np.array([[0, 0, 4, 4, 6, 6, -1, -1]])
    np.testing.assert_array_equal(no_to_background_oracle(row)[0], [[0, -1, -1, 1, 1, 1, 1, 0]])
    np.testing.assert_array_equal(no_to_background_oracle(row, add_binary_target=True)[0], [[0, 0, 1, 1, 1, 1, -1, -1]])
    np.testing.assert_array_equal(ignore_label_oracle(row)[0], [[0, 1, 1, 1, 1, -1, -1, 0]])
    np.testing.assert_array_equal(ignore_label_oracle(row, mode="inner", add_binary_target=True),
                                  [[[0, 0, 1, 1, 1, 1, -1, -1]], [[0, 0, 1, 1, 1, 1, -1, 0]]])
    # outer: background next to an object, or an object voxel whose window holds two objects (index 2 sees only 4 and
    # background); of the ignore image, the outside voxel next to it
    np.testing.assert_array_equal(ignore_label_oracle(row, mode="outer")[0], [[0, 1, 0, 1, 1, -1, 1, 0]])
    assert no_to_background_oracle(row).dtype == np.int8


def test_small_fixtures_cover_their_cases():
    fx = small_fixtures()
    vor = fx["voronoi_merged"]
    assert connected_components_oracle(vor).max() > len(np.unique(vor[vor != 0]))             # an id with two components
    assert 0 not in fx["nozero_9x11x10"] and 0 in fx["blobs_33x47"]
    sizes = np.bincount(connected_components_oracle(fx["blobs_33x47"]).ravel())[1:]
    assert (sizes < 25).any() and (sizes >= 25).any()                                          # min_size=25 splits them
    assert -1 in with_ignore(vor) and -1 not in vor
    assert connected_components_oracle(fx["nozero_9x11x10"], ensure_zero=True).min() == 0


def test_names_defaults_and_errors():
    from torch_em_amd.transform import (BoundaryTransformWithIgnoreLabel, DistanceTransform, MinSizeLabelTransform,
                                        NoToBackgroundBoundaryTransform, OneHotTransform, connected_components,
                                        label_consecutive)
    assert callable(connected_components) and callable(label_consecutive)
    with pytest.raises(ValueError, match="At least one"):
        DistanceTransform(distances=False, directed_distances=False)
    t = DistanceTransform()
    assert (t.distances, t.directed_distances, t.normalize, t.max_distance, t.foreground_id, t.invert, t.func) == \
        (True, False, True, None, 1, False, None)
    assert t.eps == 1e-7
    assert OneHotTransform(3).class_ids == [0, 1, 2] and OneHotTransform().class_ids is None
    assert OneHotTransform([4, 2]).class_ids == [4, 2]
    m = MinSizeLabelTransform()
    assert (m.min_size, m.ndim, m.ensure_zero) == (None, None, False)
    n = NoToBackgroundBoundaryTransform()
    assert (n.bg_label, n.mask_label, n.mode, n.add_binary_target, n.ndim) == (0, -1, "thick", False, None)
    b = BoundaryTransformWithIgnoreLabel()
    assert (b.ignore_label, b.mode, b.add_binary_target, b.ndim) == (-1, "thick", False, None)


def test_limits_are_refused_before_any_launch():
    """host-side argument check of the library: no device needed"""
    import ctypes

    from torch_em_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)   # never dereferenced: the shape is refused first
    rc = lib.tem_vector_edt(one, 1, one, one, one, 1, 1, 1, 4097, None)
    assert rc == -1 and b"4096" in lib.tem_last_error()
    rc = lib.tem_vector_edt(one, 1, one, one, one, 2, 1024, 1024, 1024, None)
    assert rc == -1 and b"2^31" in lib.tem_last_error()
    rc = lib.tem_distance_targets(one, one, one, one, 1, 1, 4097, 1, 2, 1, 0.0, one, 1 << 20, None)
    assert rc == -1 and b"4096" in lib.tem_last_error()
