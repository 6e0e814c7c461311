"""CPU: the per-object distance oracle, the global-EDT argument behind the HIP transform, fixtures, and the host-side
surface of PerObjectDistanceTransform / DistanceLoss / DiceBasedDistanceLoss (no GPU needed).

`pod_oracle` restates the reference's PerObjectDistanceTransform (transform/label.py:454-633) on numpy / scipy, object
by object with bounding-box crops.  Where the reference calls bioimage_cpp (not a test dependency) it uses the conventions the
HIP transform documents as unpinned assumptions: face-connected components numbered in first-occurrence order,
directed distance = (center - x) * sampling, boundary channel 0 when the crop holds no boundary voxel."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle.label_ref import boundaries_mode


# ---- fixtures ----------------------------------------------------------------------------------------------------
def blobs_2d(seed, shape=(96, 112), sigma=4.0, frac=0.5):
    """thresholded Gaussian-filtered noise (the role of skimage's binary_blobs in the reference test), as labels 0/1"""
    rng = np.random.default_rng(seed)
    img = ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
    return (img > np.quantile(img, 1 - frac)).astype("int64")


def voronoi_3d(seed, shape=(24, 40, 36), n=30, bg_frac=0.2):
    """Voronoi-like labels: nearest of n random seeds, some cells set to background"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, (n, 3)) * np.array(shape)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    best = np.full(shape, np.inf)
    lab = np.zeros(shape, "int64")
    for i, (pz, py, px) in enumerate(pts):
        d = (zz - pz) ** 2 + (yy - py) ** 2 + (xx - px) ** 2
        lab[d < best] = i + 1
        best = np.minimum(best, d)
    drop = rng.choice(np.arange(1, n + 1), int(n * bg_frac), replace=False)
    lab[np.isin(lab, drop)] = 0
    return lab


def rings_2d():
    """rings and C-shapes (centroids outside the object), an id split in two components, objects on the border,
    single voxels"""
    lab = np.zeros((64, 72), "int64")
    yy, xx = np.mgrid[:64, :72]
    r = np.hypot(yy - 20, xx - 20)
    lab[(r >= 8) & (r < 12)] = 1                                 # thick ring
    r2 = np.hypot(yy - 45, xx - 50)
    lab[(r2 >= 9) & (r2 < 10.5) & (xx < 56)] = 2                # thin C-shape
    lab[50:60, 5:9] = 3
    lab[50:60, 14:18] = 3                                       # one id, two components
    lab[0:5, 40:70] = 4                                         # on the border
    lab[30, 60] = 5
    lab[62, 30] = 6                                             # single voxels
    lab[:, 71] = 7                                              # along the border
    return lab


def rings_3d():
    lab = np.zeros((20, 30, 34), "int64")
    zz, yy, xx = np.mgrid[:20, :30, :34]
    r = np.hypot(yy - 15, xx - 15)
    lab[(r >= 6) & (r < 10) & (zz >= 3) & (zz < 16)] = 3       # tube
    lab[(zz == 0) & (yy < 4)] = 9                               # face of the volume
    lab[10, 2, 30] = 11
    return lab


def fixtures_2d():
    return {"blobs0": blobs_2d(0), "blobs1": blobs_2d(1, frac=0.35), "rings": rings_2d(),
            "empty": np.zeros((40, 50), "int64"), "full": np.full((40, 50), 5, "int64")}


def fixtures_3d():
    return {"voronoi0": voronoi_3d(0), "voronoi1": voronoi_3d(1, n=12), "rings": rings_3d(),
            "empty": np.zeros((8, 12, 10), "int64"), "full": np.full((8, 12, 10), 2, "int64")}


# ---- oracle --------------------------------------------------------------------------------------------------------
def oracle_ids(labels, apply_label=True, min_size=0):
    labels = np.asarray(labels)
    if apply_label:
        tmp = np.zeros(labels.shape, "int64")
        nxt = 0
        for i in np.unique(labels[labels != 0]):
            comp, n = ndimage.label(labels == i)   # default structure: face connectivity
            tmp[comp > 0] = comp[comp > 0] + nxt
            nxt += n
        u, first = np.unique(tmp.ravel(), return_index=True)
        order = np.argsort(first[u != 0])
        remap = np.zeros(nxt + 1, "int64")
        remap[u[u != 0][order]] = np.arange(1, len(order) + 1)
        ids = remap[tmp]
    else:
        u, inv = np.unique(labels, return_inverse=True)
        ids = (inv.reshape(labels.shape) + (0 if u[0] == 0 else 1)).astype("int64")
    if min_size > 0:
        u, cnt = np.unique(ids, return_counts=True)
        ids[np.isin(ids, u[cnt < min_size])] = 0
        u, inv = np.unique(ids, return_inverse=True)
        ids = (inv.reshape(ids.shape) + (0 if u[0] == 0 else 1)).astype("int64")
    return ids.astype("uint32")


def _bbox(mask):
    idx = np.nonzero(mask)
    return tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)


def _crop_edt(boundaries, bb, sampling):
    cb = boundaries[bb]
    if not cb.any():   # no boundary voxel in the crop (one object fills the sample): boundary distance 0
        return np.zeros(cb.shape)
    return ndimage.distance_transform_edt(cb == 0, sampling=sampling)


def pod_oracle(labels, distances=True, boundary_distances=True, directed_distances=False, foreground=True,
               instances=False, apply_label=True, min_size=0, distance_fill_value=1.0, sampling=None, return_centers=False):
    """the reference's per-object algorithm; centers[id] = the center it used"""
    eps = 1e-7
    ids = oracle_ids(labels, apply_label, min_size)
    ndim = ids.ndim
    samp = (1.0,) * ndim if sampling is None else tuple(sampling)
    boundaries = boundaries_mode(ids.astype("int64"), "inner")[0].astype("uint32")
    nch = int(distances) + int(boundary_distances) + (ndim if directed_distances else 0)
    out = np.full(ids.shape + (nch,), distance_fill_value, dtype="float32")
    centers = {}
    for lid in range(1, int(ids.max()) + 1):
        mask = ids == lid
        bb = _bbox(mask)
        cm = mask[bb]
        centroid = np.array(np.nonzero(mask), dtype="float64").mean(axis=1)
        center = np.round(centroid).astype("int")
        cc = tuple(int(c - b.start) for c, b in zip(center, bb))
        bd = _crop_edt(boundaries, bb, samp)
        bd[~cm] = 0
        maxp = np.unravel_index(np.argmax(bd), bd.shape)
        if not cm[cc]:   # the reference always corrects (correct_centers is not read)
            cc = maxp
        centers[lid] = tuple(int(c + b.start) for c, b in zip(cc, bb))
        grid = np.stack(np.meshgrid(*[np.arange(s) for s in cm.shape], indexing="ij"), -1).astype("float64")
        vec = (np.array(cc, "float64") - grid) * np.array(samp)
        chans = []
        if distances:
            chans.append(np.linalg.norm(vec, axis=-1)[..., None])
        if directed_distances:
            chans.append(vec)
        if boundary_distances:
            chans.append((bd[maxp] - bd)[..., None])
        vals = np.concatenate(chans, -1)
        vals[~cm] = 0
        vals /= (np.abs(vals).max(axis=tuple(range(ndim)), keepdims=True) + eps)
        out[bb][cm] = vals[cm]
    out = out.transpose((ndim,) + tuple(range(ndim)))
    if foreground:
        out = np.concatenate([(ids > 0).astype("float32")[None], out], 0)
    if instances:
        out = np.concatenate([ids[None], out], 0)
    return (out, centers) if return_centers else out


# ---- CPU tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [None, (2.5, 1.0), (1.0, 2.5)])
@pytest.mark.parametrize("name", sorted(fixtures_2d()))
def test_global_edt_equals_crop_edt_2d(name, sampling):
    _check_global_edt(fixtures_2d()[name], sampling)


@pytest.mark.parametrize("sampling", [None, (2.5, 1.0, 1.0), (1.0, 2.0, 2.5)])
@pytest.mark.parametrize("name", sorted(fixtures_3d()))
def test_global_edt_equals_crop_edt_3d(name, sampling):
    _check_global_edt(fixtures_3d()[name], sampling)


def _check_global_edt(labels, sampling):
    """the argument of csrc/distance.hip: one EDT of the inner-boundary mask over the whole sample equals the EDT inside
    each object's bounding-box crop, on every voxel of the object (both with and without connected components)"""
    for apply_label in (True, False):
        ids = oracle_ids(labels, apply_label)
        b = boundaries_mode(ids.astype("int64"), "inner")[0]
        if not b.any():
            continue
        glob = ndimage.distance_transform_edt(b == 0, sampling=sampling)
        for lid in range(1, int(ids.max()) + 1):
            mask = ids == lid
            bb = _bbox(mask)
            crop = _crop_edt(b, bb, sampling)
            np.testing.assert_array_equal(glob[bb][mask[bb]], crop[mask[bb]])


def test_fixtures_cover_the_degenerate_cases():
    lab = rings_2d()
    _, centers = pod_oracle(lab, return_centers=True)
    ids = oracle_ids(lab)
    # some centroid is outside its object (rings, C-shapes, the split id under apply_label=False)
    moved = [lid for lid in centers if not ids[tuple(np.round(np.array(np.nonzero(ids == lid)).mean(1)).astype(int))] == lid]
    assert moved
    assert (np.bincount(ids.ravel()) == 1).sum() >= 2            # single voxels
    assert oracle_ids(lab, apply_label=True).max() == oracle_ids(lab, apply_label=False).max() + 1   # split id
    empty = pod_oracle(np.zeros((6, 7), "int64"))
    assert (empty[0] == 0).all() and (empty[1:] == 1.0).all()
    one = pod_oracle(lab == 5)
    assert np.isclose(one[1:, 30, 60], 0).all()


def test_oracle_numbering_conventions():
    lab = np.array([[0, 7, 7, 0, 3], [0, 0, 0, 0, 3], [7, 7, 0, 9, 0]])
    np.testing.assert_array_equal(oracle_ids(lab, True), [[0, 1, 1, 0, 2], [0, 0, 0, 0, 2], [3, 3, 0, 4, 0]])
    np.testing.assert_array_equal(oracle_ids(lab, False), [[0, 2, 2, 0, 1], [0, 0, 0, 0, 1], [2, 2, 0, 3, 0]])
    np.testing.assert_array_equal(oracle_ids(lab, True, min_size=2), [[0, 1, 1, 0, 2], [0, 0, 0, 0, 2], [3, 3, 0, 0, 0]])


def test_transform_constructor_matches_the_reference():
    from torch_em_amd.transform import PerObjectDistanceTransform
    with pytest.raises(ValueError, match="At least one"):
        PerObjectDistanceTransform(distances=False, boundary_distances=False, directed_distances=False)
    t = PerObjectDistanceTransform()
    assert (t.distances, t.boundary_distances, t.directed_distances, t.foreground, t.instances, t.apply_label,
            t.correct_centers, t.min_size, t.distance_fill_value, t.sampling) == (True, True, False, True, False, True,
                                                                                  True, 0, 1.0, None)
    assert t.eps == 1e-7


def test_distance_losses_constructor_and_scope():
    import torch.nn as nn
    from torch_em_amd.loss import DiceBasedDistanceLoss, DiceLoss, DistanceLoss
    assert DistanceLoss().init_kwargs == {"mask_distances_in_bg": True}
    assert DiceBasedDistanceLoss(mask_distances_in_bg=False).init_kwargs == {"mask_distances_in_bg": False}
    DistanceLoss(False, foreground_loss=DiceLoss(eps=1e-5), distance_loss=DiceLoss())
    with pytest.raises(NotImplementedError):
        DistanceLoss(distance_loss=nn.L1Loss())
    with pytest.raises(NotImplementedError):
        DistanceLoss(distance_loss=nn.MSELoss(reduction="sum"))
    with pytest.raises(NotImplementedError):
        DistanceLoss(foreground_loss=DiceLoss(reduce_channel=None))
    loss = DiceBasedDistanceLoss(True)
    with pytest.raises(AssertionError):
        loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))


def test_loss_golden_fixture_is_complete(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g12_distance_loss.npz"))
    cases = sorted({k.split(".")[0] for k in g.files})
    assert len(cases) >= 5
    for c in cases:
        assert {f"{c}.x", f"{c}.y", f"{c}.loss", f"{c}.grad"} <= set(g.files)
        assert np.isfinite(g[f"{c}.loss"]) and g[f"{c}.grad"].shape == g[f"{c}.x"].shape
