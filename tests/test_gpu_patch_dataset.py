"""GPU: patch supply from device-resident volumes (csrc/patch.hip, ops.patch_*, data/device_dataset.py) -- every op against
numpy slicing / np.unique / np.pad, the dataset and loader against the reference's recorded runs (G21,
tests/golden/gen_golden_patch_dataset.py).  Everything compared is an integer or an exactly converted value: bit for bit, no
tolerance.  Every op runs twice and must give equal bits, and the volumes must equal their host copies afterwards.

Shapes: volume A (9, 20, 37) with patch (4, 8, 16) -- W is no multiple of 4, so rows start at every alignment --, volume B
(1, 33, 35) with patch (1, 16, 16), volume C (3, 20, 37), shorter than the patch in z (padding).  Box sets: one box at odd offsets
(M = 1), the eight corners plus one odd box (M = 9), and a mixed set over two volumes with a whole-volume box (rows that follow
each other in memory) and a box clipped by the volume."""
import pickle

import numpy as np
import pytest
import torch

from patch_dataset_kit import crop, fixture, pad_to, runs_of, sampler_of, volumes_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 2024
A, B, C = (9, 20, 37), (1, 33, 35), (3, 20, 37)
PATCH = (4, 8, 16)
NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64,
      torch.float32: np.float32}
# (volume, z0, y0, x0, dz, dy, dx)
ONE = [(0, 1, 3, 7, 4, 8, 16)]
CORNERS9 = [(0, z, y, x, 4, 8, 16) for z in (0, 5) for y in (0, 12) for x in (0, 21)] + [(0, 3, 5, 11, 3, 7, 13)]
MIXED = [(0, 0, 0, 0, 9, 20, 37), (1, 0, 17, 19, 1, 16, 16), (1, 0, 0, 0, 1, 33, 35), (0, 5, 12, 21, 4, 8, 16), (0, 8, 19, 36, 1, 1, 1)]
BOX_SETS = {"one": ONE, "corners9": CORNERS9, "mixed": MIXED}


def ops():
    from torch_em_amd import ops
    return ops


def label_arrays(np_dtype, n_ids=70):
    """label volumes A and B with runs of 5 that cross the row ends (37 and 35 are no multiples of 5), single-voxel runs, ids
    up to n_ids - 1"""
    out = []
    for shape in (A, B):
        n = int(np.prod(shape))
        flat = (np.arange(n) // 5) % n_ids
        flat[::11] = n_ids - 1
        flat[3::17] = 0
        out.append(flat.reshape(shape).astype(np_dtype))
    return out


def device_volumes(arrays):
    """PatchVolumes of host arrays [C, D, H, W] (or [D, H, W]) and the host copies"""
    arrays = [a if a.ndim == 4 else a[None] for a in arrays]
    return ops().PatchVolumes([torch.from_numpy(a.copy()).to(DEV) for a in arrays]), arrays


def box_of(arrays, b, channel=0):
    v, z0, y0, x0, dz, dy, dx = b
    return arrays[v][channel, z0:z0 + dz, y0:y0 + dy, x0:x0 + dx]


def intact(vols, arrays):
    return all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(vols.volumes, arrays))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("boxes", list(BOX_SETS))
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.int32, torch.int64])
def test_patch_count(dtype, boxes):
    vols, arrays = device_volumes(label_arrays(NP[dtype]))
    bx = BOX_SETS[boxes]
    for value in (0, 69, 3, 10 ** 6 if dtype in (torch.uint8, torch.uint16) else -1):
        got = ops().patch_count(vols, bx, value)
        again = ops().patch_count(vols, bx, value)
        want = [[int((box_of(arrays, b).astype(np.int64) != value).sum()), int((box_of(arrays, b) != box_of(arrays, b).flat[0]).sum())]
                for b in bx]
        assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want, (value, got.cpu().numpy().tolist(), want)
        assert same_bits(got, again)
    assert intact(vols, arrays)


@pytest.mark.parametrize("boxes", list(BOX_SETS))
@pytest.mark.parametrize("n_ids,path", [(1, 0), (70, 0), (9000, 1)])
def test_patch_hist_and_reduce(n_ids, path, boxes):
    o = ops()
    assert o.patch_hist_path(n_ids) == path
    vols, arrays = device_volumes(label_arrays(np.int32, n_ids))
    bx = BOX_SETS[boxes]
    hist = o.patch_hist(vols, bx, n_ids)
    want = np.stack([np.bincount(box_of(arrays, b).ravel(), minlength=n_ids) for b in bx]).astype(np.int32)
    assert np.array_equal(hist.cpu().numpy(), want)
    assert same_bits(hist, o.patch_hist(vols, bx, n_ids))
    assert int(want.sum()) == sum(b[4] * b[5] * b[6] for b in bx)
    rs = np.random.RandomState(n_ids)
    excluded = (rs.rand(n_ids) < 0.3).astype(np.int32)
    excluded[0] = 0
    for min_size in (0, 1, 3, 6):
        got = o.patch_hist_instances(hist, torch.from_numpy(excluded).to(DEV), min_size)
        ref = ((want >= max(min_size, 1)) & (excluded[None] == 0)).sum(1).astype(np.int32)
        assert np.array_equal(got.cpu().numpy(), ref), min_size
        assert same_bits(got, o.patch_hist_instances(hist, torch.from_numpy(excluded).to(DEV), min_size))
    ids = np.array([0, n_ids - 1, -1, n_ids // 2, n_ids - 1], dtype=np.int32)
    listed = o.patch_hist_listed(hist, torch.from_numpy(ids).to(DEV))
    ref = np.stack([np.where(ids >= 0, want[m][np.maximum(ids, 0)], 0) for m in range(len(bx))]).astype(np.int32)
    assert np.array_equal(listed.cpu().numpy(), ref)
    assert same_bits(listed, o.patch_hist_listed(hist, torch.from_numpy(ids).to(DEV)))
    assert intact(vols, arrays)


def test_patch_hist_paths_and_unique():
    """the path is a function of n_ids alone (LDS table up to 8192 ids); the histogram is np.unique's (ids, counts)"""
    o = ops()
    assert [o.patch_hist_path(n) for n in (0, 1, 8192, 8193)] == [-1, 0, 0, 1]
    vols, arrays = device_volumes(label_arrays(np.int32, 70))
    for n_ids in (70, 8193):   # the same boxes through both kernels
        hist = o.patch_hist(vols, MIXED, n_ids).cpu().numpy()
        for h, b in zip(hist, MIXED):
            ids, counts = np.unique(box_of(arrays, b), return_counts=True)
            assert np.array_equal(np.nonzero(h)[0], ids) and np.array_equal(h[ids], counts)
    with pytest.raises(ValueError):
        o.patch_hist(vols, MIXED, 0)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.int16, torch.float32])
def test_patch_gather_raw(dtype, channels):
    """raw of every dtype -> float32, exactly, zero-padded to the patch (np.pad constant mode), C in 1 and 3"""
    rs = np.random.RandomState(3)
    lo, hi = (-3e4, 3e4) if dtype == torch.int16 else (0, 255 if dtype == torch.uint8 else 65535)
    arrays = [rs.uniform(lo, hi, (channels,) + s).astype(NP[dtype]) for s in (A, C)]
    if dtype == torch.float32:
        arrays[0].reshape(-1)[:4] = [-0.0, np.inf, 1e-45, -3.0e38]
    vols, arrays = device_volumes(arrays)
    boxes = CORNERS9 + [(1, 0, 12, 21, 3, 8, 16), (1, 0, 0, 1, 3, 8, 16), (0, 8, 19, 36, 1, 1, 1)]   # the last three are padded
    got = ops().patch_gather(vols, boxes, PATCH, torch.float32)
    assert tuple(got.shape) == (len(boxes), channels) + PATCH and got.dtype == torch.float32
    want = np.stack([pad_to(np.stack([box_of(arrays, b, c) for c in range(channels)]).astype(np.float32), PATCH) for b in boxes])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert same_bits(got, ops().patch_gather(vols, boxes, PATCH, torch.float32))
    one = ops().patch_gather(vols, ONE, PATCH, torch.float32)
    assert np.array_equal(one.cpu().numpy()[0, 0], box_of(arrays, ONE[0]).astype(np.float32))
    assert intact(vols, arrays)


@pytest.mark.parametrize("out_dtype", [torch.int32, torch.int64, torch.float32])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.int32, torch.int64])
def test_patch_gather_labels(dtype, out_dtype):
    vols, arrays = device_volumes(label_arrays(NP[dtype]))
    if dtype == torch.int64 and out_dtype == torch.int64:
        arrays[0][0, 5, 12, 21:24] = [2 ** 40 + 1, -2 ** 50, 7]   # values only 64 bits hold
        vols, arrays = device_volumes(arrays)
    boxes = MIXED[1:]
    patch = (4, 33, 35)
    got = ops().patch_gather(vols, boxes, patch, out_dtype)
    want = np.stack([pad_to(box_of(arrays, b)[None].astype(NP[out_dtype]), patch) for b in boxes])
    assert got.dtype == out_dtype and np.array_equal(got.cpu().numpy(), want)
    assert same_bits(got, ops().patch_gather(vols, boxes, patch, out_dtype))
    assert intact(vols, arrays)


def test_boxes_are_checked_on_the_host():
    """a box that leaves its volume never reaches a kernel: the wrapper raises"""
    vols, arrays = device_volumes(label_arrays(np.int32))
    for bad in ((0, 6, 0, 0, 4, 8, 16), (0, 0, 0, 22, 4, 8, 16), (0, 0, -1, 0, 4, 8, 16), (2, 0, 0, 0, 1, 1, 1), (0, 0, 0, 0, 0, 8, 16),
                (1, 0, 0, 0, 2, 8, 16)):
        for call in (lambda b: ops().patch_count(vols, [ONE[0], b], 0), lambda b: ops().patch_hist(vols, [b], 70),
                     lambda b: ops().patch_gather(vols, [b], PATCH, torch.int32)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match="fit the patch"):
        ops().patch_gather(vols, [(0, 0, 0, 0, 5, 8, 16)], PATCH, torch.int32)
    with pytest.raises(ValueError):
        ops().patch_count(device_volumes([np.zeros(A, np.float32)])[0], ONE, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops().PatchVolumes([torch.zeros((1,) + A)])
    assert intact(vols, arrays)


def dataset_of(cfg, **kw):
    from torch_em_amd.data import DeviceSegmentationDataset
    raw, labels, roi, _, _ = volumes_of(cfg)
    return DeviceSegmentationDataset(raw, labels, tuple(cfg["patch"]), sampler=sampler_of(cfg), roi=roi,
                                     with_channels=bool(cfg.get("with_channels")), ndim=cfg.get("ndim"), device=DEV, **kw)


STORED = [n for n in fixture()["configs"] if n != "never"]


@pytest.mark.parametrize("per_round", [3, 8])
@pytest.mark.parametrize("name", STORED)
def test_loader_reproduces_the_reference(name, per_round):
    """batch 0 of a loader with batch_size 3 holds the samples 0, 1, 2 of the fixture: the boxes tried, the coins consumed, and
    the crop the reference returned -- raw converted exactly to float32, labels to int64, zero padding, squeezed axis"""
    from torch_em_amd.data import DevicePatchLoader
    cfg = fixture()["configs"][name]
    ds = dataset_of(cfg)
    runs = runs_of(name)
    loader = DevicePatchLoader(ds, batch_size=len(runs), seed=SEED, candidates_per_round=per_round)
    x, y = loader.batch(0)
    assert x.dtype == torch.float32 and y.dtype == torch.int64 and x.is_cuda and y.is_cuda and y.shape[1] == 1
    x, y = x.cpu().numpy(), y.cpu().numpy()
    for i, (starts, coins, want_raw, want_labels) in enumerate(runs):
        c = loader.last_candidates[i]
        assert np.array_equal(np.array(c.starts), starts) and c.coins == coins.tolist(), (name, i)
        got_raw = x[i] if cfg.get("with_channels") else x[i, 0]
        assert got_raw.shape == want_raw.shape and np.array_equal(got_raw, want_raw.astype(np.float32)), (name, i)
        assert np.array_equal(y[i, 0], want_labels.astype(np.int64)), (name, i)
    again = DevicePatchLoader(ds, batch_size=len(runs), seed=SEED, candidates_per_round=per_round).batch(0)
    assert np.array_equal(again[0].cpu().numpy(), x) and np.array_equal(again[1].cpu().numpy(), y)


def test_loader_sample_numbers_and_ranks():
    """sample s = (batch_index * world_size + rank) * batch_size + i: two ranks with batch size 1 deal the fixture's samples
    0, 1, 2 as rank 0 / batch 0, rank 1 / batch 0, rank 0 / batch 1; iterating advances batch_index"""
    from torch_em_amd.data import DevicePatchLoader
    cfg = fixture()["configs"]["inst"]
    ds = dataset_of(cfg, n_samples=4)
    runs = runs_of("inst")
    r0 = DevicePatchLoader(ds, 1, SEED, candidates_per_round=3, rank=0, world_size=2)
    r1 = DevicePatchLoader(ds, 1, SEED, candidates_per_round=3, rank=1, world_size=2)
    assert len(r0) == 2 and r0.shuffle is True and r0.dataset is ds and r0.batch_size == 1
    b0 = [y.cpu().numpy()[0, 0] for _, y in r0]
    assert r0.batch_index == 2 and np.array_equal(b0[0], runs[0][3]) and np.array_equal(b0[1], runs[2][3])
    assert np.array_equal(r1.batch(0)[1].cpu().numpy()[0, 0], runs[1][3])


def test_loader_gives_up_like_the_reference():
    from torch_em_amd.data import DevicePatchLoader
    cfg = fixture()["configs"]["never"]
    assert int(fixture()["never/raises"]) == 1
    loader = DevicePatchLoader(dataset_of(cfg), batch_size=2, seed=SEED, candidates_per_round=8)
    with pytest.raises(RuntimeError, match="Could not sample a valid batch in 500 attempts"):
        loader.batch(0)


def test_two_volume_dataset():
    """two volumes of different shapes whose label ids differ (one dense numbering is made for both): a sample first draws its
    volume; the boxes and crops equal a host replay of the same streams with criteria computed in numpy"""
    from torch_em_amd.data import DevicePatchLoader, DeviceSegmentationDataset, MinInstanceSampler
    from torch_em_amd.data.device_dataset import Candidate, sample_state, speculate
    fx = fixture()
    r0, l0 = fx["vol/a/raw"], fx["vol/a/labels"]
    r1, l1 = np.ascontiguousarray(r0[2:, :15, 4:]), np.ascontiguousarray(l0[2:, :15, 4:])
    l1 = np.where(l1 > 0, l1 * 1000 + 1, 0).astype(l0.dtype)
    sampler = MinInstanceSampler(min_num_instances=2, min_size=4, exclude_ids=[7001, 12], p_reject=0.9)
    ds = DeviceSegmentationDataset([r0, r1], [l0, l1], PATCH, sampler=sampler, n_samples=8, device=DEV)
    assert ds.n_ids == 1 + len(np.union1d(np.unique(l0[l0 > 0]), np.unique(l1[l1 > 0])))
    loader = DevicePatchLoader(ds, batch_size=8, seed=11, candidates_per_round=3)
    x, y = (t.cpu().numpy() for t in loader.batch(0))
    raws, labels, crit = (r0, r1), (l0, l1), sampler.device_criterion()
    seen = set()
    for i in range(8):
        rs = sample_state(11, i)
        v = int(rs.randint(0, 2))
        seen.add(v)
        cand = Candidate(rs, v, [sh - p for sh, p in zip(labels[v].shape, PATCH)])

        def judge(items):
            from patch_dataset_kit import numpy_stat
            return [crit.met(numpy_stat(crit, *crop(raws[v], labels[v], st, PATCH)), int(np.prod(PATCH))) for _, _, st in items]
        start = speculate([cand], judge, sampler.p_reject, 5)[0]
        got = loader.last_candidates[i]
        assert got.volume == v and got.starts == cand.starts and got.coins == cand.coins
        want_raw, want_labels = crop(raws[v], labels[v], start, PATCH)
        assert np.array_equal(x[i, 0], want_raw.astype(np.float32)) and np.array_equal(y[i, 0], want_labels)
    assert seen == {0, 1}


def test_dataset_pickles_without_its_volumes():
    cfg = fixture()["configs"]["inst"]
    ds = dataset_of(cfg)
    blob = pickle.dumps(ds)
    assert len(blob) < 20000   # the configuration, not 6660 voxels twice and their dense ids
    back = pickle.loads(blob)
    assert back.raw is None and back.labels is None and back.patch_shape == PATCH and back.sampler.min_num_instances == 3
    from torch_em_amd.data import DevicePatchLoader
    with pytest.raises(RuntimeError, match="has not been properly deserialized"):
        DevicePatchLoader(back, 1, 0).batch(0)
    assert ds.raw is not None and DevicePatchLoader(ds, 1, SEED).batch(0)[0].shape == (1, 1) + PATCH


def test_samplers_outside_the_device_path_are_refused():
    from torch_em_amd.data import DeviceSegmentationDataset, MinIntensitySampler
    fx = fixture()
    for sampler in (MinIntensitySampler(1, "mean"), lambda x, y: True):
        with pytest.raises(NotImplementedError, match="TensorDataset"):
            DeviceSegmentationDataset(fx["vol/a/raw"], fx["vol/a/labels"], PATCH, sampler=sampler, device=DEV)
    with pytest.raises(NotImplementedError):
        DeviceSegmentationDataset(fx["vol/a/raw"], fx["vol/a/labels"], None, device=DEV)


def test_trainer_runs_on_a_device_patch_loader(tmp_path):
    """the pieces connect: DefaultTrainer trains three iterations on 16^3 patches a MinInstanceSampler accepted, with the
    trainer's own on-device raw transform and BatchTargets, through the factory's `resident_device`"""
    import functools

    import torch_em_amd
    from torch_em_amd.data import DevicePatchLoader, DeviceSegmentationDataset, MinInstanceSampler
    from torch_em_amd.model import UNet3d
    from torch_em_amd.transform import BoundaryTransform, standardize
    from torch_em_amd.transform.label import BatchTargets
    rs = np.random.RandomState(0)
    labels = np.zeros((24, 28, 40), np.uint16)
    labels[2:12, 3:14, 5:20], labels[10:22, 12:26, 18:38], labels[14:20, 2:9, 2:10] = 1, 2, 3
    raw = (rs.rand(*labels.shape) * 100 + 100 * (labels > 0)).astype(np.uint8)
    sampler = MinInstanceSampler(min_num_instances=3)
    loader = torch_em_amd.default_segmentation_loader([raw], None, [labels], None, batch_size=2, patch_shape=(16, 16, 16),
                                                      sampler=sampler, n_samples=6, label_dtype=torch.int64, resident_device=DEV, seed=5)
    assert isinstance(loader, DevicePatchLoader) and isinstance(loader.dataset, DeviceSegmentationDataset) and len(loader) == 3
    torch.manual_seed(0)
    model = UNet3d(1, 2, depth=2, initial_features=4)
    trainer = torch_em_amd.default_segmentation_trainer(
        "patches", model, loader, loader, device=DEV, logger=None, save_root=str(tmp_path),
        raw_transform=functools.partial(standardize, per_sample=True),
        target_transform=BatchTargets(BoundaryTransform(add_binary_target=True, ndim=3)))
    before = torch.cat([p.detach().flatten() for p in model.parameters()]).cpu().clone()
    trainer.fit(iterations=3)
    after = torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()
    assert trainer._iteration == 3 and loader.batch_index >= 3 and torch.isfinite(after).all() and not torch.equal(before, after)
    for c in loader.last_candidates:   # what was trained on is what the sampler accepts
        st = c.accepted
        patch = labels[st[0]:st[0] + 16, st[1]:st[1] + 16, st[2]:st[2] + 16]
        assert len(np.unique(patch)) >= 3 or c.coins
