"""GPU: the vector EDT (tem_vector_edt) by property against the exact scipy distances, DistanceTransform against the
float64 restatement of the reference, and the six small label transforms bit for bit against their oracles
(tests/test_label_targets_cpu.py holds oracles and fixtures)."""
import itertools

import numpy as np
import pytest
import torch

from test_label_targets_cpu import (TIE_FREE, connected_components_oracle, distance_transform_oracle, ignore_label_oracle,
                                    label_consecutive_oracle, min_size_oracle, no_to_background_oracle, one_hot_oracle,
                                    small_fixtures, vdt_fixtures, vdt_oracle, with_ignore)

pytestmark = pytest.mark.gpu
DEV = "cuda"

FIX = vdt_fixtures()
SMALL = small_fixtures()
_EDT = {}
_ORACLE = {}


def _as4(lab):
    t = torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)
    return t.reshape((1,) + (1,) * (3 - lab.ndim) + lab.shape)


def _edt(name):
    """one run of the kernel per fixture, shared by the tests: (offsets [ndim, *shape], squared distance, empty flag, and
    the components of the unused leading axes)"""
    if name not in _EDT:
        from torch_em_amd import ops
        lab, fg = FIX[name]
        vec, d2, empty = ops.vector_edt(_as4(lab), fg)
        assert vec.dtype == torch.int32 and d2.dtype == torch.int32 and empty.dtype == torch.int32
        assert vec.shape == (1, 3) + tuple(_as4(lab).shape[1:]) and empty.shape == (1,)
        vec = vec.cpu().numpy()[0].reshape((3,) + lab.shape).astype("int64")
        _EDT[name] = (vec[3 - lab.ndim:], d2.cpu().numpy().reshape(lab.shape).astype("int64"), int(empty[0]),
                      vec[:3 - lab.ndim])
    return _EDT[name]


def _d2_oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = vdt_oracle(*FIX[name])
    return _ORACLE[name]


# ---- vector EDT ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIX))
def test_vector_edt_points_at_a_nearest_target(name):
    from torch_em_amd import ops
    lab, fg = FIX[name]
    vec, d2, empty, unused = _edt(name)
    exp_d2 = _d2_oracle(name)[0]
    assert (unused == 0).all()
    if exp_d2 is None:
        assert empty == 1 and (vec == 0).all() and (d2 == ops.VDT_NONE).all()
        return
    assert empty == 0
    tgt = np.indices(lab.shape) + vec
    for a, s in enumerate(lab.shape):
        assert (tgt[a] >= 0).all() and (tgt[a] < s).all()           # x + v(x) lies inside the volume ...
    assert (lab[tuple(tgt)] == fg).all()                           # ... on a target voxel ...
    np.testing.assert_array_equal((vec ** 2).sum(0), exp_d2)       # ... at the exact nearest distance,
    np.testing.assert_array_equal(d2, exp_d2)                      # which is also the distance returned
    assert (d2[lab == fg] == 0).all()


@pytest.mark.parametrize("name", TIE_FREE)
def test_vector_edt_equals_scipy_where_nothing_ties(name):
    np.testing.assert_array_equal(_edt(name)[0], _d2_oracle(name)[1])


def test_vector_edt_batch_equals_single_samples_bit_for_bit():
    from torch_em_amd import ops
    blobs, fg = FIX["blobs_33x47"]
    labs = np.stack([np.zeros_like(blobs), blobs, np.full_like(blobs, fg)])[:, None]
    t = torch.from_numpy(labs).to(DEV)
    vec, d2, empty = ops.vector_edt(t, fg)
    assert empty.tolist() == [1, 0, 0]
    assert (d2[2] == 0).all() and (vec[2] == 0).all()
    for n in range(3):
        v1, d1, e1 = ops.vector_edt(t[n:n + 1], fg)
        assert torch.equal(v1[0], vec[n]) and torch.equal(d1[0], d2[n]) and int(e1[0]) == int(empty[n])
    vol = np.stack([FIX["vol_6x7x8"][0], FIX["hyperplane_6x7x8"][0], np.zeros((6, 7, 8), "int64")])
    t = torch.from_numpy(vol).to(DEV)
    vec, d2, empty = ops.vector_edt(t, 1)
    assert empty.tolist() == [0, 0, 1]
    for n in range(3):
        v1, d1, _ = ops.vector_edt(t[n:n + 1], 1)
        assert torch.equal(v1[0], vec[n]) and torch.equal(d1[0], d2[n])


@pytest.mark.parametrize("name", ["checker_9x9", "two_symmetric", "voronoi_cell", "line_300x5"])
def test_vector_edt_two_runs_are_bit_identical(name):
    from torch_em_amd import ops
    lab, fg = FIX[name]
    a = ops.vector_edt(_as4(lab), fg)
    b = ops.vector_edt(_as4(lab), fg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- DistanceTransform ---------------------------------------------------------------------------------------------
KINDS = [dict(distances=True, directed_distances=False), dict(distances=False, directed_distances=True),
         dict(distances=True, directed_distances=True)]
CONFIGS = [dict(k, normalize=nrm, max_distance=md, invert=inv)
           for k, nrm, md, inv in itertools.product(KINDS, (True, False), (None, 5), (False, True))]


def _close(got, exp, cfg, what):
    """normalised or inverted channels: 1e-6 absolute; un-normalised ones: 2^-22 relative (one float32 sqrtf at 1 ulp plus
    the oracle's rounding to float32); every figure is printed before it is asserted"""
    got = np.asarray(got, dtype="float64")
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    err = np.abs(got - exp)
    if cfg["normalize"] or cfg["invert"]:
        print(f"{what}: max abs err {err.max():.3e} (bound 1e-6)")
        assert err.max() <= 1e-6, (what, float(err.max()))
    else:
        rel = float((err / np.maximum(np.abs(exp), 1e-300)).max()) if (exp != 0).any() else 0.0
        print(f"{what}: max rel err {rel:.3e} (bound 2^-22)")
        assert (err <= 2.0 ** -22 * np.abs(exp)).all(), (what, rel)


def _check_distance_transform(name, cfg, out):
    lab, fg = FIX[name]
    nd = 1 if cfg["distances"] else 0
    both = cfg["distances"] and cfg["directed_distances"]
    shape = lab.shape if not cfg["directed_distances"] else (nd + lab.ndim,) + lab.shape
    assert out.shape == shape and out.dtype == np.float32, (name, out.shape, out.dtype)
    pure = distance_transform_oracle(lab, foreground_id=fg, **cfg)
    if cfg["distances"]:   # independent of ties: the pure scipy oracle
        _close(out[0] if both else out, pure[0] if both else pure, cfg, f"{name} distances")
    if cfg["directed_distances"]:   # the oracle shares the kernel's (property-tested) choice among equally near voxels
        shared = distance_transform_oracle(lab, vectors=_edt(name)[0], foreground_id=fg, **cfg)
        _close(out[nd:], shared[nd:], cfg, f"{name} directed")
        if name in TIE_FREE:
            _close(out[nd:], pure[nd:], cfg, f"{name} directed, pure scipy")


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_distance_transform_matches_oracle(ci):
    from torch_em_amd.transform import DistanceTransform
    cfg = CONFIGS[ci]
    for name in sorted(FIX):
        lab, fg = FIX[name]
        out = DistanceTransform(foreground_id=fg, **cfg)(torch.from_numpy(lab).to(DEV))
        assert out.is_cuda and out.dtype == torch.float32
        _check_distance_transform(name, cfg, out.cpu().numpy())


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name", ["empty_6x7", "empty_4x5x6", "voronoi_absent"])
def test_distance_transform_empty_sample(name, invert):
    from torch_em_amd.transform import DistanceTransform
    lab, fg = FIX[name]
    for normalize in (True, False):
        cfg = dict(distances=True, directed_distances=True, normalize=normalize, max_distance=None, invert=invert)
        out = DistanceTransform(foreground_id=fg, **cfg)(torch.from_numpy(lab).to(DEV)).cpu().numpy()
        exp = distance_transform_oracle(lab, foreground_id=fg, **cfg)
        if not normalize:   # the oracle's fill behaviour itself: the fill vector, or all zeros when inverted
            fill = 0.0 if invert else np.sqrt(sum(s * s for s in lab.shape) / 2)
            np.testing.assert_allclose(exp[1:], fill, rtol=1e-12)
            np.testing.assert_allclose(exp[0], fill * np.sqrt(lab.ndim), rtol=1e-12)
        if normalize or invert:
            assert np.abs(out - exp).max() <= 1e-6
        else:
            assert (np.abs(out - exp) <= 2.0 ** -22 * np.abs(exp)).all()


def test_distance_transform_func_batches_and_numpy():
    from torch_em_amd.transform import DistanceTransform
    lab, fg = FIX["blobs_33x47"]
    t = torch.from_numpy(lab).to(DEV)
    cfg = dict(distances=True, directed_distances=False, normalize=True, max_distance=None, invert=False)
    out = DistanceTransform(foreground_id=fg, func=torch.sqrt)(t)
    exp = distance_transform_oracle(lab, foreground_id=fg, func=np.sqrt, **cfg)
    _close(out.cpu().numpy(), exp, cfg, "func=sqrt")
    # func on each part before concatenation
    both = DistanceTransform(foreground_id=fg, directed_distances=True, func=torch.abs)(t)
    plain = DistanceTransform(foreground_id=fg, directed_distances=True)(t)
    assert torch.equal(both, plain.abs()) and both.shape == (3,) + lab.shape
    # batches [N, 1, *spatial] -> [N, C, *spatial], samples independent: equal to the single calls bit for bit
    labs2 = np.stack([np.zeros_like(lab), lab, np.full_like(lab, fg)])[:, None]
    labs3 = np.stack([FIX["vol_6x7x8"][0], FIX["hyperplane_6x7x8"][0], np.zeros((6, 7, 8), "int64")])[:, None]
    for labs, f in ((labs2, fg), (labs3, 1)):
        for kw in (dict(), dict(directed_distances=True, invert=True), dict(distances=False, directed_distances=True),
                   dict(func=torch.sqrt)):
            tr = DistanceTransform(foreground_id=f, **kw)
            tb = torch.from_numpy(labs).to(DEV)
            out = tr(tb)
            nc = int(kw.get("distances", True)) + (labs.ndim - 2 if kw.get("directed_distances") else 0)
            assert out.shape == (labs.shape[0], nc) + labs.shape[2:] and out.dtype == torch.float32 and out.is_cuda
            for n in range(labs.shape[0]):
                single = tr(tb[n, 0])
                assert torch.equal(out[n] if kw.get("directed_distances") else out[n, 0], single), (kw, n)
    # numpy in -> numpy out, the same numbers
    arr = DistanceTransform(foreground_id=fg, directed_distances=True)(lab)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32
    np.testing.assert_array_equal(arr, plain.cpu().numpy())
    arrb = DistanceTransform(foreground_id=fg)(labs2)
    assert isinstance(arrb, np.ndarray) and arrb.shape == (3, 1) + lab.shape


def test_label_targets_make_no_host_sync():
    from torch_em_amd.transform import (BoundaryTransformWithIgnoreLabel, DistanceTransform, MinSizeLabelTransform,
                                        NoToBackgroundBoundaryTransform, OneHotTransform, connected_components,
                                        label_consecutive)
    labs = torch.from_numpy(np.stack([SMALL["blobs_33x47"], SMALL["blobs_33x47"][::-1].copy()])[:, None]).to(DEV)
    calls = [DistanceTransform(directed_distances=True, invert=True), MinSizeLabelTransform(5, ensure_zero=True),
             NoToBackgroundBoundaryTransform(add_binary_target=True), BoundaryTransformWithIgnoreLabel(mode="outer"),
             OneHotTransform([0, 1, 3]), lambda y: connected_components(y, ensure_zero=True),
             lambda y: label_consecutive(y, with_background=False)]
    for c in calls:
        c(labs)   # load the library, fill the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c(labs) for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(o.is_cuda and o.shape[0] == 2 for o in outs)


# ---- the small transforms ------------------------------------------------------------------------------------------
def _dev(lab):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)


def _exact(out, exp, dtype):
    assert out.is_cuda and out.dtype == dtype, (out.device, out.dtype)
    got = out.cpu().numpy()
    assert got.shape == exp.shape, (got.shape, exp.shape)
    np.testing.assert_array_equal(got, exp)


def _pair(lab):
    """two different samples of one shape, as a batch [2, 1, *spatial]"""
    return np.stack([lab, np.ascontiguousarray(lab[::-1])])[:, None]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_connected_components_and_label_consecutive(name):
    from torch_em_amd.transform import connected_components, label_consecutive
    lab = SMALL[name]
    for ez in (False, True):
        _exact(connected_components(_dev(lab), ensure_zero=ez), connected_components_oracle(lab, ez), torch.int32)
        _exact(connected_components(_dev(lab[None]), ndim=lab.ndim, ensure_zero=ez), connected_components_oracle(lab, ez),
               torch.int32)
        batch = connected_components(_dev(_pair(lab)), ensure_zero=ez)
        for n in range(2):
            _exact(batch[n, 0], connected_components_oracle(_pair(lab)[n, 0], ez), torch.int32)
    for wb in (True, False):
        _exact(label_consecutive(_dev(lab), with_background=wb), label_consecutive_oracle(lab, wb), torch.int32)
        batch = label_consecutive(_dev(_pair(lab)), with_background=wb)
        assert batch.shape == _pair(lab).shape
        _exact(batch[1, 0], label_consecutive_oracle(_pair(lab)[1, 0], wb), torch.int32)
    sparse = lab * 7 + (lab > 2) * 100          # ids far apart, still ascending
    _exact(label_consecutive(_dev(sparse)), label_consecutive_oracle(sparse), torch.int32)
    out = connected_components(lab)              # numpy in -> numpy out
    assert isinstance(out, np.ndarray) and out.dtype == np.int32
    np.testing.assert_array_equal(out, connected_components_oracle(lab))


@pytest.mark.parametrize("ensure_zero", [False, True])
@pytest.mark.parametrize("min_size", [None, 1, 25])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_min_size_label_transform(name, min_size, ensure_zero):
    from torch_em_amd.transform import MinSizeLabelTransform
    lab = SMALL[name]
    tr = MinSizeLabelTransform(min_size, ensure_zero=ensure_zero)
    _exact(tr(_dev(lab)), min_size_oracle(lab, min_size, ensure_zero), torch.int32)
    batch = tr(_dev(_pair(lab)))
    assert batch.shape == _pair(lab).shape
    for n in range(2):
        _exact(batch[n, 0], min_size_oracle(_pair(lab)[n, 0], min_size, ensure_zero), torch.int32)
    _exact(MinSizeLabelTransform(min_size, ndim=lab.ndim, ensure_zero=ensure_zero)(_dev(lab[None])),
           min_size_oracle(lab, min_size, ensure_zero), torch.int32)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_one_hot_transform(name):
    from torch_em_amd.transform import OneHotTransform
    lab = SMALL[name]
    for ids in (3, [5, 1, 42, 0], None):
        _exact(OneHotTransform(ids)(_dev(lab)), one_hot_oracle(lab, ids), torch.float32)
    batch = OneHotTransform([5, 1, 42, 0])(_dev(_pair(lab)))
    assert batch.shape == (2, 4) + lab.shape
    for n in range(2):
        _exact(batch[n], one_hot_oracle(_pair(lab)[n, 0], [5, 1, 42, 0]), torch.float32)
    with pytest.raises(ValueError, match="class_ids"):
        OneHotTransform()(_dev(_pair(lab)))
    out = OneHotTransform(3)(lab)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    np.testing.assert_array_equal(out, one_hot_oracle(lab, 3))


@pytest.mark.parametrize("add_binary", [False, True])
@pytest.mark.parametrize("mode", ["thick", "inner", "outer"])
@pytest.mark.parametrize("ignore_present", [False, True])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_masked_boundary_transforms(name, ignore_present, mode, add_binary):
    from torch_em_amd.transform import BoundaryTransformWithIgnoreLabel, NoToBackgroundBoundaryTransform
    lab = with_ignore(SMALL[name]) if ignore_present else SMALL[name]
    cases = [(NoToBackgroundBoundaryTransform(mode=mode, add_binary_target=add_binary),
              lambda a: no_to_background_oracle(a, mode=mode, add_binary_target=add_binary)),
             (NoToBackgroundBoundaryTransform(bg_label=1, mask_label=-1, mode=mode, add_binary_target=add_binary),
              lambda a: no_to_background_oracle(a, bg_label=1, mode=mode, add_binary_target=add_binary)),
             (BoundaryTransformWithIgnoreLabel(mode=mode, add_binary_target=add_binary),
              lambda a: ignore_label_oracle(a, mode=mode, add_binary_target=add_binary)),
             (BoundaryTransformWithIgnoreLabel(ignore_label=3, mode=mode, add_binary_target=add_binary),
              lambda a: ignore_label_oracle(a, ignore_label=3, mode=mode, add_binary_target=add_binary))]
    for tr, oracle in cases:
        _exact(tr(_dev(lab)), oracle(lab), torch.int8)
        batch = tr(_dev(_pair(lab)))
        assert batch.shape == (2, 2 if add_binary else 1) + lab.shape
        for n in range(2):
            _exact(batch[n], oracle(_pair(lab)[n, 0]), torch.int8)
    out = cases[0][0](lab)
    assert isinstance(out, np.ndarray) and out.dtype == np.int8
    np.testing.assert_array_equal(out, cases[0][1](lab))


# ---- limits, trainer -----------------------------------------------------------------------------------------------
def test_oversized_line_is_refused_with_the_library_error():
    from torch_em_amd import ops
    from torch_em_amd.transform import DistanceTransform, PerObjectDistanceTransform
    lab = torch.zeros((1, 4097), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        PerObjectDistanceTransform()(lab)
    with pytest.raises(ValueError, match="4096"):
        DistanceTransform()(lab)
    with pytest.raises(ValueError, match="4096"):
        ops.vector_edt(lab.reshape(1, 1, 4097, 1), 1)
    torch.cuda.synchronize()


def _two_steps(tmp_path, name, ys, target_transform):
    from torch_em_amd.loss import DistanceLoss
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.trainer import DefaultTrainer
    xs = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(0))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(xs, ys), batch_size=2)
    torch.manual_seed(0)
    model = UNet2d(1, 3, depth=2, initial_features=8)
    trainer = DefaultTrainer(name=name, train_loader=loader, val_loader=loader, model=model,
                             loss=DistanceLoss(mask_distances_in_bg=False), optimizer=FusedAdamW(model.parameters(), lr=1e-3),
                             metric=DistanceLoss(mask_distances_in_bg=False), device=DEV, save_root=str(tmp_path), logger=None,
                             target_transform=target_transform)
    trainer.fit(iterations=2)
    return {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}


def test_trainer_with_distance_targets_equals_precomputed_targets(tmp_path):
    from torch_em_amd.transform import DistanceTransform
    from test_distance_cpu import blobs_2d
    labs = torch.from_numpy(np.stack([blobs_2d(s, shape=(32, 32), sigma=2.0, frac=0.3) for s in (4, 5)])[:, None])
    tt = DistanceTransform(directed_distances=True)
    on_device = _two_steps(tmp_path, "dt_device", labs, tt)
    targets = tt(labs.to(DEV)).cpu()
    assert targets.shape == (2, 3, 32, 32) and targets.dtype == torch.float32
    precomputed = _two_steps(tmp_path, "dt_precomputed", targets, None)
    assert on_device.keys() == precomputed.keys()
    for k in on_device:
        assert torch.equal(on_device[k], precomputed[k]), k
