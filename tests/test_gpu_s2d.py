"""GPU: the Shallow2Deep front end -- the Gaussian 2-jet feature bank (csrc/filters.hip), the random forest
(csrc/forest.hip) and `torch_em_amd.shallow2deep` -- against the numpy / scipy oracle tests/s2d_ref.py.  Filters are judged
by oracle.judge's rule (error in units of 2^-23 x scale at most MARGIN * max(e32, 1)); forests and compositions bit for bit."""
import functools
import pickle
from functools import partial

import numpy as np
import pytest
import torch

import s2d_ref as R
from oracle import judge
from oracle.gpu_kit import DEV

pytestmark = pytest.mark.gpu

SHAPES = {3: (7, 19, 37), 2: (33, 70)}
SIGMAS = {"0.7": 0.7, "1.6": 1.6, "aniso": (0.7, 1.6, 3.5), "5.0": 5.0, "7.5": 7.5}    # 7.5: radius 30, x and y passes apart


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pick(a, channel):
    return a if channel is None else a[list(channel)] if isinstance(channel, tuple) else a[channel]


def as4(x, ndim):
    """[N, *sample] -> the [N, D, H, W] the ops take"""
    return x if ndim == 3 else x[:, None]


@functools.lru_cache(maxsize=None)
def noise(shape, seed=11):
    return np.random.RandomState(seed).randn(2, *shape).astype(np.float32)


def judged(name, x, sigma, outer=None):
    """one filter on a batch [N, *sample]: every sample within the band; -> the device's result [N, F, *sample]"""
    from torch_em_amd import ops
    kw = {} if outer is None else {"outer_sigma": outer}
    got = getattr(ops, name)(dev(as4(x, x.ndim - 1)), sigma, **kw).cpu().numpy().reshape((len(x), -1) + x.shape[1:])
    for n, sample in enumerate(x):
        ref, f32, scale = (R.apply(name, sample, sigma, outer, how) for how in ("f64", "f32", "scale"))
        ek, e32 = judge.units(got[n], ref, scale), judge.units(f32, ref, scale)
        print(f"S2D_ERR {name} {x.shape[1:]} sigma {sigma} outer {outer} sample {n}: kernel {ek:.2f} f32 {e32:.2f}")
        assert judge.within(ek, e32), (name, sigma, n, ek, e32)
    return got


@pytest.mark.parametrize("key", ["0.7", "1.6", "aniso"])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("name", R.FILTERS)
def test_filter_against_float64(name, ndim, key):
    sigma = SIGMAS[key] if key != "aniso" else SIGMAS[key][3 - ndim:]
    outer = None if name != R.FILTERS[4] else (tuple(2 * s for s in sigma) if key == "aniso" else 0.5 * sigma)
    judged(name, noise(SHAPES[ndim]), sigma, outer)


@pytest.mark.parametrize("name, ndim, key, shape, outer", [
    (R.FILTERS[3], 3, "5.0", (7, 19, 37), None),               # radius 20 folds more than once on two axes
    (R.FILTERS[4], 3, "5.0", (7, 19, 37), 2.5),
    (R.FILTERS[4], 3, "1.6", (9, 45, 50), 10.0),               # outer radius 40, the cap
    (R.FILTERS[3], 3, "7.5", (7, 19, 37), None),               # k_flt_line and the strided y pass
    (R.FILTERS[4], 2, "7.5", (33, 70), 3.75),
    (R.FILTERS[0], 2, "1.6", (5, 300), None),                  # more than one tile, a ragged last one
])
def test_filter_large_radii_and_paths(name, ndim, key, shape, outer):
    judged(name, noise(shape), SIGMAS[key], outer)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("field", ["constant", "ramp", "sphere", "x2"])
def test_degenerate_eigenvalues(field, ndim):
    g = np.meshgrid(*[np.arange(s, dtype=np.float32) - s // 2 for s in SHAPES[ndim]], indexing="ij")
    x = {"constant": np.full(SHAPES[ndim], 0.75, np.float32), "ramp": g[-1] + 2 * g[0], "sphere": sum(a * a for a in g),
         "x2": g[-1] ** 2}[field]
    for name, outer in ((R.FILTERS[3], None), (R.FILTERS[4], 0.8)):
        got = judged(name, np.stack([x, -x]).astype(np.float32), 1.6, outer)
        assert np.isfinite(got).all() and (np.diff(got, axis=1) <= 0).all(), "finite and descending at every voxel"


@pytest.mark.parametrize("ndim", [2, 3])
def test_bank_is_the_single_filters_bit_for_bit(ndim):
    from torch_em_amd import ops
    from torch_em_amd.shallow2deep import _get_filters
    x = dev(as4(noise(SHAPES[ndim]), ndim))
    config = _get_filters(ndim, None)
    bank = ops.feature_bank(x, config)
    singles = torch.cat([getattr(ops, f.func.tem_filter if isinstance(f, partial) else f.tem_filter)(x, s, **getattr(f, "keywords", {}))
                         for f, s in config], dim=1)
    assert bank.shape[1] == {2: 28, 3: 36}[ndim] and torch.equal(bank.view(torch.int32), singles.view(torch.int32))


@pytest.mark.parametrize("output_channel", [None, 1, (0, 1)])
@pytest.mark.parametrize("voxels", [1003, 1])
@pytest.mark.parametrize("trees", [1, 17])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("F", [1, 36, 64])
def test_forest_bit_for_bit(F, C, trees, voxels, output_channel):
    from torch_em_amd import ops
    rf = R.random_forest(100 * F + 10 * C + trees, trees, F, C)
    X = R.plant(rf, np.random.RandomState(voxels).randn(voxels, F).astype(np.float32))
    want = R.walk(rf, X).astype(np.float32).T                                        # [C, voxels]
    got = ops.forest_predict(dev(X.T.copy()[None]), ops.pack_forest(rf), output_channel)[0].cpu().numpy()
    assert judge.mismatches(got, pick(want, output_channel)) == 0
    assert len(rf.estimators_[0].tree_.feature) == 1, "a root-only tree"


@pytest.mark.parametrize("ndim", [2, 3])
def test_rf_with_filters_and_the_model_compose(ndim, tmp_path):
    from torch_em_amd import ops
    from torch_em_amd.model import UNet2d
    from torch_em_amd.shallow2deep import RFWithFilters, Shallow2DeepModel
    shape = {2: (33, 70), 3: (8, 16, 24)}[ndim]
    config = [("gaussianSmoothing", 0.7), ("hessian_of_gaussian_eigenvalues", 1.6), ("structureTensorEigenvalues", 1.6)]
    F = 1 + 2 * ndim
    rf = R.random_forest(7, 17, F, 3)
    rf_path = str(tmp_path / "rf.pkl")
    with open(rf_path, "wb") as f:
        pickle.dump(rf, f)
    x = dev(np.random.RandomState(2).randn(*shape).astype(np.float32))
    bank = ops.feature_bank(x.reshape((1,) * (4 - ndim) + shape), [(R.FILTERS[0], 0.7), (R.FILTERS[3], 1.6), (R.FILTERS[4], 1.6)])
    want = R.walk(rf, bank[0].reshape(F, -1).T.cpu().numpy()).astype(np.float32).T.reshape((3,) + shape)
    for channel in (None, 1, (0, 2)):
        got = RFWithFilters(rf_path, ndim, config, channel)(x)
        assert got.is_cuda and judge.mismatches(got.cpu().numpy(), pick(want, channel)) == 0
    assert isinstance(RFWithFilters(rf_path, ndim, config, 1)(x.cpu().numpy()), np.ndarray)
    if ndim == 3:
        return
    torch.manual_seed(0)
    net = UNet2d(1, 1, depth=2, initial_features=4).to(DEV).eval()
    torch.save(net, str(tmp_path / "enhancer.pt"))
    model = Shallow2DeepModel(str(tmp_path / "enhancer.pt"), (rf_path, ndim, config), DEV, rf_channel=1)
    xc = x[:32, :68].contiguous()                                  # a depth-2 U-Net halves twice
    with torch.no_grad():
        want_net = net(RFWithFilters(rf_path, ndim, config, 1)(xc)[None, None])
        got_net = pickle.loads(pickle.dumps(model))(xc[None, None])
    assert torch.equal(got_net, want_net) and tuple(got_net.shape) == (1, 1, 32, 68)
    with pytest.raises(NotImplementedError):
        Shallow2DeepModel(str(tmp_path / "enhancer.pt"), ("project.ilp", ndim), DEV)
