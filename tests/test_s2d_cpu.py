"""CPU: the host side of the Shallow2Deep front end -- the filter weights, the forest packing and its decision rule, the
default filter list and the argument checks (the kernels: tests/test_gpu_s2d.py)."""
import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter1d

import s2d_ref as R


@pytest.mark.parametrize("sigma", [0.7, 1.6, 3.5, 10.0])
def test_host_weights_are_scipys_impulse_responses(sigma):
    from torch_em_amd.transform.defect import gaussian_jet_weights
    w = gaussian_jet_weights(sigma)
    r = int(4 * sigma + 0.5)
    impulse = np.zeros(4 * r + 1)
    impulse[2 * r] = 1.0
    assert w.shape == (3, 2 * r + 1) and w.dtype == np.float64
    for order in range(3):
        want = gaussian_filter1d(impulse, sigma, order=order, mode="mirror", truncate=4.0)[r:3 * r + 1]
        assert np.allclose(w[order], want, rtol=1e-12, atol=1e-15 * np.abs(want).max()), order
        assert np.allclose(R.taps(sigma, order), want, rtol=1e-12, atol=1e-15 * np.abs(want).max()), "the oracle's taps"


def test_packed_forest_walks_like_predict_proba():
    ensemble = pytest.importorskip("sklearn.ensemble")
    from torch_em_amd import ops
    rs = np.random.RandomState(0)
    X = rs.randn(600, 5).astype(np.float32)
    rf = ensemble.RandomForestClassifier(n_estimators=7, max_depth=6, n_jobs=1, random_state=0).fit(X, rs.randint(0, 3, 600))
    Xp = R.plant(rf, X)
    want = rf.predict_proba(Xp)
    assert np.array_equal(R.walk(rf, Xp), want), "the oracle's walker is predict_proba"
    f = ops.pack_forest(rf)
    assert (f.n_features, f.n_classes, f.n_trees) == (5, 3, 7) and f.leaves.dtype == np.float64 and f.nodes.dtype == np.int32
    thr = f.nodes[:, 1].copy().view(np.float32)
    got = np.zeros_like(want)
    for root in f.roots:                                    # the kernel's walk, on the packed tables
        node = np.full(len(Xp), root)
        while (f.nodes[node, 0] >= 0).any():
            inner = f.nodes[node, 0] >= 0
            left = Xp[np.arange(len(Xp)), np.where(inner, f.nodes[node, 0], 0)] <= thr[node]          # float32 <= float32
            node = np.where(inner, np.where(left, f.nodes[node, 2], f.nodes[node, 3]), node)
        got += f.leaves[f.nodes[node, 2]]
    assert np.array_equal(got / f.n_trees, want)


def test_float32_floor_keeps_every_decision():
    from torch_em_amd import ops
    t = np.random.RandomState(1).randn(2000)
    f = ops.float32_floor(t)
    assert f.dtype == np.float32 and (f.astype(np.float64) <= t).all() and (np.nextafter(f, np.float32(np.inf)).astype(np.float64) > t).all()
    exact = np.float64(np.float32(0.3))
    assert ops.float32_floor([exact])[0] == np.float32(0.3)


def test_default_filter_list_and_validation():
    from torch_em_amd.shallow2deep import _get_filters, filters
    got = _get_filters(3, None)
    names = [getattr(f, "func", f).tem_filter for f, _ in got]
    assert names == [n for n in R.FILTERS for _ in range(4)] and [s for _, s in got] == [0.7, 1.6, 3.5, 5.0] * 5
    assert [f.keywords["outer_sigma"] for f, _ in got[16:]] == [0.35, 0.8, 1.75, 2.5] and not hasattr(got[0][0], "keywords")
    assert filters.gaussianSmoothing is filters.gaussian_smoothing and filters.structureTensorEigenvalues.tem_filter == R.FILTERS[4]
    ok = [("gaussianSmoothing", 1.0), ("hessian_of_gaussian_eigenvalues", (1.0, 2.0))]
    assert _get_filters(2, ok) == ok
    for ndim, bad in ((2, [("noSuchFilter", 1.0)]), (2, [("gaussianSmoothing", 1)]), (3, [("gaussianSmoothing", (1.0, 2.0))]),
                      (2, [("gaussianSmoothing", (1.0, 2))]), (2, "gaussianSmoothing")):
        with pytest.raises((AssertionError, ValueError)):
            _get_filters(ndim, bad)


def test_value_errors():
    from torch_em_amd import ops
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="radius 41"):
        ops.gaussian_smoothing(x, 10.2)
    with pytest.raises(ValueError, match="radius 41"):
        ops.structure_tensor_eigenvalues(x, 1.0, outer_sigma=10.2)
    with pytest.raises(ValueError, match="features"):
        ops.pack_forest(R.random_forest(0, 2, 65, 2))
    with pytest.raises(ValueError, match="classes"):
        ops.pack_forest(R.random_forest(0, 2, 4, 9))
    with pytest.raises(ValueError, match="fitted on 4"):
        ops.forest_predict(torch.zeros(1, 5, 10), ops.pack_forest(R.random_forest(0, 2, 4, 2)))
    with pytest.raises(ValueError, match="output_channel"):
        ops.forest_predict(torch.zeros(1, 4, 10), ops.pack_forest(R.random_forest(0, 2, 4, 2)), output_channel=2)
