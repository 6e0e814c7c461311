"""The oracle of the Shallow2Deep front end (tests/test_gpu_s2d.py, tests/test_s2d_cpu.py); numpy and scipy only, no code
shared with the library.  Filters return [F, *shape] (eigenvalues descending); `how`: "f64" scipy in float64, "f32" the
same separable chain restated in float32, "scale" the chain on |x| with |weights| (the per-element scale of the judge)."""
import itertools
from types import SimpleNamespace

import numpy as np
from scipy.ndimage import gaussian_filter

FILTERS = ("gaussian_smoothing", "laplacian_of_gaussian", "gaussian_gradient_magnitude", "hessian_of_gaussian_eigenvalues",
           "structure_tensor_eigenvalues")


def taps(sigma, order):
    """scipy's `_gaussian_kernel1d`, float64"""
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi /= phi.sum()
    return phi * (1.0, -x / sigma ** 2, x ** 2 / sigma ** 4 - 1.0 / sigma ** 2)[order]


def _pass(a, w, axis, dt):
    """correlation with the reversed kernel on the mirror extension, accumulated tap by tap in dt"""
    n, r = a.shape[axis], len(w) // 2
    i = np.arange(-r, n + r) % max(2 * (n - 1), 1)
    a = np.take(a, np.where(i < n, i, 2 * (n - 1) - i), axis=axis)
    out = np.zeros_like(a, shape=[n if k == axis else s for k, s in enumerate(a.shape)])
    for t, wt in enumerate(w[::-1].astype(dt)):
        out += wt * np.take(a, np.arange(t, t + n), axis=axis)
    return out


def jet(x, sigma, order, how):
    if how == "f64":
        return gaussian_filter(x.astype(np.float64), sigma, order=order, mode="mirror", truncate=4.0)
    a = np.abs(x).astype(np.float64) if how == "scale" else x.astype(np.float32)
    for axis in reversed(range(x.ndim)):                    # x first, as the kernels do
        w = taps(sigma[axis], order[axis])
        a = _pass(a, np.abs(w) if how == "scale" else w, axis, a.dtype)
    return a


def _unit(ndim, *axes):
    return tuple(sum(1 for b in axes if b == a) for a in range(ndim))


def _eig(m, how):
    """m[a][b] fields -> [ndim, *shape]: eigenvalues descending, or for the scale the Frobenius norm on every channel"""
    M = np.stack([np.stack(row, -1) for row in m], -2)
    if how == "scale":
        return np.repeat(np.sqrt((M ** 2).sum((-1, -2)))[None], len(m), 0)
    return np.moveaxis(np.linalg.eigvalsh(M)[..., ::-1], -1, 0)


def apply(name, x, sigma, outer_sigma=None, how="f64"):
    nd = x.ndim
    sig = (float(sigma),) * nd if np.isscalar(sigma) else tuple(sigma)
    J = lambda *axes: jet(x, sig, _unit(nd, *axes), how)   # noqa: E731
    if name == "gaussian_smoothing":
        return J()[None]
    if name == "laplacian_of_gaussian":
        return sum(J(a, a) for a in range(nd))[None]
    if name == "gaussian_gradient_magnitude":
        return np.sqrt(sum(J(a) ** 2 for a in range(nd)))[None]
    if name == "hessian_of_gaussian_eigenvalues":
        return _eig([[J(a, b) for b in range(nd)] for a in range(nd)], how)
    out = (float(outer_sigma),) * nd if np.isscalar(outer_sigma) else tuple(outer_sigma)
    g = [J(a) for a in range(nd)]
    return _eig([[jet(g[a] * g[b], out, (0,) * nd, how) for b in range(nd)] for a in range(nd)], how)


# ------------------------------------------------------------------------------------------------------- forests
def random_forest(seed, n_trees, F, C, depth=6):
    """an object with sklearn's `estimators_[i].tree_` arrays: random topology, tree 0 root-only, float64 thresholds"""
    rs = np.random.RandomState(seed)
    est = []
    for t in range(n_trees):
        left, right, feat, thr = [], [], [], []

        def grow(d):
            me = len(left)
            for arr, v in ((left, -1), (right, -1), (feat, -2), (thr, -2.0)):
                arr.append(v)
            if t > 0 and d < depth and (d == 0 or rs.rand() < 0.7):
                feat[me], thr[me] = rs.randint(F), float(rs.randn())
                left[me] = grow(d + 1)
                right[me] = grow(d + 1)
            return me
        grow(0)
        value = rs.randint(0, 5, (len(left), 1, C)).astype(np.float64)
        value[:, 0, 0] += 1.0 / 3.0                                       # fractions that are not dyadic
        est.append(SimpleNamespace(tree_=SimpleNamespace(children_left=np.array(left), children_right=np.array(right),
                                                         feature=np.array(feat), threshold=np.array(thr), value=value)))
    return SimpleNamespace(estimators_=est, n_features_in_=F)


def plant(rf, X):
    """X float32 [n, F] with rows set exactly on the float32 neighbours of the thresholds: below, nearest, above"""
    X = X.copy()
    nodes = [(f, t) for e in rf.estimators_ for f, t in zip(e.tree_.feature, e.tree_.threshold) if f >= 0]
    for j, ((f, t), d) in enumerate(itertools.product(nodes, (-1, 0, 1))):
        t32 = np.float32(t)
        X[j % len(X), f] = t32 if d == 0 else np.nextafter(t32, np.float32(d * np.inf))
    return X


def walk(rf, X):
    """predict_proba in float64: float32 feature <= float64 threshold, leaf fractions summed in tree order, / trees"""
    total = 0.0
    for e in rf.estimators_:
        t = e.tree_
        node = np.zeros(len(X), np.int64)
        while (t.children_left[node] >= 0).any():
            inner = t.children_left[node] >= 0
            go_left = X[np.arange(len(X)), np.where(inner, t.feature[node], 0)] <= t.threshold[node]
            node = np.where(inner, np.where(go_left, t.children_left[node], t.children_right[node]), node)
        v = np.asarray(t.value, np.float64)[node, 0]
        s = v.sum(1, keepdims=True)
        total = total + v / np.where(np.abs(s - 1.0) <= 1e-9, 1.0, s)    # stored fractions (sklearn >= 1.4) are taken as stored
    return total / len(rf.estimators_)
