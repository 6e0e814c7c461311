"""Timing of the Shallow2Deep front end on the device (the record: profiles/s2d_bench.txt).

The default bank (five filters at four scales) fused (ops.feature_bank) against the same bank composed from ops.blur2d /
ops.blur3d of the order-0, 1 and 2 weights plus torch pointwise arithmetic -- the best the code before csrc/filters.hip can
do -- run alternately after a warm-up, at 64^3, 128^3 and 2-D 1024^2; order-0 smoothing alone against ops.blur3d;
forest_predict (100 trees of depth 12, F = 36) in voxels/s and against the byte floor of reading its features once; and,
as context, scipy + sklearn on the host for one 64^3 volume.  Every number is a median of device-synchronised wall times;
the spread is that of a repeated identical run.
"""
import argparse
import statistics
import sys
import time
from functools import partial
from os.path import abspath, dirname, join

import numpy as np
import torch

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, join(dirname(dirname(abspath(__file__))), "tests"))

from torch_em_amd import ops                                       # noqa: E402
from torch_em_amd.shallow2deep import _get_filters                 # noqa: E402
from torch_em_amd.transform.defect import gaussian_jet_weights     # noqa: E402

SIGMAS = (0.7, 1.6, 3.5, 5.0)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def eig_sym(m):
    return torch.linalg.eigvalsh(m).flip(-1).movedim(-1, 1)


def composed_bank(x):
    """the default bank from order-wise blurs: every jet is one blur2d / blur3d call"""
    nd = 3 if x.shape[1] > 1 else 2
    feats = {k: [] for k in range(5)}

    def blur(v, sigma, order):
        w = [gaussian_jet_weights(sigma)[o][::-1].astype(np.float32).tolist() for o in order]
        return ops.blur3d(v, *w) if nd == 3 else ops.blur2d(v, *w)

    def unit(*axes):
        return tuple(sum(1 for b in axes if b == a) for a in range(nd))
    for s in SIGMAS:
        g = [blur(x, s, unit(a)) for a in range(nd)]
        h = [[blur(x, s, unit(a, b)) if b >= a else None for b in range(nd)] for a in range(nd)]
        feats[0].append(blur(x, s, unit())[:, None])
        feats[1].append(sum(h[a][a] for a in range(nd))[:, None])
        feats[2].append(torch.sqrt(sum(v * v for v in g))[:, None])
        feats[3].append(eig_sym(torch.stack([torch.stack([h[min(a, b)][max(a, b)] for b in range(nd)], -1) for a in range(nd)], -2)))
        t = [[blur(g[a] * g[b], 0.5 * s, unit()) if b >= a else None for b in range(nd)] for a in range(nd)]
        feats[4].append(eig_sym(torch.stack([torch.stack([t[min(a, b)][max(a, b)] for b in range(nd)], -1) for a in range(nd)], -2)))
    return torch.cat([f for k in range(5) for f in feats[k]], dim=1)


def deep_forest(trees, depth, F, C, seed=0):
    """complete trees of the given depth as sklearn-shaped tables"""
    from types import SimpleNamespace
    rs = np.random.RandomState(seed)
    n = 2 ** (depth + 1) - 1
    idx = np.arange(n)
    inner = idx < 2 ** depth - 1
    est = []
    for _ in range(trees):
        est.append(SimpleNamespace(tree_=SimpleNamespace(
            children_left=np.where(inner, 2 * idx + 1, -1), children_right=np.where(inner, 2 * idx + 2, -1),
            feature=np.where(inner, rs.randint(0, F, n), -2), threshold=rs.randn(n), value=rs.rand(n, 1, C) + 0.1)))
    return SimpleNamespace(estimators_=est, n_features_in_=F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host", action="store_true", help="also time scipy + sklearn on the host for one 64^3 volume")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_s2d.py measures on the device"
    med = statistics.median
    for shape in ((1, 64, 64, 64), (1, 128, 128, 128), (1, 1, 1024, 1024)):
        x = torch.randn(shape, device="cuda")
        config = _get_filters(3 if shape[1] > 1 else 2, None)
        fused, comp = partial(ops.feature_bank, x, config), partial(composed_bank, x)
        a, b = fused(), comp()
        print(f"shape {shape}: F = {a.shape[1]}, max |fused - composed| = {float((a - b).abs().max()):.3e}")
        del a, b
        fused(), comp()
        tf, tc, tf2 = [], [], []
        for _ in range(args.reps):                       # alternately; the fused bank twice for the run-to-run spread
            tf += timed(fused, 1)
            tc += timed(comp, 1)
            tf2 += timed(fused, 1)
        spread = abs(med(tf) - med(tf2))
        print(f"  fused {med(tf) * 1e3:.3f} ms (repeat {med(tf2) * 1e3:.3f} ms, spread {spread * 1e3:.3f} ms), composed {med(tc) * 1e3:.3f} ms, "
              f"ratio {med(tc) / med(tf):.2f}, faster by more than the spread: {med(tc) - med(tf) > spread}")
        if shape[1] > 1:
            w = gaussian_jet_weights(1.6)[0].astype(np.float32).tolist()
            one, blur = partial(ops.gaussian_smoothing, x, 1.6), partial(ops.blur3d, x, w, w, w)
            one(), blur()
            print(f"  smoothing alone (sigma 1.6): fused {med(timed(one, args.reps)) * 1e3:.3f} ms, blur3d {med(timed(blur, args.reps)) * 1e3:.3f} ms")
    F, V = 36, 128 ** 3
    forest = ops.pack_forest(deep_forest(100, 12, F, 2))
    bank = torch.randn(1, F, V, device="cuda")
    run = partial(ops.forest_predict, bank, forest, 1)
    run()
    t = med(timed(run, args.reps))
    print(f"forest_predict 100 trees depth 12 F {F}: {t * 1e3:.3f} ms, {V / t / 1e9:.3f} Gvoxel/s; reading the features once is "
          f"{F * V * 4 / 1e9:.3f} GB: {F * V * 4 / t / 1e12:.3f} TB/s achieved against the byte floor")
    if args.host:
        from scipy.ndimage import gaussian_filter
        import s2d_ref as R
        xs = np.random.RandomState(0).randn(64, 64, 64).astype(np.float32)
        t0 = time.perf_counter()
        feats = np.concatenate([R.apply(n, xs, s, 0.5 * s).reshape(-1, xs.size) for n in R.FILTERS for s in SIGMAS]).T.astype(np.float32)
        t1 = time.perf_counter()
        print(f"host: scipy bank of one 64^3 volume {t1 - t0:.2f} s ({gaussian_filter.__module__})")
        try:
            from sklearn.ensemble import RandomForestClassifier
            rf = RandomForestClassifier(n_estimators=100, max_depth=12, n_jobs=1, random_state=0).fit(feats[::64], np.arange(len(feats[::64])) % 2)
            t0 = time.perf_counter()
            rf.predict_proba(feats)
            print(f"host: sklearn predict_proba (100 trees, depth <= 12, n_jobs=1) {time.perf_counter() - t0:.2f} s")
        except ImportError:
            print("host: sklearn is not installed")


if __name__ == "__main__":
    main()
