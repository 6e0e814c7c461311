"""GPU: the contingency table and the instance-segmentation scores (csrc/overlap.hip, ops.label_overlaps / overlap_scores,
torch_em_amd.metric) against the numpy oracle tests/metric_ref.py.  Integer fields are compared with array_equal, the
scores that are one fixed expression of exact integers bit for bit; the two bounds (variation of information, symmetric
best Dice) and the clDice bound are derived where they are used, from the case and the number format, not measured."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter, label

import metric_ref as M
import watershed_ref as R
from oracle.gpu_kit import DEV
from torch_em_amd import metric, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -53   # one rounding of a float64
MARGIN = 4       # the project's margin on a derived bound (oracle/judge.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def misaligned(a):
    """the array in a device buffer whose base is one element past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == a.itemsize % 16 and view.is_contiguous()
    return view


def blobs(rs, shape, shift=0.0):
    """(seg, target): the labelled components of two thresholds of two correlated smoothed noise fields"""
    base = gaussian_filter(rs.rand(*shape), 1.2)
    other = base + 0.35 * gaussian_filter(rs.rand(*shape) - 0.5, 1.0)
    return label(other > np.median(other) + shift)[0].astype(np.int64), label(base > np.median(base))[0].astype(np.int64)


def build_cases():
    """name -> (seg [N, D, H, W], target [N, D, H, W], thresholds)"""
    C = {}
    rs = np.random.RandomState(11)
    one = (0.5,)
    C["single_voxel_match"] = (np.int64([[[[3]]]]), np.int64([[[[9]]]]), one)
    C["single_voxel_background"] = (np.int64([[[[3]]]]), np.int64([[[[0]]]]), one)
    for name, shape in (("line_w", (1, 1, 37)), ("line_h", (1, 37, 1)), ("line_d", (37, 1, 1))):
        C[name] = (rs.randint(0, 4, (1,) + shape), np.repeat(rs.randint(0, 3, 8), 5)[:37].reshape((1,) + shape), one)
    for shape in ((3, 5, 257), (2, 17, 130), (8, 16, 16)):
        s, t = blobs(rs, shape)
        C["blobs_%dx%dx%d" % shape] = (s[None], t[None], (0.5, 0.75))
    C["every_voxel_its_own_pair"] = (np.arange(4097).reshape(1, 1, 1, 4097), rs.permutation(4097).reshape(1, 1, 1, 4097), one)
    q = (1, 2, 9, 31)
    C["all_background"] = (np.zeros(q, np.int64), np.zeros(q, np.int64), one)
    C["all_seven"] = (np.full(q, 7), np.full(q, 7), one)
    C["background_against_seven"] = (np.zeros(q, np.int64), np.full(q, 7), one)
    C["runs_across_blocks"] = (np.repeat([1, 2, 3], [256, 444, 300]).reshape(1, 1, 1, 1000),
                               np.repeat([4, 0, 9], [300, 212, 488]).reshape(1, 1, 1, 1000), one)
    b0s, b0t = np.arange(558).reshape(2, 9, 31), rs.permutation(558).reshape(2, 9, 31)
    b2s, b2t = blobs(rs, (2, 9, 31))
    C["batch"] = (np.stack([b0s, np.zeros_like(b0s), b2s]), np.stack([b0t, np.zeros_like(b0t), b2t]), one)
    C["tie"] = (np.int64([1, 1, 1, 1, 0, 0]).reshape(1, 1, 1, 6), np.int64([1, 1, 2, 2, 0, 0]).reshape(1, 1, 1, 6), (0.5, 0.75))
    C["tie_swapped"] = (C["tie"][1], C["tie"][0], (0.5, 0.75))
    C["one_object"] = (np.full((1, 1, 280, 250), 5), np.full((1, 1, 280, 250), 2), one)   # sum n^2 = 4.9e9 > 2^32
    s, t = blobs(rs, (4, 12, 33))
    big = np.array([0, 2 ** 31 - 1, 2 ** 40, 2 ** 31 - 1, 2 ** 40, 5, 2 ** 40], np.int64)[np.minimum(t, 6)]
    for dt in (np.int32, np.uint8, np.int16):
        C["large_target_ids_" + np.dtype(dt).name] = (np.minimum(s, 100).astype(dt)[None], big[None], one)
    return C


CASES = build_cases()
MISALIGNED = "blobs_3x5x257"


@functools.lru_cache(maxsize=None)
def reference(name, n, threshold):
    """the oracle's figures of one sample of a case, computed once"""
    seg, target, _ = CASES[name]
    t = M.table(seg[n], target[n])
    sq, ent = M.sums(t)
    best = M.best_dice(t)
    return {"table": t, "sq": sq, "ent": ent, "matching": M.matching(t, threshold), "best": best,
            "sbd": M.symmetric_best_dice(t), "rand": M.adapted_rand_error(t), "voi": M.variation_of_information(t)}


def voi_bound(t):
    """each of the three sums of n log2 n, divided by n, is at most log2 n; one rounding per term (the product; log2 is
    taken as correctly rounded within the margin) and one per addition, in any order: (P + 8) roundings cover the P terms,
    the additions of either side's summation and the final expression; times the margin"""
    P = len(t.n_ab) + int((t.n_a > 0).sum()) + int((t.n_b > 0).sum())
    return MARGIN * (P + 8) * U * math.log2(max(t.n, 2))


def sbd_bound(t):
    """the maxima are exact on both sides; a mean of K values in [0, 1] is K - 1 additions and one division, each one
    rounding of a value of at most K resp. 1: relative to the mean at most (K + 2) roundings; times the margin"""
    ia, ib = M.objects(t)
    return MARGIN * (max(len(ia), len(ib)) + 2) * U


def host(x):
    return x.cpu().numpy()


def check(name, put):
    seg, target, thresholds = CASES[name]
    N = seg.shape[0]
    V = seg[0].size
    dseg, dtarget = put(seg), put(target)
    ov = ops.label_overlaps(dseg, dtarget)
    assert all(x.dtype == torch.int32 for x in ov[:6]) and tuple(ov.pa.shape) == (N, V) and tuple(ov.n_a.shape) == (N, V + 1)
    npairs = host(ov.npairs)
    rand = host(metric.AdaptedRandError()(dseg, dtarget))
    voi = host(metric.VariationOfInformation()(dseg, dtarget))
    sbd = host(metric.SymmetricBestDice()(dseg, dtarget))
    assert rand.dtype == voi.dtype == sbd.dtype == np.float64 and rand.shape == voi.shape == sbd.shape == (N,)
    for thr in thresholds:
        s = ops.overlap_scores(ov, thr)
        err = {k: host(metric.IOUError(thr, k)(dseg, dtarget)) for k in M.STATS}
        for n in range(N):
            ref = reference(name, n, thr)
            t = ref["table"]
            # exact fields
            k = len(t.n_ab)
            assert npairs[n] == k, (name, n, int(npairs[n]), k)
            for field, want in (("pa", t.pa), ("pb", t.pb), ("n_ab", t.n_ab)):
                assert np.array_equal(host(getattr(ov, field)[n, :k]), want), (name, n, field)
            assert np.array_equal(host(ov.n_a[n]), t.n_a) and np.array_equal(host(ov.n_b[n]), t.n_b), (name, n)
            m = ref["matching"]
            got = (int(s.n_pred[n]), int(s.n_true[n]), int(s.tp[n]))
            assert got == (m["n_pred"], m["n_true"], m["tp"]), (name, n, thr, got, m)
            assert (int(s.sum_ab[n]), int(s.sum_a[n]), int(s.sum_b[n])) == ref["sq"], (name, n)
            # one fixed expression of exact integers: bit for bit
            assert rand[n] == ref["rand"], (name, n, rand[n], ref["rand"])
            for stat in M.STATS:
                assert err[stat][n] == 1.0 - m[stat], (name, n, thr, stat, err[stat][n], 1.0 - m[stat])
            # variation of information: the derived absolute bound
            print(f"METRIC {name}[{n}] voi {voi[n]:.17g} ref {ref['voi']:.17g} diff {abs(voi[n] - ref['voi']):.3e} bound {voi_bound(t):.3e}")
            assert abs(voi[n] - ref["voi"]) <= voi_bound(t), (name, n)
            # best Dice: the maxima bit for bit, the score within the bound of a mean
            assert np.array_equal(host(s.best_pred[n]), ref["best"][0]) and np.array_equal(host(s.best_true[n]), ref["best"][1]), (name, n)
            want_sbd, (da, db) = ref["sbd"]
            print(f"METRIC {name}[{n}] sbd {sbd[n]:.17g} ref {want_sbd:.17g} diff {abs(sbd[n] - want_sbd):.3e} bound {sbd_bound(t):.3e}")
            assert abs(float(s.dice_pred[n]) - da) <= sbd_bound(t) and abs(float(s.dice_true[n]) - db) <= sbd_bound(t), (name, n)
            assert abs(sbd[n] - want_sbd) <= sbd_bound(t), (name, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_and_scores(name):
    check(name, dev)


def test_misaligned_base():
    check(MISALIGNED, misaligned)


def test_one_object_needs_64_bits():
    assert reference("one_object", 0, 0.5)["sq"][0] == 70000 ** 2 > 2 ** 32


def test_single_sample_forms():
    """a 2-D or 3-D tensor is one sample and gives a 0-dim score"""
    seg, target, _ = CASES["blobs_8x16x16"]
    want = reference("blobs_8x16x16", 0, 0.5)["rand"]
    got = metric.AdaptedRandError()(dev(seg[0]), dev(target[0]))
    assert got.dim() == 0 and got.dtype == torch.float64 and float(got) == want
    flat = metric.AdaptedRandError()(dev(seg[0].reshape(8, 256)), dev(target[0].reshape(8, 256)))
    assert flat.dim() == 0 and float(flat) == want


@pytest.mark.parametrize("name", ["batch", "blobs_3x5x257", "every_voxel_its_own_pair"])
def test_determinism(name):
    """twice on the same buffers: the same bits in every field (rows of the table past npairs are not part of it)"""
    seg, target, _ = CASES[name]
    dseg, dtarget = dev(seg), dev(target)
    runs = []
    for _ in range(2):
        ov = ops.label_overlaps(dseg, dtarget)
        s = ops.overlap_scores(ov, 0.5)
        k = host(ov.npairs)
        table = [host(x[n, :k[n]]) for x in (ov.pa, ov.pb, ov.n_ab) for n in range(len(k))]
        fields = [host(x) for x in (ov.npairs, ov.n_a, ov.n_b) + tuple(s[:13])]
        runs.append([x.view(np.int64) if x.dtype == np.float64 else x for x in table + fields])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------- prefab metrics
def unit(x):
    return ((x - x.min()) / (x.max() - x.min())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def prediction_batch():
    """2 samples of 8 x 16 x 16: foreground, boundaries, center distances, boundary distances; the target's ids"""
    rs = np.random.RandomState(23)
    shape = (8, 16, 16)
    maps = np.stack([[unit(gaussian_filter(rs.rand(*shape), s)) for s in (2.0, 1.0, 1.5, 1.5)] for _ in range(2)])
    ids = np.stack([label(m[0] - m[1] > 0.2)[0] for m in maps]).astype(np.int64)
    assert all(i.max() >= 2 for i in ids), "the target has several objects"
    return maps, ids


COMPONENTS = {"min_size": 4, "threshold1": 0.15, "threshold2": 0.4}
DISTANCES = {"center_distance_threshold": 0.4, "boundary_distance_threshold": 0.4, "foreground_threshold": 0.4,
             "distance_smoothing": 0, "min_size": 3}


@functools.lru_cache(maxsize=None)
def host_segmentation(segmenter):
    maps, _ = prediction_batch()
    if segmenter == "components":
        return [R.np_watershed_from_components(m[1], m[0], **COMPONENTS) for m in maps]
    kw = {k: v for k, v in DISTANCES.items() if k != "distance_smoothing"}
    return [R.np_watershed_from_smoothed_distances(m[2], m[3], m[0], **kw)[0] for m in maps]


PREFAB = {
    "iou": (lambda seg, **kw: metric.WatershedIOUMetric(seg, iou_threshold=0.5, **kw), lambda r: 1.0 - r["matching"]["precision"], None),
    "sbd": (metric.WatershedSBDMetric, lambda r: r["sbd"][0], sbd_bound),
    "voi": (metric.WatershedVOIMetric, lambda r: r["voi"], voi_bound),
    "rand": (metric.WatershedRandMetric, lambda r: r["rand"], None),
}


@pytest.mark.parametrize("segmenter", ["components", "distances"])
@pytest.mark.parametrize("kind", sorted(PREFAB))
def test_prefab_forward_without_host_synchronisation(kind, segmenter):
    make, pick, bound = PREFAB[kind]
    maps, ids = prediction_batch()
    chans = [0, 1] if segmenter == "components" else [0, 2, 3]
    input_ = dev(maps[:, chans])
    target = dev(np.stack([maps[:, 0], ids.astype(np.float32)], axis=1))    # the ids in the LAST channel, as float
    m = make(segmenter, **(COMPONENTS if segmenter == "components" else DISTANCES))
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = m(input_, target)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.cuda.get_sync_debug_mode() == before
    assert got.dim() == 0 and got.dtype == torch.float64 and got.is_cuda
    segs = host_segmentation(segmenter)
    assert all(s.max() >= 2 for s in segs), "the case has several segments"
    per_sample, tol = [], 0.0
    for seg, tid in zip(segs, ids):
        t = M.table(seg, tid)
        r = {"matching": M.matching(t, 0.5), "sbd": M.symmetric_best_dice(t), "voi": M.variation_of_information(t),
             "rand": M.adapted_rand_error(t)}
        per_sample.append(pick(r))
        tol = max(tol, bound(t) if bound else 0.0)
    want = (per_sample[0] + per_sample[1]) / 2.0    # the mean of two: one addition, one exact halving, on both sides
    print(f"METRIC prefab {kind} {segmenter}: {float(got):.17g} ref {want:.17g} bound {tol:.3e}")
    assert abs(float(got) - want) <= tol + (U * abs(want) if bound else 0.0)


def test_distance_segmenter_with_smoothing_does_not_synchronise():
    """the default smoothing adds the blur launches: the forward still completes with synchronisation forbidden"""
    maps, ids = prediction_batch()
    m = metric.WatershedSBDMetric("distances")
    got = m(dev(maps[:, [0, 2, 3]]), dev(ids[:, None]))
    assert got.dim() == 0 and 0.0 <= float(got) <= 1.0


def test_base_class_takes_any_segmenter():
    _, ids = prediction_batch()
    m = metric.BaseInstanceSegmentationMetric(lambda x: x[:, 0].to(torch.int32), metric.AdaptedRandError(), to_numpy=True)
    got = m(dev(ids[:, None].astype(np.float32)), dev(ids[:, None]))
    assert float(got) == 0.0


# ---------------------------------------------------------------------------------------------------- clDice
def test_cldice_metric():
    from torch_em_amd.loss import SoftSkeletonize
    rs = np.random.RandomState(31)
    shape = (1, 1, 8, 16, 16)
    x = (gaussian_filter(rs.rand(*shape[2:]), 1.5) > 0.5).astype(np.float32).reshape(shape)
    t = (gaussian_filter(rs.rand(*shape[2:]), 1.5) > 0.5).astype(np.float32).reshape(shape)
    got = metric.clDice(dev(x), dev(t), skeletonize_method="soft", num_iter=5)
    assert got.dim() == 0 and got.dtype == torch.float64
    skel = SoftSkeletonize(num_iter=5)
    sx, st = (host(skel(dev(a))).astype(np.float64) for a in (x, t))
    assert sx.sum() > 0 and st.sum() > 0
    t_prec = np.sum(t.astype(np.float64) * sx) / np.sum(sx)
    t_sens = np.sum(x.astype(np.float64) * st) / np.sum(st)
    want = 2.0 * (t_prec * t_sens) / max(t_prec + t_sens, 1e-7)
    # the products of two float32 are exact in float64; a sum of V non-negative terms carries at most V - 1 roundings
    # relative to itself in any order, a ratio of two such sums 2 (V - 1) + 1; the product of the two ratios twice that
    # plus one, their sum once plus one, the last division one more: 3 (2 V - 1) + 3 roundings relative to a score <= 1, on
    # either side of the comparison
    V = x.size
    bound = 2 * (3 * (2 * V - 1) + 3) * U * want
    print(f"METRIC cldice {float(got):.17g} ref {want:.17g} diff {abs(float(got) - want):.3e} bound {bound:.3e}")
    assert 0.0 < want <= 1.0 and abs(float(got) - want) <= bound
    same = metric.clDice(x[0, 0], t[0, 0])     # one numpy image, as the reference takes it
    assert float(same) == float(got)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    lab = torch.zeros((1, 2, 4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="integer type"):
        ops.label_overlaps(lab.float(), lab)
    with pytest.raises(ValueError, match="integer type"):
        metric.AdaptedRandError()(lab, lab.float())
    with pytest.raises(ValueError, match="one shape"):
        ops.label_overlaps(lab, lab[:, :1])
    ov = ops.label_overlaps(lab, lab)
    with pytest.raises(ValueError, match="assignment solver"):
        ops.overlap_scores(ov, 0.4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_overlaps(lab.cpu(), lab.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metric.WatershedSBDMetric()(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(NotImplementedError):
        metric.clDice(lab, lab, skeletonize_method="skimage")
