"""CPU: the numpy oracle of the instance-segmentation scores (tests/metric_ref.py) against a brute-force table and hand
values, the counting formula for the matches against the assignment, the host-side argument checks of
ops.label_overlaps / overlap_scores, and the checkpoint round trip of the prefab metrics' constructor arguments."""
import math

import numpy as np
import pytest
import torch

import metric_ref as M
from torch_em_amd import metric, ops
from torch_em_amd.trainer.default_trainer import _class_path, _import_class, _init_kwargs

TIE = (np.array([1, 1, 1, 1, 0, 0]), np.array([1, 1, 2, 2, 0, 0]))


def random_labels(rs, n, k):
    """n voxels in runs (so objects overlap substantially), ids drawn from 0..k"""
    cuts = np.sort(rs.choice(np.arange(1, n), size=min(k, n - 1), replace=False))
    return np.repeat(rs.randint(0, k + 1, size=len(cuts) + 1), np.diff(np.concatenate([[0], cuts, [n]])))


def test_table_against_brute_force():
    rs = np.random.RandomState(3)
    for n in (1, 2, 7, 30):
        for _ in range(10):
            a, b = rs.randint(0, 4, n) * 5, rs.randint(0, 5, n) * 1000
            t, bt = M.table(a, b), M.brute_table(a, b)
            for got, want in zip(t[:5], bt[:5]):
                assert np.array_equal(got, want)
            assert t.n_ab.sum() == n and t.n_a.sum() == n and t.n_b.sum() == n
            order = list(zip(t.pa.tolist(), t.pb.tolist()))
            assert order == sorted(set(order))


def test_dense_ids():
    assert M.dense([7, 0, 2 ** 40, 7, 3]).tolist() == [2, 0, 3, 2, 1]


def test_identical_labellings_score_zero():
    rs = np.random.RandomState(4)
    for _ in range(5):
        a = random_labels(rs, 60, 5)
        if a.max() == 0:
            continue
        s = M.all_scores(a, a * 3)
        assert all(v == 0.0 for v in s.values()), s


def test_scores_do_not_depend_on_the_ids():
    rs = np.random.RandomState(5)
    a, b = random_labels(rs, 80, 6), random_labels(rs, 80, 4)
    want = M.all_scores(a, b)
    pa, pb = rs.permutation(7) + 1, rs.permutation(5) + 1
    ra, rb = np.where(a > 0, pa[a] * 11, 0), np.where(b > 0, pb[b] * 1000, 0)
    got = M.all_scores(ra, rb)
    # the pairs are visited in another order: the integer scores are equal, the float sums within a few roundings
    for k in ("rand",) + M.STATS:
        assert got[k] == want[k], k
    assert abs(got["voi"] - want["voi"]) <= 8 * 2.0 ** -53 * math.log2(80) and abs(got["sbd"] - want["sbd"]) <= 8 * 2.0 ** -53


def test_hand_values():
    a, b = TIE
    t = M.table(a, b)
    # pairs (0,0): 2, (1,1): 2, (1,2): 2; n_a = 2, 4; n_b = 2, 2, 2
    assert M.adapted_rand_error(t) == 1.0 - 24.0 / 32.0
    assert M.variation_of_information(t) == (2 * 1 + 4 * 2 + 3 * 2 * 1 - 2.0 * 3 * 2 * 1) / 6
    best_a, best_b = M.best_dice(t)
    assert best_a[1] == 4.0 / 6.0 and best_b[1] == best_b[2] == 4.0 / 6.0
    assert M.symmetric_best_dice(t)[0] == 1.0 - 4.0 / 6.0


@pytest.mark.parametrize("swap", [False, True])
def test_tie_case(swap):
    """seg object 1 reaches IoU 0.5 with BOTH target objects: a star of two, one match"""
    a, b = TIE[::-1] if swap else TIE
    t = M.table(a, b)
    m = M.matching(t, 0.5)
    assert m["tp"] == 1 and (m["n_pred"], m["n_true"]) == ((2, 1) if swap else (1, 2))
    assert M.tp_counting(t, 0.5) == 1
    assert M.matching(t, 0.75)["tp"] == 0 and M.tp_counting(t, 0.75) == 0


def test_counting_formula_against_the_assignment():
    rs = np.random.RandomState(6)
    nonzero = 0
    for n, k in ((24, 3), (90, 8)):
        for _ in range(150):
            a, b = random_labels(rs, n, k), random_labels(rs, n, k)
            if rs.rand() < 0.3:   # near-identical labellings: many matches
                b = np.where(rs.rand(n) < 0.1, 0, a)
            t = M.table(a, b)
            for thr in (0.5, 0.6, 0.75, 1.0):
                want = M.tp_assignment(t, thr)
                assert M.tp_counting(t, thr) == want, (a.tolist(), b.tolist(), thr)
                nonzero += want > 0
    assert nonzero > 200


def test_argument_checks_on_the_host():
    lab = torch.zeros((1, 1, 4, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="integer type"):
        ops.label_overlaps(lab.float(), lab)
    with pytest.raises(ValueError, match="integer type"):
        ops.label_overlaps(lab, lab.double())
    with pytest.raises(ValueError, match="one shape"):
        ops.label_overlaps(lab, torch.zeros((1, 1, 4, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="non-empty"):
        ops.label_overlaps(lab[:, :, :0], lab[:, :, :0])
    with pytest.raises(ValueError, match="N, D, H, W"):
        ops.label_overlaps(lab[0], lab[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_overlaps(lab, lab)
    for thr in (0.4, 1.5, float("nan")):
        with pytest.raises(ValueError, match="assignment solver"):
            ops.overlap_scores(None, thr)
        with pytest.raises(ValueError, match="assignment solver"):
            metric.IOUError(thr)
    with pytest.raises(ValueError, match="metric must be one of"):
        metric.IOUError(0.5, "accuracy")
    with pytest.raises(ValueError, match="segmenter must be one of"):
        metric.WatershedSBDMetric("mws")
    with pytest.raises(TypeError):
        metric.WatershedSBDMetric("distances", debug=True)


def test_cldice_argument_checks():
    x = np.zeros((4, 4), np.float32)
    with pytest.raises(NotImplementedError, match="thinning"):
        metric.clDice(x, x, skeletonize_method="skimage")
    with pytest.raises(ValueError, match="same shape"):
        metric.clDice(x, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="Unknown option"):
        metric.clDice(x, x, skeletonize_method="thin")


@pytest.mark.parametrize("make", [
    lambda: metric.WatershedIOUMetric("components", iou_threshold=0.75, min_size=3),
    lambda: metric.WatershedIOUMetric(),
    lambda: metric.WatershedSBDMetric("distances", distance_smoothing=1.0, min_size=4),
    lambda: metric.WatershedVOIMetric("components", threshold1=0.4),
    lambda: metric.WatershedRandMetric(),
])
def test_init_kwargs_round_trip(make):
    m = make()
    again = _import_class(_class_path(m))(**_init_kwargs(m))
    assert type(again) is type(m) and again.init_kwargs == m.init_kwargs
    assert type(again.segmenter) is type(m.segmenter) and again.segmenter.kwargs == m.segmenter.kwargs
    assert type(again.metric) is type(m.metric) and vars(again.metric) == vars(m.metric)
    assert _class_path(m).startswith("torch_em_amd.metric.instance_segmentation_metric.Watershed")
