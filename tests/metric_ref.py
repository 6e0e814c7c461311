"""Numpy oracle of the instance-segmentation scores (torch_em_amd.metric, ops.label_overlaps / overlap_scores): test
infrastructure, numpy and scipy only.  The table comes from np.unique of the stacked id pairs; the scores restate the
definitions of DESIGN.md "Instance segmentation scores" in float64 and Python integers.  Two things are deliberately NOT
done the kernel's way: the matches are counted by scipy's linear_sum_assignment with elf's cost (the kernel counts
pairs and subtracts stars), and the best Dice is the literal double loop over the objects."""
import math
from collections import namedtuple

import numpy as np
from scipy.optimize import linear_sum_assignment

Table = namedtuple("Table", "pa pb n_ab n_a n_b n")   # dense ids; n_a, n_b indexed by id, length n + 1
STATS = ("precision", "recall", "segmentation_accuracy", "f1")


def dense(x):
    """0 stays 0, the other values become 1..k in ascending order"""
    x = np.asarray(x).astype(np.int64).ravel()
    vals = np.unique(x)
    vals = vals[vals != 0]
    out = np.searchsorted(vals, x) + 1
    out[x == 0] = 0
    return out


def table(seg, target):
    a, b = dense(seg), dense(target)
    assert a.shape == b.shape and a.size > 0
    n = a.size
    pairs, counts = np.unique(np.stack([a, b]), axis=1, return_counts=True)   # columns in ascending (a, b) order
    return Table(pairs[0].astype(np.int64), pairs[1].astype(np.int64), counts.astype(np.int64),
                 np.bincount(a, minlength=n + 1).astype(np.int64), np.bincount(b, minlength=n + 1).astype(np.int64), n)


def brute_table(seg, target):
    """the same table by counting every candidate pair: tiny arrays only"""
    a, b = dense(seg), dense(target)
    rows = [(i, j, int(np.sum((a == i) & (b == j)))) for i in range(a.max() + 1) for j in range(b.max() + 1)]
    rows = [r for r in rows if r[2] > 0]
    n = a.size
    n_a = [int(np.sum(a == i)) for i in range(n + 1)]
    n_b = [int(np.sum(b == i)) for i in range(n + 1)]
    return Table(*(np.array(c, np.int64) for c in zip(*rows)), np.array(n_a, np.int64), np.array(n_b, np.int64), n)


def sums(t):
    """(sum_ab, sum_a, sum_b) as Python integers, (s_ab, s_a, s_b) as float64"""
    counts = [x[x > 0].tolist() for x in (t.n_ab, t.n_a, t.n_b)]   # Python integers; the empty entries add nothing
    sq = tuple(sum(c * c for c in x) for x in counts)
    ent = tuple(math.fsum(c * math.log2(c) for c in x) for x in counts)
    return sq, ent


def adapted_rand_error(t):
    (sum_ab, sum_a, sum_b), _ = sums(t)
    return 1.0 - (2.0 * sum_ab) / (sum_a + sum_b)


def variation_of_information(t):
    _, (s_ab, s_a, s_b) = sums(t)
    return (s_a + s_b - 2.0 * s_ab) / t.n


def objects(t):
    """the non-zero ids present on each side"""
    return np.flatnonzero(t.n_a[1:] > 0) + 1, np.flatnonzero(t.n_b[1:] > 0) + 1


def _overlap_matrix(t):
    ia, ib = objects(t)
    m = np.zeros((len(ia), len(ib)), np.int64)
    ra, rb = {int(v): k for k, v in enumerate(ia)}, {int(v): k for k, v in enumerate(ib)}
    for a, b, c in zip(t.pa, t.pb, t.n_ab):
        if a > 0 and b > 0:
            m[ra[int(a)], rb[int(b)]] = c
    return m, ia, ib


def matched_matrix(t, threshold):
    """bool [objects of seg, objects of target]: n_ab >= threshold * (n_a + n_b - n_ab), in float64 as stated"""
    m, ia, ib = _overlap_matrix(t)
    union = t.n_a[ia][:, None] + t.n_b[ib][None, :] - m
    return m.astype(np.float64) >= threshold * union.astype(np.float64), m / np.maximum(union, 1)


def tp_assignment(t, threshold):
    """the true positives as elf.evaluation.matching counts them: an optimal assignment under the cost
    -(iou >= thr) - iou / (2 * n_matched), then the assigned pairs that reach the threshold"""
    ok, iou = matched_matrix(t, threshold)
    if ok.size == 0 or not ok.any():
        return 0
    n_matched = min(ok.shape)
    costs = -ok.astype(np.float64) - iou / (2.0 * n_matched)
    rows, cols = linear_sum_assignment(costs)
    return int(ok[rows, cols].sum())


def tp_counting(t, threshold):
    """the kernel's formula: matched pairs minus the objects of either side that have two of them"""
    ok, _ = matched_matrix(t, threshold)
    return int(ok.sum()) - int((ok.sum(axis=1) == 2).sum()) - int((ok.sum(axis=0) == 2).sum())


def matching(t, threshold=0.5, tp=None):
    ia, ib = objects(t)
    tp = tp_assignment(t, threshold) if tp is None else tp
    n_pred, n_true = len(ia), len(ib)
    fp, fn = n_pred - tp, n_true - tp
    if tp == 0:
        stats = dict.fromkeys(STATS, 0.0)
    else:
        stats = {"precision": tp / (tp + fp), "recall": tp / (tp + fn), "segmentation_accuracy": tp / (tp + fp + fn),
                 "f1": (2 * tp) / (2 * tp + fp + fn)}
    return dict(stats, tp=tp, n_pred=n_pred, n_true=n_true)


def best_dice(t):
    """per object of seg (and of target) the maximum over the objects of the other side of 2 n_ab / (n_a + n_b), by the
    literal double loop over ALL pairs of objects (the inner one a numpy row, so that 4096 x 4096 objects stay affordable)
    -> (best of seg's objects, best of target's), arrays of length n + 1 indexed by id"""
    m, ia, ib = _overlap_matrix(t)
    best_a, best_b = np.zeros(t.n + 1), np.zeros(t.n + 1)
    if len(ib):
        for i, a in enumerate(ia):
            d = 2.0 * m[i].astype(np.float64) / (t.n_a[a] + t.n_b[ib]).astype(np.float64)
            best_a[a] = d.max()
            best_b[ib] = np.maximum(best_b[ib], d)
    return best_a, best_b


def symmetric_best_dice(t):
    best_a, best_b = best_dice(t)
    ia, ib = objects(t)
    da = math.fsum(best_a[ia]) / len(ia) if len(ia) else 0.0
    db = math.fsum(best_b[ib]) / len(ib) if len(ib) else 0.0
    return 1.0 - min(da, db), (da, db)


def all_scores(seg, target, threshold=0.5):
    t = table(seg, target)
    m = matching(t, threshold)
    out = {"rand": adapted_rand_error(t), "voi": variation_of_information(t), "sbd": symmetric_best_dice(t)[0]}
    out.update({k: 1.0 - m[k] for k in STATS})
    return out
