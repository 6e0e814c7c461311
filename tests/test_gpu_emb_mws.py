"""GPU: the embedding mutex watershed -- ops.embedding_edges (csrc/embmws.hip) against numpy's float32 expression, bit for
bit; util.segment_embeddings_mws against the sequential oracle tests/mws_ref.py on numpy's weights; the background merge
against a float64 oracle; one end-to-end call per metric family.  Integers and bits are compared with equality."""
import functools

import numpy as np
import pytest
import torch

import mws_ref as M
from oracle.gpu_kit import DEV, wave_slot_rows

pytestmark = pytest.mark.gpu

DELTA = 0.75
# both signs, a diagonal inside the halo, dz != 0, beyond the halo (9, -5), beyond the 17 axis (27); nine: two offset groups
OFFS = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 3, -2], [1, -4, 4], [0, 0, 9], [0, -9, 0], [0, 27, 0], [2, 0, -5]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def np_edges(emb, offs, delta, n_attr, strides, l1=False):
    """the definition in numpy float32, one sample [E, D, H, W] -> (aff [C, D, H, W], edge_valid)"""
    emb = np.asarray(emb, np.float32)
    sp = emb.shape[1:]
    td = np.float32(2) * np.float32(delta)
    aff = np.zeros((len(offs),) + sp, np.float32)
    for c, o in enumerate(offs):
        if any(abs(d) >= s for d, s in zip(o, sp)):
            continue
        v = tuple(slice(max(-d, 0), s - max(d, 0)) for d, s in zip(o, sp))
        u = tuple(slice(max(d, 0), s - max(-d, 0)) for d, s in zip(o, sp))
        acc = np.zeros(aff[c][v].shape, np.float32)
        for x in emb:
            df = x[v] - x[u]
            acc = acc + (np.abs(df) if l1 else df * df)
        r = np.maximum(td - (acc if l1 else np.sqrt(acc)), np.float32(0)) / td
        aff[c][v] = np.float32(1) - r * r
    assert aff.dtype == np.float32
    return aff, M.grid_edge_valid(sp, offs, n_attr, strides)


@functools.lru_cache(maxsize=None)
def embeddings(shape, E, l1):
    """[2, E, *shape]: noise of a scale that leaves most distances (a sum of E terms for l1, the root of one for l2) below
    2 delta, a block of identical voxels (d = 0) and a block ten times as far apart (beyond 2 delta: the clamp); the
    samples differ"""
    rs = np.random.RandomState(E + sum(shape))
    emb = (rs.randn(2, E, *shape) * (0.6 / (E if l1 else np.sqrt(E)))).astype(np.float32)
    emb[0, :, :, :5, :7] = emb[0, :, :1, :1, :1]
    emb[1, :, :, -6:, -9:] *= np.float32(10)
    return emb


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("strides", [(1, 1, 1), (1, 4, 4), (2, 3, 2)])
@pytest.mark.parametrize("E", [1, 3, 16, 33])
@pytest.mark.parametrize("shape", [(1, 17, 23), (5, 9, 11), (2, 6, 136)])   # 136: 16-byte rows, two column tiles
def test_embedding_edges_bit_for_bit(shape, E, strides, l1):
    from torch_em_amd import ops
    emb = embeddings(shape, E, l1)
    aff, valid = ops.embedding_edges(dev(emb), OFFS, DELTA, 3, strides, "l1" if l1 else "l2")
    assert aff.dtype == torch.float32 and valid.dtype == torch.bool and tuple(aff.shape) == (2, len(OFFS)) + shape == tuple(valid.shape)
    wants = [np_edges(emb[n], OFFS, DELTA, 3, strides, l1) for n in range(2)]
    near = np.stack([w[0][1:3] for w in wants])
    assert (near == 1).any() and ((near > 0) & (near < 1)).any() and (wants[0][0][2, :, :5, 1:7] == 0).all(), "clamped, graded, d = 0"
    for n, (want, want_valid) in enumerate(wants):
        got = aff[n].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, int((got != want).sum()), float(np.abs(got - want).max()))
        assert np.array_equal(valid[n].cpu().numpy(), want_valid), n
    assert not np.array_equal(aff[0].cpu().numpy(), aff[1].cpu().numpy())


def cells(shape, n, seed):
    """labels 1..n: Voronoi cells of n random points"""
    rs = np.random.RandomState(seed)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    return np.argmin(((grid[..., None, :] - rs.rand(n, len(shape)) * np.array(shape)) ** 2).sum(-1), -1) + 1


OFFS_SEG = {2: [[-1, 0], [0, -1], [-3, 0], [0, -3], [-6, 5]], 3: [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-1, -4, 4]]}


@functools.lru_cache(maxsize=None)
def segmentation_case(ndim):
    """(embeddings [4, *shape], strides, the oracle's labels): a few cells with centres 3 delta apart, noise, and two single
    voxels far from everything, which a size filter of 3 removes"""
    shape = (20, 24) if ndim == 2 else (4, 10, 12)
    rs = np.random.RandomState(40 + ndim)
    lab = cells(shape, 4, 7 + ndim)
    centres = np.concatenate([np.zeros((1, 4)), 3 * DELTA * np.eye(4)])
    emb = (np.moveaxis(centres[lab], -1, 0) + 0.1 * DELTA * rs.randn(4, *shape)).astype(np.float32)
    emb[(slice(None),) + (1,) * (ndim - 2) + (4, 4)] = -5
    emb[(slice(None),) + (3,) * (ndim - 1) + (8,)] = 7
    strides = [1, 2, 2][-ndim:]
    s3 = (1,) * (3 - ndim) + shape
    aff, valid = np_edges(emb.reshape((4,) + s3), [[0] * (3 - ndim) + o for o in OFFS_SEG[ndim]], DELTA, ndim, [1] * (3 - ndim) + strides)
    want = M.sequential(aff.reshape((-1,) + shape), OFFS_SEG[ndim], ndim, None, valid.reshape((-1,) + shape))
    return emb, strides, want


def np_filter(seg, min_size):
    ids, counts = np.unique(seg, return_counts=True)
    kept = ids[(counts >= min_size) & (ids > 0)]
    return np.where(np.isin(seg, kept), np.searchsorted(kept, seg) + 1, 0)


@pytest.mark.parametrize("min_size", [0, 3])
@pytest.mark.parametrize("ndim", [2, 3])
def test_segment_embeddings_mws_is_the_sequential_result(ndim, min_size):
    from torch_em_amd.util import segment_embeddings_mws
    emb, strides, want = segmentation_case(ndim)
    assert want.max() >= 4 and np_filter(want, 3).max() < want.max(), "several segments, and the filter removes some"
    want = np_filter(want, min_size) if min_size else want
    got = segment_embeddings_mws(emb, OFFS_SEG[ndim], DELTA, strides, min_size=min_size)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    both = segment_embeddings_mws(dev(np.stack([emb, emb])), OFFS_SEG[ndim], DELTA, strides, min_size=min_size)
    assert tuple(both.shape) == (2, 1) + want.shape and both.is_cuda and all(np.array_equal(b[0].cpu().numpy(), want) for b in both)


# sizes of the regions 1..6 in flattened order; region 6 lies 0.15 delta from the largest.  The second case: 2 and 3 tie
BG_CASES = {"largest": [40, 70, 50, 30, 25, 25], "tie": [40, 60, 60, 30, 25, 25], "five": [35, 90, 20, 45, 50]}


def background_case(name, seed):
    """-> (ids [4, 6, 10], embeddings [3, 4, 6, 10], the float64 oracle's result)"""
    sizes = BG_CASES[name]
    rs = np.random.RandomState(seed)
    ids = np.repeat(np.arange(1, len(sizes) + 1), sizes).reshape(4, 6, 10)
    big = int(np.argmax(sizes))
    centres = 3 * DELTA * np.arange(len(sizes))[:, None] * np.array([1.0, 0, 0]) + np.array([0, 0.5, -0.25])
    centres[-1] = centres[big] + 0.15 * DELTA * np.array([0, 0.6, 0.8])
    emb = (np.moveaxis(centres[ids - 1], -1, 0) + 0.05 * DELTA * rs.uniform(-1, 1, (3,) + ids.shape)).astype(np.float32)
    counts = np.bincount(ids.ravel(), minlength=len(sizes) + 1)
    bg = int(np.argmax(counts[1:])) + 1
    assert bg == big + 1
    means = np.stack([[emb[e].astype(np.float64)[ids == k].mean() for e in range(3)] for k in range(1, len(sizes) + 1)])
    p = (np.maximum(2 * DELTA - np.sqrt(((means - means[bg - 1]) ** 2).sum(1)), 0) / (2 * DELTA)) ** 2
    assert (np.abs(p - 0.5) > 1e-3).all(), "the fixture keeps every p_k away from the threshold"
    assert p[bg - 1] == 1 and p[-1] > 0.5 and (p > 0.5).sum() == 2
    kept = np.flatnonzero(p <= 0.5) + 1
    want = np.where(np.isin(ids, kept), np.searchsorted(kept, ids) + 1, 0)
    return ids.astype(np.int32), emb, want


def test_background_merge_against_float64():
    from torch_em_amd import ops
    cases = [background_case(name, seed) for name, seed in (("largest", 1), ("tie", 2), ("five", 3))]
    ids = np.stack([c[0] for c in cases])
    emb = np.stack([c[1] for c in cases])
    got = ops.merge_background_by_embedding_(dev(ids), dev(emb), DELTA)
    for n, c in enumerate(cases):
        assert np.array_equal(got[n].cpu().numpy(), c[2]), n
    again = ops.merge_background_by_embedding_(dev(ids), dev(emb), DELTA)
    assert torch.equal(again, got), "a second launch: the same bits"
    zero = ids.copy()
    zero[0][ids[0] == 1] = 0       # id 0 is no segment: it stays, and the others are numbered as before without it
    got0 = ops.merge_background_by_embedding_(dev(zero), dev(emb), DELTA)[0].cpu().numpy()
    assert np.array_equal(got0, np.where(ids[0] == 1, 0, np.maximum(cases[0][2] - 1, 0)))


def test_background_merge_chosen_id_mixes_in_one_wave():
    """the counts and sums where a wave holds one segment, several, none, a partial tail and segments of two samples;
    segments 5, 20 and 81 lie 0.1 delta from the largest (segment 1) and go with it, the others 3 delta and more away"""
    from torch_em_amd import ops
    ids = wave_slot_rows()
    rs = np.random.RandomState(5)
    near = np.isin(np.arange(82), [1, 5, 20, 81])
    centre = np.where(near, 0.1 * DELTA * (np.arange(82) % 2), 3 * DELTA * (1 + np.arange(82) % 3))
    emb = np.stack([centre[ids], -centre[ids]], 1) + 0.02 * DELTA * rs.uniform(-1, 1, (2, 2, 389))
    emb = emb.astype(np.float32)
    want = np.zeros_like(ids)
    for n in range(2):
        counts = np.bincount(ids[n], minlength=82)
        assert int(np.argmax(counts[1:])) + 1 == 1
        seg = np.flatnonzero(counts[1:]) + 1
        means = np.stack([[emb[n, e].astype(np.float64)[ids[n] == k].mean() for e in range(2)] for k in seg])
        p = (np.maximum(2 * DELTA - np.sqrt(((means - means[0]) ** 2).sum(1)), 0) / (2 * DELTA)) ** 2
        assert (np.abs(p - 0.5) > 0.3).all() and np.array_equal(seg[p > 0.5], [1, 5, 20, 81])
        kept = seg[p <= 0.5]
        want[n] = np.where(np.isin(ids[n], kept), np.searchsorted(kept, ids[n]) + 1, 0)
    got = ops.merge_background_by_embedding_(dev(ids.astype(np.int32).reshape(2, 1, 1, 389)), dev(emb.reshape(2, 2, 1, 1, 389)), DELTA)
    assert np.array_equal(got.cpu().numpy().reshape(2, 389), want)


def boxes(shape, corners, size):
    target = np.zeros(shape, np.int64)
    for k, (y, x) in enumerate(corners):
        target[..., y:y + size, x:x + size] = k + 1
    return target


def test_metrics_end_to_end():
    """a prediction whose segmentation is the target scores 0; init_kwargs round-trip; the watershed metrics still run with
    host synchronisation forbidden and the mutex-watershed ones say that they cannot"""
    from torch_em_amd import metric
    target = np.stack([boxes((24, 32), [(4, 4), (12, 20)], 8), boxes((24, 32), [(8, 8), (0, 20), (16, 24)], 6)])
    offs = [[-1, 0], [0, -1], [-4, 0], [0, -4], [-9, 0], [0, -9]]
    centres = np.concatenate([np.zeros((1, 4)), 3 * DELTA * np.eye(4)])
    emb = np.moveaxis(centres[target], -1, 1).astype(np.float32)
    m = metric.EmbeddingMWSIOUMetric(DELTA, offs, min_seg_size=4, iou_threshold=0.5)
    assert float(m(dev(emb), dev(target[:, None]))) == 0.0
    shifted = [np.roll(target, tuple(-d for d in o), (1, 2)) for o in offs]
    aff = np.stack([(s != target) for s in shifted], 1).astype(np.float32)
    pred = np.concatenate([(target > 0)[:, None].astype(np.float32), aff], 1)
    w = metric.MWSIOUMetric(offs, min_seg_size=4, strides=[2, 2])
    assert float(w(dev(pred), dev(target[:, None]))) == 0.0
    for made in (m, w, metric.MWSVOIMetric(offs, 4), metric.EmbeddingMWSRandMetric(DELTA, offs, 4, strides=[2, 2])):
        assert type(made)(**made.init_kwargs).init_kwargs == made.init_kwargs and not made.sync_free
    assert m.segmenter.strides == [4, 4] and w.segmenter.strides == [2, 2], "the reference's wiring: strides reach MWS only"
    ws = metric.WatershedSBDMetric("components", min_size=2)
    assert ws.sync_free
    maps, ids = dev(np.stack([pred[:, 0], 1 - pred[:, 0]], 1)), dev(target[:, None])
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score = ws(maps, ids)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert score.is_cuda and 0.0 <= float(score) <= 1.0
