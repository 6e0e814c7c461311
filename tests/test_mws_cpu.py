"""CPU: the two oracles of the mutex watershed (tests/mws_ref.py) against each other and against literal answers -- the
sequential Kruskal with mutex constraints, and the simulation of the round schedule csrc/mws.hip runs (R1-R3).  The
subsampling helper draws from a device generator: its tests are in test_gpu_mws.py."""
import numpy as np
import pytest
from scipy import ndimage

import mws_ref as M

OFFS2 = [[-1, 0], [0, -1], [-2, 0], [0, -2], [-3, -3], [-3, 3], [-5, 0], [0, -5]]
OFFS3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-1, -2, 2], [0, -4, -4]]


def random_graph(seed):
    """one seeded small graph: 2-D or 3-D, sides 3..20, a mix of weight kinds, masks and subsampled long-range edges"""
    rs = np.random.RandomState(seed)
    ndim = 2 + seed % 2
    shape = tuple(int(s) for s in (rs.randint(3, 21, 2) if ndim == 2 else rs.randint(3, 11, 3)))
    if seed % 20 == 19:
        shape = (20, 20) if ndim == 2 else (3, 20, 5)
    offs = OFFS2 if ndim == 2 else OFFS3
    C = int(rs.randint(ndim, len(offs) + 1))
    offs = offs[:C]
    kind = seed % 4
    aff = rs.rand(C, *shape).astype(np.float32)
    if kind == 1:
        aff = np.stack([ndimage.gaussian_filter(a, 1.0) for a in aff]).astype(np.float32)
    elif kind == 2:
        aff = (np.floor(aff * 3) / 2).astype(np.float32)          # three levels: ties everywhere
    elif kind == 3 and seed % 8 == 3:
        aff = np.full_like(aff, 0.5)
    mask = None if seed % 3 == 0 else ndimage.gaussian_filter(rs.rand(*shape), 1.0) > 0.45
    ev = None
    if seed % 5 < 2:
        ev = np.ones((C,) + shape, bool)
        ev[ndim:] = rs.rand(C - ndim, *shape) < 0.25
    elif seed % 5 == 2:
        ev = M.grid_edge_valid(shape, offs, ndim, [2] * ndim)
    return aff, offs, ndim, mask, ev


@pytest.mark.parametrize("block", range(8))
def test_schedule_equals_sequential(block):
    """208 seeded graphs in 8 blocks"""
    for seed in range(block * 26, block * 26 + 26):
        aff, offs, na, mask, ev = random_graph(seed)
        want = M.sequential(aff, offs, na, mask, ev)
        got, rounds = M.schedule(aff, offs, na, mask, ev)
        assert np.array_equal(got, want), (seed, aff.shape)
        assert want.max() >= 1 or (mask is not None and not mask.any())
        if seed % 13 == 0:
            slow, more = M.schedule(aff, offs, na, mask, ev, mutual_only=True)
            assert np.array_equal(slow, want) and more >= rounds, seed
            plain, some = M.schedule(aff, offs, na, mask, ev, partners=False)
            assert np.array_equal(plain, want) and more >= some >= rounds, seed


def two_chains(repulsive):
    """1 x 6: voxels 0 1 2 | 3 4 5; attractive [0, -1] strong inside the chains (p 0.9), weak across 2-3 (p 0.4); one
    repulsive edge [0, -5] between 0 and 5 of priority `repulsive`"""
    aff = np.zeros((2, 1, 6), np.float32)
    aff[0, 0] = np.float32(0.1)
    aff[0, 0, 3] = np.float32(0.6)
    aff[1, 0, 5] = np.float32(repulsive)
    ev = np.ones((2, 1, 6), bool)
    return aff, [[0, -1], [0, -5]], 1, None, ev


def test_literal_answers():
    for fn in (M.sequential, lambda *a: M.schedule(*a)[0]):
        assert fn(*two_chains(0.7)).tolist() == [[1, 1, 1, 2, 2, 2]], "the repulsive edge comes before the joining one"
        assert fn(*two_chains(0.3)).tolist() == [[1, 1, 1, 1, 1, 1]], "the repulsive edge comes too late"
        rs = np.random.RandomState(3)
        mask = ndimage.gaussian_filter(rs.rand(12, 13), 1.0) > 0.5
        aff = rs.rand(2, 12, 13).astype(np.float32)
        assert np.array_equal(fn(aff, [[-1, 0], [0, -1]], 2, mask), ndimage.label(mask)[0]), "no repulsive channel: the components"
        aff = np.concatenate([rs.rand(2, 5, 7) * 0.5 + 0.5, rs.rand(2, 5, 7) * 0.4 + 0.6]).astype(np.float32)   # p < 0.5 | p >= 0.6
        got = fn(aff, [[-1, 0], [0, -1], [-1, 0], [0, -1]], 2)
        assert np.array_equal(got, np.arange(1, 36).reshape(5, 7)), "repulsive above attractive on every pair: all alone"
        lone = np.zeros((3, 3), bool)
        lone[0, 0] = lone[2, 2] = lone[2, 1] = True
        assert fn(np.full((2, 3, 3), 0.1, np.float32), [[-1, 0], [0, -1]], 2, lone).tolist() == [[1, 0, 0], [0, 0, 0], [0, 2, 2]]
        assert not fn(aff, [[-1, 0], [0, -1], [-1, 0], [0, -1]], 2, np.zeros((5, 7), bool)).any()


def test_ties_go_to_the_lower_edge_id():
    """1 x 3, voxels 0 1 2: attractive (0,1) id 1 and (1,2) id 2, repulsive [0, -2] (0,2) id 5; all of priority 0.5.  The
    attractive ids are lower: both merges come first and the repulsive edge finds one cluster."""
    aff = np.full((2, 1, 3), 0.5, np.float32)
    for fn in (M.sequential, lambda *a: M.schedule(*a)[0]):
        assert fn(aff, [[0, -1], [0, -2]], 1).tolist() == [[1, 1, 1]]
        # the same priorities with the attractive edge (1,2) made later than the repulsive one by its weight alone
        later = aff.copy()
        later[0, 0, 2] = np.nextafter(np.float32(0.5), np.float32(1))       # p = 1 - aff: just below 0.5
        assert fn(later, [[0, -1], [0, -2]], 1).tolist() == [[1, 1, 2]], "(0,1), then the mutex 0-2 keeps 2 out"
        # two equal attractive edges compete for a voxel that may join only one side: 0 and 2 exclusive first (p 0.9)
        aff3 = np.full((2, 1, 3), 0.5, np.float32)
        aff3[1, 0, 2] = np.float32(0.9)
        assert fn(aff3, [[0, -1], [0, -2]], 1).tolist() == [[1, 1, 2]], "edge id 1 (0,1) before edge id 2 (1,2)"
    p = np.float32([0.5, 0.5, -0.0, 0.0])
    k = M.keys(p + np.float32(0), np.arange(4))
    assert k[0] > k[1] > k[2] > k[3] and len(set(k.tolist())) == 4, "equal priority: the lower id has the larger key"


def test_keys_order_like_the_stable_sort():
    rs = np.random.RandomState(5)
    p = np.concatenate([rs.randn(500), np.floor(rs.rand(500) * 3) - 1, [0.0, -0.0, np.inf, -np.inf]]).astype(np.float32) + np.float32(0)
    ids = rs.permutation(p.size)
    by_sort = np.lexsort((ids, -p))
    by_key = np.argsort(~M.keys(p, ids), kind="stable")
    assert np.array_equal(by_sort, by_key)


def test_grid_rule():
    ev = M.grid_edge_valid((5, 6), [[-1, 0], [0, -1], [-3, 0]], 2, [2, 3])
    assert ev[:2].all() and ev[2].sum() == 3 * 2 and ev[2, 4, 3] and not ev[2, 1, 0] and not ev[2, 0, 1]


def test_public_function_is_exported_and_checks_its_arguments():
    """the host-side checks of mutex_watershed_segmentation come before anything touches a device"""
    from torch_em_amd import util
    S = util.mutex_watershed
    assert util.mutex_watershed_segmentation is S.mutex_watershed_segmentation
    assert util.repulsive_edge_subsampling is S.repulsive_edge_subsampling
    fg, aff, offs = np.zeros((6, 8), np.float32), np.zeros((4, 6, 8), np.float32), [[-1, 0], [0, -1], [-3, 0], [0, -3]]
    with pytest.raises(ValueError, match="do not match the foreground"):
        S.mutex_watershed_segmentation(fg, aff[:, :, :-1], offs)
    with pytest.raises(ValueError, match="do not match the foreground"):
        S.mutex_watershed_segmentation(fg[None, None], aff, offs)
    with pytest.raises(ValueError, match="offsets do not match"):
        S.mutex_watershed_segmentation(fg, aff, offs[:-1])
    with pytest.raises(ValueError, match="at most 32"):
        S.mutex_watershed_segmentation(fg, np.zeros((33, 6, 8), np.float32), [[0, -1]] * 33)
    with pytest.raises(ValueError, match="entries each"):
        S.mutex_watershed_segmentation(fg, aff, [o + [0] for o in offs])
    with pytest.raises(ValueError, match="strides"):
        S.repulsive_edge_subsampling((4, 4), 5, 2, [2, 2, 2])
    with pytest.raises(TypeError, match="seed must be an integer"):
        S.repulsive_edge_subsampling((4, 4), 5, 2, None, True, seed=1.5)
