"""CPU: the definition of the seeded watershed (tests/watershed_ref.py) checked against itself -- two algorithms, one forest;
hand-made cases written out; how far the definition is from a priority flood; the round bound of the kernel's Boruvka
scheme -- and the host-side argument checks of ops.seeded_watershed and torch_em_amd.util.segmentation."""
import functools

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

import watershed_ref as R

SHAPES = [(1, 32, 32), (8, 16, 16)]
SEEDS = list(range(100, 110))


@functools.lru_cache(maxsize=None)
def case(seed, shape):
    """the issue's inputs, drawn in this order: heights, mask, markers 1..8"""
    rs = np.random.RandomState(seed)
    h = gaussian_filter(rs.rand(*shape).astype(np.float32), 1.5).astype(np.float32)
    mask = gaussian_filter(rs.rand(*shape), 1.0) > 0.47
    markers = np.zeros(h.size, np.int64)
    markers[rs.choice(h.size, 8, replace=False)] = np.arange(1, 9)
    return h, markers.reshape(shape), mask


@functools.lru_cache(maxsize=None)
def forest(seed, shape):
    return R.kruskal(*case(seed, shape))


HAND = {
    # the pass voxel (height 5) has two edges of its own height: the tie goes to the lower other end, its neighbour of height 1
    "pass_line": (np.float32([[[0, 1, 5, 2, 0]]]), [[[1, 0, 0, 0, 2]]], None, [[[1, 1, 1, 2, 2]]]),
    # a plateau is not split half-way: ranks follow the raster order, so the first marker takes all of it
    "plateau_line": (np.zeros((1, 1, 5), np.float32), [[[1, 0, 0, 0, 2]]], None, [[[1, 1, 1, 1, 2]]]),
    # the corner of height 9 lies between both basins; its edges tie at its own rank, the lower other end (height 2) wins
    "pass_plane": (np.float32([[[1, 2, 9], [8, 7, 3], [4, 5, 6]]]), [[[1, 0, 0], [0, 0, 2], [0, 0, 0]]], None,
                   [[[1, 1, 1], [1, 1, 2], [2, 2, 2]]]),
    "plateau_plane": (np.ones((1, 3, 3), np.float32), [[[0, 0, 0], [0, 0, 3], [0, 7, 0]]], None, [[[3, 3, 3], [3, 3, 3], [3, 7, 3]]]),
    # the mask cuts the line: the right part has no marker and stays 0, the marker outside the mask is ignored
    "masked_line": (np.float32([[[3, 2, 1, 0, 1]]]), [[[4, 0, 9, 0, 0]]], [[[1, 1, 0, 1, 1]]], [[[4, 4, 0, 0, 0]]]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(name):
    h, markers, mask, want = HAND[name]
    for algo in (R.kruskal, R.prim):
        assert np.array_equal(algo(h, markers, mask), np.array(want)), (name, algo.__name__)
    got, rounds = R.boruvka(h, markers, mask)
    assert np.array_equal(got, np.array(want)) and rounds <= R.round_bound(h.size)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_kruskal_equals_prim(seed, shape):
    h, markers, mask = case(seed, shape)
    assert np.array_equal(forest(seed, shape), R.prim(h, markers, mask))
    assert np.array_equal(R.kruskal(h, markers), R.prim(h, markers)), "without a mask"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_forest_agrees_with_the_flood_on_untied_heights(seed, shape):
    """a condition on the DEFINITION, not a tolerance of the kernel: measured 0.9904 at worst"""
    h, markers, mask = case(seed, shape)
    assert np.unique(h).size >= h.size - 8, "smoothed noise: next to no two heights are equal"
    agree = float((forest(seed, shape) == R.flood(h, markers, mask))[mask].mean())
    print(f"WATERSHED_FLOOD seed {seed} shape {shape}: agreement {agree:.4f}")
    assert agree >= 0.98


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_round_bound(seed, shape):
    h, markers, mask = case(seed, shape)
    got, rounds = R.boruvka(h, markers, mask)
    assert np.array_equal(got, forest(seed, shape))
    assert 1 <= rounds <= R.round_bound(h.size)


def test_round_bound_is_the_librarys():
    from torch_em_amd import _lib, ops
    lib = _lib.load()
    for V in (1, 2, 3, 4, 5, 255, 256, 257, 4096, 2 ** 21, 2 ** 24 + 1, 2 ** 31 - 2):
        want = int(np.ceil(np.log2(V))) + 1
        assert R.round_bound(V) == ops.watershed_rounds(V) == lib.tem_watershed_rounds(V) == want, V
    assert lib.tem_watershed_rounds(0) == -1 and lib.tem_watershed_rounds(2 ** 31 - 1) == -1
    assert lib.tem_watershed_ws(2, 1000) >= 2 * 1000 * 20 and lib.tem_watershed_ws(1, 2 ** 31) == -1


def test_entry_point_refuses_before_any_launch():
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_watershed(None, None, None, 4, None, None, None, 1, 1, 4, 4, None, 0, None) == -1
    assert b"null pointer" in lib.tem_last_error()
    assert lib.tem_rawaug_blur_z(None, None, 1, 1, 1, None, 1, None) == -1


def test_seeded_watershed_host_checks():
    from torch_em_amd import ops
    h = torch.rand(1, 2, 4, 4)
    mk = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="float32 heights"):
        ops.seeded_watershed(h.double(), mk)
    with pytest.raises(ValueError, match="float32 heights"):
        ops.seeded_watershed(h[0], mk[0])
    with pytest.raises(ValueError, match="integer type"):
        ops.seeded_watershed(h, mk.float())
    with pytest.raises(ValueError, match="do not match"):
        ops.seeded_watershed(h, mk[:, :1])
    with pytest.raises(ValueError, match="bool mask"):
        ops.seeded_watershed(h, mk, torch.ones(1, 2, 4, 4))
    with pytest.raises(ValueError, match="bool mask"):
        ops.seeded_watershed(h, mk, torch.ones(1, 2, 4, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="rounds_out"):
        ops.seeded_watershed(h, mk, None, torch.zeros(2, dtype=torch.int32))
    neg = mk.clone()
    neg[0, 0, 0, 0] = -1
    with pytest.raises(ValueError, match="markers must be >= 0"):
        ops.seeded_watershed(h, neg)
    bad = h.clone()
    bad[0, 1, 2, 3] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        ops.seeded_watershed(bad, mk)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seeded_watershed(h, mk)                       # a valid call on host tensors: refused like every op
    with pytest.raises(ValueError, match="float32 heights"):
        ops.voxel_ranks(h.double())


def test_public_functions_host_checks():
    from torch_em_amd.util import segmentation as S
    a, b = np.zeros((4, 5), np.float32), np.zeros((4, 6), np.float32)
    with pytest.raises(ValueError, match="one shape"):
        S.connected_components_with_boundaries(a, b)
    with pytest.raises(ValueError, match="one shape"):
        S.watershed_from_components(a, b)
    with pytest.raises(ValueError, match="one shape"):
        S.watershed_from_center_and_boundary_distances(a, a, b)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        S.watershed_from_components(np.zeros(7, np.float32), np.zeros(7, np.float32))
    seg = np.zeros((4, 5), np.int64)
    assert S.size_filter(seg, 0) is seg
    with pytest.raises(ValueError, match="hmap"):
        S.size_filter(seg, 3, hmap=b)
    with pytest.raises(ValueError, match="hmap"):
        S.size_filter(seg, 3, hmap=np.zeros((2, 4, 6), np.float32))
    with pytest.raises(ValueError, match=">= 0"):
        S.size_filter(seg - 1, 3)
    assert not hasattr(S, "mutex_watershed_segmentation") and not hasattr(S, "watershed_from_maxima")
