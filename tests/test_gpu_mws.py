"""GPU: the mutex watershed (csrc/mws.hip, ops.mutex_watershed), the subsampling helper and
torch_em_amd.util.mutex_watershed.mutex_watershed_segmentation against the numpy oracle tests/mws_ref.py.  Labels and round
counts are compared with equality: there is no tolerance on integers anywhere.  The only bound here, the binomial one of the
random subsampling, is derived where it is used."""
import functools

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

import mws_ref as M
from oracle.gpu_kit import DEV

pytestmark = pytest.mark.gpu

OFFS2 = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-5, -5], [-9, 0], [0, -9], [-9, 9]]
OFFS3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-1, -2, 2], [0, -4, -4], [-3, -3, -9]]


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


def weights(kind, rs, shape):
    """affinities [C, *spatial] of one kind"""
    a = rs.rand(*shape).astype(np.float32)
    if kind == "smooth":
        a = np.stack([gaussian_filter(c, 1.5) for c in a]).astype(np.float32)
        a = (a - a.min()) / (a.max() - a.min())
    elif kind == "quantised":
        a = (np.floor(a * 4) / 4).astype(np.float32)              # four levels: ties everywhere
    elif kind == "constant":
        a = np.full(shape, 0.5, np.float32)
    return a.astype(np.float32)


def holes(rs, shape):
    return gaussian_filter(rs.rand(*shape), 1.0) > 0.45


def build_cases():
    """name -> (aff [C, *spatial], offsets, n_attractive, mask or None, edge_valid or None): one sample each"""
    C = {}
    rs = np.random.RandomState(23)
    s2 = (17, 19)
    for kind in ("random", "smooth", "quantised", "constant"):
        for masked in (False, True):
            for sub in (False, True):
                ev = None
                if sub:
                    ev = np.ones((8,) + s2, bool)
                    ev[2:] = rs.rand(6, *s2) < 0.3
                C[f"2d_{kind}_{'mask' if masked else 'full'}_{'sub' if sub else 'all'}"] = (
                    weights(kind, rs, (8,) + s2), OFFS2, 2, holes(rs, s2) if masked else None, ev)
    s3 = (5, 9, 67)
    ev3 = np.ones((9,) + s3, bool)
    ev3[3:] = rs.rand(6, *s3) < 0.25
    C["3d_random"] = (weights("random", rs, (9,) + s3), OFFS3, 3, None, None)
    C["3d_smooth_mask_sub"] = (weights("smooth", rs, (9,) + s3), OFFS3, 3, holes(rs, s3), ev3)
    C["3d_quantised_mask"] = (weights("quantised", rs, (9,) + s3), OFFS3, 3, holes(rs, s3), None)
    line = (1, 1, 600)
    C["line_600"] = (weights("random", rs, (9,) + line), OFFS3, 3, None, None)
    C["line_600_quantised"] = (weights("quantised", rs, (9,) + line), OFFS3, 3, rs.rand(*line) < 0.9, None)
    signed = np.where(rs.rand(8, *s2) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    signed[:2] = np.where(rs.rand(2, *s2) < 0.5, np.float32(1.0), np.nextafter(np.float32(1), np.float32(0)))
    C["2d_signed_zeros"] = (signed, OFFS2, 2, None, None)
    # repulsive above attractive on every pair: every voxel alone, every repulsive edge a mutex
    alone = np.concatenate([rs.rand(2, *s2) * 0.5 + 0.5, rs.rand(2, *s2) * 0.4 + 0.6]).astype(np.float32)
    C["2d_all_alone"] = (alone, [[-1, 0], [0, -1], [-1, 0], [0, -1]], 2, None, None)
    C["2d_no_repulsive"] = (weights("random", rs, (2,) + s2), OFFS2[:2], 2, holes(rs, s2), None)
    C["2d_only_repulsive"] = (weights("random", rs, (2,) + s2), OFFS2[:2], 0, None, None)
    C["2d_empty_mask"] = (weights("random", rs, (8,) + s2), OFFS2, 2, np.zeros(s2, bool), None)
    C["single_voxel"] = (np.float32([[[0.5]], [[0.5]]]), [[-1, 0], [0, -1]], 1, None, None)
    return C


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the sequential oracle's labels, the simulated schedule's working rounds); the simulation's labels are checked here"""
    want = M.sequential(*CASES[name])
    sim, rounds = M.schedule(*CASES[name])
    assert np.array_equal(sim, want)
    return want, rounds


def run(aff, offsets, n_attractive, mask=None, edge_valid=None, put=dev, **kw):
    """one sample -> (labels in the spatial shape, rounds that did work)"""
    from torch_em_amd import ops
    sp = aff.shape[1:]
    s3 = (1,) * (3 - len(sp)) + sp
    out, rounds = ops.mutex_watershed(put(aff.reshape((1, aff.shape[0]) + s3)), offsets, n_attractive,
                                      None if mask is None else put(mask.reshape((1,) + s3)),
                                      None if edge_valid is None else put(edge_valid.reshape((1, aff.shape[0]) + s3)),
                                      return_rounds=True, **kw)
    assert out.dtype == torch.int32 and tuple(out.shape) == (1,) + s3
    return out[0].cpu().numpy().astype(np.int64).reshape(sp), rounds


# ---- the kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_mutex_watershed_is_the_sequential_result(name):
    want, rounds = reference(name)
    got, r = run(*CASES[name])
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert r == rounds, (name, r, rounds)
    again, r2 = run(*CASES[name], put=misaligned)
    assert np.array_equal(again, got) and r2 == r, "misaligned inputs, a second call: one answer"


def test_literal_answers():
    aff = np.zeros((2, 1, 6), np.float32)
    aff[0, 0] = np.float32(0.1)
    aff[0, 0, 3] = np.float32(0.6)
    aff[1, 0, 5] = np.float32(0.7)
    assert run(aff, [[0, -1], [0, -5]], 1)[0].tolist() == [[1, 1, 1, 2, 2, 2]], "the repulsive edge comes first"
    aff[1, 0, 5] = np.float32(0.3)
    assert run(aff, [[0, -1], [0, -5]], 1)[0].tolist() == [[1, 1, 1, 1, 1, 1]], "the repulsive edge comes too late"
    tie = np.full((2, 1, 3), 0.5, np.float32)
    tie[1, 0, 2] = np.float32(0.9)
    assert run(tie, [[0, -1], [0, -2]], 1)[0].tolist() == [[1, 1, 2]], "equal weights: edge id 1 (0,1) before edge id 2 (1,2)"
    assert np.array_equal(reference("2d_all_alone")[0], np.arange(1, 17 * 19 + 1).reshape(17, 19))
    assert not run(*CASES["2d_empty_mask"])[0].any()
    assert run(*CASES["2d_empty_mask"])[1] == 0 and run(*CASES["single_voxel"])[1] == 0, "no edge: no round does work"
    lone = np.zeros((3, 3), bool)
    lone[0, 0] = lone[2, 2] = lone[2, 1] = True
    got, _ = run(np.full((2, 3, 3), 0.1, np.float32), [[-1, 0], [0, -1]], 2, lone)
    assert got.tolist() == [[1, 0, 0], [0, 0, 0], [0, 2, 2]], "a masked voxel without edges is a segment of its own"


def test_batch_equals_single_calls():
    """offsets with positive components: v + offset of a voxel near the end of sample 0 is a voxel of sample 1 in the flat
    batch -- that edge does not exist"""
    from torch_em_amd import ops
    rs = np.random.RandomState(31)
    sp = (3, 5, 7)
    offs = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [2, 2, 2], [0, 4, -3], [-2, 0, 6]]
    aff = np.stack([weights("random", rs, (7,) + sp), weights("quantised", rs, (7,) + sp)])
    mask = np.stack([np.ones(sp, bool), holes(rs, sp)])
    ev = rs.rand(2, 7, *sp) < 0.7
    got, rounds = ops.mutex_watershed(dev(aff), offs, 3, dev(mask), dev(ev), return_rounds=True)
    singles = [run(aff[n], offs, 3, mask[n], ev[n]) for n in range(2)]
    for n in range(2):
        assert np.array_equal(got[n].cpu().numpy(), singles[n][0]), n
        assert np.array_equal(singles[n][0], M.sequential(aff[n], offs, 3, mask[n], ev[n])), n
    assert rounds == max(s[1] for s in singles), "a round does work when it does for any sample"
    assert np.array_equal(ops.mutex_watershed(dev(aff), offs, 3).cpu().numpy(),
                          np.stack([M.sequential(aff[n], offs, 3) for n in range(2)]))


def test_more_edges_than_one_grid_sweep():
    """8 x 67 600 = 540 800 edges: more than the 2048 x 256 the capped grid covers in one trip of its loops.  Two cases whose
    answer is known in closed form.  Channels: [0, -1] attractive with priority in [0.5, 0.9), [-1, 0] attractive with
    priority in [0.1, 0.3), six repulsive offsets that all cross rows.
    Repulsive priority 0.4: the rows merge first, then every pair of neighbouring rows becomes mutually exclusive, and the
    weak vertical edges find a mutex: the segments are the rows.
    Repulsive priority 0.05: every attractive edge comes first, one segment."""
    rs = np.random.RandomState(5)
    sp = (260, 260)
    offs = [[0, -1], [-1, 0], [-1, 0], [-2, 0], [-3, 0], [-1, -1], [-1, 1], [-2, 2]]
    aff = np.empty((8,) + sp, np.float32)
    aff[0] = 1 - (0.5 + 0.4 * rs.rand(*sp))
    aff[1] = 1 - (0.1 + 0.2 * rs.rand(*sp))
    aff[2:] = 0.4
    got, rounds = run(aff, offs, 2)
    assert np.array_equal(got, np.broadcast_to(np.arange(1, 261)[:, None], sp)) and rounds >= 3
    aff[2:] = 0.05
    got, rounds = run(aff, offs, 2)
    assert (got == 1).all() and rounds >= 2


def test_round_batching_and_the_table():
    """the loop across batches: 1 and 3 rounds a batch give the labels and the round count of the default, and the count is
    the simulation's.  `2d_all_alone`: every one of its repulsive edges becomes a mutex between two single voxels, so the
    set holds as many pairs as there are repulsive edges: its size is a power of two at a load of at most 0.5."""
    from torch_em_amd import ops
    for name in ("2d_all_alone", "2d_smooth_mask_sub", "line_600"):
        want, rounds = reference(name)
        assert rounds > 3, "more than one batch"
        for per in (1, 3, ops.MWS_ROUNDS_PER_BATCH, ops.MWS_MAX_BATCH):
            got, r = run(*CASES[name], rounds_per_batch=per)
            assert np.array_equal(got, want) and r == rounds, (name, per, r, rounds)
    aff, offs, na, mask, ev = CASES["2d_all_alone"]
    c, v, u = M.edges((1, 17, 19), [[0] + o for o in offs], np.ones(17 * 19, bool), np.ones((4, 17 * 19), bool))
    n_rep = int((c >= na).sum())
    assert n_rep == 2 * 17 * 19 - 17 - 19
    slots = ops.mws_table_slots(n_rep)
    assert slots & (slots - 1) == 0 and 2 * n_rep <= slots < 4 * n_rep
    assert ops.mws_table_slots(0) >= 1 and ops.mws_table_slots(1 << 20) == 1 << 21
    with pytest.raises(ValueError, match="rounds_per_batch"):
        run(*CASES["line_600"], rounds_per_batch=0)
    with pytest.raises(ValueError, match="rounds_per_batch"):
        run(*CASES["line_600"], rounds_per_batch=ops.MWS_MAX_BATCH + 1)


def test_argument_checks():
    from torch_em_amd import ops
    aff = torch.rand(1, 8, 1, 17, 19, device=DEV)
    with pytest.raises(ValueError, match="do not match the 8 affinity channels"):
        ops.mutex_watershed(aff, OFFS2[:7], 2)
    with pytest.raises(ValueError, match="at most 32"):
        ops.mutex_watershed(torch.rand(1, 33, 1, 4, 4, device=DEV), [[0, -1]] * 33, 2)
    with pytest.raises(ValueError, match="bool mask"):
        ops.mutex_watershed(aff, OFFS2, 2, torch.ones(1, 1, 17, 18, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="edge_valid"):
        ops.mutex_watershed(aff, OFFS2, 2, None, torch.ones(1, 8, 1, 17, 19, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="n_attractive"):
        ops.mutex_watershed(aff, OFFS2, 9)
    with pytest.raises(ValueError, match="float32 affinities"):
        ops.mutex_watershed(aff.double(), OFFS2, 2)
    with pytest.raises(ValueError, match="need D = 1"):
        ops.mutex_watershed(torch.rand(1, 8, 2, 17, 19, device=DEV), OFFS2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mutex_watershed(aff.cpu(), OFFS2, 2)


# ---- the subsampling helper ---------------------------------------------------------------------------------------------
def test_subsampling_helper():
    from torch_em_amd.util import mutex_watershed as S
    for shape, strides in (((9, 10), [2, 3]), ((5, 6, 7), [1, 2, 4])):
        nd = len(shape)
        offs = [[0] * nd] * (nd + 3)
        got = S.repulsive_edge_subsampling(shape, nd + 3, nd, strides, randomize_strides=False)
        assert got.dtype == torch.bool and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), M.grid_edge_valid(shape, offs, nd, strides))
        both = S.repulsive_edge_subsampling(shape, nd + 3, nd, strides, randomize_strides=False, batch=2)
        assert tuple(both.shape) == (2, nd + 3) + shape and torch.equal(both[0], got) and torch.equal(both[1], got)
    assert S.repulsive_edge_subsampling((4, 4), 5, 2, None, False).cpu().numpy()[2:, ::2, ::2].all(), "the default: 2 an axis"
    a = S.repulsive_edge_subsampling((33, 35), 8, 2, [2, 2], True, seed=7)
    assert torch.equal(a, S.repulsive_edge_subsampling((33, 35), 8, 2, [2, 2], True, seed=7)), "a fixed seed repeats"
    assert not torch.equal(a, S.repulsive_edge_subsampling((33, 35), 8, 2, [2, 2], True, seed=8))
    assert bool(a[:2].all()) and 0 < int(a[2:].sum()) < a[2:].numel(), "attractive channels whole, repulsive ones thinned"
    np.random.seed(3)
    b = S.repulsive_edge_subsampling((33, 35), 8, 2, [2, 2], True)
    np.random.seed(3)
    assert torch.equal(b, S.repulsive_edge_subsampling((33, 35), 8, 2, [2, 2], True)), "no seed: numpy's global state pins it"
    # 64^3 draws of one repulsive channel at p = 1/8: the kept count is binomial, sd = sqrt(n p (1 - p)) = 169.3; six
    # standard deviations (a chance of 2e-9 for an honest generator)
    big = S.repulsive_edge_subsampling((64, 64, 64), 4, 3, [2, 2, 2], True, seed=11)
    n, p = 64 ** 3, 1.0 / 8
    kept = int(big[3].sum())
    print(f"MWS subsampling: kept {kept} of {n}, expected {n * p:.0f}, bound {6 * np.sqrt(n * p * (1 - p)):.0f}")
    assert bool(big[:3].all()) and abs(kept - n * p) <= 6 * np.sqrt(n * p * (1 - p))
    with pytest.raises(TypeError, match="seed must be an integer"):
        S.repulsive_edge_subsampling((4, 4), 5, 2, None, True, seed=1.5)
    with pytest.raises(ValueError, match="strides"):
        S.repulsive_edge_subsampling((4, 4), 5, 2, [2, 2, 2])


# ---- the public function ------------------------------------------------------------------------------------------------
OFFS_SEG = {2: [[-1, 0], [0, -1], [-3, 0], [0, -3], [-6, -6], [-6, 6]],
            3: [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -4, 0], [0, 0, -4], [-1, -4, 4]]}


@functools.lru_cache(maxsize=None)
def predictions(ndim):
    """(foreground, affinities [C, *spatial]) of a 2-D (26 x 28) or a 3-D (6 x 18 x 20) sample: a few Voronoi cells, the
    affinity of an edge 1 across two cells and 0 inside one (the convention of AffinityTransform), blurred, with a little
    noise; the foreground has a three-voxel island of its own, which a size filter of 5 removes"""
    rs = np.random.RandomState(60 + ndim)
    shape = (26, 28) if ndim == 2 else (6, 18, 20)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    pts = rs.rand(5, ndim) * np.array(shape)
    cells = np.argmin(((grid[..., None, :] - pts) ** 2).sum(-1), -1) + 1
    offs = OFFS_SEG[ndim]
    aff = np.zeros((len(offs),) + shape, np.float32)
    for c, o in enumerate(offs):
        shifted = np.full(shape, -1)
        src = tuple(slice(max(-d, 0), s - max(d, 0)) for d, s in zip(o, shape))
        dst = tuple(slice(max(d, 0), s - max(-d, 0)) for d, s in zip(o, shape))
        shifted[src] = cells[dst]
        aff[c] = (shifted != cells) & (shifted >= 0)
    aff = np.stack([gaussian_filter(a, 0.7) for a in aff]) + 0.1 * rs.rand(*aff.shape)
    fg = np.full(shape, 0.9, np.float32)
    fg[..., :5] = 0.1                                             # background on one side ...
    fg[(0,) * (ndim - 1) + (slice(0, 3),)] = 0.9                  # ... with a three-voxel island in its corner
    return fg, np.clip(aff, 0, 1).astype(np.float32)


def give(a, where):
    return a if where == "numpy" else dev(a)


def take(out, where):
    if where == "numpy":
        assert isinstance(out, np.ndarray)
        return out
    assert torch.is_tensor(out) and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("where", ["numpy", "device"])
@pytest.mark.parametrize("min_size", [0, 5])
@pytest.mark.parametrize("ndim", [2, 3])
def test_mutex_watershed_segmentation(ndim, min_size, where):
    from torch_em_amd.util import mutex_watershed as S
    fg, aff = predictions(ndim)
    offs = OFFS_SEG[ndim]
    for kw in ({"seed": 5}, {"randomize_strides": False}, {"seed": 6, "strides": [1, 2, 3][:ndim], "threshold": 0.5}):
        sub = {k: v for k, v in kw.items() if k != "threshold"}
        ev = S.repulsive_edge_subsampling(fg.shape, len(offs), ndim, sub.pop("strides", None), sub.pop("randomize_strides", True),
                                          sub.pop("seed", None), batch=1)[0].cpu().numpy()
        want = M.np_mutex_watershed_segmentation(fg, aff, offs, ev, min_size, 0.5)
        got = take(S.mutex_watershed_segmentation(give(fg, where), give(aff, where), offs, min_size, **kw), where)
        assert got.dtype == np.int32 and got.shape == fg.shape and np.array_equal(got, want), kw
        assert want.max() >= 2 and (want[fg < 0.5] == 0).all()
        again = take(S.mutex_watershed_segmentation(give(fg, where), give(aff, where), offs, min_size, **kw), where)
        assert np.array_equal(again, got), "the same seed, the same result"
        if min_size:
            assert want.max() < M.np_mutex_watershed_segmentation(fg, aff, offs, ev, 0, 0.5).max(), "the filter removes the island"


def test_mutex_watershed_segmentation_batch_and_errors():
    from torch_em_amd.util import mutex_watershed as S
    fg, aff = predictions(3)
    offs = OFFS_SEG[3]
    fg2, aff2 = np.stack([fg, fg[::-1].copy()])[:, None], np.stack([aff, aff[:, ::-1].copy()])
    ev = S.repulsive_edge_subsampling(fg.shape, len(offs), 3, None, True, 9, batch=2).cpu().numpy()
    got = S.mutex_watershed_segmentation(dev(fg2), dev(aff2), offs, 5, seed=9)
    assert tuple(got.shape) == fg2.shape and got.dtype == torch.int32
    for n in range(2):
        assert np.array_equal(got[n, 0].cpu().numpy(), M.np_mutex_watershed_segmentation(fg2[n, 0], aff2[n], offs, ev[n], 5)), n
    with pytest.raises(ValueError, match="do not match the foreground"):
        S.mutex_watershed_segmentation(fg, aff[:, :, :-1], offs)
    with pytest.raises(ValueError, match="do not match the foreground"):
        S.mutex_watershed_segmentation(fg2, aff, offs)
    with pytest.raises(ValueError, match="offsets do not match"):
        S.mutex_watershed_segmentation(fg, aff, offs[:-1])
    with pytest.raises(ValueError, match="at most 32"):
        S.mutex_watershed_segmentation(fg, np.zeros((33,) + fg.shape, np.float32), [[0, 0, -1]] * 33)
    with pytest.raises(ValueError, match="entries each"):
        S.mutex_watershed_segmentation(fg, aff, [o[:2] for o in offs])
