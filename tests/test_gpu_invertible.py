"""GPU: invertible augmentations -- the per-sample dihedral transform (csrc/invaug.hip, `ops.dihedral`) bit for bit against
the numpy index-map oracle (tests/invaug_ref.py, pinned to torch.flip / rot90 by tests/test_invertible_cpu.py), its autograd,
the augmenters of transform/invertible_augmentations.py, the loss classes that take predictions, and the three trainers against
runs of the REFERENCE's trainers (tests/golden/g19_invertible.npz, tests/golden/gen_golden_invertible.py; the data is G17's).

A permutation leaves no room: every comparison of the kernel is on raw bit patterns.  No test provokes a device fault:
outputs the test lays out sit between guard zones that must survive, and every extent is that of a dense tensor the test
allocated.
"""
import json
import os

import numpy as np
import pytest
import torch

import invaug_ref as ref
from conftest import GOLDEN
from test_raw_aug_cpu import gauss_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {1: torch.uint8, 2: torch.bfloat16, 4: torch.float32}
GUARD = 64   # elements around an output the test lays out (a multiple of 16 bytes in every type)
SQUARES = (1, 5, 31, 32, 33, 65, 66, 132)   # 66 and 132: one past the packed tiles of 2- and 1-byte elements (64 and 128 a side)
# N = 3 with mixed codes; together they hold every code, and the first has 3 and 5 in one call
MIXED = ((3, 5, 0), (1, 2, 7), (4, 6, 3), (6, 1, 5))


def _run(x, codes, **kw):
    from torch_em_amd import ops
    return ops.dihedral(x.to(DEV), codes, **kw)


def _same(got, x, codes):
    want = ref.dihedral_np(ref.bits(x), codes)
    g = ref.bits(got)
    return g.shape == want.shape and np.array_equal(g, want)


def _same_bits(a, b):
    """two device tensors hold the same bit patterns (torch.equal would call a NaN unequal to itself)"""
    as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


@pytest.fixture(scope="module")
def paths_seen():
    return set()


# ---- kernel and op ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eb", (1, 2, 4))
@pytest.mark.parametrize("side", SQUARES)
def test_every_code_equals_the_oracle(eb, side, paths_seen):
    """every code 0..7 uniformly, then N = 3 with mixed codes, planes 1 and 3"""
    from torch_em_amd import ops
    for planes in (1, 3):
        x = ref.patterned((3, planes, side, side), DTYPES[eb], seed=side + planes)
        xd = x.to(DEV)
        for code in range(8):
            assert _same(ops.dihedral(xd, [code] * 3), x, [code] * 3), (planes, code)
            paths_seen.add(ops.dihedral_path(xd, code))
        for codes in MIXED:
            got = ops.dihedral(xd, codes)
            assert _same(got, x, codes), (planes, codes)
            assert _same_bits(ops.dihedral(got, codes, inverse=True), xd), (planes, codes)
        assert torch.equal(xd.cpu().view(torch.uint8), x.view(torch.uint8)), "the input must not be modified"


def test_codes_given_as_a_cpu_tensor_and_bool_elements():
    x = ref.patterned((3, 2, 7, 7), torch.bool, seed=3)
    got = _run(x, torch.tensor([3, 5, 6]))
    assert got.dtype == torch.bool and _same(got, x, [3, 5, 6])
    x16 = ref.patterned((3, 2, 7, 7), torch.float16, seed=4)
    assert _same(_run(x16, torch.tensor([7, 0, 2], dtype=torch.int32)), x16, [7, 0, 2])


@pytest.mark.parametrize("eb", (1, 2, 4))
def test_five_axes_and_permuted_input(eb):
    """[N, C, D, H, W]: depth folds into the planes; a non-contiguous input is made contiguous first"""
    x = ref.patterned((2, 2, 3, 33, 33), DTYPES[eb], seed=eb)
    for codes in ((3, 6), (5, 5), (2, 4)):
        assert _same(_run(x, codes), x, codes), codes
    xt = x.to(DEV).transpose(-1, -2)
    assert not xt.is_contiguous() and _same(_run(xt, (1, 4)), xt.contiguous(), (1, 4))


@pytest.mark.parametrize("eb", (1, 2, 4))
@pytest.mark.parametrize("plane", ((4, 6), (33, 70), (7, 3), (32, 64), (16, 48), (68, 136)))
def test_non_square(eb, plane, paths_seen):
    """mixed non-transposing codes, and one uniform transposing code (the output is W x H)"""
    from torch_em_amd import ops
    x = ref.patterned((3, 2) + plane, DTYPES[eb], seed=plane[1])
    xd = x.to(DEV)
    for codes in ((0, 2, 4), (6, 4, 2), (6, 6, 0)):
        assert _same(ops.dihedral(xd, codes), x, codes), codes
        paths_seen.update(ops.dihedral_path(xd, c) for c in codes)
    for code in (1, 3, 5, 7):
        got = ops.dihedral(xd, [code] * 3)
        paths_seen.add(ops.dihedral_path(xd, code, out=got))
        assert tuple(got.shape) == (3, 2, plane[1], plane[0]) and _same(got, x, [code] * 3), code
        back = ops.dihedral(got, [code] * 3, inverse=True)
        assert _same_bits(back, xd), code
    with pytest.raises(ValueError, match="mix transposing"):
        ops.dihedral(xd, (0, 3, 0))


@pytest.mark.parametrize("eb", (1, 2, 4))
def test_offset_bases_guard_bands_and_paths(eb, paths_seen):
    """src and / or dst one element off a 16-byte boundary: rows of 16-byte multiples then stream element by element (asserted
    through the path query); the output sits between poisoned guard zones that must survive"""
    from torch_em_amd import ops
    dtype = DTYPES[eb]
    shape = (3, 2, 32, 32)
    n = int(np.prod(shape))
    x = ref.patterned(shape, dtype, seed=11 + eb)
    poison = 0xA5 if eb == 1 else -7.0
    for sshift in (0, 1):
        sbuf = torch.empty(n + 1, dtype=dtype, device=DEV)
        xd = sbuf[sshift:sshift + n].view(shape)
        xd.copy_(x)
        for dshift in (0, 1):
            raw = torch.full((n + 2 * GUARD + dshift,), poison, dtype=dtype, device=DEV)
            out = raw[GUARD + dshift:GUARD + dshift + n].view(shape)
            aligned = xd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            assert aligned == (sshift == 0 and dshift == 0)
            for codes in ((0, 6, 2), (3, 4, 5), (1, 7, 6)):
                raw.fill_(poison)
                res = ops.dihedral(xd, codes, out=out)
                assert res is out and _same(out, x, codes), (sshift, dshift, codes)
                lo, hi = raw[:GUARD + dshift], raw[GUARD + dshift + n:]
                assert hi.numel() == GUARD and bool((lo == poison).all()) and bool((hi == poison).all()), (sshift, dshift, codes)
                packed = eb < 4 and xd.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0      # H = W = 32: rows are dword multiples
                assert packed == (eb < 4 and sshift == 0 and dshift == 0)
                for c in codes:
                    path = ops.dihedral_path(xd, c, out=out)
                    tile = ops.DH_PATH_TILE_PACKED if packed else ops.DH_PATH_TILE
                    assert path == (tile if c & 1 else ops.DH_PATH_VEC if aligned else ops.DH_PATH_SCALAR)
                    paths_seen.add(path)
    with pytest.raises(ValueError, match="overlap"):
        ops.dihedral(xd, (0, 0, 0), out=xd)
    with pytest.raises(ValueError, match="contiguous tensor of the output's shape"):
        ops.dihedral(xd, (1, 1, 1), out=torch.empty(n + 1, dtype=dtype, device=DEV))


def test_every_path_was_reached(paths_seen):
    """vector stream, scalar stream, tile and packed tile: what the path query says for each, and a launch on each"""
    from torch_em_amd import ops
    x = torch.zeros(1, 1, 8, 8, device=DEV)
    # rows of 32 bytes on an aligned base: vector; rows of 20 bytes: scalar; an odd code: tile
    assert ops.dihedral_path(x, 6) == ops.DH_PATH_VEC and ops.dihedral_path(x[..., :5].contiguous(), 6) == ops.DH_PATH_SCALAR
    assert ops.dihedral_path(x, 3) == ops.DH_PATH_TILE
    # narrow elements: packed tiles when H, W and the bases are dword multiples, one element per LDS dword otherwise
    assert ops.dihedral_path(x.bfloat16(), 3) == ops.DH_PATH_TILE_PACKED and ops.dihedral_path(x.bool(), 5) == ops.DH_PATH_TILE_PACKED
    assert ops.dihedral_path(x[..., :6, :6].bfloat16().contiguous(), 3) == ops.DH_PATH_TILE_PACKED
    assert ops.dihedral_path(x[..., :7, :7].bfloat16().contiguous(), 3) == ops.DH_PATH_TILE
    assert ops.dihedral_path(x[..., :6, :6].bool().contiguous(), 3) == ops.DH_PATH_TILE
    # one launch per path here, so that this test stands alone; in a run of the whole file the tests above reached them all too
    every = {ops.DH_PATH_VEC, ops.DH_PATH_SCALAR, ops.DH_PATH_TILE, ops.DH_PATH_TILE_PACKED}
    own = set()
    for shape, dtype, code in (((2, 1, 8, 8), torch.float32, 6), ((2, 1, 8, 5), torch.float32, 6), ((2, 1, 8, 8), torch.float32, 3),
                               ((2, 1, 8, 8), torch.bfloat16, 3)):
        t = ref.patterned(shape, dtype, seed=code)
        own.add(ops.dihedral_path(t.to(DEV), code))
        assert _same(ops.dihedral(t.to(DEV), [code] * 2), t, [code] * 2), (shape, dtype, code)
    assert own == every and paths_seen <= every, (own, paths_seen)


def test_more_blocks_than_one_round_and_many_samples():
    """a sample larger than its share of the capped grid (the loops run more than once), and more samples than the cap"""
    x = ref.patterned((2, 20, 352, 352), torch.float32, seed=5)   # 2420 units of 4 KiB per sample on 1024 blocks per sample
    for codes in ((3, 6), (4, 5)):
        assert _same(_run(x, codes), x, codes), codes
    big = ref.patterned((1, 40, 352, 352), torch.float32, seed=6)   # 4840 units on 2048 blocks
    for code in (2, 7):
        assert _same(_run(big, [code]), big, [code]), code
    many = ref.patterned((2100, 1, 4, 4), torch.bfloat16, seed=7)    # one block per sample
    codes = [int(c) for c in np.random.default_rng(0).integers(0, 8, 2100)]
    assert _same(_run(many, codes), many, codes)


def test_offsets_beyond_2_31():
    """Indices past 2^31, compared on the device against torch.flip / rot90 (which tests/test_invertible_cpu.py pins to the
    oracle): three samples of 27000^2 bytes, so the third starts beyond 2^31 elements; then ONE sample of more than 2^31
    elements, whose rows are no multiple of 16 bytes -- the stream's 64-bit index arithmetic -- and the tile path over it."""
    side = 27000
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randint(0, 256, (3, 1, side, side), dtype=torch.uint8, device=DEV, generator=g)
    assert x.numel() > 2 ** 31
    got = _run(x, (5, 6, 3))
    for n, k in enumerate((1, 2, -1)):
        assert torch.equal(got[n], torch.rot90(x[n], k, (-2, -1))), n
    del x, got
    H, W = 46350, 46344
    x = torch.randint(0, 256, (1, 1, H, W), dtype=torch.uint8, device=DEV, generator=g)
    assert x.numel() > 2 ** 31 and W % 16
    assert torch.equal(_run(x, [6]), x.flip(-1, -2))
    assert torch.equal(_run(x, [2]), x.flip(-2))
    assert torch.equal(_run(x, [3]), torch.rot90(x, -1, (-2, -1)))


def test_gradient_is_the_inverse_permutation_and_runs_repeat():
    from torch_em_amd import ops
    codes = (3, 5, 6, 1)
    x = ref.patterned((4, 2, 33, 33), torch.float32, seed=21).to(DEV)
    w = torch.randn(4, 2, 33, 33, device=DEV)
    xg = torch.randn_like(x).requires_grad_(True)
    y = ops.dihedral(xg, codes)
    assert y.requires_grad
    (y * w).sum().backward()
    assert torch.equal(xg.grad.view(torch.int32), ops.dihedral(w, codes, inverse=True).view(torch.int32))
    assert torch.equal(ops.dihedral(w, codes, inverse=True), ops.dihedral(w, ops.dihedral_inverse(codes)))
    a, b = ops.dihedral(x, codes), ops.dihedral(x, codes)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs must give the same bits"
    with torch.no_grad():
        assert not ops.dihedral(xg, codes).requires_grad


def test_refusals_on_the_device():
    from torch_em_amd import _lib, ops
    x = torch.zeros(2, 1, 4, 4, device=DEV)
    lib = _lib.load()
    c = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib.tem_dihedral2d(ops._p(x), ops._p(x), ops._p(c), 2, 1, 4, 4, 4, None) == -1 and b"in-place" in lib.tem_last_error()
    with pytest.raises(ValueError, match="0..7"):
        ops.dihedral(x, (0, 8))
    with pytest.raises(ValueError, match="one code per sample"):
        ops.dihedral(x, (0,))
    with pytest.raises(ValueError, match="1, 2 or 4 bytes"):
        ops.dihedral(x.double(), (0, 0))


# ---- augmenters -------------------------------------------------------------------------------------------------------
def _count_dihedral(monkeypatch):
    from torch_em_amd import ops
    calls = []
    real = ops.dihedral

    def counted(x, codes, *a, **kw):
        calls.append(list(codes))
        return real(x, codes, *a, **kw)
    monkeypatch.setattr(ops, "dihedral", counted)
    return calls


@pytest.mark.parametrize("ndim", (2, 3))
def test_reverse_of_transform_is_the_identity_in_one_launch_each(ndim, monkeypatch):
    from torch_em_amd.transform import invertible_augmentations as ia
    calls = _count_dihedral(monkeypatch)
    torch.manual_seed(5)
    aug = ia.InvertibleAugmenter(*ia.get_default_augmentations("weak", ndim=ndim, p=0.75))
    shape = (6, 2, 24, 24) if ndim == 2 else (6, 2, 3, 24, 24)
    x = torch.randn(shape, device=DEV)
    seen = set()
    for _ in range(4):
        aug.reset()
        del calls[:]
        y = aug.transform(x)
        assert len(calls) == 1, "the geometric chain is ONE launch"
        pred = torch.randn((6, 1) + shape[2:], device=DEV)   # what comes back has another channel count
        z = aug.reverse_transform(y)
        assert len(calls) == 2 and torch.equal(z, x)
        mask = pred > 0
        fwd = ia.ops.dihedral(mask, calls[0])
        assert torch.equal(aug.reverse_transform(fwd), mask), "bool filters invert too"
        want = ref.dihedral_np(ref.bits(x), calls[0])
        assert np.array_equal(ref.bits(y), want)
        seen.update(calls[0])
    assert len(seen) >= 4 and any(c & 1 for c in seen), seen   # 24 draws at p = 0.75
    # replay: the recorded parameters give the same view
    params = aug.params
    assert torch.equal(aug.transform(x, params=params), y)


def test_clip_max_and_non_square_refusal():
    from torch_em_amd.transform import invertible_augmentations as ia
    torch.manual_seed(1)
    aug = ia.InvertibleAugmenter(*ia.get_default_augmentations("weak", ndim=2, p=0.0), clip_max=0.5)
    x = torch.randn(3, 1, 16, 16, device=DEV)
    y = aug.transform(x)
    assert torch.equal(y, x.clamp(0.0, 0.5)) and float(y.max()) == 0.5 and float(y.min()) == 0.0
    rot = ia.AugmentationSequential(ia.RandomRotation90(times=(1, 1), p=1.0))
    with pytest.raises(ValueError, match=r"times=\(0, 0\)"):
        rot(torch.zeros(2, 1, 8, 12, device=DEV))
    half = ia.AugmentationSequential(ia.RandomRotation90(times=(2, 2), p=1.0))
    z = torch.randn(2, 1, 8, 12, device=DEV)
    assert torch.equal(half(z), torch.rot90(z, 2, (-2, -1))) and torch.equal(half.inverse(half(z)), z)


def _blur_oracle(x, wy, wx):
    """float64 sum over the ky x kx taps, reflect border without edge repeat; x [..., H, W]"""
    H, W = x.shape[-2:]
    out = np.zeros(x.shape)
    refl = lambda i, n: np.where(np.abs(i) >= n, 2 * (n - 1) - np.abs(i), np.abs(i))   # noqa: E731
    for a in range(len(wy)):
        ya = refl(np.arange(H) + a - len(wy) // 2, H)
        for b in range(len(wx)):
            xb = refl(np.arange(W) + b - len(wx) // 2, W)
            out += float(wy[a]) * float(wx[b]) * x.astype(np.float64)[..., ya[:, None], xb[None, :]]
    return out


@pytest.mark.parametrize("shape", ((5, 2, 33, 40), (4, 1, 3, 17, 19)))
def test_blur_against_float64_and_losers_keep_their_bits(shape):
    """per-sample coin flip and sigma; the bound is the one tests/test_gpu_raw_aug.py derives for `ops.blur2d`:
    (ky + kx + 2) roundings of 2^-24 max|x| with weights that sum to `scale`"""
    from torch_em_amd.transform import invertible_augmentations as ia
    torch.manual_seed(2)
    blur = ia.RandomGaussianBlur(kernel_size=(3, 5), sigma=(0.1, 1.0), p=0.5)
    x = ref.patterned(shape, torch.float32, seed=31).nan_to_num(0.0, 1.0, -1.0).clamp(-4, 4)
    x[0].view(-1)[:3] = torch.tensor([-0.0, 1e-42, -1e-42])
    params = {"batch_prob": torch.tensor([True, False, True, False, True][:shape[0]]), "sigma": torch.tensor([0.1, 0.5, 1.0, 0.7, 0.37][:shape[0]],
                                                                                                           dtype=torch.float64)}
    got = blur(x.to(DEV), params=params).cpu()
    assert blur._params is params
    for n in range(shape[0]):
        if not bool(params["batch_prob"][n]):
            assert np.array_equal(ref.bits(got[n]), ref.bits(x[n])), n
            continue
        s = float(params["sigma"][n])
        wy, wx = np.float32(ia._gauss_taps(3, s)), np.float32(ia._gauss_taps(5, s))
        scale = float(wy.astype(np.float64).sum() * wx.astype(np.float64).sum())
        err = np.abs(got[n].numpy().astype(np.float64) - _blur_oracle(x[n].numpy(), wy, wx)).max()
        assert err <= (3 + 5 + 2) * 2.0 ** -24 * float(x[n].abs().max()) * scale, (n, err)
    drawn = blur(x.to(DEV))   # its own draw: per-sample decisions from torch's CPU generator
    assert drawn.shape == x.shape and set(blur._params) == {"batch_prob", "sigma"}
    assert bool(((blur._params["sigma"] >= 0.1) & (blur._params["sigma"] <= 1.0)).all())


@pytest.mark.parametrize("shape", ((5, 2, 33, 40), (4, 1, 3, 17, 19)))
def test_noise_against_float64_and_losers_keep_their_bits(shape):
    """x + fl32(std z) on the samples that won, z from row k of the stream for the k-th winner; bound:
    test_raw_aug_cpu.gauss_bound, as tests/test_gpu_raw_aug.py uses it for `ops.gauss_noise`"""
    from torch_em_amd.transform import invertible_augmentations as ia
    from torch_em_amd.transform._philox import field_words, normal_from_words
    noise = ia.RandomGaussianNoise(mean=0.0, std=0.1, p=0.5)
    x = ref.patterned(shape, torch.float32, seed=41).nan_to_num(0.0, 1.0, -1.0).clamp(-4, 4)
    x[1].view(-1)[:3] = torch.tensor([-0.0, 1e-42, -1e-42])
    prob = torch.tensor([True, False, False, True, True][:shape[0]])
    seed = 0x123456789
    got = noise(x.to(DEV), params={"batch_prob": prob, "seed": seed}).cpu()
    win = [n for n in range(shape[0]) if bool(prob[n])]
    L = x[0].numel()
    rows, i = np.meshgrid(np.arange(len(win)), np.arange(L), indexing="ij")
    w0, w1 = field_words(seed, rows, i)(0)
    z = normal_from_words(w0, w1, np.float64).reshape(len(win), L)
    std = float(np.float32(0.1))
    for k, n in enumerate(win):
        xn = x[n].numpy().reshape(-1)
        err = np.abs(got[n].numpy().reshape(-1).astype(np.float64) - (xn + std * z[k]))
        assert np.all(err <= gauss_bound(xn, std, z[k])), n
    for n in set(range(shape[0])) - set(win):
        assert np.array_equal(ref.bits(got[n]), ref.bits(x[n])), n
    np.random.seed(3)
    torch.manual_seed(3)
    a = noise(x.to(DEV))
    np.random.seed(3)
    torch.manual_seed(3)
    assert torch.equal(a, noise(x.to(DEV))), "np.random.seed and torch.manual_seed pin a call"
    none = noise(x.to(DEV), params={"batch_prob": torch.zeros(shape[0], dtype=torch.bool), "seed": 1})
    assert np.array_equal(ref.bits(none), ref.bits(x))


def test_strong_augmenter_runs_end_to_end():
    """the default strong chain (blur, noise, flips, rotation) on a 2-D and a 3-D batch: shapes, one geometric launch, and the
    inverse of the geometric part applied to the augmented view is the clipped intensity view"""
    from torch_em_amd.transform import invertible_augmentations as ia
    torch.manual_seed(0)
    np.random.seed(0)
    for ndim, shape in ((2, (4, 1, 32, 32)), (3, (4, 1, 4, 32, 32))):
        augs = ia.UniMatchv2Augmenters(ndim=ndim, clip_max=1.0)
        x = torch.rand(shape, device=DEV)
        augs.reset_all()
        views = [a.transform(x) for a in (augs.weak, augs.strong1, augs.strong2)]
        assert all(v.shape == x.shape for v in views)
        assert torch.equal(augs.weak.reverse_transform(views[0]), x)
        back = augs.strong1.reverse_transform(views[1])
        assert float(back.min()) >= 0.0 and float(back.max()) <= 1.0 and float((back - x).abs().max()) < 1.0
        augs.reset_all()
        assert augs.weak.params is None and augs.strong2.params is None


# ---- losses -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_selftrain.npz")))


@pytest.fixture(scope="module")
def g19():
    return dict(np.load(os.path.join(GOLDEN, "g19_invertible.npz")))


def test_loss_classes_against_the_reference(g19):
    """The reference's four loss classes called directly (gen_golden_invertible.py: `loss_*`), both `pred_dim`, with and
    without filter.  Margin: 2e-5 on the score, the project's first-step margin -- a float32 Dice over 256 elements per channel
    rounds 256 times at 2^-24 at most (1.5e-5), in the reference and here."""
    from torch_em_amd import self_training as st
    pred, labels, filt = (torch.from_numpy(g19[k]).to(DEV) for k in ("loss_pred", "loss_labels", "loss_filter"))
    cases = json.loads(str(g19["loss_index"]))
    assert len(cases) == 12
    for case in cases:
        fn = getattr(st, case["cls"])()
        p = pred if case["pred_dim"] == 2 else pred[0]
        kw = {} if case["pred_dim"] is None else {"pred_dim": case["pred_dim"]}
        for grad in (False, True):      # under no_grad loss and metric come from one pass; with grad from two
            with torch.set_grad_enabled(grad):
                q = p.clone().requires_grad_(grad)
                got = fn(q, labels, filt if case["filter"] else None, **kw)
            got = [float(v) for v in got] if isinstance(got, tuple) else [float(got)]
            assert len(got) == len(case["value"])
            for a, b in zip(got, case["value"]):
                assert abs(a - b) <= 2e-5 * (2.0 - b), (case, grad, got)      # two channels: score = 2 - loss
    with pytest.raises(AssertionError, match="pred_dim"):
        st.UniMatchv2Loss()(pred, labels, None, pred_dim=3)
    with pytest.raises(AssertionError, match="len 2"):
        st.UniMatchv2LossAndMetric()(torch.cat([pred, pred[:1]]), labels, None, pred_dim=2)
    # a bool filter (the one-sided labeler's) and the gradient through the mask
    q = pred[0].clone().requires_grad_(True)
    loss = st.SelfTrainingLossWithInvertibleAugmentations()(q, labels, filt.bool())
    loss.backward()
    assert abs(float(loss) - [c for c in cases if c["cls"].startswith("SelfTrainingLossWith") and c["filter"]][0]["value"][0]) < 4e-5
    assert float(q.grad[filt == 0].abs().max()) == 0.0 and float(q.grad.abs().max()) > 0


# ---- trainers against the reference's runs (tests/golden/g19_invertible.npz) ---------------------------------------------
SERIES = ("unsup", "sup", "combined", "val_metric", "val_loss")
C_OUT = 1.0   # DiceLoss sums 1 - score over the channels: score = C - loss


class Replay:
    """mixin of the test's augmenter: the geometric parameters of each `transform` call come from the fixture's (h, v, k)"""

    def transform(self, x):
        h, v, k = (torch.from_numpy(self.hvk[self.call, :, j].astype(np.int64)) for j in range(3))
        self.call += 1
        params = [{"batch_prob": h.bool()}, {"batch_prob": v.bool()}, {"batch_prob": torch.ones_like(k, dtype=torch.bool), "times": k}]
        return super().transform(x, params=params)


def _replay_augmenters(g19, tag, call=0):
    from torch_em_amd.transform import invertible_augmentations as ia

    class ReplayAugmenter(Replay, ia.InvertibleAugmenter):
        pass
    views = [str(v) for v in g19[f"ia_{tag}_views"]]
    made = {}
    for name, hvk in zip(views, g19[f"ia_{tag}_hvk"]):
        made[name] = ReplayAugmenter(ia.AugmentationSequential(), ia.AugmentationSequential(
            ia.RandomHorizontalFlip(), ia.RandomVerticalFlip(), ia.RandomRotation90()))
        made[name].hvk, made[name].call = hvk, call
    cls = ia.UniMatchv2Augmenters if len(views) == 3 else ia.MeanTeacherAugmenters
    return cls(ndim=2, **made)


def _raw_loader(a):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(a)), batch_size=2, shuffle=False)


def _pair_loader(a, b):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(a), torch.from_numpy(b)), batch_size=2, shuffle=False)


_STATES = {}


def _states(g19, tag):
    if tag not in _STATES:
        _STATES[tag] = ref.ia_states(g19, tag)
    return _STATES[tag]


def _tensors(state):
    return {k: torch.from_numpy(v) for k, v in state.items()}


def _ia_trainer(g17, g19, tag, tmp_path, **overrides):
    from torch_em_amd import self_training as st
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    cfg = json.loads(str(g19["ia_runs"]))[tag]
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    model.load_state_dict(_tensors(_states(g19, tag)[0]))
    log = {k: [] for k in SERIES + ("keep", "ct", "calls")}

    class Recorder:
        def __init__(self, trainer, save_root, **kw):
            pass

        def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
            log["calls"].append("unsup")
            log["unsup"].append(float(loss.detach()))
            log["keep"].append(1.0 if label_filter is None else float(label_filter.float().mean()))

        def log_train_augmentations(self, step, *tensors):
            log["calls"].append("aug%d" % len(tensors))

        def log_train_supervised(self, step, loss, x, y, pred):
            log["calls"].append("sup")
            log["sup"].append(float(loss.detach()))

        def log_combined_loss(self, step, loss):
            log["calls"].append("combined")
            log["combined"].append(float(loss.detach()))

        def log_lr(self, step, lr):
            log["calls"].append("lr")

        def log_ct(self, step, ct):
            log["calls"].append("ct")
            log["ct"].append(float(ct))

        def log_validation_unsupervised(self, step, metric, loss, x1, x2, pred, pseudo_labels, label_filter=None):
            log["val_metric"].append(metric)
            log["val_loss"].append(loss)

        def log_validation_augmentations(self, step, *tensors):
            log["calls"].append("valaug%d" % len(tensors))

        def log_validation_supervised(self, step, metric, loss, x, y, pred):
            log["val_metric"].append(metric)
            log["val_loss"].append(loss)

    uni = cfg["trainer"] == "uni_match"
    loss_cls, lam_cls = (st.UniMatchv2Loss, st.UniMatchv2LossAndMetric) if uni else \
        (st.SelfTrainingLossWithInvertibleAugmentations, st.SelfTrainingLossAndMetricWithInvertibleAugmentations)
    if cfg["semi"]:
        kw = dict(supervised_train_loader=_pair_loader(g17["mt_xs"], g17["mt_ys"]), supervised_val_loader=_pair_loader(g17["mt_xsv"], g17["mt_ysv"]),
                  supervised_loss=st.SelfTrainingLossWithInvertibleAugmentations(),
                  supervised_loss_and_metric=st.SelfTrainingLossAndMetricWithInvertibleAugmentations())
    else:
        kw = dict(unsupervised_val_loader=_raw_loader(g17["mt_xv1"]), unsupervised_loss_and_metric=lam_cls())
    if cfg["trainer"] == "fix_match":
        kw["source_distribution"] = cfg["source"]
    else:
        kw["momentum"] = cfg["momentum"]
    if uni:
        kw["complementary_dropout"] = False
    kw.update(dict(name="g19" + tag, model=model, optimizer=FusedAdamW(model.parameters(), lr=float(g19["ia_lr"])),
                   pseudo_labeler=st.DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]), unsupervised_loss=loss_cls(),
                   unsupervised_train_loader=_raw_loader(g17["mt_xu1"]), augmenter=_replay_augmenters(g19, tag), logger=Recorder,
                   mixed_precision=False, device=DEV, save_root=str(tmp_path)))
    kw.update(overrides)
    cls = {"mean_teacher": st.MeanTeacherTrainerWithInvertibleAugmentations, "fix_match": st.FixMatchTrainerWithInvertibleAugmentations,
           "uni_match": st.UniMatchv2Trainer}[cfg["trainer"]]
    trainer = cls(**kw)
    if hasattr(trainer, "teacher") and f"ia_{tag}_teacher0" in g19:
        assert trainer.reinit_teacher == cfg["semi"]
        trainer.teacher.load_state_dict(_tensors(ref._unflatten(g19, g19[f"ia_{tag}_teacher0"].view(np.int32))))
    return trainer, log, cfg


def test_fixture_guards(g19):
    """what the margins below rest on, re-read from the fixture: codes 3 and 5 in every run, a batch with two different codes,
    views that differ in every batch, losses above 0.02, keep shares inside (0.05, 0.95)"""
    for tag, cfg in json.loads(str(g19["ia_runs"])).items():
        codes = g19[f"ia_{tag}_codes"]
        hvk = g19[f"ia_{tag}_hvk"]
        assert codes.shape[1:] == (8, 2) and hvk.shape == codes.shape + (3,)
        from torch_em_amd import ops
        assert ops.dihedral_codes(hvk[..., 0].ravel().tolist(), hvk[..., 1].ravel().tolist(), hvk[..., 2].ravel().tolist()) == codes.ravel().tolist()
        train = codes[:, :6]
        assert 3 in train and 5 in train and (train[..., 0] != train[..., 1]).any()
        for a in range(len(codes)):
            for b in range(a + 1, len(codes)):
                assert all(not np.array_equal(codes[a, c], codes[b, c]) for c in range(8)), (tag, a, b)
        for k in ("unsup", "sup", "combined"):
            assert all(v > 0.02 for v in g19[f"ia_{tag}_{k}"])
        if cfg["threshold"] is not None:
            assert all(0.05 < v < 0.95 for v in g19[f"ia_{tag}_keep"])
    assert float(g19["ia_guard"]) == 1e-5


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_every_step_replays_the_reference(g17, g19, tag, tmp_path):
    """At the states the reference had in iteration i -- student, and teacher where there is one -- views, labels, filter,
    inversion and loss on batch i give the losses the reference logged: score within 2e-5 relative (the project's first-step
    margin; the generator's guard of 1e-5 around the thresholds makes it valid at every step), keep share the same voxel count
    out of 2048.  Run (d) takes two optimizer steps per iteration: its unsupervised half is replayed at the state after the
    supervised step."""
    trainer, _, cfg = _ia_trainer(g17, g19, tag, tmp_path, logger=None)
    states = _states(g19, tag)
    uni = cfg["trainer"] == "uni_match"
    steps = 2 if (uni and cfg["semi"]) else 1
    assert len(states) == 6 * steps + 1
    model = trainer.model.to(DEV)
    model.train()
    teachers = None
    if hasattr(trainer, "teacher"):
        teachers = ref.ia_teachers(g19, tag, [states[steps * (i + 1)] for i in range(6)], cfg["momentum"], cfg["semi"])
        trainer.teacher.to(DEV)
        assert trainer.teacher.training == (not uni)
    xu, xs, ys = (torch.from_numpy(g17[k]).to(DEV) for k in ("mt_xu1", "mt_xs", "mt_ys"))
    for i in range(6):
        b = slice(2 * i, 2 * i + 2)
        trainer.augmenter = _replay_augmenters(g19, tag, call=i)
        model.load_state_dict(_tensors(states[steps * i]))
        if teachers is not None:
            trainer.teacher.load_state_dict(teachers[i])
        if cfg["semi"]:
            with torch.no_grad():
                sup = float(trainer.supervised_loss(model(xs[b]), ys[b]))
            want_sup = float(g19[f"ia_{tag}_sup"][i])
            assert abs(sup - want_sup) < 2e-5 * (C_OUT - want_sup), (i, sup, want_sup)
        model.load_state_dict(_tensors(states[steps * i + steps - 1]))
        with torch.no_grad():
            if uni:
                x, x_w, x_s1, x_s2 = trainer._three_views(xu[b])
                labels, label_filter, labels_inv, filter_inv = trainer._inverted_labels(x_w, train=True)
                _, _, stack = trainer._student(x_s1, x_s2)
                unsup = float(trainer.unsupervised_loss(stack, labels_inv, filter_inv, pred_dim=2))
            else:
                x, x1, x2 = trainer._two_views(xu[b])
                labels, label_filter, labels_inv, filter_inv = trainer._inverted_labels(x1, train=True)
                unsup = float(trainer.unsupervised_loss(trainer.augmenter.student.reverse_transform(model(x2)), labels_inv, filter_inv))
        assert torch.equal(x, xu[b]) and labels_inv.shape == (2, 1, 32, 32)
        keep = 1.0 if filter_inv is None else float(filter_inv.float().mean())
        want = float(g19[f"ia_{tag}_unsup"][i])
        dev = abs((C_OUT - unsup) - (C_OUT - want)) / (C_OUT - want)
        print(f"INVERTIBLE_STEP run {tag} step {i}: unsup {unsup:.7f} reference {want:.7f} score dev {dev:.2e} keep {keep:.6f} "
              f"reference {float(g19[f'ia_{tag}_keep'][i]):.6f}")
        assert dev < 2e-5, (tag, i, unsup, want)
        assert abs(keep - float(g19[f"ia_{tag}_keep"][i])) < 0.5 / 2048, (tag, i, keep)
        if cfg["trainer"] != "uni_match" and cfg["semi"]:
            want_comb = float(g19[f"ia_{tag}_combined"][i])
            assert abs((sup + unsup) / 2 - want_comb) < 2e-5 * (C_OUT - want_comb), (i, sup, unsup, want_comb)


CALLS = {"a": ["unsup", "aug4", "lr", "ct"], "b": ["sup", "unsup", "aug4", "combined", "lr", "ct"], "c": ["unsup", "aug6", "lr"],
         "d": ["sup", "unsup", "aug6", "lr", "ct"]}


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_whole_trajectory(g17, g19, tag, tmp_path):
    """Six iterations and the validation against the reference's run: every series within max(5e-3, 2 x the fixture's
    scatter) on the score, the final parameters within G18's 0.15, the reference's checkpoint keys and logger calls.
    Run (c): the reference's unsupervised UniMatch loop never clears the gradients (uni_match_v2.py says so); to follow ITS
    trajectory the test switches this trainer's `zero_grad` off."""
    trainer, log, cfg = _ia_trainer(g17, g19, tag, tmp_path)
    if tag == "c":
        trainer.optimizer.zero_grad = lambda *a, **k: None
    trainer.fit(iterations=6)
    assert trainer.iteration == 6
    for k in SERIES:
        want = g19[f"ia_{tag}_{k}"]
        assert len(log[k]) == len(want), (k, len(log[k]))
        if not len(want):
            continue
        tol = max(5e-3, 2 * float(g19[f"ia_{tag}_scatter_{k}"]))      # two draws from the reference's own scatter
        got_score, want_score = C_OUT - np.array(log[k]), C_OUT - want
        dev = float(np.max(np.abs(got_score - want_score) / np.abs(want_score)))
        print(f"INVERTIBLE_RUN run {tag} {k}: {[round(float(v), 6) for v in log[k]]} reference {[round(float(v), 6) for v in want]} "
              f"worst score dev {dev:.2e} margin {tol:.1e}")
        assert dev <= tol, (tag, k, dev, tol)
    assert np.allclose(log["keep"], g19[f"ia_{tag}_keep"], atol=2e-2), (log["keep"], g19[f"ia_{tag}_keep"])
    final = _states(g19, tag)[-1]
    for k, v in trainer.model.state_dict().items():      # G18's parameter margin, the round-off-level sampler biases aside
        if "samplers" in k and k.endswith("bias"):
            continue
        a, b = v.cpu().double(), torch.from_numpy(final[k]).double()
        assert float((a - b).norm() / b.norm()) < 0.15, (tag, k)
    ckpt = torch.load(os.path.join(trainer.checkpoint_folder, "latest.pt"), weights_only=False)
    assert set(g19[f"ia_{tag}_ckpt_keys"]) <= set(ckpt), set(g19[f"ia_{tag}_ckpt_keys"]) - set(ckpt)
    assert ("teacher_state" in ckpt) == (cfg["trainer"] != "fix_match")
    assert ckpt["init"]["trainer_class"].endswith(type(trainer).__name__)
    train_calls = [c for c in log["calls"] if not c.startswith("valaug")]
    assert train_calls == CALLS[tag] * 6, train_calls
    assert [c for c in log["calls"] if c.startswith("valaug")] == ([] if cfg["semi"] else ["valaug6" if tag == "c" else "valaug4"])
    assert log["ct"] == ([] if cfg["threshold"] is None else [0.7] * 6)
    views = [getattr(trainer.augmenter, str(v)) for v in g19[f"ia_{tag}_views"]]
    assert [v.call for v in views] == [6 if cfg["semi"] else 8] * len(views) and all(v.params is not None for v in views)


def test_unimatch_runs_the_student_once_and_inverts_both_views_in_one_launch(g17, g19, tmp_path, monkeypatch):
    from torch_em_amd import ops
    trainer, log, cfg = _ia_trainer(g17, g19, "c", tmp_path, logger=None)
    forwards, launches = [], []
    trainer.model.register_forward_hook(lambda m, inp, out: forwards.append((inp[0].shape[0], torch.is_grad_enabled())))
    real = ops.dihedral

    def spy(x, codes, inverse=False, **kw):
        launches.append((list(codes), inverse, tuple(x.shape), x.requires_grad))
        return real(x, codes, inverse=inverse, **kw)
    monkeypatch.setattr(ops, "dihedral", spy)
    trainer.fit(iterations=6)
    train = [f for f in forwards if f[1]]
    assert train == [(4, True)] * 6, "one student pass per unsupervised step, on cat(x_s1, x_s2)"
    codes = g19["ia_c_codes"]
    per_step = [launches[5 * i:5 * i + 5] for i in range(6)]      # weak, strong1, strong2, labels back, both predictions back
    for i, step in enumerate(per_step):
        assert [s[1] for s in step] == [False, False, False, True, True], (i, step)
        assert [s[0] for s in step[:4]] == [codes[0, i].tolist(), codes[1, i].tolist(), codes[2, i].tolist(), codes[0, i].tolist()]
        both = step[4]
        assert both[0] == codes[1, i].tolist() + codes[2, i].tolist() and both[2] == (4, 1, 32, 32) and both[3], (i, both)
    assert not trainer.teacher.training and trainer.model.training is False      # validation left the student in eval mode


def test_refusals(g17, g19, tmp_path):
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _ia_trainer(g17, g19, "a", tmp_path, hip_graph=True)
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _ia_trainer(g17, g19, "d", tmp_path, hip_graph=True)
    with pytest.raises(NotImplementedError, match="UNETR"):
        _ia_trainer(g17, g19, "c", tmp_path, complementary_dropout=True)
    with pytest.raises(ValueError, match="augmenter lacks"):
        _ia_trainer(g17, g19, "c", tmp_path, augmenter=_replay_augmenters(g19, "a"))
    with pytest.raises(ValueError, match="view_transforms must be None"):
        _ia_trainer(g17, g19, "b", tmp_path, view_transforms=(None, None))


def _scale_raw(x):
    return x * 0.75


@pytest.mark.parametrize("tag", ["b", "d"])
def test_checkpoint_round_trip_with_the_augmenter(g17, g19, tag, tmp_path):
    """the augmenter (here the package's default random one) is part of the checkpoint record: `from_checkpoint` and
    `util.get_trainer` rebuild the trainer with it and training goes on; `raw_transform` is applied before the augmenter"""
    from torch_em_amd import util
    from torch_em_amd.transform import invertible_augmentations as ia
    augs = ia.UniMatchv2Augmenters(ndim=2, clip_max=3.0) if tag == "d" else ia.FixMatchAugmenters(ndim=2, clip_max=3.0)
    torch.manual_seed(0)
    np.random.seed(0)
    trainer, _, _ = _ia_trainer(g17, g19, tag, tmp_path, logger=None, augmenter=augs, raw_transform=_scale_raw, prefetch=False)
    views = (trainer._three_views if tag == "d" else trainer._two_views)([torch.full((2, 1, 8, 8), 8.0)])
    assert views[0].is_cuda and float(views[0].mean()) == 6.0 and all(float(v.max()) == 3.0 for v in views[1:])
    trainer.fit(iterations=6)
    folder = trainer.checkpoint_folder
    trainer2 = type(trainer).from_checkpoint(folder, name="latest")
    assert type(trainer2) is type(trainer) and trainer2.iteration == 6 and util.model_is_equal(trainer.model, trainer2.model)
    assert type(trainer2.augmenter) is type(augs) and trainer2.raw_transform is _scale_raw
    names = [type(a).__name__ for a in getattr(trainer2.augmenter, "strong1" if tag == "d" else "student").intensity_transforms.augmentations]
    assert names == ["RandomGaussianBlur", "RandomGaussianNoise"] and trainer2.augmenter.__dict__.keys() == augs.__dict__.keys()
    if tag == "d":
        assert trainer2.complementary_dropout is False and not trainer2.teacher.training and trainer2.momentum == 0.999
    else:
        assert trainer2.source_distribution == [0.6, 0.4]
    trainer2.fit(iterations=3)
    assert trainer2.iteration == 9
    trainer3 = util.get_trainer(folder, name="latest")
    assert type(trainer3) is type(trainer) and trainer3.iteration == 9 and type(trainer3.augmenter) is type(augs)
