"""CPU: the noise and blur raw augmentations -- numpy branches against the reference's outputs (g16_raw_noise.npz), the
stream's numpy implementation (transform/_philox.py) against known answers, exact distributions and exact moments, the blur's
CPU branch against float64, and the mean-teacher factory.  The helpers here are also the oracles of tests/test_gpu_raw_aug.py."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from torch_em_amd.transform import _philox  # noqa: F401  (the module under test: without it nothing here can run)

CLASSES = ["AdditiveGaussianNoise", "AdditivePoissonNoise", "PoissonNoise"]
RANGE_KEY = {"AdditiveGaussianNoise": "scale", "AdditivePoissonNoise": "lam", "PoissonNoise": "multiplier"}
ZMAX = float(np.sqrt(48 * np.log(2)))     # |z| <= sqrt(-2 ln 2^-24) = 5.768
MOMENT_LAMS = [0.05, 3, 9.99, 10, 37.5, 150]


@functools.lru_cache(maxsize=1)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "g16_raw_noise.npz")))


def case_names():
    return [str(c) for c in golden()["cases"]]


def make_noise(name, **kw):
    """the package's class of golden case `name` with the case's arguments"""
    import torch_em_amd.transform as T
    g = golden()
    cls = CLASSES[int(g[name + ".cls"])]
    kw[RANGE_KEY[cls]] = tuple(g[name + ".range"].tolist())
    if not int(g[name + ".clip"]):
        kw["clip_kwargs"] = None
    return getattr(T, cls)(**kw)


# ---- oracles shared with the GPU tests -------------------------------------------------------------------------------
def gauss_bound(x, std, z):
    """|device - (x + std z64)| allowed for y = fl32(x + fl32(std * z)), z = sqrtf(-2 logf(u1)) * cospif(2 u2).
    First term: OpenCL's single-precision limits, which the device library documents (log 3 ulp, sqrt 3 ulp, cospi 4 ulp),
    propagated through r = sqrt(-2 log u1), z = r c stay under 15 half-ulps of r <= 5.768; one more for z's own rounding:
    std * 16 * 2^-24 * 5.768.  Second term: the multiply and the add, half an ulp each of values below |x| + std |z|."""
    return std * 16 * 2.0 ** -24 * ZMAX + 2.0 ** -23 * (np.abs(x) + std * np.abs(z))


def poisson_cdf_edges(lam, k):
    """(cdf(k - 1), cdf(k)) of Poisson(lam) in float64"""
    from scipy.stats import poisson
    lam, k = np.asarray(lam, dtype=np.float64), np.asarray(k)
    return np.where(k > 0, poisson.cdf(k - 1, lam), 0.0), poisson.cdf(k, lam)


def moments_ok(k, lam):
    """5-sigma bounds of the estimators of mean and variance of n Poisson(lam) samples:
    |mean - lam| <= 5 sqrt(lam / n), |var - lam| <= 5 sqrt((2 lam^2 + lam) / n)"""
    k = np.asarray(k, dtype=np.float64).ravel()
    n, lam = k.size, float(np.float32(lam))
    dm, dv = abs(k.mean() - lam), abs(k.var() - lam)
    bm, bv = 5 * np.sqrt(lam / n), 5 * np.sqrt((2 * lam * lam + lam) / n)
    print(f"lam {lam:g}: |mean - lam| {dm:.3e} (bound {bm:.3e}), |var - lam| {dv:.3e} (bound {bv:.3e})")
    return dm <= bm and dv <= bv


def blur_ref(x, w):
    """float64: the last two axes of x convolved with the float32 weights w (taken exactly), reflect border -j -> j,
    n-1+j -> n-1-j, as a double loop over the taps"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    k, p = len(w), len(w) // 2
    H, W = x.shape[-2:]

    def reflect(i, n):
        i = np.abs(i)
        return np.where(i >= n, 2 * (n - 1) - i, i)
    out = np.zeros_like(x)
    for a in range(k):
        ya = reflect(np.arange(H) + a - p, H)
        for b in range(k):
            xb = reflect(np.arange(W) + b - p, W)
            out += w[a] * w[b] * x[..., ya[:, None], xb[None, :]]
    return out


# ---- the numpy branch is the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss_default", "gauss_range", "gauss_noclip", "padd_default", "padd_range", "padd_noclip",
                                  "pois_default", "pois_range", "pois_noclip"])
def test_numpy_branch_equals_the_reference(name):
    g = golden()
    assert name in case_names()
    x = g["input." + str(g[name + ".input"])]
    want = g[name + ".out"]
    for wrap in (lambda a: a, torch.from_numpy):      # a CPU tensor counts as numpy input
        np.random.seed(int(g[name + ".seed"]))
        got = make_noise(name)(wrap(x))
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name


def test_every_golden_case_is_run():
    params = test_numpy_branch_equals_the_reference.pytestmark[0].args[1]
    assert sorted(params) == case_names()
    shapes = {golden()["input." + str(golden()[n + ".input"])].shape for n in case_names()}
    assert shapes == {(5, 7), (2, 3, 4, 5)}


def test_numpy_per_sample_is_the_reference_sample_by_sample():
    from torch_em_amd.transform import AdditiveGaussianNoise, AdditivePoissonNoise, PoissonNoise
    x = np.random.RandomState(3).rand(3, 4, 5).astype("float32")
    for cls, kw in ((AdditiveGaussianNoise, {}), (AdditivePoissonNoise, {"lam": (1.0, 20.0)}), (PoissonNoise, {})):
        np.random.seed(4)
        got = cls(per_sample=True, **kw)(x)
        np.random.seed(4)
        assert np.array_equal(got, np.stack([cls(**kw)(s) for s in x])), cls.__name__


# ---- the stream -----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    from torch_em_amd.transform._philox import philox4x32
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = philox4x32(counter, key)
        assert all(w.dtype == np.uint32 for w in got)
        assert " ".join("%08x" % int(w) for w in got) == want


def test_stream_words_depend_on_seed_row_element_and_round_only():
    from torch_em_amd.transform._philox import philox4x32, words
    seed = (0x9e3779b9 << 32) | 0x12345678
    rows = np.array([0, 1, 65534], dtype=np.uint64)[:, None]
    i = np.concatenate([np.arange(5), 2 ** 32 - 2 + np.arange(5)]).astype(np.uint64)[None, :]
    field = np.stack(words(seed, rows, i, 3), axis=-1)               # [3, 10, 4] in one call
    for a, r in enumerate(rows[:, 0]):
        for b, e in enumerate(i[0]):
            one = words(seed, int(r), int(e), 3)                     # element by element
            raw = philox4x32((int(e) & 0xffffffff, int(e) >> 32, int(r), 3), (0x12345678, 0x9e3779b9))
            assert [int(w) for w in one] == [int(w) for w in raw] == field[a, b].tolist()
    assert len({tuple(v) for v in field.reshape(-1, 4).tolist()}) == 30                   # all different
    assert not np.array_equal(np.stack(words(seed, rows, i, 4), axis=-1), field)          # the round counts
    assert not np.array_equal(np.stack(words(seed + 1, rows, i, 3), axis=-1), field)      # the seed counts


def test_uniform_conversions_are_exact_and_half_open():
    from torch_em_amd.transform._philox import uniform_co, uniform_oc
    w = np.array([0, 255, 256, 0xffffffff], dtype=np.uint32)
    for dtype in (np.float32, np.float64):
        assert uniform_co(w, dtype).tolist() == [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24] and uniform_co(w, dtype).dtype == dtype
        assert uniform_oc(w, dtype).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]


def test_normal_float32_against_float64():
    """the float32 evaluation of the numpy implementation stays within the bound the device is held to (at x = 0, std = 1),
    |z| <= 5.768, and the moments of 2^20 samples are those of a standard normal within 5 sigma of their estimators"""
    from torch_em_amd.transform._philox import normal_from_words, words
    n = 1 << 20
    w = words(77, 2, np.arange(n))
    z64, z32 = normal_from_words(w[0], w[1], np.float64), normal_from_words(w[0], w[1], np.float32)
    assert z32.dtype == np.float32 and z64.dtype == np.float64
    err = np.abs(z32.astype(np.float64) - z64)
    print("float32 against float64: max |dz|", err.max())
    assert np.all(err <= gauss_bound(0.0, 1.0, z64))
    assert np.abs(z64).max() <= ZMAX
    assert abs(z64.mean()) <= 5 / np.sqrt(n) and abs(z64.var() - 1) <= 5 * np.sqrt(2 / n)
    edge = normal_from_words(np.array([0, 0xffffffff], dtype=np.uint32), np.array([0, 0x80000000], dtype=np.uint32), np.float64)
    assert abs(edge[0] - ZMAX) < 1e-12 and edge[1] == 0.0      # u1 = 2^-24, cospi(0) = 1; u1 = 1: log 1 = 0


def test_poisson_inversion_against_the_exact_cdf():
    """float64 inversion against scipy's Poisson cdf: for lam uniform in [0, 10) every k satisfies
    cdf(k - 1) <= u < cdf(k) up to 1e-12"""
    from torch_em_amd.transform._philox import field_words, poisson_from_words, uniform_co
    n = 200000
    lam = (np.random.RandomState(5).rand(n) * 10).astype(np.float32)
    lam[:4] = [0.0, 1e-3, 9.999999, 5.0]
    draw = field_words(123456789, 4, np.arange(n))
    k = poisson_from_words(lam, draw, np.float64)
    u = uniform_co(draw(0)[0], np.float64)
    lo, hi = poisson_cdf_edges(lam, k)
    assert k[0] == 0 and k.min() == 0 and k.max() < 80
    assert np.all(lo - 1e-12 <= u) and np.all(u < hi + 1e-12)


@pytest.mark.parametrize("lam", MOMENT_LAMS)
def test_poisson_moments(lam):
    from torch_em_amd.transform._philox import field_words, poisson_from_words
    n = 1 << 20
    k = poisson_from_words(np.full(n, lam, dtype=np.float32), field_words(2024, 1, np.arange(n)), np.float64)
    assert k.min() >= 0 and moments_ok(k, lam)


def test_poisson_branches_meet_at_ten():
    """lam = 10 takes the rejection branch, nextafter(10, 0) the inversion; 0 gives 0"""
    from torch_em_amd.transform import _philox as P
    n = 4096
    draw = P.field_words(9, 0, np.arange(n))
    below = np.full(n, np.nextafter(np.float32(10), np.float32(0)), dtype=np.float32)
    ten = np.full(n, 10, dtype=np.float32)
    assert np.array_equal(P.poisson_from_words(below, draw), P._inversion(below.astype(np.float64), P.uniform_co(draw(0)[0]), np.float64))
    assert np.array_equal(P.poisson_from_words(ten, draw), P._ptrs(ten.astype(np.float64), draw, np.arange(n), np.float64, np.float64))
    assert not np.array_equal(P.poisson_from_words(ten, draw), P.poisson_from_words(below, draw))
    assert not P.poisson_from_words(np.zeros(n, dtype=np.float32), draw).any()


def test_ptrs_float32_against_float64():
    """The transformed rejection in numpy float32 against float64 from the same words, lam uniform in [10, 200], 2^20
    elements: the share of different counts is 2.2e-5 with log Gamma in double and the same 2.2e-5 with log Gamma rounded to
    float32 (measured with this seed: the differences come from floor() of the float32 candidate, not from the log test).
    The device is allowed 1e-3 (tests/test_gpu_raw_aug.py); a float32 evaluation with a correctly rounded log Gamma must
    stay under a quarter of that, or the range of lam of that test is too wide."""
    from torch_em_amd.transform._philox import field_words, poisson_from_words
    n = 1 << 20
    lam = (10 + 190 * np.random.RandomState(6).rand(n)).astype(np.float32)
    draw = field_words(31337, 0, np.arange(n))
    k64 = poisson_from_words(lam, draw, np.float64)
    for lg in (np.float64, np.float32):
        k32 = poisson_from_words(lam, draw, np.float32, lgamma_dtype=lg)
        share = float((k32 != k64).mean())
        print("log Gamma in", np.dtype(lg).name, ": share of different counts", share)
        assert share <= 2.5e-4
        assert k32[k32 != k64].min(initial=0) >= 0


# ---- blur -------------------------------------------------------------------------------------------------------------------
def test_gaussian_weights():
    from torch_em_amd.transform.raw import gaussian_weights
    for sigma, k in ((0.01, 3), (0.34, 5), (1.0, 7), (3.0, 19), (2.999, 19), (3.001, 21)):
        w = gaussian_weights(sigma)
        assert w.dtype == torch.float32 and len(w) == k and abs(float(w.double().sum()) - 1) < 1e-6
        x = np.linspace(-(k - 1) / 2, (k - 1) / 2, k)
        pdf = np.exp(-0.5 * (x / sigma) ** 2)
        assert np.allclose(w.numpy(), pdf / pdf.sum(), rtol=1e-5, atol=1e-30)
        assert torch.equal(w, w.flip(0))
    assert gaussian_weights(0.01).tolist() == [0.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="positive"):
        gaussian_weights(0.0)


def test_blur_cpu_branch_against_float64():
    """The CPU branch (reflect pad + depth-wise conv2d with the outer-product kernel, float32) against the float64 double loop.
    Bound: k^2 products of two weights (one rounding each), k^2 multiplications by x and k^2 - 1 additions in any order:
    |d| <= (k^2 + 2) * 2^-24 * max|x| (the weights are positive and sum to 1)."""
    from torch_em_amd.transform import GaussianBlur
    from torch_em_amd.transform.raw import gaussian_weights
    x = (np.random.RandomState(8).randn(3, 9, 11) * 2 + 1).astype("float32")
    for sigma in (0.34, 1.0, 1.3):
        w = gaussian_weights(sigma).numpy()
        k = len(w)
        for inp in (x, torch.from_numpy(x)):
            got = GaussianBlur(sigma=(sigma, sigma))(inp)
            assert torch.is_tensor(got) and got.dtype == torch.float32 and tuple(got.shape) == x.shape
            assert np.abs(got.numpy() - blur_ref(x, w)).max() <= (k * k + 2) * 2.0 ** -24 * np.abs(x).max()
    delta = np.zeros((9, 11), dtype="float32")
    delta[4, 5] = 1.0
    w = gaussian_weights(1.0).numpy()
    got = GaussianBlur(sigma=(1.0, 1.0))(delta).numpy()
    want = np.zeros((9, 11))
    want[1:8, 2:9] = np.outer(w.astype(np.float64), w.astype(np.float64))
    assert np.abs(got - want).max() <= 2.0 ** -23 and np.array_equal(blur_ref(delta, w), want)
    assert torch.equal(GaussianBlur(sigma=(0.01, 0.01))(x), torch.from_numpy(x))     # weights 0, 1, 0
    assert tuple(GaussianBlur(sigma=(1.0, 1.0))(np.zeros((2, 3, 4, 8, 9), dtype="float32")).shape) == (2, 3, 4, 8, 9)
    assert GaussianBlur(sigma=(1.0, 1.0))(np.arange(64, dtype=np.int16).reshape(8, 8)).dtype == torch.float32


def test_blur_draws_sigma_with_swapped_bounds_and_steps_the_torch_generator():
    from torch_em_amd.transform import GaussianBlur
    x = np.random.RandomState(1).rand(16, 16).astype("float32")
    np.random.seed(3)
    torch.manual_seed(3)
    got = GaussianBlur(sigma=(0.5, 2.0))(x)
    after = torch.rand(1)
    np.random.seed(3)
    sigma = np.random.uniform(2.0, 0.5)
    assert torch.equal(got, GaussianBlur(sigma=(sigma, sigma))(x))
    torch.manual_seed(3)
    torch.empty(1).uniform_(sigma, sigma)
    assert torch.equal(after, torch.rand(1))


# ---- the factory ----------------------------------------------------------------------------------------------------------
def test_random_apply_follows_the_torch_seed():
    from torch_em_amd.transform.raw import _Compose, _RandomApply
    calls = []
    t = _RandomApply([lambda v: calls.append(v) or v + 1, lambda v: v * 2], p=0.5)
    torch.manual_seed(11)
    coins = [bool(0.5 < torch.rand(1)) for _ in range(32)]       # True: skipped
    torch.manual_seed(11)
    got = [t(1) for _ in range(32)]
    assert got == [1 if skip else 4 for skip in coins] and 0 < sum(coins) < 32 and len(calls) == 32 - sum(coins)
    assert [_RandomApply([lambda v: v + 1], p=1.0)(0) for _ in range(8)] == [1] * 8
    assert [_RandomApply([lambda v: v + 1], p=-1.0)(0) for _ in range(8)] == [0] * 8
    assert _Compose([lambda v: v + 1, lambda v: v * 3])(1) == 6


def test_mean_teacher_factory_structure_and_pickle():
    import torch_em_amd.transform as T
    from torch_em_amd.transform.raw import _Compose, _RandomApply
    t = T.get_default_mean_teacher_augmentations()
    assert isinstance(t, T.RawTransform) and t.normalizer is T.normalize
    a1, a2 = t.augmentation1, t.augmentation2
    assert isinstance(a1, _Compose) and a1.transforms[0] is T.normalize and len(a1.transforms) == 4
    kinds = [(type(r.transforms[0]), r.p) for r in a1.transforms[1:]]
    assert all(isinstance(r, _RandomApply) and len(r.transforms) == 1 for r in a1.transforms[1:])
    assert kinds == [(T.GaussianBlur, 0.3), (T.PoissonNoise, 0.15), (T.AdditiveGaussianNoise, 0.15)]
    assert isinstance(a2, _RandomApply) and a2.p == 0.3 and isinstance(a2.transforms[0], T.RandomContrast)
    assert a2.transforms[0].clip_kwargs == {"a_min": 0, "a_max": 1}
    blur, pois, gauss = (r.transforms[0] for r in a1.transforms[1:])
    assert blur.sigma == (0.0, 3.0) and pois.multiplier == (5.0, 10.0) and gauss.scale == (0.0, 0.3)
    assert pois.clip_kwargs == gauss.clip_kwargs == {"a_min": 0, "a_max": 1} and not pois.per_sample and not gauss.per_sample
    assert T.AdditivePoissonNoise().lam == (0.0, 0.1)

    u = T.get_default_mean_teacher_augmentations(p=0.8, norm=T.standardize, blur_kwargs={"sigma": (0.5, 1.0)},
                                                 poisson_kwargs={"multiplier": (1.0, 2.0), "per_sample": True},
                                                 gaussian_kwargs={"scale": (0.0, 0.1), "clip_kwargs": None})
    back = pickle.loads(pickle.dumps(u))
    assert back.normalizer is T.standardize and back.augmentation1.transforms[0] is T.standardize
    b, p, g = (r.transforms[0] for r in back.augmentation1.transforms[1:])
    assert [r.p for r in back.augmentation1.transforms[1:]] == [0.8, 0.4, 0.4] and back.augmentation2.p == 0.8
    assert b.sigma == (0.5, 1.0) and p.multiplier == (1.0, 2.0) and p.per_sample and g.scale == (0.0, 0.1) and g.clip_kwargs is None

    x = np.random.RandomState(2).rand(1, 16, 16).astype("float32") * 50
    for p_ in (0.0, 1.0):      # the whole chain on numpy input: reproducible under both seeds, in [0, 1]
        chain = T.get_default_mean_teacher_augmentations(p=p_)
        outs = []
        for _ in range(2):
            np.random.seed(5)
            torch.manual_seed(5)
            outs.append(np.asarray(chain(x)))
        assert np.array_equal(outs[0], outs[1]) and outs[0].shape == x.shape
        assert float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0


def test_validation_errors():
    from torch_em_amd import ops
    from torch_em_amd.transform import GaussianBlur
    with pytest.raises(ValueError, match="positive"):
        GaussianBlur(sigma=(0.0, 0.0))(np.zeros((8, 8), dtype="float32"))
    with pytest.raises(ValueError, match="at least two axes"):
        GaussianBlur(sigma=(1.0, 1.0))(np.zeros(8, dtype="float32"))
    with pytest.raises(ValueError, match="reflect border"):
        GaussianBlur(sigma=(3.0, 3.0))(np.zeros((9, 32), dtype="float32"))       # 19 taps: 9 >= H
    x = torch.zeros(2, 8)
    for call in (lambda: ops.gauss_noise(x, 0.1, 1), lambda: ops.poisson_add(x, 1.0, 1), lambda: ops.poisson_scaled(x, 5.0, 1),
                 lambda: ops.blur2d(x, [1.0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="seed"):
        ops._seed(-1)
    with pytest.raises(ValueError, match="seed"):
        ops._seed(2 ** 64)


def test_library_refuses_bad_blur_arguments_before_any_launch():
    """argument validation happens before any HIP call, so the messages can be checked without a device"""
    from torch_em_amd import _lib
    lib = _lib.load()
    one = 16      # any non-null pointers: nothing is dereferenced
    assert lib.tem_rawaug_blur2d(one, 2 * one, 1, 10, 10, one, one, 21, 3, None) == -1
    assert b"reflect border needs k/2 < size" in lib.tem_last_error()
    assert lib.tem_rawaug_blur2d(one, 2 * one, 1, 10, 10, one, one, 4, 3, None) == -1 and b"odd" in lib.tem_last_error()
    assert lib.tem_rawaug_blur2d(one, 2 * one, 1, 100, 100, one, one, 65, 3, None) == -1 and b"odd" in lib.tem_last_error()
    assert lib.tem_rawaug_blur2d(one, one, 1, 10, 10, one, one, 3, 3, None) == -1
    assert lib.tem_rawaug_gauss_noise(one, one, 65536, 4, one, 0, 0, 0, 0.0, 0.0, None) == -1
    assert lib.tem_rawaug_poisson_add(one, one, 2, 4, one, 0, 0xffffffff, 0, 0.0, 0.0, None) == -1     # rows past 2^32
    assert lib.tem_rawaug_philox_words(None, 0, 0, 0, 0, 4, None) == -1
