"""GPU: the noise and blur raw augmentations on the device (csrc/rawaug.hip, ops.philox_words / gauss_noise / poisson_add /
poisson_scaled / blur2d, transform/raw.py) against the numpy implementation of the stream (transform/_philox.py): words bit
for bit, samples against the float64 evaluation from the same words, distributions against their exact moments.  No bound
here is fitted to what the kernels return; each is derived where it is used."""
import functools

import numpy as np
import pytest
import torch

from test_raw_aug_cpu import MOMENT_LAMS, blur_ref, gauss_bound, moments_ok, poisson_cdf_edges

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = (0x1234567 << 32) | 0x89abcdef
ROW_SHAPES = [(N, L) for L in (1, 3, 4, 5, 255, 257, 1023, 65537) for N in (1, 3)]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def misaligned(x):
    """the rows in a buffer whose base is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def host(t):
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def field(N, L, seed=SEED, row0=0):
    """-> (rows, i, draw) of an [N, L] field"""
    from torch_em_amd.transform._philox import field_words
    rows, i = np.meshgrid(np.arange(row0, row0 + N), np.arange(L), indexing="ij")
    return rows, i, field_words(seed, rows, i)


@functools.lru_cache(maxsize=None)
def rows_uniform(N, L):
    return np.random.RandomState(100 * N + L % 97).rand(N, L).astype("float32")


def device_counts(lam, seed, row0=0):
    """the device's Poisson counts for the float32 means `lam` [N, L]: k / 1 + 0 is k"""
    from torch_em_amd import ops
    zero = torch.zeros(lam.shape[0], dtype=torch.float32, device=DEV)
    k = host(ops.poisson_scaled(to_dev(lam), 1.0, seed, None, row0, offset=zero))
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0
    return k.astype(np.int64)


# ---- the stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,row,i0,rnd,n", [(0, 0, 0, 0, 1000), (2 ** 63 - 1, 65534, 2 ** 32 - 5, 63, 11), (SEED, 7, 2 ** 40 + 3, 1, 257),
                                               (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 64 - 4, 2 ** 32 - 1, 4), (0, 65534, 0, 63, 1)])
def test_philox_words_equal_numpy_bit_for_bit(seed, row, i0, rnd, n):
    from torch_em_amd import ops
    from torch_em_amd.transform._philox import words
    got = ops.philox_words(seed, row, i0, rnd, n).cpu().numpy().view(np.uint32)
    i = (np.arange(n, dtype=np.uint64) + np.uint64(i0 % 2 ** 64))
    want = np.stack(words(seed, row, i, rnd), axis=-1)
    assert got.shape == (n, 4) and np.array_equal(got, want)


# ---- Gauss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", ROW_SHAPES)
def test_gauss_noise(N, L):
    """y = fl32(x + fl32(std z)) against x + std z64 from the same words; the bound: test_raw_aug_cpu.gauss_bound"""
    from torch_em_amd import ops
    from torch_em_amd.transform._philox import normal_from_words
    x = (np.random.RandomState(L + N).randn(N, L) * 2).astype("float32")
    std = [float(np.float32(s)) for s in (0.3, 1.0, 0.05)[:N]]
    xd = to_dev(x)
    y = host(ops.gauss_noise(xd, std, SEED))
    _, _, draw = field(N, L)
    w0, w1 = draw(0)
    z = normal_from_words(w0, w1, np.float64).reshape(N, L)
    s = np.asarray(std)[:, None]
    err = np.abs(y.astype(np.float64) - (x + s * z))
    print(f"[{N}, {L}] largest |error| / bound", float((err / gauss_bound(x, s, z)).max()))
    assert np.all(err <= gauss_bound(x, s, z))
    assert np.array_equal(bits(host(ops.gauss_noise(xd, std, SEED))), bits(y)), "not reproducible"
    assert not np.array_equal(host(ops.gauss_noise(xd, std, SEED + 1)), y) or L * N < 2
    for n in range(N):      # a row's samples depend on (seed, row, i) alone
        assert np.array_equal(bits(host(ops.gauss_noise(xd[n:n + 1], std[n], SEED, row0=n))), bits(y[n:n + 1])), n
    assert np.array_equal(bits(host(ops.gauss_noise(misaligned(x), std, SEED))), bits(y)), "misaligned base"
    clipped = host(ops.gauss_noise(xd, std, SEED, clip=(0.0, 1.0)))
    assert np.array_equal(bits(clipped), bits(np.clip(y, np.float32(0), np.float32(1))))
    assert np.array_equal(bits(host(ops.gauss_noise(xd, 0.0, SEED))), bits(x)), "std = 0"
    assert torch.equal(xd, to_dev(x)), "the input must not be modified"


# ---- Poisson, inversion -----------------------------------------------------------------------------------------------
def check_inversion(lam, k, seed, what):
    """Device counts k of the float32 means lam (< 10) against the float64 inversion from the same words.
    tau_k = (3 k + 8) 2^-24 bounds the error of the float32 search's running sum s_k against the exact cdf(k): p_0 = expf(-lam)
    is within 3 ulp <= 6 * 2^-24 relative (the library's documented limit); each step p_j = fl(fl(p_{j-1} lam) / j) adds two
    roundings of 2^-24 relative, so p_j carries (2 j + 6) 2^-24 relative, and sum_j<=k p_j (2 j + 6) <= (2 k + 6) cdf(k)
    <= 2 k + 6; each of the k additions s_j = fl(s_{j-1} + p_j) adds 2^-24 of s_j <= 1: together (3 k + 6) 2^-24, and two units
    are left for the second-order terms.  So a device count k is right whenever cdf(k-1) - tau_k <= u < cdf(k) + tau_k, and it
    can differ from the float64 count only for u within tau of an edge."""
    from torch_em_amd.transform._philox import poisson_from_words, uniform_co
    N, L = lam.shape
    _, _, draw = field(N, L, seed)
    u = uniform_co(draw(0)[0], np.float64).reshape(N, L)
    k64 = poisson_from_words(lam, draw, np.float64)
    lo, hi = poisson_cdf_edges(lam, k)
    tau = (3 * k + 8) * 2.0 ** -24
    assert np.all(lo - tau <= u) and np.all(u < hi + tau), what
    lo64, hi64 = poisson_cdf_edges(lam, k64)
    tau64 = (3 * k64 + 8) * 2.0 ** -24
    near = (np.abs(u - lo64) <= tau64) | (np.abs(u - hi64) <= tau64)
    print(what, "share within tau of an edge", near.mean(), "share of counts that differ from float64", (k != k64).mean())
    assert near.mean() <= 0.01, what
    assert (k == k64).mean() >= 0.999, what
    return k


@pytest.mark.parametrize("N,L", ROW_SHAPES)
def test_poisson_scaled_inversion(N, L):
    from torch_em_amd import ops
    x = rows_uniform(N, L)
    for mult in (5.0, 9.99):
        m32 = np.float32(mult)
        mn = x.min(axis=1, keepdims=True)
        lam = (x - mn) * m32
        assert lam.dtype == np.float32 and lam.max() < 10
        k = check_inversion(lam, device_counts(lam, SEED), SEED, f"mult {mult} [{N}, {L}]")
        want = (k.astype(np.float32) / m32 + mn).astype(np.float32)
        for xd in (to_dev(x), misaligned(x)):
            assert np.array_equal(bits(host(ops.poisson_scaled(xd, mult, SEED))), bits(want)), (mult, N, L)
        clipped = host(ops.poisson_scaled(to_dev(x), mult, SEED, clip=(0.25, 0.75)))
        assert np.array_equal(bits(clipped), bits(np.clip(want, np.float32(0.25), np.float32(0.75))))
    if N == 3:      # one multiplier per row; rows apart equal rows together
        mults = [5.0, 9.99, 7.5]
        y = host(ops.poisson_scaled(to_dev(x), mults, SEED))
        for n in range(3):
            assert np.array_equal(bits(host(ops.poisson_scaled(to_dev(x[n:n + 1]), mults[n], SEED, row0=n))), bits(y[n:n + 1]))


@pytest.mark.parametrize("N,L", ROW_SHAPES)
def test_poisson_add_inversion(N, L):
    from torch_em_amd import ops
    x = rows_uniform(N, L)
    for lam in (1e-3, 0.1, 9.5):
        l32 = np.float32(lam)
        k = check_inversion(np.full((N, L), l32), device_counts(np.full((N, L), l32), SEED + 2), SEED + 2, f"lam {lam} [{N}, {L}]")
        want = (x + k.astype(np.float32) / l32).astype(np.float32)
        got = host(ops.poisson_add(to_dev(x), lam, SEED + 2))
        assert np.array_equal(bits(got), bits(want)), (lam, N, L)
        assert np.array_equal(bits(host(ops.poisson_add(misaligned(x), lam, SEED + 2))), bits(want))
        assert np.array_equal(bits(host(ops.poisson_add(to_dev(x), lam, SEED + 2, clip=(0.0, 1.0)))), bits(np.clip(want, 0, 1)))


# ---- Poisson, transformed rejection -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", [(1, 257), (3, 65537)])
def test_poisson_ptrs_against_float64(N, L):
    """lam uniform in [10, 200]: the device equals the float64 evaluation of the same algorithm from the same words on at
    least 99.9 % of the elements (numpy float32 against float64: 2.2e-5 apart, tests/test_raw_aug_cpu.py), and where it
    differs the count is still a count."""
    from torch_em_amd import ops
    from torch_em_amd.transform._philox import poisson_from_words
    lam = (10 + 190 * np.random.RandomState(L).rand(N, L)).astype(np.float32)
    k = device_counts(lam, SEED + 3)
    _, _, draw = field(N, L, SEED + 3)
    k64 = poisson_from_words(lam, draw, np.float64)
    diff = k != k64
    print(f"[{N}, {L}] share of counts that differ from float64", diff.mean())
    assert diff.mean() <= 1e-3 and np.all(k[diff] >= 0)
    assert np.array_equal(device_counts(lam, SEED + 3), k), "not reproducible"
    # through the public ops: lam = (x - min) * mult with the float32 arithmetic of the kernel
    x = (lam / np.float32(200)).astype(np.float32)
    mn = x.min(axis=1, keepdims=True)
    m32 = np.float32(200.0)
    ks = device_counts((x - mn) * m32, SEED + 3)
    got = host(ops.poisson_scaled(misaligned(x), 200.0, SEED + 3))
    assert np.array_equal(bits(got), bits(ks.astype(np.float32) / m32 + mn))


@pytest.mark.parametrize("lam", [v for v in MOMENT_LAMS if v >= 10])
def test_poisson_device_moments(lam):
    n = 1 << 20
    k = device_counts(np.full((1, n), lam, dtype=np.float32), SEED + 4)
    assert moments_ok(k, lam)


def test_poisson_branch_boundary():
    """lam = 10 takes the transformed rejection, nextafter(10, 0) the inversion: each equals its own oracle, and the two
    oracles are far apart, so the comparison tells the branches from each other"""
    from torch_em_amd.transform import _philox as P
    n = 1024
    _, _, draw = field(1, n, SEED + 5)
    below = np.full((1, n), np.nextafter(np.float32(10), np.float32(0)), dtype=np.float32)
    ten = np.full((1, n), 10, dtype=np.float32)
    inv = P._inversion(below.ravel().astype(np.float64), P.uniform_co(draw(0)[0]), np.float64)
    rej = P._ptrs(ten.ravel().astype(np.float64), draw, np.arange(n), np.float64, np.float64)
    assert (inv != rej).mean() > 0.5
    assert np.array_equal(device_counts(below, SEED + 5).ravel(), inv)
    assert np.array_equal(device_counts(ten, SEED + 5).ravel(), rej)
    assert not device_counts(np.zeros((1, n), dtype=np.float32), SEED + 5).any()      # lam = 0


# ---- blur -------------------------------------------------------------------------------------------------------------
def blur_bound(k, x):
    """two fma chains of k taps with exact weights that sum to 1: k roundings of at most 2^-24 max|x| each, twice, and one
    unit each for the second-order terms"""
    return 2 * (k + 1) * 2.0 ** -24 * float(np.abs(x).max())


PLANES = [((2, 2), 0.3), ((2, 2), 0.01), ((10, 10), 3.0), ((33, 65), 0.01), ((33, 65), 0.34), ((33, 65), 1.0), ((33, 65), 3.0),
          ((64, 257), 1.0), ((64, 257), 3.0), ((32, 64), 1.0), ((31, 63), 3.0)]


@pytest.mark.parametrize("plane,sigma", PLANES)
def test_blur_class_against_float64(plane, sigma):
    from torch_em_amd.transform import GaussianBlur
    from torch_em_amd.transform.raw import gaussian_weights
    w = gaussian_weights(sigma).numpy()
    k = len(w)
    assert k == {0.01: 3, 0.3: 3, 0.34: 5, 1.0: 7, 3.0: 19}[sigma]
    leads = [(), (3,), (2, 3)] if plane == (33, 65) else [()]
    for lead in leads:
        x = (np.random.RandomState(plane[1] + len(lead)).randn(*lead, *plane) * 3 + 1).astype("float32")
        want = blur_ref(x, w)
        t = GaussianBlur(sigma=(sigma, sigma))
        for xd in (to_dev(x), misaligned(x)):
            got = t(xd)
            assert tuple(got.shape) == x.shape
            err = np.abs(host(got).astype(np.float64) - want).max()
            assert err <= blur_bound(k, x), (lead, err, blur_bound(k, x))
            if sigma == 0.01:       # weights 0, 1, 0: the identity
                assert np.array_equal(bits(host(got)), bits(x))
        assert torch.equal(t(to_dev(x)), t(to_dev(x))), "not reproducible"
    c = np.full(plane, 2.7182817, dtype="float32")
    assert np.abs(host(GaussianBlur(sigma=(sigma, sigma))(to_dev(c))).astype(np.float64) - float(c[0, 0])).max() <= blur_bound(k, c)


@pytest.mark.parametrize("plane,ky,kx", [((33, 33), 35, 35), ((40, 70), 63, 33), ((32, 32), 1, 35), ((17, 130), 3, 31), ((70, 18), 33, 1),
                                         ((5, 1), 5, 1)])
def test_blur2d_tap_counts_and_both_tiles(plane, ky, kx):
    """different weights on the two axes, tap counts on both sides of the switch from 64-wide to 32-wide tiles (16 taps to a
    side), planes that end one past a tile; against the float64 sum over ky x kx taps"""
    from torch_em_amd import ops
    rng = np.random.RandomState(ky * 64 + kx)
    wy = rng.rand(ky).astype("float32")
    wx = rng.rand(kx).astype("float32")
    wy, wx = wy / wy.sum(dtype=np.float32), wx / wx.sum(dtype=np.float32)
    x = rng.randn(2, *plane).astype("float32")
    H, W = plane
    ref = np.zeros(x.shape)
    refl = lambda i, n: np.where(np.abs(i) >= n, 2 * (n - 1) - np.abs(i), np.abs(i))   # noqa: E731
    for a in range(ky):
        ya = refl(np.arange(H) + a - ky // 2, H)
        for b in range(kx):
            xb = refl(np.arange(W) + b - kx // 2, W)
            ref += float(wy[a]) * float(wx[b]) * x.astype(np.float64)[:, ya[:, None], xb[None, :]]
    got = host(ops.blur2d(to_dev(x), wy.tolist(), wx.tolist()))
    scale = float(wy.astype(np.float64).sum() * wx.astype(np.float64).sum())      # 1 to a few 2^-24
    assert np.abs(got - ref).max() <= (ky + kx + 2) * 2.0 ** -24 * np.abs(x).max() * scale


def test_blur_errors():
    from torch_em_amd import ops
    from torch_em_amd.transform import GaussianBlur
    x = torch.rand(3, 9, 32, device=DEV)
    with pytest.raises(ValueError, match="reflect border needs k/2 < size"):
        GaussianBlur(sigma=(3.0, 3.0))(x)           # 19 taps: 9 >= H
    with pytest.raises(ValueError, match="odd and within 1..63"):
        ops.blur2d(x, [0.5, 0.5])
    with pytest.raises(ValueError, match="odd and within 1..63"):
        GaussianBlur(sigma=(11.0, 11.0))(torch.rand(80, 80, device=DEV))      # 67 taps
    with pytest.raises(ValueError, match="at least two axes"):
        GaussianBlur(sigma=(1.0, 1.0))(torch.rand(8, device=DEV))


# ---- the classes ------------------------------------------------------------------------------------------------------
def class_oracle(cls, x, per_sample, seed):
    """the numpy oracle of a device call, composed by hand from the same draws: the scalars, then the seed -> (want in
    float64 from the float64 samples, None or the float64 counts, the float32 scalars)"""
    from torch_em_amd.transform import _philox as P
    n = len(x) if per_sample else 1
    rng = {"AdditiveGaussianNoise": (0.0, 0.3), "AdditivePoissonNoise": (0.0, 0.1), "PoissonNoise": (5.0, 10.0)}[cls]
    np.random.seed(seed)
    scal = np.asarray([np.random.uniform(*rng) for _ in range(n)]).astype(np.float32)[:, None]
    fseed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
    rows = x.reshape(n, -1)
    r, i = np.meshgrid(np.arange(n), np.arange(rows.shape[1]), indexing="ij")
    draw = P.field_words(fseed, r, i)
    if cls == "AdditiveGaussianNoise":
        w0, w1 = draw(0)
        z = P.normal_from_words(w0, w1, np.float64).reshape(rows.shape)
        return rows + scal.astype(np.float64) * z, z, scal
    if cls == "AdditivePoissonNoise":
        k = P.poisson_from_words(np.broadcast_to(scal, rows.shape), draw, np.float64)
        return (rows + k.astype(np.float32) / scal).astype(np.float32), k, scal
    mn = rows.min(axis=1, keepdims=True)
    k = P.poisson_from_words((rows - mn) * scal, draw, np.float64)
    return (k.astype(np.float32) / scal + mn).astype(np.float32), k, scal


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("cls", ["AdditiveGaussianNoise", "AdditivePoissonNoise", "PoissonNoise"])
def test_classes_equal_the_oracle_composed_by_hand(cls, per_sample):
    """on [2, 1, 8, 16, 16]: np.random.seed, the device call, and the same draws by hand.  Gauss within its bound, then
    clipped; the Poisson classes (means below 10: the inversion) bit-equal to the float32 expression on the float64 counts
    on at least 99.9 % of the elements -- the counts themselves are held to their bounds in the tests above."""
    import torch_em_amd.transform as T
    x = np.random.RandomState(12).rand(2, 1, 8, 16, 16).astype("float32")
    np.random.seed(40)
    got = host(getattr(T, cls)(per_sample=per_sample)(to_dev(x)))
    after = np.random.uniform()
    want, sample, scal = class_oracle(cls, x, per_sample, 40)
    assert after == np.random.uniform(), "the device call and the oracle consume the same draws"
    assert got.shape == x.shape and got.min() >= 0 and got.max() <= 1
    got = got.reshape(want.shape)
    if cls == "AdditiveGaussianNoise":
        rows = x.reshape(want.shape)
        inside = (want > 0) & (want < 1)
        err = np.abs(got.astype(np.float64) - np.clip(want, 0, 1))
        assert np.all(err <= gauss_bound(rows, scal.astype(np.float64), sample)) and inside.mean() > 0.5
    else:
        same = bits(got) == bits(np.clip(want, np.float32(0), np.float32(1)))
        print(cls, per_sample, "share of elements equal to the oracle", same.mean())
        assert same.mean() >= 0.999
    if per_sample:
        assert scal[0, 0] != scal[1, 0]
    np.random.seed(40)
    assert np.array_equal(bits(host(getattr(T, cls)(per_sample=per_sample)(to_dev(x))).ravel()), bits(got).ravel()), "np.random.seed pins a call"


def test_class_arguments_on_the_device():
    import torch_em_amd.transform as T
    x = torch.rand(2, 1, 4, 8, 8, device=DEV)
    for cls in (T.AdditiveGaussianNoise, T.AdditivePoissonNoise, T.PoissonNoise):
        with pytest.raises(ValueError, match="a_min and a_max only"):
            cls(clip_kwargs={"a_min": 0, "a_max": 1, "out": None})(x)
        y = cls(clip_kwargs=None)(x * 3)
        assert float(y.max()) > 1.0
    with pytest.raises(ValueError, match="lam is 0"):
        T.AdditivePoissonNoise(lam=(0.0, 0.0))(x)
    np.random.seed(1)
    y = T.PoissonNoise(multiplier=(50.0, 60.0), clip_kwargs={"a_min": 0.25, "a_max": None})(x)
    assert float(y.min()) == 0.25 and float(y.max()) > 1.0
    np.random.seed(1)
    a = T.AdditiveGaussianNoise(scale=(0.2, 0.2), clip_kwargs={"a_min": 0.4, "a_max": 0.6})(x)     # the contents are ignored
    assert float(a.min()) == 0.0 and float(a.max()) == 1.0


def test_mean_teacher_augmentations_on_a_device_batch():
    """fixed numpy and torch seeds: in [0, 1] and reproducible, on the default stream and inside a side stream; with p = 1
    every stage changes the data"""
    import torch_em_amd.transform as T
    x = to_dev((np.random.RandomState(3).rand(2, 1, 8, 32, 32) * 200).astype("float32"))

    def run(t):
        np.random.seed(7)
        torch.manual_seed(7)
        return t(x)
    for p in (0.3, 1.0):
        t = T.get_default_mean_teacher_augmentations(p=p)
        y = run(t)
        assert y.is_cuda and y.dtype == torch.float32 and y.shape == x.shape
        assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0
        assert torch.equal(run(t), y)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            z = run(t)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(z, y)
    # p = 1 applies the blur and the contrast always and the two noise stages with p / 2: take the first torch seed whose
    # coins (blur, [the blur's own uniform_ draw], Poisson, Gauss) apply both
    for seed in range(64):
        torch.manual_seed(seed)
        torch.rand(1)
        torch.empty(1).uniform_(1.0, 1.0)
        if float(torch.rand(1)) <= 0.5 and float(torch.rand(1)) <= 0.5:
            break
    np.random.seed(7)
    torch.manual_seed(seed)
    y = t(x)
    np.random.seed(7)
    torch.manual_seed(seed)
    v = x
    for stage in list(t.augmentation1.transforms) + [t.normalizer, t.augmentation2]:
        nxt = stage(v)
        assert nxt.shape == v.shape and not torch.equal(nxt, v), stage
        v = nxt
    assert torch.equal(v, y) and float(y.min()) >= 0.0 and float(y.max()) <= 1.0
