"""CPU: the numpy branch of the raw transforms (transform/raw.py) against the reference's outputs recorded in
tests/golden/g15_raw_transforms.npz (tests/golden/gen_golden_raw.py), bit for bit; the seeded draws, the validation errors and
the pickle round trip of RandomPercentileNormalization; and the host half of the device percentile -- ranks and weight as
the installed numpy forms them."""
import functools
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN

KINDS = {0: "normalize", 1: "percentile", 2: "rpn", 3: "contrast", 4: "chain"}


@functools.lru_cache(maxsize=1)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "g15_raw_transforms.npz")))


def case_names():
    return [str(c) for c in golden()["cases"]]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def axis_of(mode, ndim):
    return None if mode == 0 else tuple(range(int(mode), ndim))


def make_rpn(a, **kw):
    from torch_em_amd.transform import RandomPercentileNormalization
    if a[1]:
        kw.update(distribution="normal", distribution_kwargs={"mean": a[2], "std": a[3]})
    return RandomPercentileNormalization(lower_percentile_bounds=(a[4], a[5]), upper_percentile_bounds=(a[6], a[7]), seed=int(a[0]), **kw)


def run_case(name, wrap=lambda a: a):
    """The transforms of golden case `name` on wrap(float32 input) -> {golden key: result}."""
    from torch_em_amd.transform import RandomContrast, get_raw_transform, normalize, normalize_percentile
    g = golden()
    kind, a = KINDS[int(g[name + ".kind"])], g[name + ".args"].tolist()   # python floats, as the generator passed them
    x = g["input." + str(g[name + ".input"])].astype("float32")
    if kind == "normalize":
        return {"out": normalize(wrap(x), axis=axis_of(a[0], x.ndim))}
    if kind == "percentile":
        return {"out": normalize_percentile(wrap(x), a[0], a[1], axis=axis_of(a[2], x.ndim))}
    if kind == "rpn":
        return {"out": make_rpn(a)(wrap(x)), "out_per_sample": make_rpn(a, per_sample=True)(wrap(x))}
    if kind == "contrast":
        clip = {"a_min": 0, "a_max": 1} if a[3] else None
        np.random.seed(int(a[4]))
        out = RandomContrast(alpha=(a[0], a[1]), mean=a[2], clip_kwargs=clip)(wrap(x))
        np.random.seed(int(a[4]))
        return {"out": out, "out_per_sample": RandomContrast(alpha=(a[0], a[1]), mean=a[2], clip_kwargs=clip, per_sample=True)(wrap(x))}
    t = get_raw_transform(normalizer=functools.partial(normalize_percentile, lower=a[0], upper=a[1]),
                          augmentation2=RandomContrast(alpha=(a[2], a[3]), mean=a[4]))
    np.random.seed(int(a[5]))
    return {"out": t(wrap(x))}


@pytest.mark.parametrize("name", ["norm_all", "norm_sample", "norm_channel", "pct_all", "pct_sample", "pct_channel", "pct_bytes",
                                  "pct_u8", "pct_i16", "rpn_uniform", "rpn_normal", "contrast", "contrast_noclip", "chain"])
def test_numpy_branch_equals_the_reference(name):
    assert name in case_names()
    g = golden()
    for key, got in run_case(name).items():
        assert same_bits(got, g[f"{name}.{key}"]), (name, key)


def test_every_golden_case_is_run():
    params = test_numpy_branch_equals_the_reference.pytestmark[0].args[1]
    assert sorted(params) == case_names()


@pytest.mark.parametrize("name", ["pct_u8", "pct_i16"])
def test_integer_input_takes_the_reference_float64_interpolation(name):
    """On the integer array itself the numpy branch is the reference's expression too: percentiles interpolated in float64.
    That differs from the float32-cast result (which the device path computes) in the last bits only."""
    from torch_em_amd.transform import normalize_percentile
    g = golden()
    a = g[name + ".args"].tolist()
    x = g["input." + str(g[name + ".input"])]
    assert x.dtype.kind in "iu"
    got = normalize_percentile(x, a[0], a[1], axis=axis_of(a[2], x.ndim))
    assert same_bits(got, g[name + ".out_int"])
    assert np.allclose(got, g[name + ".out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["rpn_uniform", "rpn_normal"])
def test_seeded_draws_equal_the_reference(name):
    g = golden()
    t = make_rpn(g[name + ".args"].tolist())
    draws = np.asarray([t.sample_percentiles() for _ in range(4)], dtype=np.float64)
    assert np.array_equal(draws, g[name + ".draws"])
    lo, up = t.lower_percentile_bounds, t.upper_percentile_bounds
    assert all(lo[0] <= d[0] <= lo[1] and up[0] <= d[1] <= up[1] for d in draws)


def test_numpy_axis_modes_and_in_place_safety():
    from torch_em_amd.transform import normalize, normalize_percentile
    rng = np.random.RandomState(0)
    x = rng.rand(3, 2, 5, 7).astype("float32")
    keep = x.copy()
    for fn in (normalize, functools.partial(normalize_percentile, lower=2.0, upper=97.0)):
        per_sample = fn(x, per_sample=True)
        assert np.array_equal(x, keep), "the input must not be modified"
        assert same_bits(per_sample, fn(x, axis=(1, 2, 3)))
        assert same_bits(per_sample, np.stack([fn(s) for s in x]))
    assert float(normalize(x).min()) == 0.0 and abs(float(normalize(x).max()) - 1.0) < 1e-6
    rows = normalize_percentile(x, lower=[1.0, 2.0, 3.0], upper=[99.0, 98.0, 97.0])
    assert same_bits(rows, np.stack([normalize_percentile(s, lo, up) for s, lo, up in zip(x, (1.0, 2.0, 3.0), (99.0, 98.0, 97.0))]))


def test_validation_errors_match_the_reference():
    from torch_em_amd.transform import RandomPercentileNormalization as T
    bad = [
        (dict(lower_percentile_bounds=(0.0,)), ValueError, "lower_percentile_bounds must contain exactly two values."),
        (dict(lower_percentile_bounds=5.0), ValueError, "lower_percentile_bounds must contain exactly two values."),
        (dict(lower_percentile_bounds=(-1.0, 5.0)), ValueError, r"lower_percentile_bounds must be a finite interval within \[0, 50\)."),
        (dict(lower_percentile_bounds=(5.0, 1.0)), ValueError, "lower_percentile_bounds must be a finite interval"),
        (dict(lower_percentile_bounds=(0.0, 50.0)), ValueError, "lower_percentile_bounds must be a finite interval"),
        (dict(lower_percentile_bounds=(0.0, float("nan"))), ValueError, "lower_percentile_bounds must be a finite interval"),
        (dict(upper_percentile_bounds=(50.0, 99.0)), ValueError, r"upper_percentile_bounds must be a finite interval within \(50, 100\]."),
        (dict(upper_percentile_bounds=(95.0, 100.5)), ValueError, "upper_percentile_bounds must be a finite interval"),
        (dict(upper_percentile_bounds=[95.0, 96.0, 97.0]), ValueError, "upper_percentile_bounds must contain exactly two values."),
        (dict(distribution="gamma"), ValueError, "distribution must be 'uniform' or 'normal'."),
        (dict(distribution_kwargs={"mean": 1.0, "std": 1.0}), ValueError, "Uniform sampling does not accept distribution_kwargs."),
        (dict(distribution="normal"), ValueError, "Normal sampling requires exactly the distribution_kwargs 'mean' and 'std'."),
        (dict(distribution="normal", distribution_kwargs={"mean": 1.0}), ValueError, "Normal sampling requires exactly"),
        (dict(distribution="normal", distribution_kwargs={"mean": 1.0, "std": 1.0, "x": 0}), ValueError, "Normal sampling requires exactly"),
        (dict(distribution="normal", distribution_kwargs={"mean": 7.0, "std": 1.0}), ValueError,
         "The normal distribution mean must be finite and within lower_percentile_bounds."),
        (dict(distribution="normal", distribution_kwargs={"mean": float("nan"), "std": 1.0}), ValueError, "mean must be finite"),
        (dict(distribution="normal", distribution_kwargs={"mean": 1.0, "std": -1.0}), ValueError,
         "The normal distribution std must be finite and non-negative."),
        (dict(distribution="normal", distribution_kwargs={"mean": 1.0, "std": float("inf")}), ValueError, "std must be finite"),
        (dict(rounding_decimals=-1), ValueError, "rounding_decimals must be a non-negative integer or None."),
        (dict(rounding_decimals=1.0), ValueError, "rounding_decimals must be a non-negative integer or None."),
        (dict(rounding_decimals=True), ValueError, "rounding_decimals must be a non-negative integer or None."),
        (dict(eps=0.0), ValueError, "eps must be finite and greater than zero."),
        (dict(eps=float("inf")), ValueError, "eps must be finite and greater than zero."),
        (dict(seed=1.5), TypeError, "seed must be an integer or None."),
        (dict(seed=True), TypeError, "seed must be an integer or None."),
        (dict(seed=-3), ValueError, "seed must be non-negative."),
    ]
    for kw, exc, msg in bad:
        with pytest.raises(exc, match=msg):
            T(**kw)
    ok = T(lower_percentile_bounds=[1, 4], seed=np.int64(5), rounding_decimals=None, distribution="normal",
           distribution_kwargs={"mean": 2, "std": 0})
    assert ok.upper_percentile_bounds == (96.0, 99.0) and ok.seed == 5 and type(ok.seed) is int
    assert ok.distribution_kwargs == {"mean": 2.0, "std": 0.0} and ok.sample_percentiles() == (2.0, 98.0)
    with pytest.raises(ValueError, match="not both"):
        T(axis=(1, 2), per_sample=True)


def test_pickle_round_trip_keeps_arguments_and_stream():
    from torch_em_amd.transform import RandomContrast, RandomPercentileNormalization, RawTransform, get_raw_transform, normalize
    t = RandomPercentileNormalization(lower_percentile_bounds=(1.0, 4.0), seed=9, per_sample=True, eps=1e-6)
    t.sample_percentiles()                      # the generator exists and has advanced
    back = pickle.loads(pickle.dumps(t))
    assert isinstance(back, RandomPercentileNormalization)
    for key in ("lower_percentile_bounds", "upper_percentile_bounds", "distribution", "distribution_kwargs", "rounding_decimals",
                "axis", "seed", "eps", "per_sample"):
        assert getattr(back, key) == getattr(t, key), key
    assert [back.sample_percentiles() for _ in range(3)] == [t.sample_percentiles() for _ in range(3)]
    x = np.random.RandomState(1).rand(2, 1, 6, 6).astype("float32")
    assert same_bits(back(x), t(x))
    chain = get_raw_transform(normalize, augmentation2=RandomContrast(alpha=(0.7, 1.3), mean=0.4, clip_kwargs=None))
    again = pickle.loads(pickle.dumps(chain))
    assert isinstance(again, RawTransform) and again.normalizer is normalize and again.augmentation1 is None
    assert again.augmentation2.alpha == (0.7, 1.3) and again.augmentation2.mean == 0.4 and again.augmentation2.clip_kwargs is None
    np.random.seed(3)
    want = chain(x)
    np.random.seed(3)
    assert same_bits(again(x), want)


def lerp32(a, b, t):
    """numpy's _lerp on float32 scalars -- what tem_rawnorm_percentile_coef evaluates on the device"""
    a, b, t = np.float32(a), np.float32(b), np.float32(t)
    d = b - a
    return b - d * (np.float32(1) - t) if t >= 0.5 else a + d * t


@pytest.mark.parametrize("L", [1, 2, 3, 64, 1000, 1001, 65537, 300001])
def test_percentile_plan_reproduces_numpy(L):
    """ops.percentile_plan (host) + the float32 lerp == np.percentile on float32 data for every q the GPU test uses, with
    even and odd L: t == 0.5, both lerp branches, the clamped upper neighbour."""
    from torch_em_amd import ops
    rng = np.random.RandomState(L)
    for data in (rng.randn(L).astype("float32") * 50, rng.randint(0, 256, size=L).astype("float32")):
        srt = np.sort(data)
        for q in (0, 0.1, 1, 2.5, 50, 99, 99.7, 100):
            lo, hi, t = ops.percentile_plan(L, q)
            assert 0 <= lo <= hi <= L - 1 and hi - lo <= 1
            want = np.percentile(data, q)
            assert want.dtype == np.float32
            assert np.float32(lerp32(srt[lo], srt[hi], t)).tobytes() == want.tobytes(), (L, q, lo, hi, t)
    with pytest.raises(ValueError):
        ops.percentile_plan(10, 101.0)
