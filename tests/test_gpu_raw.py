"""GPU: min-max / percentile normalisation and contrast on the device (csrc/rawnorm.hip, ops.row_*, transform/raw.py).

Everything here is compared bit for bit (order statistics by value: -0.0 == 0.0).  That is the expectation, not a tuned
number: min / max and the radix select are exact, and every other step is one correctly rounded float32 operation in
numpy's order.  A mismatch is a finding -- look for fma contraction or a fast-math division first."""
import functools
import os

import numpy as np
import pytest
import torch

from test_raw_cpu import case_names, golden, run_case, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"

DATA = ["normal", "huge", "tiny", "equal", "quant8", "bytes", "zeros"]


def make_rows(kind, N, L, seed):
    rng = np.random.RandomState(seed)
    if kind == "normal":      # mixed sign
        x = rng.randn(N, L)
    elif kind == "huge":
        x = rng.randn(N, L) * 1e30
    elif kind == "tiny":      # down to 1e-42: denormals among normals
        x = rng.randn(N, L) * 1e-30
        x[:, ::3] *= 1e-12
    elif kind == "equal":
        x = np.full((N, L), -3.25)
    elif kind == "quant8":    # 8 levels: massive ties
        x = rng.randint(0, 8, size=(N, L)) / 8.0 - 0.5
    elif kind == "bytes":     # 0..255 as float: constant top byte of the key
        x = rng.randint(0, 256, size=(N, L))
    else:                     # both zeros next to small values of both signs
        x = rng.randint(-1, 2, size=(N, L)) * 1e-3
        x[:, ::2] = 0.0
        x[:, 1::4] = -0.0
    x = x.astype("float32")
    if kind == "zeros" and L >= 4:
        assert np.signbit(x[0, 1]) and x[0, 1] == 0 and not np.signbit(x[0, 0])
    return x


def rank_sets(N, L):
    four = [min(max(L // 3 - 1, 0) + i, L - 1) for i in range(4)]
    return {
        "ends": [0, L - 1],
        "consecutive": four,
        "duplicated": [L // 2, L // 2, L - 1, L // 2],
        "per_row": [[(7 * n + (k * L) // 5 + k) % L for k in range(4)] for n in range(N)],
    }


def misaligned(x):
    """the rows in a buffer whose base is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def sorted_rows(kind, N, L):
    x = make_rows(kind, N, L, 1000 + L)
    return x, np.sort(x, axis=1)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 63, 255, 256, 257, 1023, 65537, 300001])
def test_row_order_statistics_are_exact(N, L):
    from torch_em_amd import ops
    for kind in DATA:
        x, srt = sorted_rows(kind, N, L)
        xd = torch.from_numpy(x).to(DEV)
        for name, ranks in rank_sets(N, L).items():
            per_row = ranks if isinstance(ranks[0], list) else [ranks] * N
            want = np.stack([srt[n][per_row[n]] for n in range(N)])
            got = ops.row_order_statistics(xd, ranks)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (kind, name, N, L)
            again = ops.row_order_statistics(xd, ranks)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (kind, name, "not reproducible")
    x, srt = sorted_rows("normal", N, L)
    ranks = rank_sets(N, L)["consecutive"]
    got = ops.row_order_statistics(misaligned(x), ranks).cpu().numpy()
    assert np.array_equal(got, srt[:, ranks]), ("misaligned base", N, L)


def test_row_order_statistics_rank_counts_and_errors():
    from torch_em_amd import ops
    x, srt = sorted_rows("normal", 3, 1023)
    xd = torch.from_numpy(x).to(DEV)
    for K in (1, 8, 9, 17):     # one call takes 8 ranks per row; more are split
        ranks = [int(v) for v in np.linspace(0, 1022, K)]
        assert np.array_equal(ops.row_order_statistics(xd, ranks).cpu().numpy(), srt[:, ranks]), K
    with pytest.raises(ValueError, match="outside"):
        ops.row_order_statistics(xd, [0, 1023])
    with pytest.raises(ValueError):
        ops.row_order_statistics(xd, [[0], [1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_order_statistics(torch.from_numpy(x), [0])


@pytest.mark.parametrize("L", [1, 257, 65537, 300001])
def test_row_minmax(L):
    from torch_em_amd import ops
    for kind in ("normal", "huge", "tiny", "bytes", "equal"):
        x, srt = sorted_rows(kind, 3, L)
        for xd in (torch.from_numpy(x).to(DEV), misaligned(x)):
            mn, mx = ops.row_minmax(xd)
            assert np.array_equal(mn.cpu().numpy(), srt[:, 0]) and np.array_equal(mx.cpu().numpy(), srt[:, -1]), (kind, L)


def ulp_equal(got, want, exact):
    """bit-equal; on a numpy other than the one the golden file records (its percentile arithmetic has changed between
    releases) within 1 float32 ulp"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if exact:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return bool(np.all(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1))


@pytest.mark.parametrize("L", [1000, 1001, 65536, 65537])
def test_percentiles_equal_numpy(L):
    """v_lower / v_upper of ops.normalize_percentile == np.percentile on the same float32 rows: q = 50 on even L has weight
    0.5 exactly, 0.1 / 1 take the a + d*t branch, 99 / 99.7 the b - d*(1-t) branch, 100 clamps the upper neighbour."""
    from torch_em_amd import ops
    exact = np.__version__ == str(golden()["numpy_version"])
    qs = [0, 0.1, 1, 50, 99, 99.7, 100]
    for kind in ("normal", "bytes", "tiny"):
        x, _ = sorted_rows(kind, 3, L)
        xd = torch.from_numpy(x).to(DEV)
        for qa, qb in zip(qs, reversed(qs)):
            y, v = ops.normalize_percentile(xd, qa, qb, 1e-7, return_percentiles=True)
            v = v.cpu().numpy()
            want = np.stack([[np.percentile(r, qa), np.percentile(r, qb)] for r in x])
            assert want.dtype == np.float32
            assert ulp_equal(v, want, exact), (kind, L, qa, qb, v, want)
    # per-row percentiles in one call
    x, _ = sorted_rows("normal", 3, L)
    lows, ups = [0.5, 2.0, 10.0], [99.5, 98.0, 90.0]
    _, v = ops.normalize_percentile(torch.from_numpy(x).to(DEV), lows, ups, 1e-7, return_percentiles=True)
    want = np.stack([[np.percentile(r, a), np.percentile(r, b)] for r, a, b in zip(x, lows, ups)])
    assert ulp_equal(v.cpu().numpy(), want, exact)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
    return t.cpu().numpy()


@pytest.mark.parametrize("name", ["norm_all", "norm_sample", "norm_channel", "pct_all", "pct_sample", "pct_channel", "pct_bytes",
                                  "pct_u8", "pct_i16", "rpn_uniform", "rpn_normal", "contrast", "contrast_noclip", "chain"])
def test_device_transforms_equal_the_reference(name):
    assert name in case_names()
    g = golden()
    for key, got in run_case(name, wrap=to_dev).items():
        assert same_bits(host(got), g[f"{name}.{key}"]), (name, key)


@pytest.mark.parametrize("name", ["pct_u8", "pct_i16"])
def test_integer_tensors_are_cast_to_float32(name):
    from torch_em_amd.transform import normalize, normalize_percentile
    g = golden()
    a = g[name + ".args"].tolist()
    x = g["input." + str(g[name + ".input"])]
    axis = None if a[2] == 0 else tuple(range(int(a[2]), x.ndim))
    assert same_bits(host(normalize_percentile(to_dev(x), a[0], a[1], axis=axis)), g[name + ".out"])
    assert same_bits(host(normalize(to_dev(x), axis=axis)), normalize(x.astype("float32"), axis=axis))
    half = torch.from_numpy(x.astype("float32")).to(DEV).half()
    assert same_bits(host(normalize_percentile(half, a[0], a[1], axis=axis)),
                     normalize_percentile(half.float().cpu().numpy(), a[0], a[1], axis=axis))


@pytest.mark.parametrize("shape", [(2, 1, 9, 17, 33), (3, 2, 8, 8)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_device_transforms_equal_their_numpy_branch(shape, mode):
    """fresh inputs, all three axis modes (whole array, per sample, per channel)"""
    from torch_em_amd.transform import RandomContrast, RandomPercentileNormalization, get_raw_transform, normalize, normalize_percentile
    axis = None if mode == 0 else tuple(range(mode, len(shape)))
    rng = np.random.RandomState(10 * len(shape) + mode)
    inputs = {"uniform": rng.rand(*shape), "normal": rng.randn(*shape) * 40 - 7, "bytes": rng.randint(0, 256, size=shape),
              "two-level": (rng.rand(*shape) > 0.7) * 3.0, "constant": np.full(shape, 2.5)}
    for kind, x in inputs.items():
        x = x.astype("float32")
        xd = to_dev(x)
        assert same_bits(host(normalize(xd, axis=axis)), normalize(x, axis=axis)), (kind, "normalize")
        for lo, up in ((1.0, 99.0), (0.0, 100.0), (0.3, 50.0), (25.0, 99.9)):
            assert same_bits(host(normalize_percentile(xd, lo, up, axis=axis)), normalize_percentile(x, lo, up, axis=axis)), (kind, lo, up)
        assert same_bits(host(normalize_percentile(xd, 2.0, 98.0, axis=axis, eps=1e-3)), normalize_percentile(x, 2.0, 98.0, axis=axis, eps=1e-3))
        assert torch.equal(xd, to_dev(x)), "the input must not be modified"
        if mode == 1:
            assert same_bits(host(normalize(xd, per_sample=True)), normalize(x, axis=axis))
            assert same_bits(host(normalize_percentile(xd, 1.0, 99.0, per_sample=True)), normalize_percentile(x, 1.0, 99.0, axis=axis))
            for kw in ({}, {"distribution": "normal", "distribution_kwargs": {"mean": 1.0, "std": 2.0}}):
                a = RandomPercentileNormalization(seed=1, per_sample=True, **kw)
                b = RandomPercentileNormalization(seed=1, **kw)
                assert same_bits(host(a(xd)), np.stack([b(s) for s in x])), (kind, kw)
            np.random.seed(5)
            got = host(RandomContrast(per_sample=True)(xd))
            np.random.seed(5)
            assert same_bits(got, np.stack([RandomContrast()(s) for s in x]))
        else:
            t = RandomPercentileNormalization(axis=axis, seed=3, lower_percentile_bounds=(0.0, 10.0))
            u = RandomPercentileNormalization(axis=axis, seed=3, lower_percentile_bounds=(0.0, 10.0))
            assert same_bits(host(t(xd)), u(x)), kind
        assert same_bits(host(normalize(xd, 10.0, 200.0)), normalize(x, 10.0, 200.0)), (kind, "explicit minval / maxval")
        assert same_bits(host(normalize(xd, minval=-300.0, axis=axis)), normalize(x, minval=-300.0, axis=axis)), (kind, "minval alone")
        assert same_bits(host(normalize(xd, maxval=180.0, axis=axis)), normalize(x, maxval=180.0, axis=axis)), (kind, "maxval alone")
        for clip in ({"a_min": 0, "a_max": 1}, None, {"a_min": -1.0, "a_max": None}, {"a_min": None, "a_max": 0.75}):
            chain = get_raw_transform(functools.partial(normalize_percentile, lower=1.0, upper=99.0, axis=axis),
                                      augmentation2=RandomContrast(alpha=(0.5, 2), mean=0.3, clip_kwargs=clip))
            np.random.seed(8)
            got = host(chain(xd))
            np.random.seed(8)
            assert same_bits(got, chain(x)), (kind, clip)


def test_unsupported_device_axes_raise():
    from torch_em_amd.transform import normalize, normalize_percentile
    x = torch.rand(2, 3, 4, 5, device=DEV)
    for fn in (normalize, normalize_percentile):
        for axis in (0, (0, 1), (1, 3), (2,)):
            with pytest.raises(NotImplementedError, match="trailing run of axes"):
                fn(x, axis=axis)
        assert tuple(fn(x, axis=(-1, -2)).shape) == (2, 3, 4, 5) and tuple(fn(x, axis=3).shape) == (2, 3, 4, 5)
    with pytest.raises(NotImplementedError, match="python number"):
        normalize(x, minval=np.zeros(1, dtype="float32"))
    from torch_em_amd.transform import RandomContrast
    with pytest.raises(ValueError, match="a_min and a_max only"):
        RandomContrast(clip_kwargs={"a_min": 0, "a_max": 1, "out": None})(x)
    with pytest.raises(ValueError, match="range"):
        normalize_percentile(x, -1.0, 99.0)


def test_predict_with_halo_takes_a_percentile_preprocess():
    """util/prediction.py hands each gathered block to `preprocess` as a CUDA tensor: the device transform there equals the
    same call with every block normalised by the numpy branch."""
    from torch_em_amd.model import UNet3d
    from torch_em_amd.transform import normalize_percentile
    from torch_em_amd.util import predict_with_halo
    torch.manual_seed(0)
    model = UNet3d(1, 2, depth=2, initial_features=4).to(DEV).eval()
    x = (np.random.default_rng(4).random((32, 32, 32)) * 255).astype("float32")
    seen = []

    def on_host(block):
        seen.append(tuple(block.shape))
        return torch.from_numpy(normalize_percentile(block.cpu().numpy(), lower=1, upper=99)).to(block.device)

    got = predict_with_halo(x, model, [DEV], (16, 16, 16), (8, 8, 8), disable_tqdm=True,
                            preprocess=functools.partial(normalize_percentile, lower=1, upper=99))
    want = predict_with_halo(x, model, [DEV], (16, 16, 16), (8, 8, 8), disable_tqdm=True, preprocess=on_host)
    assert len(seen) == 8 and got.shape == (2, 32, 32, 32) and float(np.abs(got).max()) > 0
    assert np.array_equal(got, want)


def test_trainer_runs_the_percentile_normalisation_in_its_pre_pass(tmp_path):
    """DefaultTrainer(raw_transform=RandomPercentileNormalization(seed=1, per_sample=True), prefetch=True): the first batch is
    the eager numpy computation, sample by sample, and a trainer rebuilt from the checkpoint carries the transform."""
    import torch_em_amd
    from torch_em_amd.model import UNet3d
    from torch_em_amd.trainer import DefaultTrainer
    from torch_em_amd.transform import RandomPercentileNormalization
    rng = np.random.RandomState(0)
    raw = torch.from_numpy((rng.rand(4, 1, 16, 16, 16) * 255).astype("float32"))
    lab = torch.from_numpy((rng.rand(4, 2, 16, 16, 16) > 0.5).astype("float32"))
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(raw, lab), batch_size=2, shuffle=False, pin_memory=True)
    torch.manual_seed(0)
    model = UNet3d(1, 2, depth=2, initial_features=4)
    transform = RandomPercentileNormalization(seed=1, per_sample=True)
    trainer = torch_em_amd.default_segmentation_trainer("rpn", model, loader, loader, device=DEV, logger=None, save_root=str(tmp_path),
                                                        raw_transform=transform, prefetch=True)
    seen = [x.clone() for x, _ in trainer._batches(loader, train=False)]
    oracle = RandomPercentileNormalization(seed=1)
    x0 = np.stack([oracle(s) for s in raw[:2].numpy()])
    x1 = np.stack([oracle(s) for s in raw[2:].numpy()])      # draws 2 and 3 of the same stream
    assert len(seen) == 2 and same_bits(seen[0].cpu().numpy(), x0) and same_bits(seen[1].cpu().numpy(), x1)
    assert float(x0.min()) == 0.0 and float(x0.max()) == 1.0
    trainer.fit(iterations=2)
    init = torch.load(os.path.join(trainer.checkpoint_folder, "latest.pt"), weights_only=False)["init"]
    assert init["unpicklable_transforms"] == []
    back = DefaultTrainer.from_checkpoint(trainer.checkpoint_folder, name="latest", device=DEV)
    t = back.raw_transform
    assert isinstance(t, RandomPercentileNormalization) and t.per_sample and t.seed == 1
    assert t.lower_percentile_bounds == (0.0, 5.0) and t.upper_percentile_bounds == (95.0, 100.0) and t.distribution == "uniform"
    back.fit(iterations=1)   # the restored pre-pass runs
