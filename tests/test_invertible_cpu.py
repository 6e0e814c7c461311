"""CPU: invertible augmentations -- the numpy oracle of the dihedral transform (tests/invaug_ref.py) against torch.flip / rot90,
the host tables of `ops` (codes, inverses, composition), the draws of the augmentation classes, and every refusal that is
raised before a launch.  Nothing here needs a device: `ops.dihedral` is replaced by the oracle where a chain is run."""
import numpy as np
import pytest
import torch

import invaug_ref as ref


def _torch_chain(x, h, v, k):
    if h:
        x = x.flip(-1)
    if v:
        x = x.flip(-2)
    return torch.rot90(x, k, (-2, -1))


@pytest.fixture
def oracle_dihedral(monkeypatch):
    """`ops.dihedral` on the CPU: the host-side plan of the real op (every check it makes), then the oracle; counts calls"""
    from torch_em_amd import ops
    calls = []

    def fake(x, codes, inverse=False, out=None):
        codes, shape = ops._dh_plan(x, codes, inverse)
        calls.append(codes)
        y = torch.from_numpy(ref.dihedral_np(x.contiguous().numpy(), codes))
        assert tuple(y.shape) == shape
        return y
    monkeypatch.setattr(ops, "dihedral", fake)
    return calls


@pytest.mark.parametrize("shape", ((1, 2, 5, 5), (1, 1, 4, 6), (1, 2, 3, 7, 3)))
def test_oracle_and_code_table_against_torch(shape):
    """all 16 (h, v, k): the issue's table, `ops.dihedral_codes`, and the oracle's index map agree with torch"""
    from torch_em_amd import ops
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    for (h, v), row in ref.CODE_TABLE.items():
        for k, code in zip((-1, 0, 1, 2), row):
            assert ops.dihedral_codes(h, v, k) == [code], (h, v, k)
            want = _torch_chain(x, h, v, k)
            got = ref.dihedral_np(x.numpy(), [code])
            assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy()), (h, v, k)
    assert ops.dihedral_codes([0, 1], [1, 1], [5, -2]) == [ref.CODE_TABLE[(0, 1)][2], ref.CODE_TABLE[(1, 1)][3]]   # k mod 4
    assert ops.dihedral_codes(torch.tensor([True, False]), torch.tensor([0, 0]), torch.tensor([0, 3])) == [4, 3]


def test_inverse_and_composition_tables():
    from torch_em_amd import ops
    assert ops.dihedral_inverse(range(8)) == list(ref.INVERSE) == [0, 1, 2, 5, 4, 3, 6, 7]
    x = np.arange(2 * 49).reshape(1, 2, 7, 7)
    for a in range(8):
        assert ops.dihedral_compose(a, ref.INVERSE[a]) == 0 and ops.dihedral_compose(ref.INVERSE[a], a) == 0
        assert np.array_equal(ref.dihedral_np(ref.dihedral_np(x, [a]), [ref.INVERSE[a]]), x)
        for b in range(8):
            both = ref.dihedral_np(ref.dihedral_np(x, [a]), [b])
            assert np.array_equal(both, ref.dihedral_np(x, [ops.dihedral_compose(a, b)])), (a, b)
    assert sorted({ops.dihedral_compose(a, b) for a in range(8) for b in range(8)}) == list(range(8))


def test_oracle_keeps_bit_patterns():
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.bool):
        x = ref.patterned((2, 1, 6, 6), dtype, seed=1)
        b = ref.bits(x)
        assert b.dtype.itemsize == x.element_size()
        out = ref.dihedral_np(b, [3, 6])
        assert sorted(out[0].ravel().tolist()) == sorted(b[0].ravel().tolist())
    f = ref.bits(ref.patterned((1, 1, 8, 8), torch.float32))
    assert 0x80000000 in f and 0x7FC00001 in f, "the pattern holds -0.0 and a NaN payload"


def test_dihedral_refusals_before_a_launch():
    """ValueError for a code outside 0..7, a wrong count, mixed transposition on a non-square plane, a bad rank or element
    size -- all from the host-side plan, on CPU tensors; a CPU tensor that passes it is refused as every op refuses one"""
    from torch_em_amd import ops
    x = torch.zeros(2, 1, 4, 6)
    for bad in ((0, 8), (-1, 0), torch.tensor([9, 0])):
        with pytest.raises(ValueError, match="0..7"):
            ops.dihedral(x, bad)
    with pytest.raises(ValueError, match="one code per sample"):
        ops.dihedral(x, (0, 0, 0))
    with pytest.raises(ValueError, match="mix transposing"):
        ops.dihedral(x, (0, 3))
    with pytest.raises(ValueError, match="mix transposing"):
        ops.dihedral(x, (5, 6), inverse=True)
    with pytest.raises(ValueError, match="4d .* or 5d"):
        ops.dihedral(torch.zeros(2, 4, 6), (0, 0))
    with pytest.raises(ValueError, match="1, 2 or 4 bytes"):
        ops.dihedral(x.double(), (0, 0))
    with pytest.raises(ValueError, match="integers"):
        ops.dihedral(x, (0.5, 0))
    with pytest.raises(ValueError, match="0..7"):
        ops.dihedral_inverse([8])
    with pytest.raises(ValueError, match="one entry per sample"):
        ops.dihedral_codes([0, 1], [0], [0, 0])
    assert ops._dh_plan(x, (3, 3), False) == ([3, 3], (2, 1, 6, 4)) and ops._dh_plan(x, (3, 5), True) == ([5, 3], (2, 1, 6, 4))
    assert ops._dh_plan(torch.zeros(2, 1, 5, 5), (0, 3), False)[1] == (2, 1, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dihedral(x, (0, 6))


def test_library_refuses_bad_arguments_without_a_device():
    """argument validation happens before any HIP call"""
    import ctypes

    from torch_em_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    src, dst, codes = ctypes.c_void_p(a), ctypes.c_void_p(a + 2048), ctypes.c_void_p(a)
    assert lib.tem_dihedral2d(None, dst, codes, 1, 1, 4, 4, 4, None) == -1 and b"null pointer" in lib.tem_last_error()
    assert lib.tem_dihedral2d(src, dst, None, 1, 1, 4, 4, 4, None) == -1 and b"null pointer" in lib.tem_last_error()
    assert lib.tem_dihedral2d(src, dst, codes, 1, 1, 4, 0, 4, None) == -1 and b"bad sizes" in lib.tem_last_error()
    assert lib.tem_dihedral2d(src, dst, codes, 1, 1, 4, 4, 3, None) == -1 and b"elem_bytes" in lib.tem_last_error()
    assert lib.tem_dihedral2d(src, src, codes, 1, 1, 4, 4, 4, None) == -1 and b"in-place" in lib.tem_last_error()
    assert lib.tem_dihedral2d(src, ctypes.c_void_p(a + 32), codes, 1, 1, 4, 4, 4, None) == -1 and b"overlapping" in lib.tem_last_error()
    # the path query: aligned bases and rows of 16 bytes stream by vectors, anything else even element by element, odd codes tile
    assert [lib.tem_dihedral2d_path(src, dst, c, 1, 1, 4, 4, 4) for c in range(8)] == [0, 2, 0, 2, 0, 2, 0, 2]
    assert lib.tem_dihedral2d_path(src, dst, 6, 1, 1, 4, 4, 2) == 1 and lib.tem_dihedral2d_path(src, dst, 6, 1, 1, 4, 8, 2) == 0
    assert lib.tem_dihedral2d_path(src, dst, 6, 1, 1, 4, 16, 1) == 0 and lib.tem_dihedral2d_path(src, dst, 6, 1, 1, 4, 15, 1) == 1
    assert lib.tem_dihedral2d_path(ctypes.c_void_p(a + 4), dst, 6, 1, 1, 4, 4, 4) == 1
    assert lib.tem_dihedral2d_path(src, ctypes.c_void_p(a + 2052), 6, 1, 1, 4, 4, 4) == 1
    # narrow elements tile packed when H, W and both bases are multiples of 4 bytes
    assert lib.tem_dihedral2d_path(src, dst, 3, 1, 1, 4, 4, 2) == 3 and lib.tem_dihedral2d_path(src, dst, 3, 1, 1, 8, 4, 1) == 3
    assert lib.tem_dihedral2d_path(src, dst, 3, 1, 1, 3, 4, 2) == 2 and lib.tem_dihedral2d_path(src, dst, 3, 1, 1, 4, 6, 1) == 2
    assert lib.tem_dihedral2d_path(ctypes.c_void_p(a + 2), dst, 3, 1, 1, 4, 4, 2) == 2
    assert lib.tem_dihedral2d_path(src, ctypes.c_void_p(a + 2050), 3, 1, 1, 4, 4, 2) == 2
    assert lib.tem_dihedral2d_path(src, dst, 8, 1, 1, 4, 4, 4) == -1 and b"0..7" in lib.tem_last_error()
    assert lib.tem_dihedral2d_path(src, src, 0, 1, 1, 4, 4, 4) == -1


# ---- the augmentation classes -------------------------------------------------------------------------------------------
def test_rotation_draws_are_pinned_by_the_seed():
    from torch_em_amd.transform.invertible_augmentations import RandomRotation90
    rot = RandomRotation90(times=(-1, 2), p=0.5)
    torch.manual_seed(7)
    a = rot.generate_parameters((64, 1, 8, 8))
    torch.manual_seed(7)
    want_prob = torch.rand(64) < 0.5
    want_times = torch.randint(-1, 3, (64,))
    assert torch.equal(a["batch_prob"], want_prob) and torch.equal(a["times"], want_times)
    assert set(a["times"].tolist()) == {-1, 0, 1, 2}, "the range is closed"
    torch.manual_seed(7)
    b = rot.generate_parameters((64, 1, 8, 8))
    assert torch.equal(a["times"], b["times"]) and torch.equal(a["batch_prob"], b["batch_prob"])
    same = RandomRotation90(times=(-1, 2), p=0.5, same_on_batch=True).generate_parameters((9, 1, 8, 8))
    assert len(set(same["times"].tolist())) == 1 and len(set(same["batch_prob"].tolist())) == 1
    with pytest.raises(ValueError, match="times"):
        RandomRotation90(times=(2, 1))


@pytest.mark.parametrize("ndim", (2, 3))
def test_chain_composes_to_one_code_per_sample(ndim, oracle_dihedral):
    """flip, flip, rotation drawn per sample: ONE `ops.dihedral` call whose codes are the (h, v, k) table's, the result is
    torch's chain sample by sample, `inverse` is one more call and restores the input; recorded parameters replay"""
    from torch_em_amd import ops
    from torch_em_amd.transform import invertible_augmentations as ia
    torch.manual_seed(11)
    chain = ia.get_geometrical_augmentations(ndim, aug_name="weak", p=0.5)
    assert type(chain) is (ia.AugmentationSequential if ndim == 2 else ia.AugmentationSequential3D)
    assert [type(a).__name__ for a in chain.augmentations] == ["RandomHorizontalFlip", "RandomVerticalFlip", "RandomRotation90"]
    shape = (16, 2, 6, 6) if ndim == 2 else (16, 2, 3, 6, 6)
    x = torch.randn(shape)
    y = chain(x)
    assert len(oracle_dihedral) == 1
    ph, pv, pr = chain._params
    h, v = ph["batch_prob"].int().tolist(), pv["batch_prob"].int().tolist()
    k = [int(t) if b else 0 for t, b in zip(pr["times"], pr["batch_prob"])]
    assert oracle_dihedral[0] == ops.dihedral_codes(h, v, k) == chain.codes(chain._params, 16)
    assert len(set(oracle_dihedral[0])) >= 4 and len(set(zip(h, v))) == 4
    for n in range(16):
        assert torch.equal(y[n], _torch_chain(x[n], h[n], v[n], k[n])), n
    assert torch.equal(chain.inverse(y), x) and len(oracle_dihedral) == 2
    assert oracle_dihedral[1] == ops.dihedral_inverse(oracle_dihedral[0])
    recorded = chain._params
    torch.manual_seed(99)
    assert torch.equal(chain(x, params=recorded), y) and chain._params[2] is recorded[2]
    assert torch.equal(chain.inverse(y, params=recorded), x)
    with pytest.raises(RuntimeError, match="Expected"):
        chain(x[0])
    with pytest.raises(ValueError, match="parameters for 3 augmentations"):
        chain(x, params=recorded[:2])


def test_p_zero_and_p_one(oracle_dihedral):
    from torch_em_amd.transform import invertible_augmentations as ia
    x = torch.randn(5, 1, 4, 4)
    never = ia.get_geometrical_augmentations(2, aug_name="weak", p=0.0)
    assert torch.equal(never(x), x) and oracle_dihedral[-1] == [0] * 5
    always = ia.get_geometrical_augmentations(2, aug_dict={"RandomHorizontalFlip": {}, "RandomVerticalFlip": {}}, p=1.0)
    assert torch.equal(always(x), x.flip(-1, -2)) and oracle_dihedral[-1] == [6] * 5
    rot = ia.AugmentationSequential(ia.RandomRotation90(times=(1, 1), p=1.0))
    assert torch.equal(rot(x), torch.rot90(x, 1, (-2, -1))) and oracle_dihedral[-1] == [5] * 5
    assert torch.equal(rot.inverse(rot(x)), x)
    single = ia.RandomRotation90(times=(-1, -1), p=1.0)
    assert torch.equal(single(x), torch.rot90(x, -1, (-2, -1))) and torch.equal(single.inverse(single(x)), x)
    for cls, kw in ((ia.RandomGaussianBlur, {"kernel_size": (3, 3), "sigma": (0.1, 1.0)}), (ia.RandomGaussianNoise, {"mean": 0.0, "std": 0.1})):
        aug = cls(p=0.0, **kw)
        assert aug(x) is x and not aug._params["batch_prob"].any()      # nobody won: no launch, the very tensor
        assert bool(cls(p=1.0, **kw).generate_parameters(x.shape)["batch_prob"].all())
    empty = ia.get_intensity_augmentations(2, aug_name="weak")
    assert len(empty.augmentations) == 0 and empty(x) is x and empty._params == []


def test_non_square_transposing_draw_is_refused(oracle_dihedral):
    from torch_em_amd.transform import invertible_augmentations as ia
    x = torch.randn(3, 1, 4, 6)
    with pytest.raises(ValueError, match=r"times=\(0, 0\).*\(2, 2\)"):
        ia.AugmentationSequential(ia.RandomRotation90(times=(1, 1), p=1.0))(x)
    assert oracle_dihedral == []
    half = ia.AugmentationSequential(ia.RandomVerticalFlip(p=1.0), ia.RandomRotation90(times=(2, 2), p=1.0))
    assert torch.equal(half(x), torch.rot90(x.flip(-2), 2, (-2, -1)))


def test_intensity_draws_and_arguments():
    from torch_em_amd.transform import invertible_augmentations as ia
    blur = ia.RandomGaussianBlur(kernel_size=(3, 3), sigma=(0.1, 1.0), p=0.5)
    torch.manual_seed(4)
    a = blur.generate_parameters((32, 1, 8, 8))
    torch.manual_seed(4)
    prob = torch.rand(32) < 0.5
    sigma = torch.rand(32, dtype=torch.float64) * 0.9 + 0.1
    assert torch.equal(a["batch_prob"], prob) and torch.equal(a["sigma"], sigma)
    w = ia._gauss_taps(3, 0.5)
    assert len(w) == 3 and abs(sum(w) - 1) < 1e-6 and w[0] == w[2] and abs(w[0] / w[1] - np.exp(-2.0)) < 1e-6
    noise = ia.RandomGaussianNoise(mean=0.0, std=0.1, p=0.5)
    np.random.seed(5)
    torch.manual_seed(5)
    b = noise.generate_parameters((8, 1, 4, 4))
    np.random.seed(5)
    assert b["seed"] == int(np.random.randint(0, 2 ** 63, dtype=np.int64)), "the seed follows transform/raw.py's _field_seed"
    for bad in (dict(kernel_size=(4, 3), sigma=(0.1, 1.0)), dict(kernel_size=3, sigma=(0.0, 1.0)), dict(kernel_size=3, sigma=(1.0, 0.5))):
        with pytest.raises(ValueError):
            ia.RandomGaussianBlur(**bad)
    with pytest.raises(ValueError):
        ia.RandomGaussianNoise(std=-1.0)
    with pytest.raises(NotImplementedError, match="no invertible"):
        ia.AugmentationSequential(torch.nn.Identity())
    with pytest.raises(AssertionError, match="not found"):
        ia.get_geometrical_augmentations(2, aug_dict={"RandomAffine": {}})
    with pytest.raises(ValueError, match="weak"):
        ia.get_default_augmentations("medium", ndim=2)


def test_trainer_refusals_before_anything_runs():
    """`hip_graph=True`, `complementary_dropout=True`, an augmenter without the views the trainer needs, `view_transforms`"""
    from torch_em_amd import self_training as st
    from torch_em_amd.transform import invertible_augmentations as ia
    args = dict(model=torch.nn.Identity(), unsupervised_train_loader=[0], unsupervised_loss=None, pseudo_labeler=None,
                unsupervised_val_loader=[0], unsupervised_loss_and_metric=lambda *a: None)
    for cls, augs in ((st.MeanTeacherTrainerWithInvertibleAugmentations, ia.MeanTeacherAugmenters(2)),
                      (st.FixMatchTrainerWithInvertibleAugmentations, ia.FixMatchAugmenters(2)),
                      (st.UniMatchv2Trainer, ia.UniMatchv2Augmenters(2))):
        with pytest.raises(NotImplementedError, match="hip_graph=True is not supported"):
            cls(augmenter=augs, hip_graph=True, **args)
        with pytest.raises(ValueError, match="view_transforms must be None"):
            cls(augmenter=augs, view_transforms=(None, None), **args)
    with pytest.raises(NotImplementedError, match="complementary_dropout=True needs the decoder"):
        st.UniMatchv2Trainer(complementary_dropout=True, augmenter=ia.UniMatchv2Augmenters(2), **args)
    with pytest.raises(ValueError, match="augmenter lacks .*weak"):
        st.UniMatchv2Trainer(augmenter=ia.MeanTeacherAugmenters(2), **args)
    with pytest.raises(ValueError, match="augmenter lacks .*teacher"):
        st.MeanTeacherTrainerWithInvertibleAugmentations(augmenter=ia.UniMatchv2Augmenters(2), **args)
    assert "augmenter" in st.UniMatchv2Trainer._PARTS and "view_transforms" not in st.FixMatchTrainerWithInvertibleAugmentations._PARTS
    assert "sampler" in st.MeanTeacherTrainerWithInvertibleAugmentations._PARTS and "sampler" not in st.FixMatchTrainerWithInvertibleAugmentations._PARTS


def test_g19_loss_cases_are_complete(golden_dir):
    """the four reference loss classes, both `pred_dim`, with and without filter (the values are compared on the GPU:
    tests/test_gpu_invertible.py -- this package's DiceLoss has no CPU path)"""
    import json
    import os
    g19 = np.load(os.path.join(golden_dir, "g19_invertible.npz"))
    cases = json.loads(str(g19["loss_index"]))
    assert sorted((c["cls"], c["pred_dim"] or 0, c["filter"]) for c in cases) == sorted(
        [(c, 0, f) for c in ("SelfTrainingLossWithInvertibleAugmentations", "SelfTrainingLossAndMetricWithInvertibleAugmentations")
         for f in (False, True)] + [(c, d, f) for c in ("UniMatchv2Loss", "UniMatchv2LossAndMetric") for d in (1, 2) for f in (False, True)])
    assert all(len(c["value"]) == (2 if "AndMetric" in c["cls"] else 1) and all(0 < v < 2 for v in c["value"]) for c in cases)
    by = {(c["cls"], c["pred_dim"], c["filter"]): c["value"] for c in cases}
    # the reference's own consistency: pred_dim = 1 is the plain class; the metric ignores the filter
    assert by[("UniMatchv2Loss", 1, True)] == by[("SelfTrainingLossWithInvertibleAugmentations", None, True)]
    assert by[("UniMatchv2LossAndMetric", 2, True)][1] == by[("UniMatchv2LossAndMetric", 2, False)][1]
    with pytest.raises(RuntimeError, match="no CPU"):
        from torch_em_amd.self_training import UniMatchv2Loss
        UniMatchv2Loss()(torch.from_numpy(g19["loss_pred"]), torch.from_numpy(g19["loss_labels"]), None, pred_dim=2)


def test_augmenter_containers_and_pickle(oracle_dihedral):
    """the reference's names; the default views; `reset_all`; the augmenters survive pickling with their parameters (the
    trainers store them in the checkpoint)"""
    import pickle

    from torch_em_amd.transform import invertible_augmentations as ia
    assert set(ia.DEFAULT_WEAK_AUGMENTATIONS) == set(ia.DEFAULT_STRONG_AUGMENTATIONS) == {"intensity", "geometrical"}
    assert ia.DEFAULT_WEAK_AUGMENTATIONS["intensity"] == {} and list(ia.DEFAULT_STRONG_AUGMENTATIONS["intensity"]) == ["RandomGaussianBlur", "RandomGaussianNoise"]
    assert ia.DEFAULT_WEAK_AUGMENTATIONS["geometrical"]["RandomRotation90"] == {"times": (-1, 2)}
    mt, fm, um = ia.MeanTeacherAugmenters(ndim=2), ia.FixMatchAugmenters(ndim=3, clip_max=1.0), ia.UniMatchv2Augmenters(ndim=2)
    assert len(mt.student.intensity_transforms.augmentations) == 0 and len(fm.student.intensity_transforms.augmentations) == 2
    assert fm.teacher.clip_max == 1.0 and type(fm.student.geometrical_transforms) is ia.AugmentationSequential3D
    assert [len(getattr(um, v).intensity_transforms.augmentations) for v in ("weak", "strong1", "strong2")] == [0, 2, 2]
    assert all(a.p == 0.75 for a in um.weak.geometrical_transforms.augmentations)
    own = ia.InvertibleAugmenter(*ia.get_default_augmentations("weak", 2))
    assert ia.MeanTeacherAugmenters(ndim=2, teacher=own).teacher is own
    x = torch.rand(4, 1, 6, 6)
    torch.manual_seed(0)
    y = mt.teacher.transform(x)
    assert mt.teacher.params is mt.teacher.geometrical_transforms._params and torch.equal(mt.teacher.reverse_transform(y), x)
    again = pickle.loads(pickle.dumps(mt))
    assert torch.equal(again.teacher.reverse_transform(y), x)
    clipped = ia.InvertibleAugmenter(*ia.get_default_augmentations("weak", 2, p=0.0), clip_max=0.5).transform(x)
    assert torch.equal(clipped, x.clamp(0.0, 0.5))
    mt.reset_all()
    assert mt.teacher.params is None and mt.student.params is None
