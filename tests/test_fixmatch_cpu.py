"""CPU: FixMatch without a device -- the numpy oracle of the distribution alignment (tests/fixmatch_ref.py) against what the
REFERENCE's `get_distribution_alignment` computed (tests/golden/g18_fixmatch.npz, made by tests/golden/gen_golden_fixmatch.py),
the argument checks of `ops.label_count_partials` / `ops.distribution_align`, which run before the library is loaded, and the
host logic of FixMatchTrainer with a stub model (nothing is launched)."""
import json
import os

import numpy as np
import pytest
import torch

import fixmatch_ref as ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def g18():
    return dict(np.load(os.path.join(GOLDEN, "g18_fixmatch.npz")))


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_selftrain.npz")))


def test_fixture_is_small_and_has_the_cases(g18):
    assert os.path.getsize(os.path.join(GOLDEN, "g18_fixmatch.npz")) < os.path.getsize(os.path.join(GOLDEN, "g17_selftrain.npz"))
    cases = ref.da_cases(g18)
    # 3 dtypes x 2 shapes x 2 thresholds x 3 sources, 2 single-class tensors per dtype, one fp32 case with a NaN
    assert len(cases) == 3 * 2 * 2 * 3 + 3 * 2 + 1
    assert {c["dtype"] for c in cases} == set(ref.DTYPES)
    assert {tuple(c["source"]) for c in cases} == {(0.7, 0.3), (0.2, 0.8), (0.5, 0.5)}
    assert {c["threshold"] for c in cases} == {0.5, 0.3}
    shapes = {ref.da_array(g18, c["x"], c["dtype"]).shape for c in cases}
    assert shapes == {(2, 1, 5, 7, 9), (1, 2, 33, 31)}
    for c in cases:
        x = ref.da_array(g18, c["x"], c["dtype"])
        assert not np.isinf(x).any() and not (np.signbit(x) & (x == 0)).any(), c["key"]
        if "single" in c["key"]:
            assert len(np.unique(x)) == 1
            continue
        # the threshold in that dtype and its two neighbours, and the values on and beyond the clip's bounds
        t = float(ref.threshold_in(c["threshold"], c["dtype"]))
        below, above = x[x < t].max(), x[x > t].min()
        eps = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[c["dtype"]]
        assert (x == t).any() and t - below <= 2 * eps * t and above - t <= 2 * eps * t, c["key"]
        for v in (0.0, 1.0, -0.25, 1.5):
            assert (x == v).any(), (c["key"], v)
    assert np.isnan(ref.da_array(g18, "da_f32_nan_x", "f32")).sum() == 1


def test_oracle_matches_the_reference_bit_for_bit(g18):
    n_clipped = 0
    for c in ref.da_cases(g18):
        x, want = ref.da_array(g18, c["x"], c["dtype"]), ref.da_array(g18, c["key"], c["dtype"])
        got = ref.align(x, c["source"], c["threshold"], c["dtype"])
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["key"], int((got != want).sum()))
        n_clipped += int((want == 1).any())
        c1 = ref.count(x, c["threshold"], c["dtype"])
        assert 0 <= c1 <= x.size
        if "single_low" in c["key"]:
            assert c1 == 0 and np.array_equal(got, ref.round_to(x * np.float32(0.7), c["dtype"]))     # the ratio is source / 1
        if "single_high" in c["key"]:
            assert c1 == x.size and np.array_equal(got, ref.round_to(x * np.float32(0.3), c["dtype"]))
    assert n_clipped > 20
    nan = ref.da_array(g18, "da_f32_nan", "f32")
    assert np.isnan(nan).sum() == 1 and np.isnan(nan.reshape(-1)[100])     # NaN comes through the clip


def test_oracle_rounding_helpers():
    assert float(ref.round_to(np.float32(1.00390625), "bf16")) == 1.0          # tie: to even (down)
    assert float(ref.round_to(np.float32(1.01171875), "bf16")) == 1.015625     # tie: to even (up)
    assert float(ref.threshold_in(0.3, "f16")) == float(np.float16(0.3))
    assert float(ref.threshold_in(0.3, "bf16")) == float(torch.tensor(0.3, dtype=torch.float64).to(torch.bfloat16))
    assert np.isnan(ref.round_to(np.float32(np.nan), "bf16"))
    a = np.linspace(-2, 2, 4001, dtype=np.float32)
    assert np.array_equal(ref.round_to(a, "bf16"), torch.from_numpy(a).to(torch.bfloat16).float().numpy())
    assert ref.count(np.array([np.nan, 0.5, 0.4, 0.6], dtype=np.float32), 0.5, "f32") == 2   # NaN is below
    assert ref.ratios(0, 8, (0.7, 0.3)) == (np.float32(0.7), np.float32(0))                     # an empty class cannot poison


def test_state_chain_decodes(g18):
    for tag in "abc":
        states = ref.fm_states(g18, tag)
        assert len(states) == 7 and all(sorted(s) == sorted(states[0]) for s in states)
        for s in states:
            assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in s.values())
        moved = [max(float(np.abs(states[i + 1][k] - states[i][k]).max()) for k in states[0]) for i in range(6)]
        assert all(0 < m < 5e-3 for m in moved), moved      # six AdamW steps at lr 1e-3
    a, b = ref.fm_states(g18, "a"), ref.fm_states(g18, "b")
    assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and any(not np.array_equal(a[6][k], b[6][k]) for k in a[0])


def test_fixture_runs_meet_the_generators_conditions(g18):
    runs = json.loads(str(g18["fm_runs"]))
    assert runs == {"a": {"threshold": None, "semi": False, "source": None},
                    "b": {"threshold": 0.7, "semi": False, "source": [0.7, 0.3]},
                    "c": {"threshold": 0.7, "semi": True, "source": [0.6, 0.4]}}
    assert float(g18["fm_guard"]) > 1e-5
    for tag, cfg in runs.items():
        assert len(g18[f"fm_{tag}_unsup"]) == 6 and g18[f"fm_{tag}_unsup"].min() > 0.02
        assert len(g18[f"fm_{tag}_sup"]) == len(g18[f"fm_{tag}_combined"]) == (6 if cfg["semi"] else 0)
        keep = g18[f"fm_{tag}_keep"]
        assert (keep == 1).all() if cfg["threshold"] is None else ((keep > 0.05) & (keep < 0.95)).all()
        assert "teacher_state" not in set(g18[f"fm_{tag}_ckpt_keys"])
        assert 0 < float(g18[f"fm_{tag}_scatter_unsup"]) < 5e-2


# ---- ops: every argument check runs before the library is loaded ---------------------------------------------------------
def test_ops_validate_before_the_library_is_loaded(monkeypatch):
    from torch_em_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    x = torch.rand(2, 1, 4, 4)
    for call in (lambda t: ops.label_count_partials(t), lambda t: ops.distribution_align(t, [0.7, 0.3])):
        with pytest.raises(ValueError, match="on the GPU"):
            call(x)                                              # a CPU tensor
        with pytest.raises(ValueError, match="on the GPU"):
            call(x.numpy())
    # the remaining checks need a tensor that claims to be on the device: a meta tensor has device, dtype and strides, no data
    dev = torch.device("meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: self.device.type == "meta"))
    m = torch.empty(2, 1, 4, 4, device=dev)
    for call in (lambda t, **k: ops.label_count_partials(t, **k), lambda t, **k: ops.distribution_align(t, [0.7, 0.3], **k)):
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            call(m.double())
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            call(m.to(torch.int64))
        with pytest.raises(ValueError, match="non-empty"):
            call(torch.empty(0, 3, device=dev))
        with pytest.raises(ValueError, match="dense"):
            call(m[:, :, ::2])
        with pytest.raises(ValueError, match="dense"):
            call(m[..., :3])
    with pytest.raises(ValueError, match="threshold must be finite"):
        ops.label_count_partials(m, threshold=float("nan"))
    with pytest.raises(ValueError, match="threshold must be finite"):
        ops.distribution_align(m, [0.7, 0.3], label_threshold=float("inf"))
    for bad in ([0.7], [0.2, 0.3, 0.5], [0.7, 0.0], [0.7, -0.3], [float("nan"), 0.3], [float("inf"), 0.3], [], 0.5,
                torch.tensor([0.5, 0.25, 0.25])):
        with pytest.raises(ValueError, match="source_distribution"):
            ops.distribution_align(m, bad)
    with pytest.raises(ValueError, match="laid out like the labels"):
        ops.distribution_align(m, [0.7, 0.3], out=torch.empty(2, 1, 4, 4, device=dev, dtype=torch.float16))
    with pytest.raises(ValueError, match="laid out like the labels"):
        ops.distribution_align(m, [0.7, 0.3], out=torch.empty(2, 4, 4, 1, device=dev).permute(0, 3, 1, 2))
    # a permuted dense tensor passes the checks and reaches the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        ops.label_count_partials(torch.empty(2, 4, 4, 3, device=dev).permute(0, 3, 1, 2))
    with pytest.raises(AssertionError, match="the library was loaded"):
        ops.distribution_align(m.to(torch.bfloat16), torch.tensor([0.6, 0.4]), 0.3)


def test_count_query_needs_no_device():
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_label_count_parts(1, 0) == 1 and lib.tem_label_count_parts(1024, 0) == 1 and lib.tem_label_count_parts(1025, 0) == 2
    assert lib.tem_label_count_parts(2048, 1) == 1 and lib.tem_label_count_parts(2049, 2) == 2       # 8 elements per load
    assert lib.tem_label_count_parts(2048 * 256 * 4 + 4099, 0) == 2048 == lib.tem_label_count_parts(1 << 33, 1)   # the cap
    assert lib.tem_label_count_parts(0, 0) == 0 and lib.tem_label_count_parts(-3, 0) == 0 and lib.tem_label_count_parts(8, 3) == 0
    # refused arguments answer with an error, not a launch
    assert lib.tem_label_count_st(None, 8, 0.5, None, 1, 0, None) == -1 and b"bad arguments" in lib.tem_last_error()
    assert lib.tem_distribution_align_st(None, None, 8, 0.5, 0.7, 0.3, None, 1, 0, None) == -1


# ---- host logic of the trainer ----------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    init_kwargs = {}

    def __init__(self):
        super().__init__()
        self.out_conv = torch.nn.Conv2d(1, 1, 1)

    def forward(self, x):
        return self.out_conv(x)


def _loader(n):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.zeros(n, 1, 4, 4), torch.zeros(n, 1, 4, 4)), batch_size=1)


def _trainer(tmp_path, **kw):
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            FixMatchTrainer)
    model = _Stub()
    args = dict(name="fm", model=model, optimizer=torch.optim.AdamW(model.parameters()), pseudo_labeler=DefaultPseudoLabeler(),
                unsupervised_loss=DefaultSelfTrainingLoss(), unsupervised_loss_and_metric=DefaultSelfTrainingLossAndMetric(),
                device="cpu", mixed_precision=False, save_root=str(tmp_path))
    args.update(kw)
    return FixMatchTrainer(**args)


def test_constructor_signature_is_the_references_plus_view_transforms():
    import inspect
    from torch_em_amd.self_training import FixMatchTrainer
    names = list(inspect.signature(FixMatchTrainer.__init__).parameters)
    assert names == ["self", "model", "unsupervised_train_loader", "unsupervised_loss", "pseudo_labeler", "supervised_train_loader",
                     "unsupervised_val_loader", "supervised_val_loader", "supervised_loss", "unsupervised_loss_and_metric",
                     "supervised_loss_and_metric", "logger", "source_distribution", "view_transforms", "kwargs"]
    assert inspect.signature(FixMatchTrainer.__init__).parameters["logger"].default is None


def test_trainer_selects_loaders_like_the_reference(tmp_path):
    from torch_em_amd.self_training import DefaultSelfTrainingLoss
    u5, u3, s4, v2, sv2 = _loader(5), _loader(3), _loader(4), _loader(2), _loader(2)
    t = _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2)
    assert t.train_loader is u5 and t._train_epoch_impl == t._train_epoch_unsupervised
    assert t.val_loader is v2              # the unsupervised VALIDATION loader (the mean teacher takes the train loader)
    assert t.logger_class is None and t.hip_graph is False and t.source_distribution is None
    assert not hasattr(t, "teacher") and not hasattr(t, "sampler") and t._labeling_model() is t.model
    t = _trainer(tmp_path, unsupervised_train_loader=u5, supervised_train_loader=s4, supervised_val_loader=sv2,
                 supervised_loss=DefaultSelfTrainingLoss())
    assert t.train_loader is s4 and t.val_loader is sv2 and t._train_epoch_impl == t._train_epoch_semisupervised
    t = _trainer(tmp_path, unsupervised_train_loader=u3, supervised_train_loader=s4, supervised_val_loader=sv2,
                 unsupervised_val_loader=v2, supervised_loss=DefaultSelfTrainingLoss())
    assert t.train_loader is u3 and t.val_loader is v2      # the shorter train loader; the unsupervised one where both exist
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5)                                            # no validation loader
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5, supervised_train_loader=s4, supervised_val_loader=sv2)   # no supervised loss
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2, unsupervised_loss_and_metric=None)
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2, hip_graph=True)
    with pytest.raises(ValueError, match="teacher_augmentation, student_augmentation"):
        _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2, view_transforms=(lambda x: x,))


def test_source_distribution_is_validated(tmp_path):
    kw = dict(unsupervised_train_loader=_loader(3), unsupervised_val_loader=_loader(1))
    for bad in ([1.0], [0.2, 0.3, 0.5], torch.tensor([0.5, 0.25, 0.25]), [], [0.7, 0.0], [-0.7, 0.3], [float("nan"), 0.3]):
        with pytest.raises(ValueError, match="exactly two finite positive entries"):
            _trainer(tmp_path, source_distribution=bad, **kw)
    assert _trainer(tmp_path, source_distribution=(0.7, 0.3), **kw).source_distribution == [0.7, 0.3]
    assert _trainer(tmp_path, source_distribution=torch.tensor([0.25, 0.75]), **kw).source_distribution == [0.25, 0.75]
    # without a source distribution the labels come back as the very tensor (reference :170, :181) -- also on the CPU
    t = _trainer(tmp_path, **kw)
    x = torch.rand(2, 1, 4, 4)
    assert t.get_distribution_alignment(x) is x
    # with one, there is no CPU path
    with pytest.raises(ValueError, match="on the GPU"):
        _trainer(tmp_path, source_distribution=[0.7, 0.3], **kw).get_distribution_alignment(x)


def test_pseudo_labeler_is_not_stepped_after_validation(tmp_path):
    """the base FixMatch trainer does not advance the threshold schedule (only the reference's invertible variant does);
    MeanTeacherTrainer does -- both through the one shared validation loop"""
    from torch_em_amd.self_training import MeanTeacherTrainer
    t = _trainer(tmp_path, unsupervised_train_loader=_loader(3), unsupervised_val_loader=_loader(1))
    calls = []
    t.pseudo_labeler = type("L", (), {"step": lambda self, m, e: calls.append((m, e)), "confidence_threshold": None})()
    t._after_unsupervised_validation(0.5)
    assert calls == []
    MeanTeacherTrainer._after_unsupervised_validation(t, 0.5)
    assert calls == [(0.5, t._epoch)]


def _halve(x):
    return x * 0.5


def test_checkpoint_keys_and_round_trip(tmp_path, g18):
    from torch_em_amd import util
    from torch_em_amd.self_training import DefaultSelfTrainingLoss, FixMatchTrainer
    kw = dict(unsupervised_train_loader=_loader(3), supervised_train_loader=_loader(3), supervised_val_loader=_loader(1),
              supervised_loss=DefaultSelfTrainingLoss())
    t = _trainer(tmp_path, raw_transform=_halve, source_distribution=[0.6, 0.4], **kw)
    t._initialize(3, None)
    t.save_checkpoint("latest", 0.5, 0.5)
    ckpt = torch.load(os.path.join(t.checkpoint_folder, "latest.pt"), weights_only=False)
    for tag in "abc":
        assert set(g18[f"fm_{tag}_ckpt_keys"]) - {"scheduler_state", "scaler_state"} <= set(ckpt)
        # `init`: the entries the reference's save_checkpoint writes itself (its serialiser adds one per constructor argument;
        # here those travel in `init.self_training`, as for MeanTeacherTrainer)
        assert {"train_loader_kwargs", "train_dataset", "val_loader_kwargs", "val_dataset", "loss_class", "loss_kwargs",
                "metric_class", "metric_kwargs"} <= set(g18[f"fm_{tag}_init_keys"]) & set(ckpt["init"])
        assert str(g18[f"fm_{tag}_loss_class"]) == "torch_em.self_training.mean_teacher.Dummy"
    assert "teacher_state" not in ckpt
    init = ckpt["init"]
    assert init["loss_class"] == init["metric_class"] == "torch_em_amd.self_training.mean_teacher.Dummy"
    assert init["loss_kwargs"] == {} and init["metric_kwargs"] == {}
    assert init["trainer_class"] == "torch_em_amd.self_training.fix_match.FixMatchTrainer"
    st = init["self_training"]
    assert st["source_distribution"] == [0.6, 0.4] and "sampler" not in st and "momentum" not in st
    for t2 in (FixMatchTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu"),
               util.get_trainer(t.checkpoint_folder, name="latest", device="cpu")):
        assert type(t2) is FixMatchTrainer and t2.source_distribution == [0.6, 0.4] and t2.raw_transform is _halve
        assert len(t2.supervised_train_loader) == 3 and t2.train_loader is t2.unsupervised_train_loader
        v1, v2 = t2._views((torch.ones(1, 1, 2, 2), 2 * torch.ones(1, 1, 2, 2)))
        assert float(v1.mean()) == 0.5 and float(v2.mean()) == 1.0
    with pytest.raises(TypeError, match="unexpected arguments"):
        FixMatchTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu", sampler=None)
