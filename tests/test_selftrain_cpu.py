"""CPU: self-training without a device -- the float64 oracle of the pseudo-labelling step (tests/selftrain_ref.py) against what
the REFERENCE's DefaultPseudoLabeler computed (tests/golden/g17_selftrain.npz, made by tests/golden/gen_golden_selftrain.py),
the threshold schedule of ScheduledPseudoLabeler against the reference's, and the host logic of MeanTeacherTrainer with a stub
model (nothing is launched)."""
import json
import os

import numpy as np
import pytest
import torch

import selftrain_ref as ref
from conftest import GOLDEN


THRESHOLDS = (None, 0.9, 0.6)   # as tests/golden/gen_golden_selftrain.py


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_selftrain.npz")))


def pl_cases():
    for act in (False, True):
        for both in (True, False):
            for t in THRESHOLDS:
                for mc in ((None,) if t is None else (None, 1)):
                    yield act, both, t, mc


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_oracle_matches_the_reference_labeler(g17, dt):
    x = g17[f"pl_{dt}_x"].astype(np.float64)
    assert x.shape == (2, 3, 4, 6)
    # the fixture carries the tie values: round(t), round(1 - t) and both neighbours, in both samples
    for t in (0.9, 0.6, 1.0 - 0.9, 1.0 - 0.6):
        v = float(ref.round_dtype(t, dt))
        for w in (v - float(ref.ulp(v, dt)), v, v + float(ref.ulp(v, dt))):
            assert (x[0] == w).any() and (x[1] == w).any(), (dt, t, w)
    n = 0
    for act, both, t, mc in pl_cases():
        key = f"pl_{dt}_{'sigmoid' if act else 'none'}_{'both' if both else 'one'}_{t}_{mc}"
        want_labels = g17[key + "_labels"].astype(np.float64)
        labels = ref.labels_ref(x, act, dt)
        if not act:
            assert np.array_equal(labels, want_labels) and np.array_equal(want_labels, x), key   # bit-equal: exact values
        else:
            # torch's CPU sigmoid against float64: 1 ulp of the storage type for the 16-bit types (fp32 result rounded), 2 in fp32
            err = np.abs(labels - want_labels) / ref.ulp(labels, dt)
            assert err.max() <= (2.0 if dt == "f32" else 1.0), (key, err.max())
        if t is None:
            assert key + "_mask" not in g17
            continue
        want = g17[key + "_mask"]
        assert want.dtype == (np.float32 if both else np.bool_), key
        # the compare semantics: the oracle's compare applied to the labels the reference stored gives the reference's mask
        got = ref.mask_ref(want_labels, t, both, dt, mc)
        assert got.dtype == want.dtype and np.array_equal(got, want), key
        # ... and so does the oracle end to end on these inputs (no label of the fixture lies an ulp from a threshold
        # on the wrong side of the reference's own sigmoid error)
        full = ref.mask_ref(labels, t, both, dt, mc)
        assert np.array_equal(full, want), key
        if mc is not None:
            assert np.array_equal(want[0], want[1]), key     # the batch-axis quirk: every sample carries sample 1's mask
        n += 1
    assert n == 16


def test_compare_runs_in_the_storage_type():
    """The two facts the kernel's compare is built on, on the CPU: float32(0.9) >= 0.9 and bfloat16(0.10009765625) <= 0.1."""
    assert bool(torch.tensor(0.9, dtype=torch.float32) >= 0.9)
    assert bool(torch.tensor(0.10009765625, dtype=torch.bfloat16) <= 1.0 - 0.9)
    assert float(ref.round_dtype(0.9, "f32")) == float(np.float32(0.9)) and float(ref.round_dtype(1.0 - 0.9, "bf16")) == 0.10009765625
    from torch_em_amd import ops
    for dt, dtype in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        for t in (0.9, 0.6, 1.0 - 0.9, 1.0 - 0.6, 0.52):
            assert ops.round_to(t, dtype) == float(ref.round_dtype(t, dt)), (dt, t)


def test_scheduled_labeler_follows_the_reference_schedule(g17, capsys):
    from torch_em_amd.self_training import ScheduledPseudoLabeler
    metric = g17["sched_metric"]
    configs = json.loads(str(g17["sched_configs"]))
    assert sorted(configs) == ["dec_abs", "dec_rel", "increase", "no_metric", "warm_up"]
    for name, kw in configs.items():
        labeler = ScheduledPseudoLabeler(**kw)
        seq = []
        for epoch in range(40):
            labeler.step(None if name == "no_metric" else metric[epoch], epoch)
            seq.append(labeler.confidence_threshold)
        want = g17[f"sched_{name}"]
        assert len(set(want)) > 3, name                                # the schedule moved
        assert np.array_equal(np.array(seq, dtype=np.float64), want), (name, seq, want.tolist())   # bit-equal doubles
    out = capsys.readouterr().out
    assert "ScheduledPseudoLabeler: Increasing confidence_threshold every 2 epochs; until epoch 20" in out
    assert "End of warm-up phase reached: setting confidence threshold to 0.95" in out
    lab = ScheduledPseudoLabeler(confidence_threshold=0.9, patience=0, verbose=True)
    lab.step(1.0, 1)
    lab.step(1.0, 2)
    assert "Epoch 2: reducing confidence threshold from 0.9 to 0.85" in capsys.readouterr().out


def test_scheduled_labeler_constructor_errors():
    from torch_em_amd.self_training import DefaultPseudoLabeler, ScheduledPseudoLabeler
    with pytest.raises(ValueError, match="Invalid mode"):
        ScheduledPseudoLabeler(mode="best")
    with pytest.raises(AssertionError, match="Factor must be smaller than 1"):
        ScheduledPseudoLabeler(factor=1.5)
    with pytest.raises(ValueError, match="Invalid threshold mode"):
        ScheduledPseudoLabeler(threshold_mode="ratio")
    with pytest.raises(ValueError, match="warm_up_epochs > 0 is only supported when increase=False"):
        ScheduledPseudoLabeler(increase=True, last_step_epoch=10, warm_up_epochs=2)
    with pytest.raises(NotImplementedError, match="mask_channel"):
        ScheduledPseudoLabeler(mask_channel=0)
    lab = ScheduledPseudoLabeler(confidence_threshold=0.8, threshold_from_both_sides=False)
    assert lab.init_kwargs == {"activation": None, "confidence_threshold": 0.8, "threshold_from_both_sides": False,
                               "mask_channel": None}
    lab = DefaultPseudoLabeler(activation=torch.nn.Sigmoid(), confidence_threshold=0.7, mask_channel=1)
    assert lab.init_kwargs == {"activation": None, "confidence_threshold": 0.7, "threshold_from_both_sides": True,
                               "mask_channel": 1}
    assert lab.step(0.5, 3) is None and lab.confidence_threshold == 0.7


def test_cpu_tensors_raise():
    from torch_em_amd import ops
    from torch_em_amd.self_training import DefaultPseudoLabeler, DefaultSelfTrainingLoss
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        DefaultPseudoLabeler(confidence_threshold=0.9)(lambda inp: inp, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dice_sums_pair(x, x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        DefaultSelfTrainingLoss()(lambda inp: inp, x, x, x)


# ---- host logic of the trainer ----------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """direct children with and without reset_parameters, and a nested one that must stay untouched"""
    init_kwargs = {}

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 1))
        self.out_conv = torch.nn.Conv2d(2, 1, 1)

    def forward(self, x):
        return self.out_conv(self.body(x))


def _loader(n):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.zeros(n, 1, 4, 4), torch.zeros(n, 1, 4, 4)), batch_size=1)


def _trainer(tmp_path, **kw):
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            MeanTeacherTrainer)
    model = _Stub()
    args = dict(name="mt", model=model, optimizer=torch.optim.AdamW(model.parameters()), pseudo_labeler=DefaultPseudoLabeler(),
                unsupervised_loss=DefaultSelfTrainingLoss(), unsupervised_loss_and_metric=DefaultSelfTrainingLossAndMetric(),
                device="cpu", mixed_precision=False, save_root=str(tmp_path))
    args.update(kw)
    return MeanTeacherTrainer(**args)


def test_trainer_selects_loaders_like_the_reference(tmp_path):
    from torch_em_amd.self_training import DefaultSelfTrainingLoss
    u5, u3, s4, v2, sv2 = _loader(5), _loader(3), _loader(4), _loader(2), _loader(2)
    t = _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2)
    assert t.train_loader is u5 and t._train_epoch_impl == t._train_epoch_unsupervised
    assert t.val_loader is u5              # the reference takes the unsupervised TRAIN loader here (:117-120)
    assert t.reinit_teacher is False and t.logger_class is None and t.hip_graph is False
    t = _trainer(tmp_path, unsupervised_train_loader=u5, supervised_train_loader=s4, supervised_val_loader=sv2,
                 supervised_loss=DefaultSelfTrainingLoss())
    assert t.train_loader is s4 and t.val_loader is sv2 and t._train_epoch_impl == t._train_epoch_semisupervised
    assert t.reinit_teacher is True
    t = _trainer(tmp_path, unsupervised_train_loader=u3, supervised_train_loader=s4, supervised_val_loader=sv2,
                 supervised_loss=DefaultSelfTrainingLoss(), reinit_teacher=False)
    assert t.train_loader is u3 and t.reinit_teacher is False
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5)                                            # no validation loader
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5, supervised_train_loader=s4, supervised_val_loader=sv2)   # no supervised loss
    with pytest.raises(AssertionError):
        _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2, unsupervised_loss_and_metric=None)
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _trainer(tmp_path, unsupervised_train_loader=u5, unsupervised_val_loader=v2, hip_graph=True)


def test_teacher_initialisation_and_momentum_ramp(tmp_path):
    from torch_em_amd.self_training import DefaultSelfTrainingLoss
    t = _trainer(tmp_path, unsupervised_train_loader=_loader(3), unsupervised_val_loader=_loader(1), momentum=0.9)
    assert all(torch.equal(a, b) for a, b in zip(t.model.parameters(), t.teacher.parameters()))
    assert not any(p.requires_grad for p in t.teacher.parameters()) and all(p.requires_grad for p in t.model.parameters())
    for it in range(6):
        t._iteration = it
        assert t._current_momentum() == 0.9
    t = _trainer(tmp_path, unsupervised_train_loader=_loader(3), supervised_train_loader=_loader(3), supervised_val_loader=_loader(1),
                 supervised_loss=DefaultSelfTrainingLoss(), momentum=0.8)
    # only direct children with reset_parameters are reinitialised: out_conv, not the conv inside `body`
    assert torch.equal(t.model.body[0].weight, t.teacher.body[0].weight)
    assert not torch.equal(t.model.out_conv.weight, t.teacher.out_conv.weight)
    got = []
    for it in range(6):
        t._iteration = it
        got.append(t._current_momentum())
    assert got == [0.0, 0.5, 1 - 1 / 3, 0.75, 0.8, 0.8]
    t._iteration = 0
    with pytest.raises(RuntimeError, match="MI355X only"):
        t._momentum_update()


def test_checkpoint_has_the_reference_keys(tmp_path, g17):
    t = _trainer(tmp_path, unsupervised_train_loader=_loader(3), unsupervised_val_loader=_loader(1))
    t._initialize(3, None)
    t.save_checkpoint("latest", 0.5, 0.5)
    ckpt = torch.load(os.path.join(t.checkpoint_folder, "latest.pt"), weights_only=False)
    assert set(g17["mt_a_ckpt_keys"]) - {"scheduler_state", "scaler_state"} <= set(ckpt), set(g17["mt_a_ckpt_keys"]) - set(ckpt)
    assert sorted(ckpt["teacher_state"]) == sorted(ckpt["model_state"])
    init = ckpt["init"]
    assert str(g17["mt_a_loss_class"]) == "torch_em.self_training.mean_teacher.Dummy"
    assert init["loss_class"] == init["metric_class"] == "torch_em_amd.self_training.mean_teacher.Dummy"
    assert init["loss_kwargs"] == {} and init["metric_kwargs"] == {}
    assert init["trainer_class"] == "torch_em_amd.self_training.mean_teacher.MeanTeacherTrainer"
    assert init["train_dataset"] is not None and init["val_dataset"] is not None
    # the teacher travels through load_checkpoint
    with torch.no_grad():
        for p in t.teacher.parameters():
            p.add_(1.0)
    t.load_checkpoint("latest")
    assert all(torch.equal(a, b) for a, b in zip(t.teacher.state_dict().values(), ckpt["teacher_state"].values()))


def _halve(x):
    return x * 0.5


def _plus_one(y):
    return y + 1.0


def test_from_checkpoint_restores_the_device_pre_pass(tmp_path):
    """The on-device raw / target transforms and `prefetch` of a saved trainer come back through from_checkpoint and
    util.get_trainer; they can be overridden; one that could not be pickled must be passed again (RuntimeError)."""
    from torch_em_amd import util
    from torch_em_amd.self_training import DefaultSelfTrainingLoss, MeanTeacherTrainer
    kw = dict(unsupervised_train_loader=_loader(3), supervised_train_loader=_loader(3), supervised_val_loader=_loader(1),
              supervised_loss=DefaultSelfTrainingLoss())
    t = _trainer(tmp_path, raw_transform=_halve, target_transform=_plus_one, prefetch=False, **kw)
    t._initialize(3, None)
    t.save_checkpoint("latest", 0.5, 0.5)
    for t2 in (MeanTeacherTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu"),
               util.get_trainer(t.checkpoint_folder, name="latest", device="cpu")):
        assert isinstance(t2, MeanTeacherTrainer)
        assert t2.raw_transform is _halve and t2.target_transform is _plus_one and t2.augmentation is None and t2.prefetch is False
        assert len(t2.supervised_train_loader) == 3 and t2.reinit_teacher is True
        x, y = t2._prepass(train=True)(torch.ones(1, 1, 2, 2), torch.ones(1, 1, 2, 2))
        assert float(x.mean()) == 0.5 and float(y.mean()) == 2.0
        # the raw transform reaches the unsupervised views too
        v1, v2 = t2._views((torch.ones(1, 1, 2, 2), 2 * torch.ones(1, 1, 2, 2)))
        assert float(v1.mean()) == 0.5 and float(v2.mean()) == 1.0
    t3 = MeanTeacherTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu", raw_transform=None)
    assert t3.raw_transform is None and t3.target_transform is _plus_one
    with pytest.raises(TypeError, match="unexpected arguments"):
        MeanTeacherTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu", no_such_argument=1)
    # a lambda cannot travel in the checkpoint
    t = _trainer(tmp_path / "lam", raw_transform=lambda x: x * 0.5, **kw)
    with pytest.warns(UserWarning, match="cannot be pickled"):
        t._initialize(3, None)
    t.save_checkpoint("latest", 0.5, 0.5)
    with pytest.raises(RuntimeError, match="raw_transform"):
        MeanTeacherTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu")
    with pytest.raises(RuntimeError, match="raw_transform"):
        util.get_trainer(t.checkpoint_folder, name="latest", device="cpu")
    t4 = MeanTeacherTrainer.from_checkpoint(t.checkpoint_folder, name="latest", device="cpu", raw_transform=_halve)
    assert t4.raw_transform is _halve
