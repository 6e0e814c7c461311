"""G17: golden vectors for self-training, made by RUNNING THE REFERENCE (build container only; CPU).

    cd /tmp/somewhere && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen_golden_selftrain.py

(from a scratch directory: the reference's trainer writes ./checkpoints when save_root is not honoured by a code path).

  pl_*     `torch_em.self_training.DefaultPseudoLabeler` on fp32 / fp16 / bf16 CPU tensors: no activation or sigmoid, both
           sides or one side, threshold None / 0.9 / 0.6, mask_channel None / 1 (N = 2, C = 3).  The inputs are seeded
           N(0, 2) values with, per dtype, the tie values round(t), round(1 - t) and their two neighbours in that dtype
           written into both samples -- they pin that the compare runs in the tensor's dtype against the rounded threshold.
  sched_*  `ScheduledPseudoLabeler.confidence_threshold` after each of 40 `step(metric, epoch)` calls on a recorded metric
           sequence, for five configurations (constructor kwargs stored as JSON).
  mt_*     `MeanTeacherTrainer.fit(iterations=6)` on the CPU, UNet2d(1, 1, depth=2, initial_features=4, sigmoid), batch 2,
           32 x 32: (a) unsupervised without threshold, (b) unsupervised with threshold 0.7, (c) semi-supervised with
           threshold and reinitialised teacher: data, initial / final student and teacher state, logged losses, validation
           metric, share of voxels the mask keeps.

The reference's self_training/logger.py imports torch.utils.tensorboard, which this image lacks: a stand-in module with a
`SummaryWriter` attribute is placed in sys.modules first.  The fixture holds data only.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_trainer import import_reference  # noqa: E402

FIXTURE = os.path.join(HERE, "g17_selftrain.npz")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
THRESHOLDS = (None, 0.9, 0.6)
PL_SHAPE = (2, 3, 4, 6)

SCHEDULES = {
    "dec_abs": dict(confidence_threshold=0.9, patience=2, factor=0.05, threshold_mode="abs", verbose=False),
    "dec_rel": dict(confidence_threshold=0.9, patience=1, factor=0.07, threshold_mode="rel", mode="max", verbose=False),
    "no_metric": dict(confidence_threshold=0.95, patience=3, factor=0.05, verbose=False),
    "increase": dict(confidence_threshold=0.5, increase=True, last_step_epoch=20, factor=0.05, verbose=False),
    "warm_up": dict(confidence_threshold=0.6, warm_up_epochs=5, patience=1, factor=0.1, verbose=False),
}
SCHEDULE_WITHOUT_METRIC = ("no_metric",)


def neighbours(value: float, dtype):
    """[below, round(value), above] in `dtype`, as a float32 tensor (exact)"""
    v = torch.tensor(value, dtype=torch.float64).to(dtype)
    if dtype == torch.float32:
        return torch.stack([torch.nextafter(v, torch.tensor(-1e9)), v, torch.nextafter(v, torch.tensor(1e9))])
    bits = v.view(torch.int16)   # positive values: the neighbours are the neighbouring bit patterns
    return torch.stack([(bits - 1).view(dtype).float(), v.float(), (bits + 1).view(dtype).float()])


def tie_values(dtype):
    vals = []
    for t in THRESHOLDS[1:]:
        vals += [neighbours(t, dtype), neighbours(1.0 - t, dtype)]
    return torch.cat(vals)   # 12 values


def pl_input(dtype):
    g = torch.Generator().manual_seed(17)
    x = (2.0 * torch.randn(*PL_SHAPE, generator=g)).to(dtype)
    ties = tie_values(dtype).to(dtype)
    x[0, 0, 0:2, :] = ties.view(2, 6)
    x[1, 1, 0:2, :] = ties.flip(0).view(2, 6)
    return x


def pl_key(dt, act, both, t, mc):
    return f"pl_{dt}_{'sigmoid' if act else 'none'}_{'both' if both else 'one'}_{t}_{mc}"


def pl_cases():
    for act in (False, True):
        for both in (True, False):
            for t in THRESHOLDS:
                for mc in ((None,) if t is None else (None, 1)):
                    yield act, both, t, mc


def gen_pseudo_labels(st, out):
    for dt, dtype in DTYPES.items():
        x = pl_input(dtype)
        out[f"pl_{dt}_x"] = x.float().numpy()
        for act, both, t, mc in pl_cases():
            labeler = st.DefaultPseudoLabeler(activation=torch.nn.Sigmoid() if act else None, confidence_threshold=t,
                                              threshold_from_both_sides=both, mask_channel=mc)
            labels, mask = labeler(lambda inp: inp, x)
            assert labels.dtype == dtype
            key = pl_key(dt, act, both, t, mc)
            out[key + "_labels"] = labels.float().numpy()
            if t is None:
                assert mask is None
            else:
                assert mask.dtype == (torch.float32 if both else torch.bool) and mask.shape == x.shape
                out[key + "_mask"] = mask.contiguous().numpy()
    print("pl: cases per dtype", len(list(pl_cases())))


def gen_schedules(st, out):
    rng = np.random.RandomState(5)
    metric = 0.5 + np.cumsum(rng.randn(40) * 0.02) - 0.004 * np.arange(40)   # drifts down with plateaus
    out["sched_metric"] = metric
    out["sched_configs"] = np.array(json.dumps(SCHEDULES))
    for name, kw in SCHEDULES.items():
        labeler = st.ScheduledPseudoLabeler(**kw)
        seq = []
        for epoch in range(40):
            labeler.step(None if name in SCHEDULE_WITHOUT_METRIC else metric[epoch], epoch)
            seq.append(labeler.confidence_threshold)
        out[f"sched_{name}"] = np.array(seq, dtype=np.float64)
        print("sched", name, sorted(set(seq), reverse=True))


class Recorder:
    """Stands in for SelfTrainingTensorboardLogger: same constructor / method names, keeps the scalars."""
    log = None

    def __init__(self, trainer, save_root, **unused):
        Recorder.log = {"unsup": [], "sup": [], "combined": [], "keep": [], "val_metric": [], "val_loss": [], "ct": []}

    def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
        Recorder.log["unsup"].append(float(loss.item()))
        Recorder.log["keep"].append(1.0 if label_filter is None else float(label_filter.float().mean()))

    def log_train_supervised(self, step, loss, x, y, pred):
        Recorder.log["sup"].append(float(loss.item()))

    def log_combined_loss(self, step, loss):
        Recorder.log["combined"].append(float(loss.item()))

    def log_lr(self, step, lr):
        pass

    def log_ct(self, step, ct):
        Recorder.log["ct"].append(float(ct))

    def log_validation_unsupervised(self, step, metric, loss, x1, x2, pred, pseudo_labels, label_filter=None):
        Recorder.log["val_metric"].append(float(metric))
        Recorder.log["val_loss"].append(float(loss))

    def log_validation_supervised(self, step, metric, loss, x, y, pred):
        Recorder.log["val_metric"].append(float(metric))
        Recorder.log["val_loss"].append(float(loss))


MT_THRESHOLD = 0.7
MT_RUNS = {"a": dict(threshold=None, semi=False, momentum=0.9),
           "b": dict(threshold=MT_THRESHOLD, semi=False, momentum=0.9),
           "c": dict(threshold=MT_THRESHOLD, semi=True, momentum=0.999)}
MT_LR, MT_ITERS, MT_PAIR_NOISE = 1e-3, 6, 0.5
# the output convolution of the fresh model is scaled up: with the default initialisation the sigmoid outputs stay within a few
# per cent of 0.5 and the Dice loss between the two views is below 1e-2 even at pair noise 0.5
MT_HEAD_GAIN = 6.0


def mt_data():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(16, 1, 32, 32, generator=g)
    x2 = x + MT_PAIR_NOISE * torch.randn(16, 1, 32, 32, generator=g)
    xs = torch.randn(16, 1, 32, 32, generator=g)
    ys = (torch.rand(16, 1, 32, 32, generator=g) > 0.5).float()
    # 12 training samples (6 iterations at batch size 2), 4 validation samples
    return dict(xu1=x[:12], xu2=x2[:12], xv1=x[12:], xv2=x2[12:], xs=xs[:12], ys=ys[:12], xsv=xs[12:], ysv=ys[12:])


def loader(*tensors):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(*tensors), batch_size=2, shuffle=False)


def gen_trainer_runs(torch_em, st, out, tmp):
    from torch_em.model import UNet2d
    data = mt_data()
    out.update({f"mt_{k}": v.numpy() for k, v in data.items()})
    out["mt_lr"], out["mt_runs"] = np.float64(MT_LR), np.array(json.dumps(MT_RUNS))
    for tag, cfg in MT_RUNS.items():
        torch.manual_seed(0)
        model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
        with torch.no_grad():
            model.out_conv.weight.mul_(MT_HEAD_GAIN)
        out.update({f"mt_{tag}_sd0.{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()})
        kw = {}
        if cfg["semi"]:
            kw = dict(supervised_train_loader=loader(data["xs"], data["ys"]), supervised_val_loader=loader(data["xsv"], data["ysv"]),
                      supervised_loss=st.DefaultSelfTrainingLoss(), supervised_loss_and_metric=st.DefaultSelfTrainingLossAndMetric())
        else:
            kw = dict(unsupervised_val_loader=loader(data["xv1"], data["xv2"]),
                      unsupervised_loss_and_metric=st.DefaultSelfTrainingLossAndMetric())
        trainer = st.MeanTeacherTrainer(
            name="g17" + tag, model=model, optimizer=torch.optim.AdamW(model.parameters(), lr=MT_LR),
            pseudo_labeler=st.DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]),
            unsupervised_loss=st.DefaultSelfTrainingLoss(), unsupervised_train_loader=loader(data["xu1"], data["xu2"]),
            momentum=cfg["momentum"], logger=Recorder, mixed_precision=False, device=torch.device("cpu"),
            compile_model=False, save_root=tmp, **kw)
        assert trainer.reinit_teacher == cfg["semi"]
        if trainer.reinit_teacher:   # the teacher's reinitialised head gets the student's gain (see MT_HEAD_GAIN)
            with torch.no_grad():
                trainer.teacher.out_conv.weight.mul_(MT_HEAD_GAIN)
        out.update({f"mt_{tag}_teacher_sd0.{k}": v.detach().numpy().copy() for k, v in trainer.teacher.state_dict().items()})
        trainer.fit(iterations=MT_ITERS)
        log = Recorder.log
        assert len(log["unsup"]) == MT_ITERS and trainer.iteration == MT_ITERS
        if cfg["threshold"] is None:
            assert min(log["unsup"]) > 0.02, log["unsup"]
        else:
            assert all(0.05 < k < 0.95 for k in log["keep"]), log["keep"]
        ckpt = torch.load(os.path.join(tmp, "checkpoints", "g17" + tag, "latest.pt"), weights_only=False)
        out.update({f"mt_{tag}_sd1.{k}": v.detach().numpy().copy() for k, v in ckpt["model_state"].items()})
        out.update({f"mt_{tag}_teacher_sd1.{k}": v.detach().numpy().copy() for k, v in ckpt["teacher_state"].items()})
        for k in ("unsup", "sup", "combined", "keep", "val_metric", "val_loss"):
            out[f"mt_{tag}_{k}"] = np.array(log[k], dtype=np.float64)
        out[f"mt_{tag}_ckpt_keys"] = np.array(sorted(ckpt.keys()))
        out[f"mt_{tag}_loss_class"] = np.array(ckpt["init"]["loss_class"])
        print("mt", tag, "unsup", [f"{v:.5f}" for v in log["unsup"]], "sup", [f"{v:.5f}" for v in log["sup"]],
              "keep", [f"{v:.2f}" for v in log["keep"]], "val", log["val_metric"])


if __name__ == "__main__":
    torch.set_num_threads(4)
    torch.use_deterministic_algorithms(True)
    stand_in = types.ModuleType("torch.utils.tensorboard")
    stand_in.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = stand_in
    torch_em = import_reference()
    import torch_em.self_training as st
    out = {}
    gen_pseudo_labels(st, out)
    gen_schedules(st, out)
    with tempfile.TemporaryDirectory() as tmp:
        gen_trainer_runs(torch_em, st, out, tmp)
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
