"""G19: golden vectors for self-training with invertible augmentations, made by RUNNING THE REFERENCE (build container only; CPU).

    cd /tmp/somewhere && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen_golden_invertible.py

(from a scratch directory, as gen_golden_fixmatch.py; the reference is imported through `import_reference` of
gen_golden_trainer.py -- which also meets its kornia import with a stub -- and its tensorboard import by the stand-in module of
gen_golden_selftrain.py.)

The reference's augmenters are built on kornia, which is not available: the augmenter handed to the reference is the torch-only
stand-in below (`ReplayAugmenter`: per sample `flip(-1)` if h, `flip(-2)` if v, `torch.rot90(., k, (-2, -1))`, from a recorded
list; no intensity part).  The recorded (h, v, k) and the codes they compose to are in the fixture (`ia_<run>_hvk`: [view,
call, sample, 3]; `ia_<run>_codes`: [view, call, sample]; views in the order `ia_<run>_views`).  A "call" is one batch, training
batches first, then the batches of the unsupervised validation.

  loss_*  direct calls of the reference's `SelfTrainingLossWithInvertibleAugmentations`,
          `SelfTrainingLossAndMetricWithInvertibleAugmentations`, `UniMatchv2Loss` and `UniMatchv2LossAndMetric` (default
          DiceLoss inside) on small tensors: `pred_dim` 1 and 2, with and without a label filter (`loss_index`: JSON).
  ia_*    six iterations each, with the model, data (G17's, 32 x 32, batch 2; the unsupervised loaders yield the raw batch
          `mt_xu1` / `mt_xv1`), head gain and learning rate of G17:
            (a) MeanTeacherTrainerWithInvertibleAugmentations, unsupervised, threshold 0.7, momentum 0.9
            (b) FixMatchTrainerWithInvertibleAugmentations, semi-supervised, threshold 0.7, source distribution [0.6, 0.4]
            (c) UniMatchv2Trainer, unsupervised, no threshold, momentum 0.9
            (d) UniMatchv2Trainer, semi-supervised, threshold 0.7, momentum 0.999, reinitialised teacher (head gain applied)
          Per run, in G18's compressed form: logged series, keep share, validation metric and loss, checkpoint keys, and the
          student's state after EVERY optimizer step as int32 differences of bit patterns from `ia_pre0` (`ia_<run>_chain`;
          run (d) takes two optimizer steps per iteration, so it has twelve rows: the state the unsupervised half of iteration
          i saw is row 2 i).  For the runs with a teacher: `ia_<run>_teacher0`, the teacher before the first iteration;
          the teachers before the later ones follow from the chain by the reference's update (`ema_teachers`, asserted
          here to give the recorded teachers and the checkpoint's bit for bit).  `ia_<run>_scatter_<series>` as in G18: three repeats from
          initial parameters multiplied by 1 + 1e-4 * randn, worst relative deviation of the score.
          The reference's unsupervised UniMatch loop never clears the gradients, so run (c) applies the gradients summed
          since the start of training; the run is the reference as it is.

Asserted here, so that the tests' margins are valid: every run's codes contain 3 and 5; every run has a batch whose two
samples have different codes in some view; the views' codes differ from one another in every batch; every logged loss exceeds
0.02; the keep share is inside (0.05, 0.95) where there is a threshold; at every stored pre-iteration state no label the
labeler computes is within 1e-5 of 0.7 or 0.3 (and of 0.5 where labels are aligned).  The code seed is the first of 0, 1, 2, ...
that meets all of it; it is printed and stored (`ia_code_seed`).
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
from gen_golden_fixmatch import flat_bits, fresh_model, score_deviation  # noqa: E402
from gen_golden_selftrain import MT_HEAD_GAIN, MT_LR, Recorder, mt_data  # noqa: E402
from gen_golden_trainer import import_reference  # noqa: E402

FIXTURE = os.path.join(HERE, "g19_invertible.npz")
IA_THRESHOLD = 0.7
IA_RUNS = {"a": dict(trainer="mean_teacher", threshold=IA_THRESHOLD, semi=False, momentum=0.9, source=None),
           "b": dict(trainer="fix_match", threshold=IA_THRESHOLD, semi=True, momentum=None, source=[0.6, 0.4]),
           "c": dict(trainer="uni_match", threshold=None, semi=False, momentum=0.9, source=None),
           "d": dict(trainer="uni_match", threshold=IA_THRESHOLD, semi=True, momentum=0.999, source=None)}
IA_VIEWS = {"mean_teacher": ("teacher", "student"), "fix_match": ("teacher", "student"), "uni_match": ("weak", "strong1", "strong2")}
IA_ITERS, IA_CALLS, IA_GUARD, IA_SCATTER_REPEATS = 6, 8, 1e-5, 3
IA_SERIES = ("unsup", "sup", "combined", "val_metric", "val_loss")
# (h, v) -> code for k = -1, 0, 1, 2 (checked against flip / rot90 by tests/test_invertible_cpu.py)
CODE_TABLE = {(0, 0): (3, 0, 5, 6), (0, 1): (1, 2, 7, 4), (1, 0): (7, 4, 1, 2), (1, 1): (5, 6, 3, 0)}


def code_of(h, v, k):
    return CODE_TABLE[(int(h), int(v))][int(k) + 1]


class ReplayAugmenter:
    """Stands in for the reference's `InvertibleAugmenter`: `reset` / `transform` / `reverse_transform`, geometric part only,
    the (h, v, k) of each call read from a list."""

    def __init__(self, hvk):
        self.hvk, self.call, self.params = hvk, 0, None

    def reset(self):
        self.params = None

    def transform(self, x):
        self.params = self.hvk[self.call]
        self.call += 1
        assert len(self.params) == x.shape[0]
        out = []
        for sample, (h, v, k) in zip(x, self.params):
            if h:
                sample = sample.flip(-1)
            if v:
                sample = sample.flip(-2)
            out.append(torch.rot90(sample, int(k), (-2, -1)))
        return torch.stack(out)

    def reverse_transform(self, x):
        out = []
        for sample, (h, v, k) in zip(x, self.params):
            sample = torch.rot90(sample, -int(k), (-2, -1))
            if v:
                sample = sample.flip(-2)
            if h:
                sample = sample.flip(-1)
            out.append(sample)
        return torch.stack(out)


class ReplayAugmenters:
    def __init__(self, views, hvk):
        self.views = views
        for name, seq in zip(views, hvk):
            setattr(self, name, ReplayAugmenter(seq))

    def reset_all(self):
        for name in self.views:
            getattr(self, name).reset()


def draw_codes(seed, n_views):
    """-> hvk [view, call, sample, 3] or None when the structural conditions fail"""
    rng = np.random.RandomState(seed)
    hvk = np.stack([rng.randint(0, 2, (n_views, IA_CALLS, 2)), rng.randint(0, 2, (n_views, IA_CALLS, 2)),
                    rng.randint(-1, 3, (n_views, IA_CALLS, 2))], axis=-1)
    codes = np.vectorize(code_of)(hvk[..., 0], hvk[..., 1], hvk[..., 2])
    train = codes[:, :IA_ITERS]
    ok = 3 in train and 5 in train and bool((train[..., 0] != train[..., 1]).any())
    for a in range(n_views):
        for b in range(a + 1, n_views):
            ok = ok and all(not np.array_equal(codes[a, c], codes[b, c]) for c in range(IA_CALLS))
    return (hvk, codes) if ok else None


class RawBatches(torch.utils.data.Dataset):
    """yields the bare tensor (a TensorDataset would yield a one-element list, which the reference's loops do not unpack)"""

    def __init__(self, x):
        self.x = x

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


def raw_loader(x):
    return torch.utils.data.DataLoader(RawBatches(x), batch_size=2, shuffle=False)


def pair_loader(x, y):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=2, shuffle=False)


class StateRecorder(Recorder):
    """... and the teacher as it is when a training step is logged: after the student's update, before its own"""
    teachers = None

    def __init__(self, trainer, save_root, **unused):
        super().__init__(trainer, save_root, **unused)
        self.trainer = trainer
        StateRecorder.teachers = []

    def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
        super().log_train_unsupervised(step, loss, x1, x2, pred, pseudo_labels, label_filter)
        if hasattr(self.trainer, "teacher"):
            StateRecorder.teachers.append({k: v.detach().clone() for k, v in self.trainer.teacher.state_dict().items()})

    def log_train_augmentations(self, *args):
        pass

    def log_validation_augmentations(self, *args):
        pass


def run(ref, UNet2d, data, tag, cfg, hvk, tmp, perturb_seed=None):
    """-> (log, student states after every optimizer step (initial first), teachers before every iteration, checkpoint)"""
    lo = ref["loss"]
    model = fresh_model(UNet2d, perturb_seed)
    states = [{k: v.detach().clone() for k, v in model.state_dict().items()}]
    optimizer = torch.optim.AdamW(model.parameters(), lr=MT_LR)
    optimizer.register_step_post_hook(lambda *a: states.append({k: v.detach().clone() for k, v in model.state_dict().items()}))
    uni = cfg["trainer"] == "uni_match"
    loss_cls, lam_cls = (lo.UniMatchv2Loss, lo.UniMatchv2LossAndMetric) if uni else \
        (lo.SelfTrainingLossWithInvertibleAugmentations, lo.SelfTrainingLossAndMetricWithInvertibleAugmentations)
    if cfg["semi"]:
        kw = dict(supervised_train_loader=pair_loader(data["xs"], data["ys"]), supervised_val_loader=pair_loader(data["xsv"], data["ysv"]),
                  supervised_loss=lo.SelfTrainingLossWithInvertibleAugmentations(),
                  supervised_loss_and_metric=lo.SelfTrainingLossAndMetricWithInvertibleAugmentations())
    else:
        kw = dict(unsupervised_val_loader=raw_loader(data["xv1"]), unsupervised_loss_and_metric=lam_cls())
    if cfg["trainer"] == "fix_match":
        kw["source_distribution"] = cfg["source"]
    else:
        kw["momentum"] = cfg["momentum"]
    if uni:
        kw["complementary_dropout"] = False
    name = f"g19{tag}" + ("" if perturb_seed is None else f"p{perturb_seed}")
    trainer = ref[cfg["trainer"]](
        name=name, model=model, optimizer=optimizer, pseudo_labeler=ref["st"].DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]),
        unsupervised_loss=loss_cls(), unsupervised_train_loader=raw_loader(data["xu1"]),
        augmenter=ReplayAugmenters(IA_VIEWS[cfg["trainer"]], hvk.tolist()), logger=StateRecorder, mixed_precision=False,
        device=torch.device("cpu"), compile_model=False, save_root=tmp, **kw)
    teacher0 = None
    if hasattr(trainer, "teacher"):
        assert trainer.reinit_teacher == cfg["semi"]
        if trainer.reinit_teacher:   # the teacher's reinitialised head gets the student's gain (gen_golden_selftrain.py)
            with torch.no_grad():
                trainer.teacher.out_conv.weight.mul_(MT_HEAD_GAIN)
        teacher0 = {k: v.detach().clone() for k, v in trainer.teacher.state_dict().items()}
        assert uni == (not trainer.teacher.training)
    trainer.fit(iterations=IA_ITERS)
    log = Recorder.log
    steps = 2 if (uni and cfg["semi"]) else 1
    assert len(log["unsup"]) == IA_ITERS and trainer.iteration == IA_ITERS and len(states) == steps * IA_ITERS + 1
    ckpt = torch.load(os.path.join(tmp, "checkpoints", name, "latest.pt"), weights_only=False)
    teachers = None
    if teacher0 is not None:
        teachers = StateRecorder.teachers + [ckpt["teacher_state"]]
        assert len(teachers) == IA_ITERS + 1 and all(torch.equal(teacher0[k], teachers[0][k]) for k in teacher0)
    return log, states, teachers, ckpt


def guard_distance(ref, UNet2d, data, cfg, hvk, states, teachers):
    """smallest distance of a label from the thresholds over the training batches, each at the state the reference had
    before that iteration (the labeling model in the mode the reference runs it in)"""
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    uni, steps = cfg["trainer"] == "uni_match", 2 if (cfg["trainer"] == "uni_match" and cfg["semi"]) else 1
    model.train(not uni)
    aug = ReplayAugmenter(hvk[0].tolist())
    worst = 1.0
    for i in range(IA_ITERS):
        model.load_state_dict(states[steps * i] if teachers is None else teachers[i])
        with torch.no_grad():
            labels = model(aug.transform(data["xu1"][2 * i:2 * i + 2]))
        for t in (IA_THRESHOLD, 1.0 - IA_THRESHOLD) + ((0.5,) if cfg["source"] else ()):
            worst = min(worst, float((labels.double() - t).abs().min()))
    return worst


def attempt(ref, UNet2d, data, seed, tmp):
    """all four runs with the codes of `seed` -> {tag: (hvk, codes, log, states, teachers, ckpt)} or None"""
    result = {}
    for tag, cfg in IA_RUNS.items():
        drawn = draw_codes(1000 * seed + ord(tag), len(IA_VIEWS[cfg["trainer"]]))
        if drawn is None:
            return None
        hvk, codes = drawn
        log, states, teachers, ckpt = run(ref, UNet2d, data, tag, cfg, hvk, tmp)
        if not all(v > 0.02 for k in ("unsup", "sup", "combined") for v in log[k]):
            print("seed", seed, tag, "a loss is below 0.02", log)
            return None
        if cfg["threshold"] is not None:
            if not all(0.05 < k < 0.95 for k in log["keep"]):
                print("seed", seed, tag, "keep share", log["keep"])
                return None
            dist = guard_distance(ref, UNet2d, data, cfg, hvk, states, teachers)
            if not dist > IA_GUARD:
                print("seed", seed, tag, "guard distance", dist)
                return None
            print("run", tag, "guard distance", dist)
        result[tag] = (hvk, codes, log, states, teachers, ckpt)
    return result


def ema_teachers(teacher0, students_after, momentum, reinit):
    """the teacher before iteration 0, 1, ... and after the last one, from the student after each iteration: the reference's
    update, teacher * m + student * (1 - m) in float32 with m = min(1 - 1 / (iteration + 1), momentum) for a reinitialised
    teacher -- element-wise float32 arithmetic, so recomputing it gives the reference's bits (asserted below); the fixture
    stores `teacher0` only (tests/invaug_ref.py: `ia_teachers` is this function)"""
    teachers = [{k: v.clone() for k, v in teacher0.items()}]
    for i, student in enumerate(students_after):
        m = min(1 - 1 / (i + 1), momentum) if reinit else momentum
        teachers.append({k: teachers[-1][k] * m + student[k] * (1.0 - m) for k in teacher0})
    return teachers


def chain(states):
    bits = [flat_bits(sd) for sd in states]
    return bits[0], np.stack([bits[i + 1] - bits[i] for i in range(len(bits) - 1)])   # int32, wraps: exact


def gen_trainer_runs(ref, out, tmp):
    from torch_em.model import UNet2d
    data = mt_data()   # G17's data (tests/golden/g17_selftrain.npz: mt_xu1 ...), not stored a second time
    for seed in range(200):
        result = attempt(ref, UNet2d, data, seed, tmp)
        if result is not None:
            break
    else:
        raise SystemExit("no code seed meets the conditions")
    print("code seed", seed)
    out["ia_code_seed"], out["ia_guard"] = np.int64(seed), np.float64(IA_GUARD)
    out["ia_lr"], out["ia_runs"] = np.float64(MT_LR), np.array(json.dumps(IA_RUNS))
    for tag, cfg in IA_RUNS.items():
        hvk, codes, log, states, teachers, ckpt = result[tag]
        assert (len(log["ct"]) == IA_ITERS) == (cfg["threshold"] is not None)
        assert ("teacher_state" in ckpt) == (teachers is not None)
        for k, v in ckpt["model_state"].items():
            assert torch.equal(v, states[-1][k]) and v.dtype == torch.float32
        out[f"ia_{tag}_hvk"], out[f"ia_{tag}_codes"] = hvk.astype(np.int8), codes.astype(np.int8)
        out[f"ia_{tag}_views"] = np.array(IA_VIEWS[cfg["trainer"]])
        first, diffs = chain(states)
        if "ia_pre0" not in out:
            out["ia_pre0"] = first.view(np.float32).copy()
            out["ia_state_keys"] = np.array(json.dumps(list(states[0].keys())))
            out["ia_state_shapes"] = np.array(json.dumps([list(v.shape) for v in states[0].values()]))
        assert np.array_equal(out["ia_pre0"].view(np.int32), first)
        out[f"ia_{tag}_chain"] = diffs
        if teachers is not None:
            steps = (len(states) - 1) // IA_ITERS
            again = ema_teachers(teachers[0], [states[steps * (i + 1)] for i in range(IA_ITERS)], cfg["momentum"], cfg["semi"])
            assert all(torch.equal(a[k], b[k]) for a, b in zip(again, teachers) for k in a), "the teachers do not follow from the chain"
            out[f"ia_{tag}_teacher0"] = flat_bits(teachers[0]).view(np.float32).copy()
        for k in IA_SERIES + ("keep",):
            out[f"ia_{tag}_{k}"] = np.array(log[k], dtype=np.float64)
        out[f"ia_{tag}_ckpt_keys"] = np.array(sorted(ckpt.keys()))
        out[f"ia_{tag}_init_keys"] = np.array(sorted(ckpt["init"].keys()))
        scatter = {k: 0.0 for k in IA_SERIES}
        for rep in range(IA_SCATTER_REPEATS):
            plog = run(ref, UNet2d, data, tag, cfg, hvk, tmp, perturb_seed=100 + rep)[0]
            for k in IA_SERIES:
                scatter[k] = max(scatter[k], score_deviation(log[k], plog[k]))
        for k in IA_SERIES:
            out[f"ia_{tag}_scatter_{k}"] = np.float64(scatter[k])
        print("ia", tag, "codes", codes[:, :IA_ITERS].tolist(), "unsup", [f"{v:.5f}" for v in log["unsup"]], "sup", [f"{v:.5f}" for v in log["sup"]],
              "keep", [f"{v:.3f}" for v in log["keep"]], "val", log["val_metric"], log["val_loss"],
              "scatter", {k: f"{v:.1e}" for k, v in scatter.items()})


def gen_losses(lo, out):
    g = torch.Generator().manual_seed(19)
    pred = torch.rand(2, 2, 2, 8, 8, generator=g)      # the stack of two views of [B, C, H, W]
    labels = torch.rand(2, 2, 8, 8, generator=g)
    filt = (torch.rand(2, 2, 8, 8, generator=g) > 0.4).float()
    out["loss_pred"], out["loss_labels"], out["loss_filter"] = pred.numpy(), labels.numpy(), filt.numpy()
    index = []
    for cls in ("SelfTrainingLossWithInvertibleAugmentations", "SelfTrainingLossAndMetricWithInvertibleAugmentations",
                "UniMatchv2Loss", "UniMatchv2LossAndMetric"):
        fn = getattr(lo, cls)()
        for pred_dim in ((1, 2) if cls.startswith("UniMatch") else (None,)):
            for with_filter in (False, True):
                p = pred if pred_dim == 2 else pred[0]
                kw = {} if pred_dim is None else {"pred_dim": pred_dim}
                res = fn(p, labels, filt if with_filter else None, **kw)
                res = [float(v) for v in res] if isinstance(res, tuple) else [float(res)]
                index.append(dict(cls=cls, pred_dim=pred_dim, filter=with_filter, value=res))
    out["loss_index"] = np.array(json.dumps(index))
    print("loss cases", len(index))


if __name__ == "__main__":
    torch.set_num_threads(4)
    torch.use_deterministic_algorithms(True)
    stand_in = types.ModuleType("torch.utils.tensorboard")
    stand_in.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = stand_in
    torch_em = import_reference()
    import torch_em.self_training as st
    import torch_em.self_training.loss as lo
    ref = {"st": st, "loss": lo, "mean_teacher": st.MeanTeacherTrainerWithInvertibleAugmentations,
           "fix_match": st.FixMatchTrainerWithInvertibleAugmentations, "uni_match": st.UniMatchv2Trainer}
    out = {}
    gen_losses(lo, out)
    with tempfile.TemporaryDirectory() as tmp:
        gen_trainer_runs(ref, out, tmp)
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
