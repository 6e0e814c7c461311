"""G18: golden vectors for FixMatch self-training, made by RUNNING THE REFERENCE (build container only; CPU).

    cd /tmp/somewhere && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen_golden_fixmatch.py

(from a scratch directory, as gen_golden_selftrain.py; the reference is imported through `import_reference` of
gen_golden_trainer.py and its tensorboard import is met by the stand-in module of gen_golden_selftrain.py.)

  da_*  `FixMatchTrainer.get_distribution_alignment` (reference self_training/fix_match.py:164-181), called on a stand-in
        object that carries only `source_distribution`, on fp32 / fp16 / bf16 CPU tensors of two shapes, for three source
        distributions and label thresholds 0.5 and 0.3.  The inputs are seeded rand^2 values with these written in: the
        threshold and its two neighbours in that dtype, 0, 1, -0.25, 1.5 and a value below 1 whose product exceeds 1.  Plus
        single-class tensors (all 0.2, all 0.9) and one fp32 case with a NaN.  No -0.0 and no infinities.  `da_index` lists
        the cases (JSON: output key, input key, dtype, source, threshold); 16-bit tensors are stored as their bit patterns
        (int16; tests/fixmatch_ref.py: `da_array` widens them).
  fm_*  `FixMatchTrainer.fit(iterations=6)` on the CPU with the model, head gain and learning rate of G17 (UNet2d(1, 1,
        depth=2, initial_features=4, sigmoid), batch 2, 32 x 32): (a) unsupervised without threshold and without source
        distribution, (b) unsupervised with threshold 0.7 and source [0.7, 0.3], (c) semi-supervised with threshold 0.7 and
        source [0.6, 0.4].  Per run: logged losses, keep share, validation metric and loss, checkpoint keys, final state and
        the student's state BEFORE every iteration.  A state is one float32 vector (`fm_state_keys` / `fm_state_shapes`:
        the state dict's order); `fm_pre0` is the state before the first iteration, the same for all runs, and row i of
        `fm_<run>_chain` is the int32 difference of the BIT PATTERNS of the states after and before iteration i (exact, and
        it compresses to half of what the states take; tests/fixmatch_ref.py: `fm_states` adds them up).  The data is
        G17's (tests/golden/g17_selftrain.npz: mt_xu1 ...), not stored a second time.
        `fm_<run>_scatter_<series>`: the run is repeated three times with the initial parameters multiplied by
        1 + 1e-4 * randn; the worst relative deviation of the score (1 - value) over the series is what the reference itself
        moves by under a perturbation of the size of fp32 kernel differences -- labels crossing 0.5 or a threshold and Adam's
        sign-like first steps make the trajectory jump, so it does not shrink with the perturbation.

Asserted here, so that the tests' margins are valid: every logged loss exceeds 0.02; the keep share of (b) and (c) is inside
(0.05, 0.95); on every training batch of (b) and (c), evaluated at the stored pre-iteration state, no pre-alignment label is
within 1e-5 of 0.5, 0.7 or 0.3 (G17's data seed, 21, meets it).
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
from gen_golden_selftrain import MT_HEAD_GAIN, MT_LR, Recorder, loader, mt_data, neighbours  # noqa: E402
from gen_golden_trainer import import_reference  # noqa: E402

FIXTURE = os.path.join(HERE, "g18_fixmatch.npz")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DA_SHAPES = ((2, 1, 5, 7, 9), (1, 2, 33, 31))
DA_SOURCES = ((0.7, 0.3), (0.2, 0.8), (0.5, 0.5))
DA_THRESHOLDS = (0.5, 0.3)

FM_THRESHOLD = 0.7
FM_RUNS = {"a": dict(threshold=None, semi=False, source=None),
           "b": dict(threshold=FM_THRESHOLD, semi=False, source=[0.7, 0.3]),
           "c": dict(threshold=FM_THRESHOLD, semi=True, source=[0.6, 0.4])}
FM_ITERS, FM_GUARD, FM_SCATTER_EPS, FM_SCATTER_REPEATS = 6, 1e-5, 1e-4, 3
FM_SERIES = ("unsup", "sup", "combined", "val_metric", "val_loss")


# ---- distribution alignment -------------------------------------------------------------------------------------------
def da_input(dtype, shape, threshold, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(*shape, generator=g) ** 2).to(dtype)
    special = torch.cat([neighbours(threshold, dtype), torch.tensor([0.0, 1.0, -0.25, 1.5, 0.995])]).to(dtype)
    flat = x.view(-1)
    flat[3:3 + special.numel()] = special
    flat[-special.numel():] = special.flip(0)
    return x


def da_call(fm, x, source, threshold):
    stand_in = types.SimpleNamespace(source_distribution=torch.FloatTensor(list(source)))
    out = fm.FixMatchTrainer.get_distribution_alignment(stand_in, x, label_threshold=threshold)
    assert out.dtype == x.dtype and out.shape == x.shape
    return out


def gen_alignment(fm, out):
    index, wide = [], {}

    def store(key, t):   # fp32 as it is, 16-bit types as their bit patterns
        out[key] = t.numpy() if t.dtype == torch.float32 else t.view(torch.int16).numpy()
        wide[key] = t.float().numpy()

    def add(key, xkey, dt, x, source, threshold):
        if xkey not in out:
            store(xkey, x)
        store(key, da_call(fm, x, source, threshold))
        index.append(dict(key=key, x=xkey, dtype=dt, source=list(source), threshold=threshold))

    for dt, dtype in DTYPES.items():
        for si, shape in enumerate(DA_SHAPES):
            for ti, threshold in enumerate(DA_THRESHOLDS):
                x = da_input(dtype, shape, threshold, seed=18 + 10 * si + ti)
                for ki, source in enumerate(DA_SOURCES):
                    add(f"da_{dt}_s{si}_t{ti}_k{ki}", f"da_{dt}_s{si}_t{ti}_x", dt, x, source, threshold)
        for name, value in (("low", 0.2), ("high", 0.9)):   # one class only: unique() returns one count, the ratio is source / 1
            add(f"da_{dt}_single_{name}", f"da_{dt}_single_{name}_x", dt, torch.full(DA_SHAPES[0], value).to(dtype), (0.7, 0.3), 0.5)
    x = da_input(torch.float32, DA_SHAPES[0], 0.5, seed=99)
    x.view(-1)[100] = float("nan")
    add("da_f32_nan", "da_f32_nan_x", "f32", x, (0.7, 0.3), 0.5)
    for rec in index:
        for a in (wide[rec["key"]], wide[rec["x"]]):
            assert not np.isinf(a).any() and not (np.signbit(a) & (a == 0)).any()
        y = wide[rec["key"]]
        assert np.nanmin(y) >= 0 and np.nanmax(y) <= 1
    assert sum(int((wide[r["key"]] == 1).any()) for r in index) > len(index) // 2   # products above 1 meet the clip
    assert np.isnan(wide["da_f32_nan"]).sum() == 1
    out["da_index"] = np.array(json.dumps(index))
    print("da: cases", len(index))


# ---- trainer runs ---------------------------------------------------------------------------------------------------------
class StateRecorder(Recorder):
    """... and the student's state after every training step: the state BEFORE the next one"""
    states = None

    def __init__(self, trainer, save_root, **unused):
        super().__init__(trainer, save_root, **unused)
        self.trainer = trainer
        StateRecorder.states = []

    def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
        super().log_train_unsupervised(step, loss, x1, x2, pred, pseudo_labels, label_filter)
        StateRecorder.states.append({k: v.detach().clone() for k, v in self.trainer.model.state_dict().items()})


def fresh_model(UNet2d, perturb_seed=None):
    torch.manual_seed(0)
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    with torch.no_grad():
        model.out_conv.weight.mul_(MT_HEAD_GAIN)
        if perturb_seed is not None:
            g = torch.Generator().manual_seed(perturb_seed)
            for p in model.parameters():
                p.mul_(1 + FM_SCATTER_EPS * torch.randn(p.shape, generator=g))
    return model


def run(st, fm, UNet2d, data, tag, cfg, tmp, perturb_seed=None):
    """-> (log, states before each iteration, checkpoint)"""
    model = fresh_model(UNet2d, perturb_seed)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if cfg["semi"]:
        kw = dict(supervised_train_loader=loader(data["xs"], data["ys"]), supervised_val_loader=loader(data["xsv"], data["ysv"]),
                  supervised_loss=st.DefaultSelfTrainingLoss(), supervised_loss_and_metric=st.DefaultSelfTrainingLossAndMetric())
    else:
        kw = dict(unsupervised_val_loader=loader(data["xv1"], data["xv2"]),
                  unsupervised_loss_and_metric=st.DefaultSelfTrainingLossAndMetric())
    name = f"g18{tag}" + ("" if perturb_seed is None else f"p{perturb_seed}")
    trainer = fm.FixMatchTrainer(
        name=name, model=model, optimizer=torch.optim.AdamW(model.parameters(), lr=MT_LR),
        pseudo_labeler=st.DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]),
        unsupervised_loss=st.DefaultSelfTrainingLoss(), unsupervised_train_loader=loader(data["xu1"], data["xu2"]),
        source_distribution=cfg["source"], logger=StateRecorder, mixed_precision=False, device=torch.device("cpu"),
        compile_model=False, save_root=tmp, **kw)
    trainer.fit(iterations=FM_ITERS)
    log, states = Recorder.log, [sd0] + StateRecorder.states
    assert len(log["unsup"]) == FM_ITERS and trainer.iteration == FM_ITERS and len(states) == FM_ITERS + 1
    ckpt = torch.load(os.path.join(tmp, "checkpoints", name, "latest.pt"), weights_only=False)
    return log, states, ckpt


def flat_bits(state):
    """a state dict as the int32 bit patterns of one float32 vector (the state dict's order)"""
    return np.concatenate([v.detach().float().numpy().reshape(-1) for v in state.values()]).view(np.int32)


def guard_distance(UNet2d, data, states):
    """smallest distance of a pre-alignment label from 0.5, 0.7 and 0.3 over the training batches, each at the state the
    reference had before that iteration (train mode, as the labeler runs the model)"""
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    model.train()
    worst = 1.0
    for i in range(FM_ITERS):
        model.load_state_dict(states[i])
        with torch.no_grad():
            labels = model(data["xu1"][2 * i:2 * i + 2])
        for t in (0.5, FM_THRESHOLD, 1.0 - FM_THRESHOLD):
            worst = min(worst, float((labels.double() - t).abs().min()))
    return worst


def score_deviation(a, b):
    a, b = 1.0 - np.asarray(a, dtype=np.float64), 1.0 - np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(a))) if a.size else 0.0


def gen_trainer_runs(st, fm, out, tmp):
    from torch_em.model import UNet2d
    data = mt_data()   # G17's data (tests/golden/g17_selftrain.npz: mt_xu1 ...), not stored a second time
    runs = {tag: run(st, fm, UNet2d, data, tag, cfg, tmp) for tag, cfg in FM_RUNS.items()}
    dist = {tag: guard_distance(UNet2d, data, runs[tag][1]) for tag in ("b", "c")}
    print("guard distances", dist)
    assert min(dist.values()) > FM_GUARD, dist
    out["fm_guard"] = np.float64(min(dist.values()))
    out["fm_lr"], out["fm_runs"] = np.float64(MT_LR), np.array(json.dumps(FM_RUNS))
    for tag, cfg in FM_RUNS.items():
        log, states, ckpt = runs[tag]
        for k in ("unsup", "sup", "combined"):
            assert all(v > 0.02 for v in log[k]), (tag, k, log[k])
        if cfg["threshold"] is not None:
            assert all(0.05 < k < 0.95 for k in log["keep"]), log["keep"]
        assert (len(log["ct"]) == FM_ITERS) == (cfg["threshold"] is not None)
        assert "teacher_state" not in ckpt
        for k, v in ckpt["model_state"].items():
            assert torch.equal(v, states[FM_ITERS][k]) and v.dtype == torch.float32
        bits = [flat_bits(sd) for sd in states]
        if "fm_pre0" not in out:
            out["fm_pre0"] = bits[0].view(np.float32).copy()
            out["fm_state_keys"] = np.array(json.dumps(list(states[0].keys())))
            out["fm_state_shapes"] = np.array(json.dumps([list(v.shape) for v in states[0].values()]))
        assert np.array_equal(out["fm_pre0"].view(np.int32), bits[0])
        out[f"fm_{tag}_chain"] = np.stack([bits[i + 1] - bits[i] for i in range(FM_ITERS)])   # int32, wraps: exact
        for k in FM_SERIES + ("keep",):
            out[f"fm_{tag}_{k}"] = np.array(log[k], dtype=np.float64)
        out[f"fm_{tag}_ckpt_keys"] = np.array(sorted(ckpt.keys()))
        out[f"fm_{tag}_init_keys"] = np.array(sorted(ckpt["init"].keys()))
        out[f"fm_{tag}_loss_class"] = np.array(ckpt["init"]["loss_class"])
        scatter = {k: 0.0 for k in FM_SERIES}
        for rep in range(FM_SCATTER_REPEATS):
            plog, _, _ = run(st, fm, UNet2d, data, tag, cfg, tmp, perturb_seed=100 + rep)
            for k in FM_SERIES:
                scatter[k] = max(scatter[k], score_deviation(log[k], plog[k]))
        for k in FM_SERIES:
            out[f"fm_{tag}_scatter_{k}"] = np.float64(scatter[k])
        print("fm", tag, "unsup", [f"{v:.5f}" for v in log["unsup"]], "sup", [f"{v:.5f}" for v in log["sup"]],
              "keep", [f"{v:.3f}" for v in log["keep"]], "val", log["val_metric"], log["val_loss"],
              "scatter", {k: f"{v:.1e}" for k, v in scatter.items()})


if __name__ == "__main__":
    torch.set_num_threads(4)
    torch.use_deterministic_algorithms(True)
    stand_in = types.ModuleType("torch.utils.tensorboard")
    stand_in.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = stand_in
    torch_em = import_reference()
    import torch_em.self_training as st
    import torch_em.self_training.fix_match as fm
    out = {}
    gen_alignment(fm, out)
    with tempfile.TemporaryDirectory() as tmp:
        gen_trainer_runs(st, fm, out, tmp)
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
