"""GPU: FixMatch -- the class count and the distribution alignment (csrc/selftrain.hip) against the numpy oracle
(tests/fixmatch_ref.py, pinned bit for bit to the reference's `get_distribution_alignment` by tests/test_fixmatch_cpu.py) and
against the fixture itself, a `no_grad` forward of a model between two of its gradient forwards, and FixMatchTrainer against
runs of the REFERENCE's trainer (tests/golden/g18_fixmatch.npz, tests/golden/gen_golden_fixmatch.py; the data is G17's).

Alignment results are compared bit for bit: one fp32 product rounded once leaves no room.  No test provokes a device fault:
outputs the test lays out sit between guard zones that must survive, and every extent is that of a dense tensor the test
allocated.
"""
import json
import os

import numpy as np
import pytest
import torch

import fixmatch_ref as ref
from conftest import GOLDEN, check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GUARD = 64      # elements around an output the test lays out (a multiple of 16 bytes in every type)
POISON = -7.0   # the clip never produces it
TWO_ROUNDS = 2048 * 256 * 4 + 4099   # fp32: the capped grid of 2048 blocks x 256 threads x 4 elements runs its loop twice
# name -> shape; every case is seeded rand^2 in the storage type
CASES = {"n1": (1,), "n3": (3,), "n255": (255,), "tail": (1027,), "offset": (1027,), "channels_last": (2, 3, 5, 7, 9),
         "two_rounds": (TWO_ROUNDS,), "ties": (2, 1, 16, 33)}
SOURCES = ((0.7, 0.3), (0.2, 0.8))


@pytest.fixture(scope="module")
def g18():
    return dict(np.load(os.path.join(GOLDEN, "g18_fixmatch.npz")))


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_selftrain.npz")))


def _np32(t):
    return t.detach().float().cpu().numpy()


def _same_bits(got, want):
    """bit for bit, any NaN for a NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _neighbours(value, dtype):
    v = torch.tensor(value, dtype=torch.float64).to(dtype)
    if dtype == torch.float32:
        return torch.stack([torch.nextafter(v, torch.tensor(-1e9)), v, torch.nextafter(v, torch.tensor(1e9))])
    bits = v.view(torch.int16)
    return torch.stack([(bits - 1).view(dtype), v, (bits + 1).view(dtype)])


_INPUTS = {}


def _input(case, dt):
    """-> (device tensor, its values as float32 numpy in STORAGE order); built once per (case, dtype)"""
    key = (case, dt)
    if key not in _INPUTS:
        dtype = DTYPES[dt]
        g = torch.Generator().manual_seed(1800 + list(CASES).index(case))
        x = (torch.rand(CASES[case], generator=g) ** 2).to(dtype)
        if case == "ties":   # the thresholds and their neighbours in that dtype, the clip's bounds and beyond, NaN
            special = torch.cat([_neighbours(0.5, dtype), _neighbours(0.3, dtype),
                                 torch.tensor([0.0, 1.0, -0.25, 1.5, 0.995, float("nan")]).to(dtype)])
            x.view(-1)[5:5 + special.numel()] = special
            x.view(-1)[-special.numel():] = special.flip(0)
        if case == "channels_last":
            x = x.to(DEV).contiguous(memory_format=torch.channels_last_3d)
            assert x.stride(1) == 1
            flat = _np32(x.permute(0, 2, 3, 4, 1)).reshape(-1)
        elif case == "offset":   # a dense view that starts one element into its buffer: the base is not 16-byte aligned
            buf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
            buf[1:].copy_(x)
            flat, x = _np32(x), buf[1:]
            assert x.data_ptr() % 16 != 0
        else:
            x = x.to(DEV)
            flat = _np32(x).reshape(-1)
        _INPUTS[key] = (x, flat)
    return _INPUTS[key]


def _storage_order(t):
    """the values of a dense tensor in the order of its storage, as float32 numpy"""
    if t.dim() == 5 and t.stride(1) == 1 and t.shape[1] > 1:
        return _np32(t.permute(0, 2, 3, 4, 1)).reshape(-1)
    return _np32(t).reshape(-1)


# ---- count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_count_against_numpy(dt):
    from torch_em_amd import _lib, ops
    for case in CASES:
        x, flat = _input(case, dt)
        for threshold in ((0.5, 0.3) if case == "ties" else (0.5,)):
            parts = ops.label_count_partials(x, threshold)
            assert parts.dtype == torch.int64 and parts.is_cuda
            assert parts.numel() == _lib.load().tem_label_count_parts(x.numel(), {"f32": 0, "f16": 1, "bf16": 2}[dt])
            assert int(parts.min()) >= 0      # every block wrote its partial (the buffer comes uncleared)
            assert int(parts.sum()) == ref.count(flat, threshold, dt), (case, threshold)
    x, flat = _input("two_rounds", dt)
    # fp32: the grid is at its cap and the loop runs twice; the 16-bit types take 8 elements per load and fit in one round
    assert ops.label_count_partials(x).numel() == (2048 if dt == "f32" else 1027)
    # the compare runs on the stored value against the ROUNDED threshold: the value equal to it counts, its lower neighbour
    # does not, and NaN is below
    t = _neighbours(0.3, DTYPES[dt]).to(DEV)
    assert int(ops.label_count_partials(t, 0.3).sum()) == 2
    nan = torch.tensor([float("nan"), 0.75, float("nan")], dtype=DTYPES[dt], device=DEV)
    assert int(ops.label_count_partials(nan).sum()) == 1
    assert int(ops.label_count_partials(nan, -1.0).sum()) == 1


def _big_f16():
    """fp16, n = 2^24 + 3 with 2^24 + 1 labels in the upper class: neither n nor the count is a float32"""
    if "big" not in _INPUTS:
        n = (1 << 24) + 3
        g = torch.Generator(device=DEV).manual_seed(7)
        x = (0.5 + 0.5 * torch.rand(n, generator=g, device=DEV)).to(torch.float16).clamp_(0.5, 0.99)
        x[12345], x[n - 2] = 0.25, 0.125
        _INPUTS["big"] = (x, _np32(x))
    return _INPUTS["big"]


def test_count_and_align_where_the_float_count_rounds():
    from torch_em_amd import ops
    x, flat = _big_f16()
    n = x.numel()
    c1 = int(ops.label_count_partials(x).sum())
    assert c1 == n - 2 == ref.count(flat, 0.5, "f16") and c1 % 2 == 1 and float(np.float32(c1)) != c1 and float(np.float32(n)) != n
    got = ops.distribution_align(x, (0.7, 0.3))
    assert _same_bits(_np32(got), ref.align(flat, (0.7, 0.3), 0.5, "f16"))


# ---- align --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_align_matches_the_reference_fixture_bit_for_bit(g18, dt):
    from torch_em_amd import ops
    n = 0
    for c in ref.da_cases(g18):
        if c["dtype"] != dt:
            continue
        x = torch.from_numpy(ref.da_array(g18, c["x"], dt)).to(DTYPES[dt]).to(DEV)
        before = x.clone()
        got = ops.distribution_align(x, c["source"], c["threshold"])
        assert got.dtype == x.dtype and got.shape == x.shape and got.data_ptr() != x.data_ptr()
        assert _same_bits(_np32(got), ref.da_array(g18, c["key"], dt)), c["key"]
        assert torch.equal(x.view(torch.int32 if dt == "f32" else torch.int16), before.view(torch.int32 if dt == "f32" else torch.int16))
        n += 1
    assert n == 14 + (dt == "f32")      # 12 grid cases and 2 single-class tensors per dtype, the NaN case in fp32
    if dt == "f32":
        assert bool(torch.isnan(got).sum() == 1)      # the NaN case is the last one: NaN comes through the clip


@pytest.mark.parametrize("dt", list(DTYPES))
def test_align_against_the_oracle_in_every_layout(dt):
    from torch_em_amd import ops
    for case in CASES:
        x, flat = _input(case, dt)
        before = x.clone()
        for source in SOURCES:
            for threshold in ((0.5, 0.3) if case == "ties" else (0.5,)):
                got = ops.distribution_align(x, source, threshold)
                assert got.dtype == x.dtype and got.shape == x.shape and got.stride() == x.stride(), case
                assert _same_bits(_storage_order(got), ref.align(flat, source, threshold, dt)), (case, source, threshold)
        assert _same_bits(_storage_order(x), _storage_order(before))      # the input is unchanged
    x, _ = _input("ties", dt)
    got = ops.distribution_align(x, (0.7, 0.3))
    assert bool((torch.isnan(got) == torch.isnan(x)).all()) and int(torch.isnan(got).sum()) == 2
    ok = got[~torch.isnan(got)]
    assert float(ok.min()) == 0.0 and float(ok.max()) == 1.0


@pytest.mark.parametrize("dt", list(DTYPES))
def test_align_writes_inside_its_output_only(dt):
    """the output sits between poisoned guard zones, on a 16-byte boundary and one element off it"""
    from torch_em_amd import ops
    dtype = DTYPES[dt]
    for case in ("n1", "n3", "n255", "tail", "channels_last", "ties"):
        x, flat = _input(case, dt)
        want = ref.align(flat, (0.2, 0.8), 0.5, dt)
        for shift in (0, 1):
            raw = torch.full((x.numel() + 2 * GUARD + shift,), POISON, dtype=dtype, device=DEV)
            out = raw.as_strided(x.shape, x.stride(), GUARD + shift)
            assert (out.data_ptr() % 16 == 0) == (shift == 0)      # the vector path and the scalar one
            res = ops.distribution_align(x, (0.2, 0.8), 0.5, out=out)
            assert res is out
            assert _same_bits(_storage_order(out), want), (case, shift)
            lo, hi = raw[:GUARD + shift], raw[GUARD + shift + x.numel():]
            assert hi.numel() == GUARD and bool((lo == POISON).all()) and bool((hi == POISON).all()), (case, shift)
    x, _ = _input("tail", dt)
    with pytest.raises(ValueError, match="overlap"):
        ops.distribution_align(x, (0.7, 0.3), out=x)
    with pytest.raises(ValueError, match="laid out like the labels"):
        ops.distribution_align(x, (0.7, 0.3), out=torch.empty(x.numel() + 1, dtype=dtype, device=DEV))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_align_single_class(dt):
    from torch_em_amd import ops
    for value, k in ((0.2, 0), (0.9, 1)):
        x = torch.full((3, 1, 5, 41), value, dtype=DTYPES[dt], device=DEV)
        got = ops.distribution_align(x, (0.7, 0.3))
        flat = _np32(x).reshape(-1)
        # the ratio collapses to source / 1; the empty class's ratio (0 here, inf in a naive division) touches nothing
        assert _same_bits(_np32(got).reshape(-1), ref.round_to(flat * np.float32((0.7, 0.3)[k]), dt))
        assert _same_bits(_np32(got).reshape(-1), ref.align(flat, (0.7, 0.3), 0.5, dt))
    # an empty upper class and a NaN, which is not "< threshold" and takes that class's ratio: NaN stays NaN, nothing else moves
    x = torch.full((515,), 0.25, dtype=DTYPES[dt], device=DEV)
    x[100] = float("nan")
    got = ops.distribution_align(x, (0.5, 0.5))
    assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[100]))
    assert _same_bits(_np32(got), ref.align(_np32(x), (0.5, 0.5), 0.5, dt))


def test_align_has_no_host_round_trip():
    """captured once, replayed on other contents: the class counts never pass through the host"""
    from torch_em_amd import ops
    g = torch.Generator().manual_seed(3)
    first = (torch.rand(2, 1, 24, 43, generator=g) ** 2)                 # about 29 % of the labels are >= 0.5
    second = torch.rand(2, 1, 24, 43, generator=g) ** 0.25              # about 94 %
    x = first.to(DEV)
    src = (0.7, 0.3)
    eager = ops.distribution_align(x, src)                               # warms the library up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.distribution_align(x, src)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager) and _same_bits(_np32(y), ref.align(first.numpy(), src, 0.5, "f32"))
    x.copy_(second.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    c_first, c_second = ref.count(first.numpy(), 0.5, "f32"), ref.count(second.numpy(), 0.5, "f32")
    assert c_second > 2 * c_first
    assert _same_bits(_np32(y), ref.align(second.numpy(), src, 0.5, "f32"))


# ---- weight sharing: a no_grad forward between a gradient forward and its backward --------------------------------
def test_no_grad_forward_between_two_live_forwards():
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    torch.manual_seed(0)
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid").to(DEV)
    model.train()
    g = torch.Generator().manual_seed(9)
    x1, x2 = torch.randn(2, 1, 32, 32, generator=g).to(DEV), torch.randn(2, 1, 32, 32, generator=g).to(DEV)
    t1, t2 = (torch.rand(2, 1, 32, 32, generator=g) > 0.5).float().to(DEV), torch.rand(2, 1, 32, 32, generator=g).to(DEV)
    x3 = torch.randn(2, 1, 32, 32, generator=g).to(DEV)
    loss = DiceLoss()
    single = []
    for x, t in ((x1, t1), (x2, t2)):
        model.zero_grad()
        loss(model(x), t).backward()
        single.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    with torch.no_grad():
        y3_alone = model(x3).clone()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    opt.zero_grad()
    y1 = model(x1)
    y1_before = y1.detach().clone()
    with torch.no_grad():
        y3 = model(x3)      # the labeler's pass: same model, train mode, while y1's activations wait for the backward pass
    assert not y3.requires_grad and torch.equal(y3, y3_alone) and torch.equal(y1.detach(), y1_before)
    y2 = model(x2)
    ((loss(y1, t1) + loss(y2, t2)) / 2).backward()
    want = {k: ((single[0][k] + single[1][k]) / 2).cpu() for k in single[0]}
    check_grads({k: p.grad.cpu() for k, p in model.named_parameters()}, want, 1e-5, what="two nodes around a no_grad pass: ")
    opt.step()
    opt.zero_grad()
    loss(model(x1), t1).backward()
    opt.step()
    assert opt._arena.grads_flat() is not None      # a single-forward step is back on the one-launch path


# ---- the trainer against the reference's runs -------------------------------------------------------------------------
SERIES = ("unsup", "sup", "combined", "val_metric", "val_loss")


def _loader(*arrays):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(*(torch.from_numpy(a) for a in arrays)), batch_size=2,
                                       shuffle=False)


def _state(g18, tag, i):
    return {k: torch.from_numpy(v) for k, v in _states(g18, tag)[i].items()}


_STATES = {}


def _states(g18, tag):
    if tag not in _STATES:
        _STATES[tag] = ref.fm_states(g18, tag)
    return _STATES[tag]


def _fm_trainer(g17, g18, tag, tmp_path, **overrides):
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            FixMatchTrainer)
    cfg = json.loads(str(g18["fm_runs"]))[tag]
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    model.load_state_dict(_state(g18, tag, 0))
    log = {k: [] for k in SERIES + ("keep", "ct", "calls")}

    class Recorder:
        def __init__(self, trainer, save_root, **kw):
            pass

        def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
            log["calls"].append("unsup")
            log["unsup"].append(float(loss.detach()))
            log["keep"].append(1.0 if label_filter is None else float(label_filter.float().mean()))

        def log_train_supervised(self, step, loss, x, y, pred):
            log["calls"].append("sup")
            log["sup"].append(float(loss.detach()))

        def log_combined_loss(self, step, loss):
            log["calls"].append("combined")
            log["combined"].append(float(loss.detach()))

        def log_lr(self, step, lr):
            log["calls"].append("lr")

        def log_ct(self, step, ct):
            log["calls"].append("ct")
            log["ct"].append(float(ct))

        def log_validation_unsupervised(self, step, metric, loss, x1, x2, pred, pseudo_labels, label_filter=None):
            log["val_metric"].append(metric)
            log["val_loss"].append(loss)

        def log_validation_supervised(self, step, metric, loss, x, y, pred):
            log["val_metric"].append(metric)
            log["val_loss"].append(loss)

    if cfg["semi"]:
        kw = dict(supervised_train_loader=_loader(g17["mt_xs"], g17["mt_ys"]), supervised_val_loader=_loader(g17["mt_xsv"], g17["mt_ysv"]),
                  supervised_loss=DefaultSelfTrainingLoss(), supervised_loss_and_metric=DefaultSelfTrainingLossAndMetric())
    else:
        kw = dict(unsupervised_val_loader=_loader(g17["mt_xv1"], g17["mt_xv2"]),
                  unsupervised_loss_and_metric=DefaultSelfTrainingLossAndMetric())
    kw.update(dict(name="g18" + tag, model=model, optimizer=FusedAdamW(model.parameters(), lr=float(g18["fm_lr"])),
                   pseudo_labeler=DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]),
                   unsupervised_loss=DefaultSelfTrainingLoss(), unsupervised_train_loader=_loader(g17["mt_xu1"], g17["mt_xu2"]),
                   source_distribution=cfg["source"], logger=Recorder, mixed_precision=False, device=DEV, save_root=str(tmp_path)))
    kw.update(overrides)
    return FixMatchTrainer(**kw), log, cfg


C_OUT = 1.0   # DiceLoss sums 1 - score over the channels: score = C - loss


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_every_step_replays_the_reference(g17, g18, tag, tmp_path):
    """At the state the reference had before iteration i, labels, filter, alignment and loss on batch i give the loss the
    reference logged: score within 2e-5 relative (the first-step margin of the mean-teacher tests; the generator's guard of
    1e-5 around 0.5, 0.7 and 0.3 makes it valid at every step), keep share the same voxel count out of 2048."""
    trainer, _, cfg = _fm_trainer(g17, g18, tag, tmp_path, logger=None)
    model = trainer.model.to(DEV)
    model.train()
    xu1, xu2, xs, ys = (torch.from_numpy(g17[k]).to(DEV) for k in ("mt_xu1", "mt_xu2", "mt_xs", "mt_ys"))
    for i in range(6):
        model.load_state_dict(_state(g18, tag, i))
        b = slice(2 * i, 2 * i + 2)
        with torch.no_grad():
            raw_labels, _ = trainer.pseudo_labeler(model, xu1[b])
        labels, label_filter = trainer._aligned_labels(xu1[b])
        assert not labels.requires_grad and labels.shape == (2, 1, 32, 32)
        if cfg["source"] is None:
            assert torch.equal(labels, raw_labels)
        else:      # the alignment the trainer applied is the oracle's on the labels it got
            assert _same_bits(_np32(labels), ref.align(_np32(raw_labels), cfg["source"], 0.5, "f32"))
        keep = 1.0 if label_filter is None else float(label_filter.float().mean())
        with torch.no_grad():
            unsup = float(trainer.unsupervised_loss(model, xu2[b], labels, label_filter))
        want = float(g18[f"fm_{tag}_unsup"][i])
        dev = abs((C_OUT - unsup) - (C_OUT - want)) / (C_OUT - want)
        print(f"FIXMATCH_STEP run {tag} step {i}: unsup {unsup:.7f} reference {want:.7f} score dev {dev:.2e} keep {keep:.6f} "
              f"reference {float(g18[f'fm_{tag}_keep'][i]):.6f}")
        assert dev < 2e-5, (tag, i, unsup, want)
        assert abs(keep - float(g18[f"fm_{tag}_keep"][i])) < 0.5 / 2048, (tag, i, keep)
        if cfg["semi"]:
            with torch.no_grad():
                sup = float(trainer.supervised_loss(model, xs[b], ys[b]))
            want_sup, want_comb = float(g18[f"fm_{tag}_sup"][i]), float(g18[f"fm_{tag}_combined"][i])
            assert abs(sup - want_sup) < 2e-5 * (C_OUT - want_sup), (i, sup, want_sup)
            assert abs((sup + unsup) / 2 - want_comb) < 2e-5 * (C_OUT - want_comb), (i, sup, unsup, want_comb)


def _check_trajectory(trainer, log, g18, tag):
    for k in SERIES:
        want = g18[f"fm_{tag}_{k}"]
        assert len(log[k]) == len(want), (k, len(log[k]))
        if not len(want):
            continue
        tol = max(5e-3, 2 * float(g18[f"fm_{tag}_scatter_{k}"]))      # two draws from the reference's own scatter
        got_score, want_score = C_OUT - np.array(log[k]), C_OUT - want
        dev = float(np.max(np.abs(got_score - want_score) / np.abs(want_score)))
        print(f"FIXMATCH_RUN run {tag} {k}: {[round(float(v), 6) for v in log[k]]} reference {[round(float(v), 6) for v in want]} "
              f"worst score dev {dev:.2e} margin {tol:.1e}")
        assert dev <= tol, (tag, k, dev, tol)
    assert np.allclose(log["keep"], g18[f"fm_{tag}_keep"], atol=2e-2), (log["keep"], g18[f"fm_{tag}_keep"])
    final = _states(g18, tag)[6]
    for k, v in trainer.model.state_dict().items():      # G7's parameter margin, the round-off-level sampler biases aside
        if "samplers" in k and k.endswith("bias"):
            continue
        a, b = v.cpu().double(), torch.from_numpy(final[k]).double()
        assert float((a - b).norm() / b.norm()) < 0.15, (tag, k)
    ckpt = torch.load(os.path.join(trainer.checkpoint_folder, "latest.pt"), weights_only=False)
    assert set(g18[f"fm_{tag}_ckpt_keys"]) <= set(ckpt), set(g18[f"fm_{tag}_ckpt_keys"]) - set(ckpt)
    assert "teacher_state" not in ckpt and ckpt["init"]["trainer_class"].endswith("fix_match.FixMatchTrainer")
    return ckpt


def test_fixmatch_unsupervised_without_threshold(g17, g18, tmp_path):
    trainer, log, _ = _fm_trainer(g17, g18, "a", tmp_path)
    trainer.fit(iterations=6)
    assert trainer.iteration == 6 and not hasattr(trainer, "teacher")
    ckpt = _check_trajectory(trainer, log, g18, "a")
    assert ckpt["init"]["self_training"]["source_distribution"] is None
    assert log["calls"] == ["unsup", "lr"] * 6 and log["ct"] == []      # the reference's logger calls, in its order
    assert trainer.optimizer._arena.grads_flat() is not None     # one gradient node per step: the one-launch optimizer path


def test_fixmatch_unsupervised_with_threshold_and_alignment(g17, g18, tmp_path):
    trainer, log, _ = _fm_trainer(g17, g18, "b", tmp_path)
    trainer.fit(iterations=6)
    ckpt = _check_trajectory(trainer, log, g18, "b")
    assert ckpt["init"]["self_training"]["source_distribution"] == [0.7, 0.3]
    assert log["calls"] == ["unsup", "lr", "ct"] * 6 and log["ct"] == [0.7] * 6
    assert trainer.pseudo_labeler.confidence_threshold == 0.7      # no schedule step after validation


def test_fixmatch_semisupervised(g17, g18, tmp_path):
    trainer, log, _ = _fm_trainer(g17, g18, "c", tmp_path)
    assert trainer.train_loader is trainer.unsupervised_train_loader and trainer.val_loader is trainer.supervised_val_loader
    trainer.fit(iterations=6)
    _check_trajectory(trainer, log, g18, "c")
    assert log["calls"] == ["sup", "unsup", "combined", "lr", "ct"] * 6


def _scale_raw(x):
    return x * 0.75


def test_checkpoint_round_trip(g17, g18, tmp_path):
    from torch_em_amd import util
    from torch_em_amd.self_training import FixMatchTrainer
    trainer, _, _ = _fm_trainer(g17, g18, "c", tmp_path, logger=None, raw_transform=_scale_raw, prefetch=False)
    v1, _ = trainer._views((torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4)))
    assert v1.is_cuda and float(v1.mean()) == 0.75          # the raw transform reaches the unsupervised views
    trainer.fit(iterations=6)
    folder = trainer.checkpoint_folder
    assert os.path.exists(os.path.join(folder, "best.pt")) and os.path.exists(os.path.join(folder, "latest.pt"))
    trainer2 = FixMatchTrainer.from_checkpoint(folder, name="latest")
    assert type(trainer2) is FixMatchTrainer and trainer2.iteration == trainer.iteration == 6
    assert util.model_is_equal(trainer.model, trainer2.model)
    assert trainer2.source_distribution == [0.6, 0.4] and trainer2.raw_transform is _scale_raw and trainer2.prefetch is False
    assert len(trainer2.supervised_train_loader) == len(trainer.supervised_train_loader)
    assert trainer2.pseudo_labeler.confidence_threshold == 0.7
    trainer2.fit(iterations=3)
    assert trainer2.iteration == 9
    trainer3 = util.get_trainer(folder, name="latest")
    assert type(trainer3) is FixMatchTrainer and trainer3.iteration == 9 and trainer3.source_distribution == [0.6, 0.4]
    assert trainer3.raw_transform is _scale_raw


def test_view_transforms_form_the_two_views_on_the_device(g17, g18, tmp_path):
    from torch_em_amd.transform.raw import get_default_mean_teacher_augmentations
    x = np.abs(g17["mt_xu1"][:4])
    augs = (get_default_mean_teacher_augmentations(p=0.9), get_default_mean_teacher_augmentations(p=0.9))
    single = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(x)), batch_size=2, shuffle=False)
    trainer, log, _ = _fm_trainer(g17, g18, "b", tmp_path, view_transforms=augs, unsupervised_train_loader=single,
                                  unsupervised_val_loader=single)
    batch = next(iter(single))
    torch.manual_seed(5)
    np.random.seed(5)
    v1, v2 = trainer._views(batch)
    torch.manual_seed(5)
    np.random.seed(5)
    xd = batch[0].to(DEV)
    w1, w2 = augs[0](xd), augs[1](xd)
    assert v1.is_cuda and v1.shape == xd.shape and torch.equal(v1, w1) and torch.equal(v2, w2)
    assert not torch.equal(v1, v2) and not torch.equal(v1, xd)
    trainer.fit(iterations=2)
    assert trainer.iteration == 2 and len(log["unsup"]) == 2 and all(np.isfinite(log["unsup"]))
    with pytest.raises(ValueError, match="one raw batch"):
        trainer._views((batch[0], batch[0]))


def test_fixmatch_mixed_precision(g17, g18, tmp_path):
    """Run (b) with fp16 operands and storage against the reference's fp32 run, within the margin of the mean-teacher mixed
    test (3e-2 on the score); fp16 labels go through the trainer's alignment as they are."""
    from torch_em_amd import ops
    trainer, log, _ = _fm_trainer(g17, g18, "b", tmp_path, mixed_precision=True, mixed_precision_dtype="float16")
    assert trainer._amp and trainer.scaler is not None
    seen, align = [], ops.distribution_align

    def spy(labels, *a, **k):
        seen.append(labels.dtype)
        return align(labels, *a, **k)
    ops.distribution_align = spy
    try:
        trainer.fit(iterations=6)
    finally:
        ops.distribution_align = align
    # the engine keeps the network's prediction in fp32 in the mixed modes (model/engine.py), so the labels the labeler hands
    # on are fp32 here; a model that returns fp16 gives the kernel fp16 labels, which the trainer passes through as they are
    assert seen == [torch.float32] * 6
    half = (torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(4)) ** 2).to(torch.float16).to(DEV)
    got = trainer.get_distribution_alignment(half)
    assert got.dtype == torch.float16 and _same_bits(_np32(got), ref.align(_np32(half), (0.7, 0.3), 0.5, "f16"))
    want = g18["fm_b_unsup"]
    print("FIXMATCH_RUN amp b unsup", [round(v, 6) for v in log["unsup"]], "reference fp32", [round(float(v), 6) for v in want])
    assert np.allclose(C_OUT - np.array(log["unsup"]), C_OUT - want, rtol=3e-2, atol=0), (log["unsup"], want)
    assert np.allclose(C_OUT - np.array(log["val_metric"]), C_OUT - g18["fm_b_val_metric"], rtol=3e-2)
    assert np.allclose(C_OUT - np.array(log["val_loss"]), C_OUT - g18["fm_b_val_loss"], rtol=3e-2)


def test_hip_graph_is_refused(g17, g18, tmp_path):
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _fm_trainer(g17, g18, "a", tmp_path, hip_graph=True)
