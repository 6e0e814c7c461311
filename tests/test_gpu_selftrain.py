"""GPU: self-training -- the pseudo-label kernel (csrc/selftrain.hip) against the float64 oracle (tests/selftrain_ref.py, pinned to
the reference's DefaultPseudoLabeler by tests/test_selftrain_cpu.py), the one-pass masked / unmasked Dice sums, the fused
self-training loss, two live forward passes of one model in one backward pass, and MeanTeacherTrainer against runs of the
REFERENCE's trainer (tests/golden/g17_selftrain.npz, tests/golden/gen_golden_selftrain.py).

Sigmoid labels are judged in ulps of the storage type against the float64 sigmoid; the bound is not chosen here: it is twice
what torch's CPU sigmoid (the reference's) shows on the same inputs, and at least 1 ulp.  The figures print as SELFTRAIN_ERR
lines (profiles/selftrain_errors.txt).  No test provokes a device fault: outputs the test lays out sit between guard zones
that must survive, and every extent is that of a dense tensor the test allocated.
"""
import json
import os

import numpy as np
import pytest
import torch

import selftrain_ref as ref
from conftest import GOLDEN, check_grads, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = {"v1": (1, 1, 1), "v7": (1, 1, 7), "c2": (1, 2, 3, 5), "blocks": (2, 3, 5, 7, 9), "c1": (2, 1, 4, 8, 8)}
LAYOUTS = list(SHAPES) + ["channels_last", "odd_offset", "ties"]
GUARD = 64   # elements around every output the test lays out (a multiple of 16 bytes in every type: the vector path stays reachable)


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_selftrain.npz")))


def _np64(t):
    return t.detach().float().cpu().double().numpy()


_INPUTS = {}


def _input(layout, dt, g17):
    """seeded N(0, 2) logits in the storage type, laid out as the case asks; built once per (layout, dtype)"""
    key = (layout, dt)
    if key not in _INPUTS:
        dtype = DTYPES[dt]
        if layout == "ties":
            x = torch.from_numpy(g17[f"pl_{dt}_x"]).to(dtype).to(DEV)
        else:
            shape = SHAPES.get(layout, SHAPES["blocks"])
            g = torch.Generator().manual_seed(1000 + LAYOUTS.index(layout))
            x = (2.0 * torch.randn(shape, generator=g)).to(dtype)
            if layout == "channels_last":
                x = x.to(DEV).contiguous(memory_format=torch.channels_last_3d)
                assert x.stride(1) == 1
            elif layout == "odd_offset":   # a dense view that starts one element into its buffer: the base is not 16-byte aligned
                buf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
                buf[1:].copy_(x.flatten())
                x = buf[1:].view(shape)
                assert x.storage_offset() == 1 and x.data_ptr() % 16 != 0
            else:
                x = x.to(DEV)
        _INPUTS[key] = x
    return _INPUTS[key]


class Guarded:
    """An output tensor with x's shape and strides inside a poisoned buffer with GUARD elements on either side."""

    def __init__(self, x, dtype, shift=0):
        """shift: extra elements in front, so that the output does NOT start on a 16-byte boundary"""
        n = x.numel()
        poison = 0xAB if dtype == torch.bool else float("nan")
        self.raw = torch.full((n + 2 * GUARD + shift,), poison, dtype=torch.uint8 if dtype == torch.bool else dtype, device=DEV)
        buf = self.raw.view(torch.bool) if dtype == torch.bool else self.raw
        self.view = buf.as_strided(x.shape, x.stride(), GUARD + shift)
        self.n, self.is_bool, self.lo = n, dtype == torch.bool, GUARD + shift

    def check(self, what):
        raw = self.raw.cpu()
        inner, guards = raw[self.lo:self.lo + self.n], torch.cat([raw[:self.lo], raw[self.lo + self.n:]])
        if self.is_bool:
            assert bool((guards == 0xAB).all()), f"{what}: wrote outside the output"
            assert bool((inner <= 1).all()), f"{what}: an element was not written (or is not 0 / 1)"
        else:
            assert bool(torch.isnan(guards).all()), f"{what}: wrote outside the output"
            assert not bool(torch.isnan(inner).any()), f"{what}: an element was not written"


ERR = {}   # (dt) -> [kernel worst ulps, reference worst ulps, bound]


@pytest.fixture(scope="module", autouse=True)
def _print_errors():
    yield
    for dt, (ek, er, bound) in sorted(ERR.items()):
        print(f"\nSELFTRAIN_ERR sigmoid labels {dt}: kernel {ek:.3f} ulp, torch CPU sigmoid {er:.3f} ulp, bound {bound:.3f} ulp")


def _sigmoid_errors(x, labels, dt):
    """(kernel error, reference error) in ulps of the storage type against the float64 sigmoid, per element"""
    x64 = _np64(x)
    exact = ref.sigmoid64(x64)
    u = ref.ulp(exact, dt)
    cpu = torch.sigmoid(x.detach().cpu())          # the reference's activation, on the CPU, in the storage type
    return np.abs(_np64(labels) - exact) / u, np.abs(_np64(cpu) - exact) / u


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pseudo_label_against_the_oracle(layout, dt, g17):
    from torch_em_amd import ops
    x = _input(layout, dt, g17)
    x64 = _np64(x)
    dtype = DTYPES[dt]
    N = x.shape[0]
    # ---- no activation: the labels ARE the input, the mask is exactly the oracle's ----
    for both in (True, False):
        for t in (0.9, 0.6):
            for ms in (None,) + ((1,) if N > 1 else ()):
                mask_out = Guarded(x, torch.float32 if both else torch.bool)
                labels, mask = ops.pseudo_label(x, None, t, both, ms, out=(None, mask_out.view))
                what = (layout, dt, "none", both, t, ms)
                assert labels is x and mask.data_ptr() == mask_out.view.data_ptr(), what
                mask_out.check(what)
                want = ref.mask_ref(x64, t, both, dt, ms)
                assert mask.dtype == (torch.float32 if both else torch.bool) and mask.stride() == x.stride(), what
                assert np.array_equal(mask.cpu().numpy(), want), what
                if ms is not None:
                    assert all(torch.equal(mask[n], mask[1]) for n in range(N)), what
    labels, mask = ops.pseudo_label(x, None, None)
    assert labels is x and mask is None
    # ---- sigmoid ----
    lab_out = Guarded(x, dtype)
    labels, mask = ops.pseudo_label(x, "sigmoid", None, out=(lab_out.view, None))
    lab_out.check((layout, dt, "sigmoid"))
    assert mask is None and labels.dtype == dtype and labels.stride() == x.stride()
    ek, er = _sigmoid_errors(x, labels, dt)
    bound = max(2.0 * float(er.max()), 1.0)
    cur = ERR.get(dt, [0.0, 0.0, 0.0])
    ERR[dt] = [max(cur[0], float(ek.max())), max(cur[1], float(er.max())), max(cur[2], bound)]
    print(f"SELFTRAIN_ERR {layout} {dt}: kernel {ek.max():.3f} ulp, torch CPU sigmoid {er.max():.3f} ulp, bound {bound:.3f}")
    assert float(ek.max()) <= bound, (layout, dt, float(ek.max()), bound)
    oracle_labels = ref.labels_ref(x64, True, dt)
    for both in (True, False):
        for t in (0.9, 0.6):
            for ms in (None,) + ((1,) if N > 1 else ()):
                what = (layout, dt, "sigmoid", both, t, ms)
                lab_out, mask_out = Guarded(x, dtype), Guarded(x, torch.float32 if both else torch.bool)
                labels2, mask = ops.pseudo_label(x, "sigmoid", t, both, ms, out=(lab_out.view, mask_out.view))
                lab_out.check(what)
                mask_out.check(what)
                assert torch.equal(labels2, labels), what                  # the same labels with and without a mask
                # the mask follows from the kernel's OWN labels, everywhere: the reference compare (torch, CPU) applied to them
                lc = labels2.cpu()
                src = lc if ms is None else lc[ms:ms + 1]
                want = ((src >= t) + (src <= 1.0 - t)).to(torch.float32) if both else (src >= t)
                want = want.expand(*lc.shape)
                assert mask.dtype == want.dtype and torch.equal(mask.cpu(), want), what
                assert np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(labels2), t, both, dt, ms)), what
                # against the oracle's mask: differences only where the oracle's label lies within the bound of a threshold
                oracle_mask = ref.mask_ref(oracle_labels, t, both, dt, ms)
                differ = mask.cpu().numpy() != oracle_mask
                near = ref.threshold_distance(oracle_labels, t, both, dt) <= bound
                if ms is not None:
                    near = np.broadcast_to(near[ms:ms + 1], near.shape)
                assert not (differ & ~near).any(), what
                assert differ.mean() <= 1e-3, (what, float(differ.mean()))


def test_seeded_inputs_stay_away_from_the_thresholds(g17):
    """On the CPU: how often the reference's own sigmoid puts a seeded input on the other side of a threshold than the float64
    oracle -- far below the 1e-3 the kernel test allows for voxels near a threshold."""
    total = flips = 0
    for dt in DTYPES:
        for layout in LAYOUTS[:-1]:
            x = _input(layout, dt, g17).cpu()
            lab_cpu, lab64 = _np64(torch.sigmoid(x)), ref.labels_ref(_np64(x), True, dt)
            for both in (True, False):
                for t in (0.9, 0.6):
                    flips += int((ref.mask_ref(lab_cpu, t, both, dt) != ref.mask_ref(lab64, t, both, dt)).sum())
                    total += x.numel()
    print(f"SELFTRAIN_ERR reference-only mask flips on the seeded inputs: {flips} of {total}")
    assert flips <= 1e-4 * total


@pytest.mark.parametrize("dt", list(DTYPES))
def test_pseudo_label_with_misaligned_outputs(dt, g17):
    """An aligned input with `labels` or `mask` off the 16-byte grid: the launch drops to the scalar loop and writes the same
    values as the vector path, inside the output only."""
    from torch_em_amd import ops
    x = _input("blocks", dt, g17)
    assert x.data_ptr() % 16 == 0
    for both in (True, False):
        mdtype = torch.float32 if both else torch.bool
        want_l, want_m = ops.pseudo_label(x, "sigmoid", 0.6, both, 1)
        for shift_l, shift_m in ((1, 0), (0, 1), (3, 5)):
            lab_out, mask_out = Guarded(x, DTYPES[dt], shift_l), Guarded(x, mdtype, shift_m)
            assert (lab_out.view.data_ptr() % 16 != 0) == bool(shift_l) and (mask_out.view.data_ptr() % 16 != 0) == bool(shift_m)
            labels, mask = ops.pseudo_label(x, "sigmoid", 0.6, both, 1, out=(lab_out.view, mask_out.view))
            what = (dt, both, shift_l, shift_m)
            lab_out.check(what)
            mask_out.check(what)
            assert torch.equal(labels, want_l) and torch.equal(mask, want_m), what
        mask_out = Guarded(x, mdtype, 1)
        _, mask = ops.pseudo_label(x, None, 0.6, both, None, out=(None, mask_out.view))
        mask_out.check((dt, both, "none"))
        assert np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(x), 0.6, both, dt))


def test_pseudo_label_makes_other_layouts_contiguous():
    """a slice view is not dense: the wrapper copies it; mask_sample needs sample-major storage"""
    from torch_em_amd import ops
    g = torch.Generator().manual_seed(3)
    big = (2.0 * torch.randn(2, 4, 6, 10, generator=g)).to(DEV)
    x = big[:, 1:3, :, 2:9]
    labels, mask = ops.pseudo_label(x, "sigmoid", 0.6, True)
    assert labels.is_contiguous() and np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(labels), 0.6, True, "f32"))
    xt = big.permute(1, 0, 2, 3)        # dense, but the batch axis of the VIEW is not the outermost in storage
    labels, mask = ops.pseudo_label(xt, None, 0.6, False, 1)
    assert all(torch.equal(mask[n], mask[1]) for n in range(4))
    assert np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(xt), 0.6, False, "f32", 1))
    with pytest.raises(ValueError, match="out of range"):
        ops.pseudo_label(big, None, 0.6, True, 2)


def test_labeler_classes_on_the_device():
    """nn.Sigmoid() and torch.sigmoid take the kernel; another callable is applied with torch and the kernel computes the mask"""
    from torch_em_amd.self_training import DefaultPseudoLabeler, ScheduledPseudoLabeler
    g = torch.Generator().manual_seed(4)
    x = (2.0 * torch.randn(2, 3, 8, 8, generator=g)).to(DEV)
    teacher = lambda inp: inp * 1.0   # noqa: E731
    want_l, want_m = DefaultPseudoLabeler(torch.nn.Sigmoid(), 0.9, mask_channel=1)(teacher, x)
    for act in (torch.sigmoid, lambda v: torch.sigmoid(v)):
        labels, mask = DefaultPseudoLabeler(act, 0.9, mask_channel=1)(teacher, x)
        assert mask.dtype == torch.float32 and torch.equal(mask[0], mask[1])
        assert rel_err(labels.cpu(), want_l.cpu()) < 1e-6
        assert np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(labels), 0.9, True, "f32", 1))
    labels, mask = ScheduledPseudoLabeler(torch.nn.Sigmoid(), 0.6, threshold_from_both_sides=False, verbose=False)(teacher, x)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), ref.mask_ref(_np64(labels), 0.6, False, "f32"))


# ---- Dice: one pass for masked and unmasked sums ------------------------------------------------------------------
def _dice_inputs():
    g = torch.Generator().manual_seed(7)
    shape = SHAPES["blocks"]
    p = torch.rand(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last_3d)   # as the engine leaves it
    t = torch.rand(shape, generator=g).to(DEV)                                                    # NCDHW
    m = (torch.rand(shape, generator=g) > 0.4).float().to(DEV)
    return p, t, m


def test_dice_sums_pair_equals_two_calls():
    from torch_em_amd import _lib, ops
    p, t, m = _dice_inputs()
    assert p.stride(1) == 1 and t.is_contiguous()
    old = _lib.get_option("dice_vox")
    try:
        for vox in (1, 0):
            _lib.set_option("dice_vox", vox)
            pair = ops.dice_sums_pair(p, t, m)[0].cpu()
            masked, plain = ops.dice_sums(p, t, m)[0].cpu(), ops.dice_sums(p, t)[0].cpu()
            assert pair.shape == (2, 3, 3) and pair.dtype == torch.float64
            for got, want in ((pair[0], masked), (pair[1], plain)):
                assert float(((got - want).abs() / want.abs()).max()) <= 1e-12, (vox, got, want)
            assert float((pair[0] - pair[1]).abs().max()) > 1.0      # the halves are different quantities
    finally:
        _lib.set_option("dice_vox", old)
    with pytest.raises(ValueError, match="share the target's strides"):
        ops.dice_sums_pair(p, t, m.contiguous(memory_format=torch.channels_last_3d))


@pytest.mark.parametrize("C,layout", [(4, "cl"), (2, "cl"), (1, "cl"), (3, "ncdhw"), (20, "cl"), (20, "ncdhw")])
def test_dice_sums_pair_on_every_partial_kernel(C, layout):
    """Every PAIR instantiation of the partial-sum kernels: k_dice_partial_vox<4> (C = 4, channels-last), <2> (C = 2), <1> (any
    other C <= 16), and with dice_vox = 0 or C > 16 k_dice_partial<true> (channels-last) / <false> (NCDHW prediction).  Same
    rule as above: each half within 1e-12 relative of the call that computes it alone."""
    from torch_em_amd import _lib, ops
    g = torch.Generator().manual_seed(70 + C)
    shape = (2, C, 5, 7, 9)
    p = torch.rand(shape, generator=g).to(DEV)
    if layout == "cl":
        p = p.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)     # NDHWC storage behind the NCDHW view
        assert p.stride(1) == 1 or C == 1
    t = torch.rand(shape, generator=g).to(DEV)
    m = (torch.rand(shape, generator=g) > 0.4).float().to(DEV)
    old = _lib.get_option("dice_vox")
    try:
        for vox in (1, 0):
            _lib.set_option("dice_vox", vox)
            pair = ops.dice_sums_pair(p, t, m)[0].cpu()
            masked, plain = ops.dice_sums(p, t, m)[0].cpu(), ops.dice_sums(p, t)[0].cpu()
            assert pair.shape == (2, C, 3)
            for got, want in ((pair[0], masked), (pair[1], plain)):
                assert float(((got - want).abs() / want.abs()).max()) <= 1e-12, (C, layout, vox)
            want64 = torch.stack([(p * t * m * m).double().sum((0, 2, 3, 4)), (p * t).double().sum((0, 2, 3, 4))]).cpu()
            assert rel_err(pair[:, :, 0], want64) < 1e-5
    finally:
        _lib.set_option("dice_vox", old)


def test_loss_and_metric_one_pass_equals_two_calls():
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.self_training import DefaultSelfTrainingLossAndMetric
    p, t, m = _dice_inputs()
    model = lambda inp: inp   # noqa: E731
    lm = DefaultSelfTrainingLossAndMetric()
    with torch.no_grad():
        assert lm._one_pass(p, m)
        loss, metric = lm(model, p, t, m)
        want_loss, want_metric = DiceLoss()(p, t, mask=m), DiceLoss()(p, t)
    assert loss.shape == metric.shape == ()
    assert abs(float(loss) - float(want_loss)) <= 1e-6 and abs(float(metric) - float(want_metric)) <= 1e-6
    assert abs(float(loss) - float(metric)) > 1e-3
    # with gradients, different settings or another inner loss the two existing calls run
    pg = p.clone().requires_grad_(True)
    assert not lm._one_pass(pg, m) and not DefaultSelfTrainingLossAndMetric(metric=DiceLoss(reduce_channel="mean"))._one_pass(p, m)
    loss_g, metric_g = lm(model, pg, t, m)
    assert loss_g.requires_grad and abs(float(loss_g.detach()) - float(want_loss)) <= 1e-6 and abs(float(metric_g) - float(want_metric)) <= 1e-6
    mse = torch.nn.MSELoss()
    with torch.no_grad():
        l2, m2 = DefaultSelfTrainingLossAndMetric(loss=mse, metric=mse)(model, p, t, m)
    assert abs(float(l2) - float(mse(p * m, t * m))) <= 1e-6 and abs(float(m2) - float(mse(p, t))) <= 1e-6


def test_fused_loss_against_explicit_products():
    """DefaultSelfTrainingLoss(DiceLoss()) with a filter = the reference's loss(prediction * filter, labels * filter): value
    within 3e-6 max(1, |ref|) and gradient within 2e-5 of its maximum (what tests/test_gpu_dice.py holds the masked Dice to);
    the gradient is exactly zero where the filter is zero."""
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.self_training import DefaultSelfTrainingLoss
    p, t, m = _dice_inputs()
    model = lambda inp: inp   # noqa: E731
    for filt in (m, m > 0.5, m.to(torch.float16)):      # float32 0 / 1, bool (one-sided masks), 16-bit
        pa = p.clone().requires_grad_(True)
        fused = DefaultSelfTrainingLoss(DiceLoss())(model, pa, t, filt)
        ga, = torch.autograd.grad(fused, pa)
        pb = p.clone().requires_grad_(True)
        explicit = DiceLoss()(pb * filt, t * filt)
        gb, = torch.autograd.grad(explicit, pb)
        assert abs(float(fused) - float(explicit)) <= 3e-6 * max(1.0, abs(float(explicit)))
        assert rel_err(ga.cpu(), gb.cpu()) < 2e-5
        assert float(ga[m == 0].abs().max()) == 0.0 and float(ga[m == 1].abs().max()) > 0
    # 16-bit labels and mask in the prediction's layout, as the labeler leaves them under mixed precision
    labels16 = t.to(torch.float16).contiguous(memory_format=torch.channels_last_3d)
    mask16 = m.contiguous(memory_format=torch.channels_last_3d)
    pa = p.clone().requires_grad_(True)
    fused = DefaultSelfTrainingLoss()(model, pa, labels16, mask16)
    explicit = DiceLoss()(p * m, labels16.float() * m)
    assert abs(float(fused) - float(explicit)) <= 3e-6 * max(1.0, abs(float(explicit)))


# ---- two gradient nodes of one model in one backward pass -----------------------------------------------------------
def test_two_live_forwards_in_one_backward():
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    torch.manual_seed(0)
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid").to(DEV)
    g = torch.Generator().manual_seed(9)
    x1, x2 = torch.randn(2, 1, 32, 32, generator=g).to(DEV), torch.randn(2, 1, 32, 32, generator=g).to(DEV)
    t1, t2 = (torch.rand(2, 1, 32, 32, generator=g) > 0.5).float().to(DEV), torch.rand(2, 1, 32, 32, generator=g).to(DEV)
    loss = DiceLoss()
    single = []
    for x, t in ((x1, t1), (x2, t2)):
        model.zero_grad()
        loss(model(x), t).backward()
        single.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    opt.zero_grad()
    y1 = model(x1)
    y2 = model(x2)          # the first pass's activations stay alive
    ((loss(y1, t1) + loss(y2, t2)) / 2).backward()
    want = {k: ((single[0][k] + single[1][k]) / 2).cpu() for k in single[0]}
    check_grads({k: p.grad.cpu() for k, p in model.named_parameters()}, want, 1e-5, what="two nodes: ")
    opt.step()              # the general per-tensor path: autograd added the second arena into the first
    opt.zero_grad()
    loss(model(x1), t1).backward()
    opt.step()
    assert opt._arena.grads_flat() is not None      # a single-forward step is back on the one-launch path


# ---- the trainer against the reference's runs -----------------------------------------------------------------------
def _loader(*arrays):
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(*(torch.from_numpy(a) for a in arrays)), batch_size=2,
                                       shuffle=False)


def _mt_trainer(g17, tag, tmp_path, hooks=None, **overrides):
    from torch_em_amd.model import UNet2d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            MeanTeacherTrainer)
    cfg = json.loads(str(g17["mt_runs"]))[tag]
    model = UNet2d(1, 1, depth=2, initial_features=4, final_activation="Sigmoid")
    pre = f"mt_{tag}_sd0."
    model.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in g17.items() if k.startswith(pre)})
    log = {"unsup": [], "sup": [], "combined": [], "keep": [], "val_metric": [], "val_loss": []}

    class Recorder:
        def __init__(self, trainer, save_root, **kw):
            self.trainer = trainer

        def log_train_unsupervised(self, step, loss, x1, x2, pred, pseudo_labels, label_filter=None):
            log["unsup"].append(float(loss))
            log["keep"].append(1.0 if label_filter is None else float(label_filter.float().mean()))
            if hooks is not None:
                hooks(self.trainer, step)

        def log_train_supervised(self, step, loss, x, y, pred):
            log["sup"].append(float(loss))

        def log_combined_loss(self, step, loss):
            log["combined"].append(float(loss))

        def log_lr(self, step, lr):
            pass

        def log_ct(self, step, ct):
            pass

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
    kw.update(dict(name="g17" + tag, model=model, optimizer=FusedAdamW(model.parameters(), lr=float(g17["mt_lr"])),
                   pseudo_labeler=DefaultPseudoLabeler(confidence_threshold=cfg["threshold"]),
                   unsupervised_loss=DefaultSelfTrainingLoss(), unsupervised_train_loader=_loader(g17["mt_xu1"], g17["mt_xu2"]),
                   momentum=cfg["momentum"], logger=Recorder, mixed_precision=False, device=DEV, save_root=str(tmp_path)))
    kw.update(overrides)
    trainer = MeanTeacherTrainer(**kw)
    assert trainer.reinit_teacher == cfg["semi"]
    pre = f"mt_{tag}_teacher_sd0."
    trainer.teacher.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in g17.items() if k.startswith(pre)})
    return trainer, log, cfg


def _check_states(trainer, g17, tag):
    """G7's parameter margin: relative L2 below 0.15 per tensor, the round-off-level sampler biases aside"""
    for name, module in (("sd1", trainer.model), ("teacher_sd1", trainer.teacher)):
        for k, v in module.state_dict().items():
            if "samplers" in k and k.endswith("bias"):
                continue
            a, b = v.cpu().double(), torch.from_numpy(g17[f"mt_{tag}_{name}.{k}"]).double()
            assert float((a - b).norm() / b.norm()) < 0.15, (tag, name, k)
    assert not any(p.requires_grad or p.grad is not None for p in trainer.teacher.parameters())


C_OUT = 1.0   # DiceLoss sums 1 - score over the channels: score = C - loss


def test_mean_teacher_unsupervised_without_threshold(g17, tmp_path):
    trainer, log, _ = _mt_trainer(g17, "a", tmp_path)
    trainer.fit(iterations=6)
    want = g17["mt_a_unsup"]
    assert want.min() > 0.02 and len(log["unsup"]) == 6 and trainer.iteration == 6
    got_score, want_score = C_OUT - np.array(log["unsup"]), C_OUT - want
    print("mt a loss", [round(v, 6) for v in log["unsup"]], "reference", [round(float(v), 6) for v in want])
    assert abs(got_score[0] - want_score[0]) < 2e-5 * want_score[0]
    assert np.allclose(got_score, want_score, rtol=5e-3, atol=0), (got_score, want_score)
    assert np.allclose(C_OUT - np.array(log["val_metric"]), C_OUT - g17["mt_a_val_metric"], rtol=5e-3)
    _check_states(trainer, g17, "a")
    assert trainer.optimizer._arena.grads_flat() is not None     # one gradient node per step: the one-launch optimizer path
    ckpt = torch.load(os.path.join(trainer.checkpoint_folder, "latest.pt"), weights_only=False)
    assert set(g17["mt_a_ckpt_keys"]) <= set(ckpt), set(g17["mt_a_ckpt_keys"]) - set(ckpt)


def test_mean_teacher_unsupervised_with_threshold(g17, tmp_path):
    trainer, log, _ = _mt_trainer(g17, "b", tmp_path)
    trainer.fit(iterations=6)
    want = g17["mt_b_unsup"]
    assert ((g17["mt_b_keep"] > 0.05) & (g17["mt_b_keep"] < 0.95)).all()
    print("mt b loss", [round(v, 6) for v in log["unsup"]], "reference", [round(float(v), 6) for v in want], "keep", log["keep"])
    assert np.allclose(C_OUT - np.array(log["unsup"]), C_OUT - want, rtol=5e-3, atol=0), (log["unsup"], want)
    # share of voxels the mask keeps: predictions within the trajectory margin (5e-3 of ~0.7) of a threshold may fall the other
    # way -- a window of 7e-3 around 0.7 and 0.3 at a density of at most ~1.5 per unit of probability: 2e-2
    assert np.allclose(log["keep"], g17["mt_b_keep"], atol=2e-2)
    # validation goes through the one-pass masked / unmasked Dice sums: the metric is the unmasked half
    assert np.allclose(C_OUT - np.array(log["val_metric"]), C_OUT - g17["mt_b_val_metric"], rtol=5e-3)
    assert np.allclose(C_OUT - np.array(log["val_loss"]), C_OUT - g17["mt_b_val_loss"], rtol=5e-3)
    _check_states(trainer, g17, "b")


def test_mean_teacher_semisupervised(g17, tmp_path):
    seen = {}

    def hook(trainer, step):
        # called from the logger, BEFORE the momentum update of this step: keep what the update will read
        seen[step] = ({k: v.detach().clone() for k, v in trainer.teacher.state_dict().items()},
                      {k: v.detach().clone() for k, v in trainer.model.state_dict().items()})

    trainer, log, cfg = _mt_trainer(g17, "c", tmp_path, hooks=hook)
    trainer.fit(iterations=6)
    want = g17["mt_c_unsup"]
    assert ((g17["mt_c_keep"] > 0.05) & (g17["mt_c_keep"] < 0.95)).all()
    print("mt c unsup", [round(v, 6) for v in log["unsup"]], "reference", [round(float(v), 6) for v in want])
    print("mt c sup", [round(v, 6) for v in log["sup"]], "reference", [round(float(v), 6) for v in g17["mt_c_sup"]])
    assert np.allclose(C_OUT - np.array(log["unsup"]), C_OUT - want, rtol=5e-3, atol=0), (log["unsup"], want)
    assert np.allclose(C_OUT - np.array(log["sup"]), C_OUT - g17["mt_c_sup"], rtol=5e-3, atol=0), (log["sup"], g17["mt_c_sup"])
    assert np.allclose(2 * C_OUT - 2 * np.array(log["combined"]), 2 * C_OUT - 2 * g17["mt_c_combined"], rtol=5e-3, atol=0)
    _check_states(trainer, g17, "c")
    # the teacher before step k + 1 is the teacher after the update of step k: momentum min(1 - 1 / (k + 1), 0.999)
    for k in range(5):
        m = min(1 - 1 / (k + 1), cfg["momentum"])
        teacher_before, student_after = seen[k][0], seen[k][1]
        teacher_after = seen[k + 1][0]
        for key, v in teacher_after.items():
            if not v.is_floating_point() or key not in dict(trainer.model.named_parameters()):
                continue
            if k == 0:     # momentum 0: the teacher IS the student, bit for bit
                assert torch.equal(v, student_after[key]), key
            else:
                exp = teacher_before[key] * m + student_after[key] * (1 - m)
                assert rel_err(v.cpu(), exp.cpu()) < 1e-6, (k, key)


def _scale_raw(x):
    return x * 0.75


def test_checkpoint_round_trip(g17, tmp_path):
    from torch_em_amd import util
    from torch_em_amd.self_training import MeanTeacherTrainer
    trainer, _, _ = _mt_trainer(g17, "b", tmp_path, logger=None, raw_transform=_scale_raw, prefetch=False)
    v1, _ = trainer._views((torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4)))
    assert v1.is_cuda and float(v1.mean()) == 0.75          # the raw transform reaches the unsupervised views
    trainer.fit(iterations=6)
    folder = trainer.checkpoint_folder
    assert os.path.exists(os.path.join(folder, "best.pt")) and os.path.exists(os.path.join(folder, "latest.pt"))
    trainer2 = MeanTeacherTrainer.from_checkpoint(folder, name="latest")
    assert trainer2.iteration == trainer.iteration == 6
    assert util.model_is_equal(trainer.model, trainer2.model) and util.model_is_equal(trainer.teacher, trainer2.teacher)
    assert len(trainer2.unsupervised_train_loader) == len(trainer.unsupervised_train_loader)
    assert trainer2.pseudo_labeler.confidence_threshold == trainer.pseudo_labeler.confidence_threshold
    assert not any(p.requires_grad for p in trainer2.teacher.parameters())
    assert trainer2.raw_transform is _scale_raw and trainer2.prefetch is False      # the on-device pre-pass survives the resume
    trainer2.fit(iterations=3)
    assert trainer2.iteration == 9
    trainer3 = util.get_trainer(folder, name="latest")
    assert isinstance(trainer3, MeanTeacherTrainer) and trainer3.iteration == 9 and trainer3.raw_transform is _scale_raw


def test_view_transforms_form_the_two_views_on_the_device(g17, tmp_path):
    from torch_em_amd.transform.raw import get_default_mean_teacher_augmentations
    x = np.abs(g17["mt_xu1"][:4])
    augs = (get_default_mean_teacher_augmentations(p=0.9), get_default_mean_teacher_augmentations(p=0.9))
    single = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(x)), batch_size=2, shuffle=False)
    trainer, log, _ = _mt_trainer(g17, "a", tmp_path, view_transforms=augs, unsupervised_train_loader=single,
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


def test_mean_teacher_mixed_precision(g17, tmp_path):
    """One unsupervised run with fp16 operands and storage against the reference's fp32 run, within the margin of G7b
    (tests/test_gpu_trainer.py: 3e-2 on the trajectory), on the score."""
    trainer, log, _ = _mt_trainer(g17, "a", tmp_path, mixed_precision=True, mixed_precision_dtype="float16")
    assert trainer._amp and trainer.scaler is not None
    trainer.fit(iterations=6)
    want = g17["mt_a_unsup"]
    print("mt amp loss", [round(v, 6) for v in log["unsup"]], "reference fp32", [round(float(v), 6) for v in want])
    assert np.allclose(C_OUT - np.array(log["unsup"]), C_OUT - want, rtol=3e-2, atol=0), (log["unsup"], want)
    assert np.allclose(C_OUT - np.array(log["val_metric"]), C_OUT - g17["mt_a_val_metric"], rtol=3e-2)


def test_hip_graph_is_refused(g17, tmp_path):
    with pytest.raises(NotImplementedError, match="one model and one loss"):
        _mt_trainer(g17, "a", tmp_path, hip_graph=True)
