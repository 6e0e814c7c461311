"""CPU: the float64 references of the optimizer and loss-scaler kernels (oracle/optim_ref.py) pinned against torch.
Inputs, error metric and overflow sequences: oracle/optim_cases.py (shared with tests/test_gpu_optim.py).
"""
import numpy as np
import torch

from oracle import optim_ref
from oracle.optim_cases import DEFAULT, SCALER_SETS, adamw_inputs, overflow_sequence


def test_adamw_step_f64_is_torch_adamw():
    """hyper_as_float32=False is torch.optim.AdamW with Python-double scalars: 5 steps on float64 CPU tensors,
    |delta| <= 1e-13 (|ref| + lr) on p, m and v (both sides float64; measured 3.5e-16)."""
    n = 4099
    for hp, seed in ((DEFAULT, 0), (dict(lr=1e-2, b1=0.8, b2=0.99, eps=1e-6, wd=0.1, grad_scale=1.0), 1)):
        p0, _ = adamw_inputs(n, seed)
        tp = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
        opt = torch.optim.AdamW([tp], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"],
                                weight_decay=hp["wd"], foreach=False)
        p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
        worst = 0.0
        rng = np.random.RandomState(seed)
        for step in range(1, 6):
            # gradients of one magnitude: the bound is relative to |ref| + lr, and exp_avg is a difference of its inputs
            g = rng.randn(n) * (rng.rand(n) >= 0.01)
            tp.grad = torch.from_numpy(g.copy())
            opt.step()
            p, m, v = optim_ref.adamw_step_f64(p, g, m, v, step, **hp, hyper_as_float32=False)
            st = opt.state[tp]
            for mine, ref in ((p, tp.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
                rel = np.abs(mine - ref) / (np.abs(ref) + hp["lr"])
                worst = max(worst, float(rel.max()))
                assert rel.max() <= 1e-13, (step, rel.max())
        print(f"adamw_step_f64 vs torch.optim.AdamW(float64): worst {worst:.2e}")
    # grad_scale multiplies the gradient and nothing else
    a = optim_ref.adamw_step_f64(p0, 3.0 * g, m, v, 7, hyper_as_float32=False, grad_scale=0.25)
    b = optim_ref.adamw_step_f64(p0, 0.75 * g, m, v, 7, hyper_as_float32=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_scaler_model_is_torch_amp_update_scale():
    """ScalerState.update against torch._amp_update_scale_ on CPU tensors: scale and tracker exactly equal after every
    step of a seeded overflow sequence, the applied-step count equal to the number of clean steps."""
    for key in SCALER_SETS:
        growth, backoff, interval = key
        seq = overflow_sequence(key)
        assert len(seq) >= 200 and 0 < seq.sum() < len(seq)
        model = optim_ref.ScalerState(scale=2.0 ** 16)
        scale, tracker = torch.tensor([2.0 ** 16]), torch.zeros(1, dtype=torch.int32)
        grew = shrank = 0
        for i, bad in enumerate(seq):
            before = model.scale
            if bad:
                model.raise_flag()
            model.update(growth, backoff, interval)
            torch._amp_update_scale_(scale, tracker, torch.tensor([float(bad)]), growth, backoff, interval)
            assert model.scale == float(scale) and model.growth_tracker == int(tracker), (key, i)
            assert model.found_inf == 0.0
            assert model.applied_steps == float((seq[:i + 1] == 0).sum()), (key, i)
            assert 2.0 ** -100 < model.scale < 2.0 ** 100, "the sequence left the range this comparison is meant for"
            grew += model.scale > before
            shrank += model.scale < before
        assert grew >= 3 and shrank >= 3, (key, grew, shrank)   # the sequence exercises both transitions


def test_gain_deviation_is_bounded_by_the_rounding_of_beta2():
    """The kernels' second-moment gain is 1.f - b2_f, torch's is float(1 - b2).  The difference is the rounding of b2
    to float (relative 2^-24) amplified by 1 / (1 - b2): |delta| <= 2^-24 b2 / (1 - b2) = 5.95e-5 for b2 = 0.999; the
    actual value is -1.29e-5, about 110 fp32 ulps of exp_avg_sq."""
    b2 = 0.999
    delta = ((float(np.float32(1) - np.float32(b2))) - (1 - b2)) / (1 - b2)
    assert delta == optim_ref.gain_deviation(b2)
    assert abs(delta) <= 2.0 ** -24 * b2 / (1 - b2)
    assert 1.2e-5 < abs(delta) < 1.4e-5
    # decay plus gain are exactly 1 in the kernel's arithmetic: the update is a convex combination
    assert float(np.float32(b2)) + float(np.float32(1) - np.float32(b2)) == 1.0
    # the EMA weight 1.f - mom has the same property, and is exact for mom >= 0.5
    for mom in (0.999, 0.5):
        assert float(np.float32(1) - np.float32(mom)) == 1.0 - float(np.float32(mom))
