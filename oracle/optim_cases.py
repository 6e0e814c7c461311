"""Inputs, error metric and overflow sequences shared by tests/test_optim_cpu.py and tests/test_gpu_optim.py (TEST
INFRASTRUCTURE, see oracle/__init__.py; the references themselves are in oracle/optim_ref.py).

Error metric of the AdamW comparisons: units of 2^-23 times a per-quantity scale, every scale floored at 2^-126 (the
smallest normal float: an fp32 result cannot be expected to agree below it):
  p: |p_ref| + lr / (1 - b1^step)     the parameter plus the size of one full Adam update
  m: |m_old| + |g * grad_scale|       the lerp cancels, so the result itself is the wrong scale
  v: |v_ref|
"""
import numpy as np

from .judge import TINY, U

DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, grad_scale=1.0)

# (growth, backoff, interval) -> probability of an overflow per step, chosen so that the scale keeps away from both
# ends of the float range over 200 steps (torch refuses to grow the scale to inf, the kernel has no such case)
SCALER_SETS = {(2.0, 0.5, 3): 0.2, (2.0, 0.5, 1): 0.5, (1.5, 0.25, 5): 0.06}
SCALER_STEPS = 240


def adamw_inputs(n, seed):
    """p ~ N(0,1); g = N(0,1) * 10^U(-6,3) per element, about 1 % of them exactly 0."""
    rng = np.random.RandomState(seed)
    p = rng.randn(n).astype(np.float32)
    g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    g[rng.rand(n) < 0.01] = 0
    return p, g


def resumed_state(n, seed):
    """m ~ 0.1 N(0,1), v ~ U(1e-3, 0.5): a state as it looks late in a run."""
    rng = np.random.RandomState(seed)
    return (0.1 * rng.randn(n)).astype(np.float32), rng.uniform(1e-3, 0.5, n).astype(np.float32)


def adamw_scales(ref, m_old, g, step, hp):
    """The per-element scales of the metric for (p, m, v), in absolute terms (already times 2^-23)."""
    p_ref, _, v_ref = ref
    b1 = float(np.float32(hp["b1"]))
    full = float(np.float32(hp["lr"])) / (1.0 - b1 ** step)
    gs = float(np.float32(hp["grad_scale"]))
    sp = np.maximum(np.abs(p_ref) + full, TINY)
    sm = np.maximum(np.abs(np.asarray(m_old, np.float64)) + np.abs(np.asarray(g, np.float64) * gs), TINY)
    sv = np.maximum(np.abs(v_ref), TINY)
    return U * sp, U * sm, U * sv


def adamw_metric(out, ref, scales):
    """Worst error of (p, m, v) in metric units; non-finite disagreement counts as inf."""
    worst = []
    for o, r, s in zip(out, ref, scales):
        with np.errstate(invalid="ignore"):
            e = np.abs(np.asarray(o, np.float64) - r) / s
        e = np.where(np.isnan(e), np.inf, e)
        worst.append(float(e.max()))
    return tuple(worst)


def overflow_sequence(key, steps=SCALER_STEPS):
    """Seeded 0/1 sequence for one of SCALER_SETS: 1 = this step's gradients overflowed."""
    growth, backoff, interval = key
    rng = np.random.RandomState(1000 + interval)
    return (rng.rand(steps) < SCALER_SETS[key]).astype(np.float32)
