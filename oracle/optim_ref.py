"""CPU restatement of the optimizer arithmetic (TEST INFRASTRUCTURE, see oracle/__init__.py).

adamw_step(): torch.optim.AdamW single-tensor update as configured by the reference
  (/root/reference/torch_em/segmentation.py:543: lr, betas=(0.9,0.999), eps=1e-8, weight_decay=1e-2).
ema(): SPOCOTrainer._momentum_update /root/reference/torch_em/trainer/spoco_trainer.py:45-47.

Float64 references of the kernels in torch_em_amd/csrc/optim.hip (tests/test_optim_cpu.py pins them on the CPU,
tests/test_gpu_optim.py judges the kernels against them):
adamw_step_f64(): the formula in the header of optim.hip in float64.  `hyper_as_float32=True` rounds the scalars to
  float32 first -- what the C ABI receives -- so the gains are 1 - b1_f and 1 - b2_f like the kernel's `1.f - b1`;
  `hyper_as_float32=False` is torch.optim.AdamW with Python-double scalars (gains float(1 - b1), float(1 - b2)).
adamw_step_kernel_f32(): the same formula with every operation rounded to float32, in the kernel's order and with the
  kernel's host-side scalars (step_size, inv_sqrt_bc2 from doubles).  A REFERENCE for how far plain fp32 arithmetic
  sits from float64 on given inputs (no fma contraction), not a model of the compiled code.
gain_deviation(): the relative difference of the kernel's second-moment gain `1.f - b2_f` from torch's float(1 - b2).
ema_f64(), ema_kernel_f32(): the EMA update likewise (float-valued momentum).
ScalerState: host model of the device-side GradScaler state [scale, growth_tracker, found_inf, applied_steps]
  (tem_amp_update_dev; the two flag writers tem_amp_unscale_dev / tem_adamw_step_tab raise found_inf).
"""
import numpy as np


def adamw_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2):
    p = p * np.float32(1.0 - lr * weight_decay)
    m = m + np.float32(1 - beta1) * (g - m)
    v = np.float32(beta2) * v + np.float32(1 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = np.sqrt(v) / np.float32(np.sqrt(bc2)) + np.float32(eps)
    p = p - np.float32(lr / bc1) * (m / denom)
    return p.astype("float32"), m.astype("float32"), v.astype("float32")


def ema(theta_k, theta_q, momentum):
    return (theta_k * np.float32(momentum) + theta_q * np.float32(1.0 - momentum)).astype("float32")


def _f32(x):
    return float(np.float32(x))


def adamw_step_f64(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, grad_scale=1.0,
                   hyper_as_float32=True):
    """One AdamW step in float64 on float64 copies of the inputs; returns (p, m, v) as float64 arrays."""
    if hyper_as_float32:
        lr, b1, b2, eps, wd, grad_scale = (_f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    g = g * grad_scale
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adamw_step_kernel_f32(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, grad_scale=1.0):
    """The header formula of optim.hip with one float32 rounding per operation; returns float32 (p, m, v)."""
    f = np.float32
    lr_, b1_, b2_, eps_, wd_, gs_ = (f(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    step_size = f(float(lr_) / (1.0 - float(b1_) ** step))
    inv_sqrt_bc2 = f(1.0 / np.sqrt(1.0 - float(b2_) ** step))
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    with np.errstate(over="ignore", invalid="ignore"):
        gr = g * gs_
        pp = p * (f(1) - lr_ * wd_)
        mm = m + (f(1) - b1_) * (gr - m)
        vv = b2_ * v + (f(1) - b2_) * gr * gr
        denom = np.sqrt(vv) * inv_sqrt_bc2 + eps_
        pp = pp - step_size * (mm / denom)
    assert pp.dtype == mm.dtype == vv.dtype == np.float32
    return pp, mm, vv


def gain_deviation(b2=0.999):
    """((1.f - b2_f) - (1 - b2)) / (1 - b2): the kernel's float gain against torch's double gain, relative."""
    kernel_gain = float(np.float32(1) - np.float32(b2))
    return (kernel_gain - (1.0 - b2)) / (1.0 - b2)


def ema_f64(k, q, momentum):
    mom = _f32(momentum)
    return np.asarray(k, dtype=np.float64) * mom + np.asarray(q, dtype=np.float64) * (1.0 - mom)


def ema_kernel_f32(k, q, momentum):
    mom = np.float32(momentum)
    return np.asarray(k, np.float32) * mom + np.asarray(q, np.float32) * (np.float32(1) - mom)


class ScalerState:
    """[scale, growth_tracker, found_inf, applied_steps] as four float32 values, updated as the device updates them."""

    def __init__(self, scale=2.0 ** 16, growth_tracker=0.0, found_inf=0.0, applied_steps=0.0):
        self.s = np.array([scale, growth_tracker, found_inf, applied_steps], dtype=np.float32)

    scale = property(lambda self: float(self.s[0]))
    growth_tracker = property(lambda self: int(self.s[1]))
    found_inf = property(lambda self: float(self.s[2]))
    applied_steps = property(lambda self: float(self.s[3]))

    def raise_flag(self):
        self.s[2] = 1.0

    def update(self, growth, backoff, interval):
        """tem_amp_update_dev: torch's _amp_update_scale_ (without its refusal to grow the scale to inf, which the
        kernel does not have), the count of applied steps in float32 (it saturates at 2^24), the flag reset."""
        s = self.s
        if s[2] != 0:
            s[0] = s[0] * np.float32(backoff)
            s[1] = 0
        else:
            t = s[1] + np.float32(1)
            if int(t) == int(interval):
                s[0] = s[0] * np.float32(growth)
                s[1] = 0
            else:
                s[1] = t
            s[3] = s[3] + np.float32(1)
        s[2] = 0
        return self

    def as_array(self):
        return self.s.copy()
