"""GPU: every kernel of csrc/optim.hip, op by op, against the float64 references of oracle/optim_ref.py (which
tests/test_optim_cpu.py pins to torch on the CPU).

AdamW rule.  Errors are counted in units of 2^-23 times a per-quantity scale
(oracle/optim_cases.py, adamw_scales: p: |p_ref| + lr/(1-b1^step); m: |m_old| + |g grad_scale|; v: |v_ref|; floored at 2^-126).
On the same inputs the test evaluates a numpy float32 restatement of the header formula (one rounding per operation,
optim_ref.adamw_step_kernel_f32 -- a reference, not the code under test) and takes its worst metric e32 against
adamw_step_f64; the kernel must stay within MARGIN * max(e32, 1) with the MARGIN of oracle/judge.py, 4: fma contraction and another
association order change WHICH roundings happen, not how many.  A wrong coefficient shows at 50 units or more (the
documented gain deviation 1.f - b2_f vs float(1 - b2) alone is 110 units of v, which is why the float64 reference
takes the float-valued scalars the C ABI receives; test_second_moment_gain_deviates_from_torch_as_documented pins that
deviation against torch itself).  The reference is evaluated from the fp32 state the kernel got: one-step error, no
drift.
Observed on the MI355X (profiles/optim_op_errors.txt): worst kernel error / max(e32, 1) = 1.00 (OBSERVED_WORST_RATIO
below; p 3.21 / m 0.47 / v 2.11 units at most, all three in the resumed configuration), i.e. the kernels are as close
to float64 as plain fp32 arithmetic is.

tem_amp_unscale* are compared bit for bit (int32 views) with numpy's `g * f32(inv_scale)`, subnormal products
included.  They raise the flag on a non-finite PRODUCT where torch's _amp_foreach_non_finite_check_and_unscale_ looks
at the input: the two differ only when a finite gradient times inv_scale overflows, i.e. for loss scales below 1
(test_unscale_flags_the_product_not_the_input).
tem_amp_update_dev is compared state for state with optim_ref.ScalerState (pinned to torch._amp_update_scale_ on the
CPU), tem_ema_update with ema_f64 under the derived bound 2^-23 (|k mom| + |q (1-mom)|).

No test provokes a device fault: every refusal tested here is a host-side argument check or a device-side flag.
"""
import numpy as np
import pytest
import torch

from oracle import optim_ref
from oracle.judge import MARGIN
from oracle.optim_cases import (DEFAULT, SCALER_SETS, TINY, U, adamw_inputs, adamw_metric, adamw_scales,
                                overflow_sequence, resumed_state)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBSERVED_WORST_RATIO = 1.00      # informational; the assertion uses MARGIN

PASS4 = 2048 * 256 * 4           # tem_grid_1d caps the grid at 2048 blocks: floats per grid pass of the float4 kernels
PASS1 = 2048 * 256               # ... of the scalar kernels (k_ema, the unaligned path of the unscale kernels)
BIG = 2 * PASS4 + 1027           # a partial third pass plus a 3-element tail
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1027, 262147, BIG]

CONFIGS = {
    "fresh": dict(hp=DEFAULT, steps=(1, 2, 3, 4, 5), resumed=False),
    "resumed": dict(hp=dict(DEFAULT, lr=1e-4, grad_scale=1.0 / 3.0), steps=tuple(range(100000, 100005)), resumed=True),
    "nodecay": dict(hp=dict(DEFAULT, lr=1e-2, wd=0.0, grad_scale=0.5), steps=(1, 2, 3), resumed=False),
}
ADAMW_CASES = [(n, "fresh") for n in SIZES] + [(n, c) for n in (1027, BIG) for c in ("resumed", "nodecay")]


def _ops():
    from torch_em_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def _bits_equal(a, b):
    """bit for bit, -0.0 and NaN payloads included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _step_args(hp, step):
    return (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, hp["grad_scale"])


def _grad_of_round(g0, k):
    """a new gradient per step from one drawn array: rotated, sign flipped on odd rounds (k = 0: g0 itself)"""
    return g0 if k == 0 else np.ascontiguousarray(np.roll(g0, 7919 * k) * np.float32(-1 if k & 1 else 1))


def _judge(tag, out, state, g, step, hp, only=None, quantities="pmv"):
    """The AdamW rule on one step: `out` = the kernel's (p, m, v), `state` = the fp32 (p, m, v) it started from.
    `only`: boolean mask of the elements to judge."""
    ref = optim_ref.adamw_step_f64(state[0], g, state[1], state[2], step, **hp)
    r32 = optim_ref.adamw_step_kernel_f32(state[0], g, state[1], state[2], step, **hp)
    scales = adamw_scales(ref, state[1], g, step, hp)
    if only is not None:
        out, ref, r32, scales = ([x[only] for x in t] for t in (out, ref, r32, scales))
    e32 = adamw_metric(r32, ref, scales)
    ek = adamw_metric(out, ref, scales)
    print(f"OPTIM_ERR {tag} step={step} " + " ".join(
        f"{q}: kernel {ek[i]:.2f} f32 {e32[i]:.2f}" for i, q in enumerate("pmv") if q in quantities))
    for i, q in enumerate("pmv"):
        if q in quantities:
            assert ek[i] <= MARGIN * max(e32[i], 1.0), \
                f"{tag} step {step}: {q} is {ek[i]:.2f} units from float64, plain fp32 arithmetic {e32[i]:.2f}"
    return ek, e32


def _decay_factor(hp):
    """fl(1.f - lr * wd) -- the same value with or without contraction of the product into the subtraction"""
    f = np.float32
    two_roundings = f(1) - f(hp["lr"]) * f(hp["wd"])
    contracted = f(1.0 - float(f(hp["lr"])) * float(f(hp["wd"])))
    assert two_roundings == contracted
    return two_roundings


def _run_config(launch, n, cfg, tag):
    c = CONFIGS[cfg]
    hp = c["hp"]
    p, g0 = adamw_inputs(n, 100 + n % 997 + len(cfg))
    if n >= 3:
        g0[-1] = 0                      # a zero gradient in the scalar tail / the last float4
    m, v = resumed_state(n, n + 1) if c["resumed"] else (np.zeros(n, np.float32), np.zeros(n, np.float32))
    pd, md, vd = _dev(p), _dev(m), _dev(v)
    for k, step in enumerate(c["steps"]):
        g = _grad_of_round(g0, k)
        gd = _dev(g)
        launch(pd, gd, md, vd, hp, step)
        out = _host(pd, md, vd)
        assert np.array_equal(_host(gd), g), "the gradient is an input"
        _judge(f"{tag} n={n} {cfg}", out, (p, m, v), g, step, hp)
        if k == 0 and not c["resumed"]:
            z = g == 0
            assert n < 3 or z.any()
            assert not out[1][z].any() and not out[2][z].any(), "g = 0 on a zero state: m and v stay 0"
            assert np.array_equal(out[0][z], p[z] * _decay_factor(hp)), "g = 0 on a zero state: decay only"
        p, m, v = out


def _launch_step(pd, gd, md, vd, hp, step):
    _ops().adamw_step(pd, gd, md, vd, *_step_args(hp, step))


@pytest.mark.parametrize("n,cfg", ADAMW_CASES)
def test_adamw_step_against_float64(n, cfg):
    _run_config(_launch_step, n, cfg, "adamw_step")


def test_adamw_step_refuses_an_unaligned_arena():
    ops = _ops()
    n = 1027
    p, g = adamw_inputs(n, 5)
    m, v = resumed_state(n, 6)
    bufs = [torch.zeros(n + 1, device=DEV) for _ in range(4)]
    for b, a in zip(bufs, (p, g, m, v)):
        b[1:].copy_(_dev(a))
    before = [b.clone() for b in bufs]
    for bad in range(4):           # each of the four pointers in turn 4 bytes off a 16-byte boundary
        views = [b[1:] if i == bad else b[:n] for i, b in enumerate(bufs)]
        assert views[bad].data_ptr() % 16 == 4
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.adamw_step(*views, *_step_args(DEFAULT, 3))
        torch.cuda.synchronize()
        assert all(_bits_equal(b, b0) for b, b0 in zip(bufs, before))


def test_adamw_step_overflow_class_follows_torch_fp32():
    """|g| = 1e25: g^2 is inf in fp32.  v = inf, m finite, and the update m / inf = 0 leaves the decayed parameter --
    what torch.optim.AdamW does on fp32 CPU tensors."""
    ops = _ops()
    n = 1027
    p, g = adamw_inputs(n, 7)
    ovf = np.arange(n) % 2 == 1
    g[ovf] = np.where(np.random.RandomState(8).rand(ovf.sum()) < 0.5, -1e25, 1e25).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    topt = torch.optim.AdamW([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, foreach=False)
    tp.grad = torch.from_numpy(g.copy())
    topt.step()
    tv = topt.state[tp]["exp_avg_sq"].numpy()
    assert np.isposinf(tv[ovf]).all() and np.isfinite(tv[~ovf]).all()

    z = np.zeros(n, np.float32)
    pd, md, vd = _dev(p), _dev(z), _dev(z)
    ops.adamw_step(pd, _dev(g), md, vd, *_step_args(DEFAULT, 1))
    out = _host(pd, md, vd)
    assert np.isposinf(out[2][ovf]).all()
    assert np.isfinite(out[1]).all()
    assert np.array_equal(out[0][ovf], tp.detach().numpy()[ovf]), "p: torch's fp32 result, bit for bit"
    assert np.array_equal(out[0][ovf], p[ovf] * _decay_factor(DEFAULT)), "p: the decay-only value"
    _judge("adamw_step overflow-class", out, (p, z, z), g, 1, DEFAULT, only=ovf, quantities="m")
    _judge("adamw_step overflow-class, other elements", out, (p, z, z), g, 1, DEFAULT, only=~ovf)


def test_second_moment_gain_deviates_from_torch_as_documented():
    """The kernels' gain of g^2 is 1.f - b2_f, torch.optim.AdamW's is float(1 - b2): after step 1 from a zero state
    v_gpu / v_torch - 1 = delta +- 4 * 2^-23 with delta = -1.29e-5 (bounded on the CPU by
    test_optim_cpu.test_gain_deviation_is_bounded_by_the_rounding_of_beta2).  A change of the gain arithmetic fails here."""
    ops = _ops()
    b2 = 0.999
    delta = ((float(np.float32(1) - np.float32(b2))) - (1 - b2)) / (1 - b2)
    for n in (1027, 262147):
        p, g = adamw_inputs(n, 9)
        tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
        topt = torch.optim.AdamW([tp], lr=1e-3, betas=(0.9, b2), eps=1e-8, weight_decay=1e-2, foreach=False)
        tp.grad = torch.from_numpy(g.astype(np.float64))
        topt.step()
        tv = topt.state[tp]["exp_avg_sq"].numpy()
        pd, md, vd = _dev(p), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        ops.adamw_step(pd, _dev(g), md, vd, 1e-3, 0.9, b2, 1e-8, 1e-2, 1)
        v = _host(vd).astype(np.float64)
        nz = g != 0
        assert nz.sum() > 0.9 * n and not v[~nz].any()
        r = v[nz] / tv[nz] - 1.0
        print(f"OPTIM_ERR gain deviation n={n}: delta {delta:.4e}, v_gpu/v_torch - 1 in [{r.min():.4e}, {r.max():.4e}]")
        assert np.abs(r - delta).max() <= 4 * U


# ------------------------------------------------------------------------------------------ tem_adamw_step_dev
def _hyper(hp, step):
    host = torch.zeros(12, dtype=torch.float32)
    _ops().adamw_hyper(host, *_step_args(hp, step))
    return host


@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_adamw_hyper_rows(step):
    """slots 5 / 6 are the bias-corrected step size and 1 / sqrt(1 - b2^step), from doubles, of the FLOAT-valued
    scalars (what the C ABI receives; float32(lr / (1 - 0.9^2)) and float32(lr_f / (1 - b1_f^2)) differ by an ulp)."""
    for hp in (DEFAULT, CONFIGS["resumed"]["hp"], dict(DEFAULT, lr=3e-2, b1=0.5, b2=0.99, eps=1e-6, wd=0.25)):
        h = _hyper(hp, step).numpy()
        f = {k: float(np.float32(x)) for k, x in hp.items()}
        assert h[5] == np.float32(f["lr"] / (1.0 - f["b1"] ** step))
        assert h[6] == np.float32(1.0 / np.sqrt(1.0 - f["b2"] ** step))
        # ... and of the Python doubles themselves: the same values up to the rounding of lr, b1 and b2 to float
        for got, exact, b in ((h[5], hp["lr"] / (1.0 - hp["b1"] ** step), hp["b1"]),
                              (h[6], 1.0 / np.sqrt(1.0 - hp["b2"] ** step), hp["b2"])):
            # relative: 2^-24 for the scalar in the numerator, 2^-24 b^t t / (1 - b^t) for b^t, 2^-24 for the result
            amp = step * b ** step / (1.0 - b ** step)
            assert abs(float(got) - exact) <= 2.0 ** -24 * (2.0 + amp) * exact, (step, got, exact)
        assert np.array_equal(h[:5], np.array([hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"]], np.float32))
        assert h[7] == np.float32(hp["grad_scale"]) and not h[8:].any()


def _state_for(n, cfg, seed):
    p, g = adamw_inputs(n, seed)
    m, v = resumed_state(n, seed + 1) if CONFIGS[cfg]["resumed"] else (np.zeros(n, np.float32), np.zeros(n, np.float32))
    return p, g, m, v


@pytest.mark.parametrize("n", [1027, BIG])
def test_adamw_step_dev_is_bit_equal_to_adamw_step(n):
    ops = _ops()
    for cfg, step in (("fresh", 1), ("resumed", 100002), ("nodecay", 3)):
        hp = CONFIGS[cfg]["hp"]
        p, g, m, v = _state_for(n, cfg, 11)
        gd = _dev(g)
        a, b = [_dev(x) for x in (p, m, v)], [_dev(x) for x in (p, m, v)]
        ops.adamw_step(a[0], gd, a[1], a[2], *_step_args(hp, step))
        hyper = _hyper(hp, step).to(DEV)
        ops.adamw_step_dev(b[0], gd, b[1], b[2], hyper)
        assert not _bits_equal(a[0], _dev(p)), "the step moved the parameters"
        assert all(_bits_equal(x, y) for x, y in zip(a, b)), (cfg, step)
        assert np.array_equal(_host(hyper), _hyper(hp, step).numpy()), "hyper is an input"
        # skip != 0: nothing is touched
        hyper[8] = 1.0
        ops.adamw_step_dev(b[0], gd, b[1], b[2], hyper)
        assert all(_bits_equal(x, y) for x, y in zip(a, b)), "hyper[8] = 1 skips the step"


# ------------------------------------------------------------------------------------------ tem_adamw_step_tab
TABLE_ROWS = 16


def _table(applied, hp, rows=TABLE_ROWS):
    """What FusedAdamW.refresh_table(applied) uploads: [lo = applied + 1, rows, -, -] + one adamw_hyper row per step."""
    host = torch.zeros(4 + 12 * rows, dtype=torch.float32)
    host[0], host[1] = float(applied + 1), float(rows)
    for j in range(rows):
        _ops().adamw_hyper(host[4 + 12 * j:4 + 12 * (j + 1)], *_step_args(hp, applied + 1 + j))
    return host.to(DEV)


def _sstate(scale, tracker, flag, applied):
    return torch.tensor([scale, tracker, flag, applied], dtype=torch.float32, device=DEV)


def test_adamw_step_tab_selects_the_row_of_the_device_step_count():
    """16 rows for steps 3 .. 18: neighbouring rows differ by tens of percent in step_size, a wrong row cannot hide."""
    ops = _ops()
    n, lo, hp = 1027, 3, CONFIGS["resumed"]["hp"]
    p, g, m, v = _state_for(n, "resumed", 13)
    gd, table = _dev(g), _table(lo - 1, hp)
    table0 = table.clone()
    assert float(table[0]) == lo and float(table[1]) == TABLE_ROWS

    for applied in (lo - 1, lo, lo + 14):                       # rows 0, 1, 15
        ss = _sstate(65536.0, 1.0, 0.0, applied)
        a, b = [_dev(x) for x in (p, m, v)], [_dev(x) for x in (p, m, v)]
        ops.adamw_step(a[0], gd, a[1], a[2], *_step_args(hp, applied + 1))
        ops.adamw_step_tab(b[0], gd, b[1], b[2], table, ss)
        assert all(_bits_equal(x, y) for x, y in zip(a, b)), applied
        assert not _bits_equal(b[0], _dev(p))
        assert _bits_equal(ss, _sstate(65536.0, 1.0, 0.0, applied)), "sstate is read only on an applied step"

    for applied in (lo - 2, lo + 15):                           # rows -1 and 16: outside the window
        ss = _sstate(65536.0, 1.0, 0.0, applied)
        b = [_dev(x) for x in (p, m, v)]
        ops.adamw_step_tab(b[0], gd, b[1], b[2], table, ss)
        assert all(_bits_equal(x, _dev(y)) for x, y in zip(b, (p, m, v))), "refused: nothing is updated"
        assert _bits_equal(ss, _sstate(65536.0, 1.0, 1.0, applied)), "refused: reported like an overflow"
        ops.amp_update_dev(ss, 2.0, 0.5, 2000)
        assert _bits_equal(ss, _sstate(32768.0, 0.0, 0.0, applied)), "the refused step backs off and is not counted"

    ss = _sstate(65536.0, 1.0, 1.0, lo)                         # flag up, row inside the window
    b = [_dev(x) for x in (p, m, v)]
    ops.adamw_step_tab(b[0], gd, b[1], b[2], table, ss)
    assert all(_bits_equal(x, _dev(y)) for x, y in zip(b, (p, m, v)))
    assert _bits_equal(ss, _sstate(65536.0, 1.0, 1.0, lo)), "the flag stays up for the update kernel"
    assert _bits_equal(table, table0) and np.array_equal(_host(gd), g)


def test_adamw_step_tab_keeps_stepping_when_the_float_step_count_saturates():
    """sstate[3] is a float: it counts to 2^24 and stays there.  float(2^24 + 1) rounds to 2^24 too, so the table the
    host builds from a count of 2^24 starts at lo = 2^24 and the kernel takes row 1 -- a step number at which the bias
    corrections have long been 1.  The step is applied and the flag stays down."""
    ops = _ops()
    n, hp = 1027, DEFAULT
    p, g0, m, v = _state_for(n, "resumed", 17)
    pd, md, vd = _dev(p), _dev(m), _dev(v)
    ss = _sstate(65536.0, 0.0, 0.0, 2.0 ** 24 - 2)
    model = optim_ref.ScalerState(65536.0, 0.0, 0.0, 2.0 ** 24 - 2)
    for k in range(4):
        known = int(_host(ss)[3])
        table = _table(known, hp)
        row = int(np.float32(known)) + 1 - int(_host(table)[0])
        assert 0 <= row < TABLE_ROWS
        g = _grad_of_round(g0, k)
        ops.adamw_step_tab(pd, _dev(g), md, vd, table, ss)
        out = _host(pd, md, vd)
        assert float(ss[2]) == 0.0, "the flag never rises"
        assert not np.array_equal(out[0], p), "the step is applied"
        _judge(f"adamw_step_tab saturated count, round {k} row {row}", out, (p, m, v), g, known + 1 + row, hp)
        p, m, v = out
        ops.amp_update_dev(ss, 2.0, 0.5, 3)
        model.update(2.0, 0.5, 3)
        assert np.array_equal(_host(ss), model.as_array())
    assert float(ss[3]) == 2.0 ** 24


# ------------------------------------------------------------------------------------------ tem_amp_unscale(_dev)
class _Plain:
    """tem_amp_unscale: inv_scale by value, the flag a 1-float tensor"""

    def __init__(self, inv_scale):
        self.inv = np.float32(inv_scale)

    def new_state(self, up=False):
        return torch.tensor([1.0 if up else 0.0], dtype=torch.float32, device=DEV)

    def launch(self, gd, st):
        _ops().amp_unscale(gd, float(self.inv), st)

    def flag(self, st):
        return float(st[0])

    def check_rest(self, st):
        pass


class _OnDevice:
    """tem_amp_unscale_dev: inv_scale = 1.f / sstate[0] on the device, the flag is sstate[2]"""

    def __init__(self, scale):
        self.scale = np.float32(scale)
        self.inv = np.float32(1) / self.scale

    def new_state(self, up=False):
        return _sstate(float(self.scale), 7.0, 1.0 if up else 0.0, 41.0)

    def launch(self, gd, st):
        _ops().amp_unscale_dev(gd, st)

    def flag(self, st):
        return float(st[2])

    def check_rest(self, st):
        assert _bits_equal(st[[0, 1, 3]], _sstate(float(self.scale), 7.0, 0.0, 41.0)[[0, 1, 3]])


def _unscale_inputs(n, seed):
    _, g = adamw_inputs(n, seed)
    g *= np.float32(2.0 ** 16)          # gradients as they arrive: scaled
    tiny = np.array([1e-36, -3e-37, 1.2e-38, -1.5e-38, 1e-42], np.float32)    # products (or inputs) below 2^-126
    if n >= 1027:
        g[3:3 + 5], g[n - 5:] = tiny, tiny[::-1]
        g[n // 4 * 4 - 2] = np.float32(-2e-37)
    return g


def _placements(n, pass_elems):
    n4 = n // 4
    pos = {0, n - 1} | set(range(4 * n4, n))                    # first, last, every position of the scalar tail
    if n4:
        pos |= {4 * (n4 // 2) + 1, 4 * n4 - 1}                  # the middle of the float4 body, lane 3 of the last float4
    pos |= {q for q in (pass_elems + 5, 2 * pass_elems + 2) if q < n}   # the second and third grid pass
    return sorted(pos)


def _view(arr, aligned):
    """a device copy of arr: 16-byte aligned, or 4 bytes past a 16-byte boundary (the kernels' scalar path)"""
    n = arr.size
    if aligned:
        t = _dev(arr)
    else:
        t = torch.zeros(n + 1, dtype=torch.float32, device=DEV)[1:1 + n]
        t.copy_(_dev(arr))
    assert t.data_ptr() % 16 == (0 if aligned else 4)
    return t


def _check_unscale(kind, n, aligned=True):
    g = _unscale_inputs(n, 21 + n % 89)
    with np.errstate(under="ignore"):
        exp = g * kind.inv
    if n >= 1027 and float(kind.inv) < 1e-3:
        sub = (exp != 0) & (np.abs(exp) < TINY)
        assert sub.sum() >= 5, "the inputs hold subnormal products"
    exp_d = _dev(exp)

    def fresh():
        return _view(g, aligned)

    def equal_except(gd, pos):
        chk = gd.clone()
        if pos is not None:
            chk[pos] = exp_d[pos]
        return _bits_equal(chk, exp_d)

    st, gd = kind.new_state(), fresh()                         # clean input: values bit-equal, flag stays down
    kind.launch(gd, st)
    assert equal_except(gd, None), "values differ from numpy's g * f32(inv_scale)"
    assert kind.flag(st) == 0.0
    kind.check_rest(st)
    clean = gd
    st, gd = kind.new_state(up=True), fresh()                  # a raised flag stays raised
    kind.launch(gd, st)
    assert kind.flag(st) == 1.0 and equal_except(gd, None)

    for pos in _placements(n, PASS4 if aligned else PASS1):
        for bad in (np.inf, -np.inf, np.nan):
            st, gd = kind.new_state(), fresh()
            gd[pos] = bad
            kind.launch(gd, st)
            assert kind.flag(st) == 1.0, (n, pos, bad)
            got = float(gd[pos])
            assert np.isnan(got) if np.isnan(bad) else got == bad, (n, pos, bad, got)
            assert equal_except(gd, pos), (n, pos, bad)
            kind.check_rest(st)
    return clean


@pytest.mark.parametrize("n", [1, 3, 5, 1027, BIG])
def test_amp_unscale_values_and_flag(n):
    _check_unscale(_Plain(2.0 ** -16), n)
    if n <= 1027:
        _check_unscale(_Plain(1e-3), n)                         # an inv_scale that rounds


@pytest.mark.parametrize("n", [3, 1027, 2 * PASS1 + 3])
def test_amp_unscale_unaligned_view_takes_the_scalar_path(n):
    kind = _Plain(2.0 ** -16)
    a = _check_unscale(kind, n, aligned=False)
    b = _check_unscale(kind, n, aligned=True)
    assert _bits_equal(a, b)


def test_unscale_flags_the_product_not_the_input():
    """g = 3e38 is finite, g * 2 is not: the kernel raises the flag on the PRODUCT.  torch's unscale checks the
    input.  The two differ only for inv_scale > 1, i.e. a loss scale below 1, which the scaler reaches only after
    17 consecutive overflows from its initial 2^16."""
    ops = _ops()
    g = np.array([1.0, -2.0, 3e38, 4.0, 5.0], np.float32)
    gd, flag = _dev(g), torch.zeros(1, device=DEV)
    ops.amp_unscale(gd, 2.0, flag)
    assert float(flag[0]) == 1.0
    assert np.array_equal(_host(gd), np.array([2.0, -4.0, np.inf, 8.0, 10.0], np.float32))
    gd, ss = _dev(g), _sstate(0.5, 0.0, 0.0, 0.0)
    ops.amp_unscale_dev(gd, ss)
    assert np.array_equal(_host(ss), np.array([0.5, 0.0, 1.0, 0.0], np.float32))
    assert np.array_equal(_host(gd), np.array([2.0, -4.0, np.inf, 8.0, 10.0], np.float32))


@pytest.mark.parametrize("scale,n,aligned", [(65536.0, 3, True), (65536.0, 1027, True), (2.0 ** -3, 5, True),
                                             (2.0 ** -3, 1027, True), (1000.0, 1, True), (1000.0, 1027, True),
                                             (1000.0, 1027, False), (1000.0, BIG, True), (65536.0, 2 * PASS1 + 3, False)])
def test_amp_unscale_dev_values_and_flag(scale, n, aligned):
    """expected values g * (f32(1) / f32(scale)): the device divides once, correctly rounded"""
    _check_unscale(_OnDevice(scale), n, aligned=aligned)


# ------------------------------------------------------------------------------------------ tem_amp_update_dev
@pytest.mark.parametrize("key", list(SCALER_SETS))
def test_amp_update_dev_follows_the_host_model(key):
    ops = _ops()
    growth, backoff, interval = key
    seq = overflow_sequence(key)
    flags = _dev(seq)
    ss = _sstate(65536.0, 0.0, 0.0, 0.0)
    snaps = torch.zeros(len(seq), 4, dtype=torch.float32, device=DEV)
    model, exp = optim_ref.ScalerState(65536.0), []
    for i, bad in enumerate(seq):
        ss[2:3].copy_(flags[i:i + 1])
        ops.amp_update_dev(ss, growth, backoff, interval)
        snaps[i].copy_(ss)
        if bad:
            model.raise_flag()
        exp.append(model.update(growth, backoff, interval).as_array())
    got = _host(snaps)
    exp = np.stack(exp)
    assert np.array_equal(got.view(np.int32), exp.view(np.int32)), \
        f"first difference at step {int(np.argmax((got != exp).any(axis=1)))}"
    assert exp[-1, 3] == (seq == 0).sum()


def test_amp_update_dev_refuses_bad_arguments():
    ops = _ops()
    ss = _sstate(65536.0, 1.0, 1.0, 5.0)
    for growth, backoff, interval in ((1.0, 0.5, 3), (0.5, 0.5, 3), (2.0, 1.0, 3), (2.0, 1.5, 3), (2.0, 0.5, 0),
                                      (2.0, 0.5, -1)):
        with pytest.raises(ValueError):
            ops.amp_update_dev(ss, growth, backoff, interval)
    assert _bits_equal(ss, _sstate(65536.0, 1.0, 1.0, 5.0))


# ------------------------------------------------------------------------------------------ the three kernels in sequence
def test_device_side_sequence_against_float64():
    """24 rounds of amp_unscale_dev -> adamw_step_tab -> amp_update_dev (interval 3) on gradients pre-multiplied by the
    current scale; rounds 2, 3 and 9 carry one inf and must be skipped.  The final p against a float64 AdamW chain that
    saw only the clean rounds, steps 1, 2, ...: within 4 x the deviation of the numpy float32 restatement chain from
    that float64 chain, both in units of 2^-23 * sum over the steps of (|p_ref| + lr / (1 - b1^step)).  No floor of one
    unit here: the bound is 4 x what the restatement chain shows (0.57 units for p on these inputs, so 2.3)."""
    ops = _ops()
    n, hp, bad_rounds = 4099, DEFAULT, {2: 0, 3: 2050, 9: 4098}
    growth, backoff, interval = 2.0, 0.5, 3
    p0, _ = adamw_inputs(n, 31)
    z = np.zeros(n, np.float32)
    pd, md, vd = _dev(p0), _dev(z), _dev(z)
    ss = _sstate(65536.0, 0.0, 0.0, 0.0)
    snaps = torch.zeros(24, 4, dtype=torch.float32, device=DEV)
    model, exp = optim_ref.ScalerState(65536.0), []
    c64, c32 = (p0.astype(np.float64), z.astype(np.float64), z.astype(np.float64)), (p0, z, z)
    scale_sum, scale_sum_v, step = np.zeros(n), np.zeros(n), 0
    for r in range(24):
        g = adamw_inputs(n, 40 + r)[1]
        scaled = g * np.float32(model.scale)
        assert np.array_equal(scaled / np.float32(model.scale), g), "a power-of-two scale: unscaling is exact"
        if r in bad_rounds:
            scaled[bad_rounds[r]] = np.inf
            model.raise_flag()
        else:
            step += 1
            c64 = optim_ref.adamw_step_f64(*c64[:1], g, *c64[1:], step, **hp)
            c32 = optim_ref.adamw_step_kernel_f32(*c32[:1], g, *c32[1:], step, **hp)
            scale_sum += U * np.maximum(np.abs(c64[0]) + float(np.float32(hp["lr"])) /
                                        (1.0 - float(np.float32(hp["b1"])) ** step), TINY)
            scale_sum_v += U * np.maximum(c64[2], TINY)
        gd = _dev(scaled)
        table = _table(int(model.applied_steps), hp)
        ops.amp_unscale_dev(gd, ss)
        ops.adamw_step_tab(pd, gd, md, vd, table, ss)
        ops.amp_update_dev(ss, growth, backoff, interval)
        snaps[r].copy_(ss)
        exp.append(model.update(growth, backoff, interval).as_array())
    assert step == 21
    assert np.array_equal(_host(snaps), np.stack(exp)), "sstate follows the host model round by round"
    e32 = float((np.abs(c32[0].astype(np.float64) - c64[0]) / scale_sum).max())
    ek = float((np.abs(_host(pd).astype(np.float64) - c64[0]) / scale_sum).max())
    print(f"OPTIM_ERR device sequence n={n}, 21 applied steps p: kernel {ek:.3f} f32 {e32:.3f}")
    assert ek <= MARGIN * e32
    # the second moment saw the same 21 gradients: the same rule, in units of 2^-23 * sum over the steps of |v_ref|
    e32 = float((np.abs(c32[2].astype(np.float64) - c64[2]) / scale_sum_v).max())
    ek = float((np.abs(_host(vd).astype(np.float64) - c64[2]) / scale_sum_v).max())
    print(f"OPTIM_ERR device sequence n={n}, 21 applied steps v: kernel {ek:.3f} f32 {e32:.3f}")
    assert ek <= MARGIN * e32


# ------------------------------------------------------------------------------------------ tem_ema_update
@pytest.mark.parametrize("n", [1, 3, 1027, BIG])
def test_ema_update_against_float64(n):
    """|delta| <= 2^-23 (|k mom| + |q (1 - mom)|): three roundings of 2^-24 each (two products, one sum; 1.f - mom is
    exact for mom >= 0.5 and for 0).  BIG is 9 grid passes of this scalar kernel."""
    ops = _ops()
    rng = np.random.RandomState(n % 1000)
    k = (rng.randn(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    q = (rng.randn(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    qd = _dev(q)
    for mom in (0.999, 0.5, 0.0):
        kd = _dev(k)
        ops.ema_update(kd, qd, mom)
        got = _host(kd).astype(np.float64)
        ref = optim_ref.ema_f64(k, q, mom)
        mf = float(np.float32(mom))
        bound = U * (np.abs(k.astype(np.float64) * mf) + np.abs(q.astype(np.float64) * (1.0 - mf)))
        ratio = float((np.abs(got - ref) / np.maximum(bound, TINY)).max())
        r32 = float((np.abs(optim_ref.ema_kernel_f32(k, q, mom).astype(np.float64) - ref) / np.maximum(bound, TINY)).max())
        print(f"OPTIM_ERR ema_update n={n} mom={mom}: kernel {ratio:.3f} f32 {r32:.3f} of the bound")
        assert (np.abs(got - ref) <= bound).all(), (mom, ratio)
        if mom == 0.0:
            assert np.array_equal(_host(kd), q)
    assert np.array_equal(_host(qd), q), "theta_q is an input"


# ------------------------------------------------------------------------------------------ FusedAdamW, one launch per tensor
def test_fused_adamw_on_plain_tensors():
    """Two groups with different lr / weight_decay: FusedAdamW launches tem_adamw_step once per parameter.  3 steps
    against torch.optim.AdamW in float64 on the CPU (Python-double scalars).  Per tensor, in the chain form of the
    rule: |p - p_torch| <= 4 max(e32, 1) S + sum over the steps of |delta| / 2 * lr / (1 - b1^step), S = 2^-23 * sum
    over the steps of (|p_ref| + lr / (1 - b1^step)), e32 the float32 restatement chain against the float64 chain with
    float-valued scalars, delta the documented gain deviation (sqrt(v) moves by delta / 2).  The floor of one unit is
    the AdamW rule's own (module docstring), applied to the chain: a 1-element tensor has a restatement error near 0.
    exp_avg_sq likewise: |v - v_torch| <= 4 max(e32v, 1) Sv + (|delta| + 2 |b2_f - b2| / b2) v_torch, Sv = 2^-23 * sum
    over the steps of |v_ref|.
    state_dict: the per-parameter keys, the parameter indices of the groups and the top-level keys equal torch's;
    FusedAdamW holds a (step 0) entry for the parameter without a gradient, torch creates its entries lazily."""
    from torch_em_amd.optim import FusedAdamW
    shapes = [(1,), (5,), (2, 513), (4099,), (3,)]               # the last one never gets a gradient
    groups = [dict(idx=(0, 2, 4), lr=1e-3, wd=1e-2), dict(idx=(1, 3), lr=3e-3, wd=0.1)]
    rng = np.random.RandomState(51)
    init = [rng.randn(*s).astype(np.float32) for s in shapes]
    dp = [torch.nn.Parameter(_dev(x)) for x in init]
    tp = [torch.nn.Parameter(torch.from_numpy(x.astype(np.float64))) for x in init]
    opt = FusedAdamW([dict(params=[dp[i] for i in g["idx"]], lr=g["lr"], weight_decay=g["wd"]) for g in groups])
    topt = torch.optim.AdamW([dict(params=[tp[i] for i in g["idx"]], lr=g["lr"], weight_decay=g["wd"]) for g in groups],
                             betas=(0.9, 0.999), eps=1e-8, foreach=False)
    hp_of = {i: dict(DEFAULT, lr=g["lr"], wd=g["wd"]) for g in groups for i in g["idx"]}
    delta = abs(optim_ref.gain_deviation(0.999))
    c64 = {i: (init[i].astype(np.float64).ravel(), np.zeros(init[i].size), np.zeros(init[i].size)) for i in range(4)}
    c32 = {i: (init[i].ravel(), np.zeros(init[i].size, np.float32), np.zeros(init[i].size, np.float32)) for i in range(4)}
    S = {i: np.zeros(init[i].size) for i in range(4)}
    Sv = {i: np.zeros(init[i].size) for i in range(4)}
    widen = {i: 0.0 for i in range(4)}
    for step in (1, 2, 3):
        for i in range(4):
            g = adamw_inputs(init[i].size, 60 + 10 * step + i)[1]
            dp[i].grad = _dev(g.reshape(shapes[i]))
            tp[i].grad = torch.from_numpy(g.astype(np.float64).reshape(shapes[i]))
            hp = hp_of[i]
            c64[i] = optim_ref.adamw_step_f64(c64[i][0], g, c64[i][1], c64[i][2], step, **hp)
            c32[i] = optim_ref.adamw_step_kernel_f32(c32[i][0], g, c32[i][1], c32[i][2], step, **hp)
            full = float(np.float32(hp["lr"])) / (1.0 - float(np.float32(0.9)) ** step)
            S[i] += U * np.maximum(np.abs(c64[i][0]) + full, TINY)
            widen[i] += delta / 2 * full
            Sv[i] += U * np.maximum(c64[i][2], TINY)
        opt.step()
        topt.step()
    for i in range(4):
        got = _host(dp[i].detach()).astype(np.float64).ravel()
        ref = tp[i].detach().numpy().ravel()
        e32 = float((np.abs(c32[i][0].astype(np.float64) - c64[i][0]) / S[i]).max())
        allowed = MARGIN * max(e32, 1.0) * S[i] + widen[i]
        err = np.abs(got - ref)
        print(f"OPTIM_ERR FusedAdamW per-tensor n={init[i].size}: |p - p_torch| / allowed {float((err / allowed).max()):.3f}, "
              f"f32 chain {e32:.2f} units")
        assert (err <= allowed).all(), (i, float((err / allowed).max()))
        assert float(opt.state[dp[i]]["step"]) == 3.0
        assert opt.state[dp[i]]["exp_avg"].shape == dp[i].shape
        tv = topt.state[tp[i]]["exp_avg_sq"].numpy().ravel()
        v = _host(opt.state[dp[i]]["exp_avg_sq"]).astype(np.float64).ravel()
        # exp_avg_sq, the same chain form: the rule against the float64 chain with float-valued scalars (units of
        # 2^-23 * sum over the steps of |v_ref|, e32v from the restatement chain on these inputs), and from that chain
        # to torch's the gain deviation delta on every term plus the rounding of b2 itself in the two decays a term
        # of step 1 has seen by step 3
        e32v = float((np.abs(c32[i][2].astype(np.float64) - c64[i][2]) / Sv[i]).max())
        decays = 2 * abs(float(np.float32(0.999)) - 0.999) / 0.999
        allowed_v = MARGIN * max(e32v, 1.0) * Sv[i] + (delta + decays) * tv
        print(f"OPTIM_ERR FusedAdamW per-tensor n={init[i].size}: |v - v_torch| / allowed "
              f"{float((np.abs(v - tv) / np.maximum(allowed_v, TINY)).max()):.3f}, f32 chain {e32v:.2f} units")
        assert (np.abs(v - tv) <= allowed_v).all(), "exp_avg_sq: torch's, within the deviation"
    assert np.array_equal(_host(dp[4].detach()), init[4]), "no gradient: bit-unchanged"
    assert float(opt.state[dp[4]]["step"]) == 0.0
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert sd.keys() == tsd.keys()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in tsd["param_groups"]]
    assert set(tsd["state"]) <= set(sd["state"])
    for idx, entry in tsd["state"].items():
        assert sd["state"][idx].keys() == entry.keys()
        assert float(sd["state"][idx]["step"]) == float(entry["step"])
