"""Inputs and coefficient sets shared by tests/test_dice_cpu.py and tests/test_gpu_dice.py (TEST INFRASTRUCTURE).

Logits: 2 randn with planted +-16, +-17, +-40, +-90 (sigmoid rounds to 1 - 2^-24 / 1, underflows, is a float32
subnormal).  Probabilities: uniform with planted exact 0, 1, 1e-8 and 1 - 2^-24 (the log clamp at -100, the 1e-12 clamp of
the cross-entropy gradient).  Targets: binary or soft.  Masks: binary, about 30 % zeros.
The LAST voxel of every (sample, channel) row and the first voxel of the row's last 256-voxel tile are anchors -- prediction
0.75 (logit 1.5), target 1 (soft: 0.875), mask 1 -- so a kernel that drops a tail loses terms of order 1 from every column.
"""
import numpy as np

from . import dice_ref

PLANT_LOGITS = np.array([16, -16, 17, -17, 40, -40, 90, -90], np.float32)
PLANT_PROBS = np.array([0.0, 1.0, 1e-8, 1.0 - 2.0 ** -24, 0.0, 1.0, 1e-8, 1.0 - 2.0 ** -24], np.float32)


def _plant(a, values, rng):
    flat = a.reshape(-1)
    if flat.size >= 4 * values.size:
        flat[rng.choice(flat.size, values.size, replace=False)] = values
    else:                                   # tiny tensors: as many as fit into every other element
        k = min(values.size, flat.size // 2)
        flat[:2 * k:2] = values[:k]


def anchors(V):
    """voxel indices of the anchors of a row of V voxels"""
    return sorted({V - 1, 256 * ((V - 1) // 256)})


def make_inputs(N, C, V, seed, logits, soft, masked=True):
    """-> (p, t, m): float32 [N, C, V]; m is None unless `masked`"""
    rng = np.random.RandomState(seed)
    if logits:
        p = (2.0 * rng.randn(N, C, V)).astype(np.float32)
        _plant(p, PLANT_LOGITS, rng)
    else:
        p = rng.uniform(0.0, 1.0, (N, C, V)).astype(np.float32)
        _plant(p, PLANT_PROBS, rng)
    t = rng.uniform(0.0, 1.0, (N, C, V)).astype(np.float32)
    if not soft:
        t = (t < 0.5).astype(np.float32)
    m = (rng.uniform(0.0, 1.0, (N, C, V)) >= 0.3).astype(np.float32) if masked else None
    for v in anchors(V):
        p[:, :, v] = 1.5 if logits else 0.75
        t[:, :, v] = 0.875 if soft else 1.0
        if m is not None:
            m[:, :, v] = 1.0
    return p, t, m


def coefficients(p, t, mask, flags, special=True):
    """the float32-rounded (ca, cb) of DiceLoss (channelwise, sum) on these inputs from the float64 oracle; with
    `special`, channel 0 gets cb = 0 and the last channel ca = cb = 0 (C >= 2)"""
    sums = dice_ref.dice_sums_f64(p, t, mask, flags & dice_ref.LOGITS)
    _, ca, cb = dice_ref.dice_finalize_f64(sums, 1e-7, True, True, "sum")
    ca, cb = ca.astype(np.float32), cb.astype(np.float32)
    if special and ca.size >= 2:
        cb[0] = 0.0
        ca[-1] = cb[-1] = 0.0
    return ca, cb


def gout_variant(kind, C, seed):
    """kind 0: NULL (= 1); 1: a scalar; 2: per channel (one of them negative).  -> (array or None, per_channel)"""
    if kind == 0:
        return None, False
    rng = np.random.RandomState(seed)
    if kind == 1:
        return np.array([0.37], np.float32), False
    g = rng.uniform(0.25, 2.0, C).astype(np.float32)
    g[C // 2] *= -1
    return g, True


FLAG_SETS = (0, dice_ref.LOGITS, dice_ref.BCE, dice_ref.LOGITS | dice_ref.BCE)


def flag_name(flags, masked=False):
    return {0: "plain", 1: "logits", 2: "bce", 3: "logits|bce"}[flags] + ("+mask" if masked else "")
