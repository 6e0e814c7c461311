"""Inputs and the case tables shared by tests/test_upsample_cpu.py and tests/test_gpu_upsample.py (TEST INFRASTRUCTURE).

Tensors: seeded randn, channel c scaled by 2^((c % 5) - 2) (a channel mix-up moves an element by a factor of 2 or more).
grid "f32": the float32 values; grid "16": rounded to values fp16, bf16 and fp32 all hold exactly (judge.round_common16),
so the two 16-bit types of a case share one float64 reference and a fp32 launch can run on the very same values.
Coefficients (a, m1, m2r, mean) per (sample, channel), float32: a in [0.5, 2.5], m1 about 0.1, m2r about 0.05, mean about 1.

Pair counts: upsample_bwd_impl (csrc/pool_upsample.hip) counts N * ceil(D / fz) * ceil(H / 2) * ceil(W / 2) * (C / 4) coarse pairs
and takes the factor-2 kernel from PAIRS_CH4 on, its 8-channel 16-bit instantiation from PAIRS_CH8 on.
"""
import numpy as np

from . import upsample_ref as R

PAIRS_CH4, PAIRS_CH8 = 65536, 131072
GATHER1, GATHER4, FACTOR2_CH4, FACTOR2_CH8 = 0, 1, 2, 3
PATH_NAME = {0: "gather<1>", 1: "gather<4>", 2: "factor2<4>", 3: "factor2<8>"}


def pairs(shape, f):
    N, D, H, W, C = shape
    return N * -(-D // f[0]) * -(-H // 2) * -(-W // 2) * (C // 4)


def fine(shape, f):
    N, D, H, W, C = shape
    return (N, D * f[0], H * f[1], W * f[2], C)


def grid_of(dtype):
    return "f32" if dtype == "f32" else "16"


def make_tensor(shape, seed, grid="f32"):
    """float32 [N, D, H, W, C]"""
    rng = np.random.RandomState(seed)
    a = rng.randn(*shape) * 2.0 ** ((np.arange(shape[-1]) % 5) - 2)
    a = a.astype(np.float32)
    if grid == "16":
        a = R.round_common16(a).astype(np.float32)
    return a


def make_coef(N, C, seed):
    """float32 [N, C, 4] = (a, m1, m2r, mean)"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.5, 2.5, (N, C))
    m1 = 0.1 * (1.0 + 0.3 * rng.randn(N, C))
    m2r = 0.05 * (1.0 + 0.3 * rng.randn(N, C))
    mean = 1.0 + 0.3 * rng.randn(N, C)
    return np.stack([a, m1, m2r, mean], axis=-1).astype(np.float32)


def seed_of(name, shape, f):
    return (sum(map(ord, name)) * 131 + sum(s * (7 + i) for i, s in enumerate(shape)) + 17 * f[0] + 3 * f[2]) % (2 ** 31)


# ---------------------------------------------------------------------------------------------------------- backward
# id: (factor, coarse [N, D, H, W, C], storage types, intended path, layout, options)
#   layout: None dense | ("gy", W, lo) / ("gx", W, lo) / ("both", W, lo): that tensor is channels [lo, lo + C) of a W-channel buffer
BWD = {
    "b1": ((2, 2, 2), (1, 15, 63, 63, 32), ("f32", "f16", "bf16"), FACTOR2_CH4, None, {}),        # exactly the threshold
    "b2": ((2, 2, 2), (1, 15, 63, 61, 32), ("f32",), GATHER4, None, {}),                          # just below it
    "b3": ((1, 2, 2), (2, 4, 63, 63, 32), ("f32", "f16", "bf16"), FACTOR2_CH4, None, {}),
    "b4": ((2, 2, 2), (2, 15, 63, 63, 32), ("f16", "bf16"), FACTOR2_CH8, None, {}),
    "b5": ((2, 2, 2), (2, 15, 63, 63, 32), ("f16", "bf16"), FACTOR2_CH4, None, {"upsample2_ch8": 0}),
    "b6": ((1, 2, 2), (2, 8, 63, 63, 32), ("f16", "bf16"), FACTOR2_CH8, None, {}),
    "b7": ((2, 2, 2), (1, 15, 63, 85, 24), ("f32", "f16"), FACTOR2_CH4, None, {}),                # cq = 6, Wp cq = 258
    "b8": ((2, 2, 2), (1, 1, 1, 4095, 128), ("f32", "bf16"), FACTOR2_CH4, None, {}),              # degenerate z and y
    "b9": ((2, 2, 2), (1, 1, 4095, 1, 128), ("f32",), FACTOR2_CH4, None, {}),                     # degenerate x
    "b10": ((2, 2, 2), (2, 15, 63, 63, 32), ("f16",), FACTOR2_CH4, ("both", 40, 4), {}),          # 8-byte aligned rows
    "b11": ((2, 2, 2), (1, 15, 63, 63, 32), ("f32",), GATHER1, ("gx", 36, 2), {}),                # gx 8-byte aligned
    "b12": ((2, 2, 2), (1, 15, 63, 63, 32), ("f32", "f16"), FACTOR2_CH4, ("gy", 64, 0), {}),      # the decoder's concat
    "b13a": ((1, 3, 3), (1, 3, 9, 7, 8), ("f32", "f16"), GATHER4, None, {}),
    "b13b": ((2, 2, 2), (1, 5, 7, 9, 6), ("f32", "f16"), GATHER1, None, {"upsample_generic": 1}),
}
# what the table says about the thresholds (asserted on the CPU)
BWD_PAIRS = {"b1": 65536, "b2": 63488, "b3": 65536, "b4": 131072, "b5": 131072, "b6": 131072, "b7": 66048, "b8": 65536,
             "b9": 65536, "b10": 131072, "b11": 65536, "b12": 65536}

# ---------------------------------------------------------------------------------------------------------- forward
# id: (factor, coarse shape, storage types, intended path, stats wanted, layout of y)
FWD = {
    "f1": ((2, 2, 2), (2, 3, 5, 7, 32), ("f32", "f16", "bf16"), FACTOR2_CH4, True, None),
    "f2": ((1, 2, 2), (2, 3, 5, 7, 32), ("f32",), FACTOR2_CH4, True, None),
    "f3": ((1, 2, 2), (2, 3, 5, 7, 32), ("f16", "bf16"), FACTOR2_CH8, True, None),
    "f4a": ((2, 2, 2), (1, 1, 1, 1, 8), ("f32",), FACTOR2_CH4, True, None),
    "f4b": ((2, 2, 2), (1, 2, 1, 3, 12), ("f32",), FACTOR2_CH4, False, None),                     # cq = 3: stats_ok = 0
    "f5": ((2, 2, 2), (1, 2, 3, 70, 256), ("f32", "f16"), FACTOR2_CH4, True, None),                # cq = 64, 18 trips
    "f6a": ((1, 3, 3), (1, 2, 3, 4, 6), ("f32",), GATHER1, False, None),
    "f6b": ((2, 2, 2), (1, 2, 3, 4, 6), ("f32",), GATHER1, False, None),
    "f6c": ((1, 3, 3), (1, 2, 3, 4, 8), ("f32", "f16"), GATHER4, False, None),                    # the gather kernel's vector form
    "f7": ((2, 2, 2), (2, 3, 5, 7, 32), ("f32", "f16"), FACTOR2_CH4, True, (64, 0)),
    "f8": ((2, 2, 2), (2, 3, 5, 7, 32), ("f32",), GATHER1, False, (36, 2)),
}
U_STATS = ("f1", "f2", "f3", "f5")               # ops.upsample_stats and the finalize of both kinds of partials


# ---------------------------------------------------------------------------------------------------------- shared data
_CACHE = {}


def _cached(key, make):
    """inputs, float64 references, scales and the restatement's errors of one (shape, factor, grid): computed once, shared
    by the storage types and the cases of that shape, left unchanged"""
    if key not in _CACHE:
        if len(_CACHE) >= 3:
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def _variants(f):
    """the float32 evaluations of the source index whose worse error is e32 (upsample_ref._src32)"""
    return (False, True) if R.inexact_weights(f) else (False,)


def bwd_data(shape, f, grid):
    """-> dict: g [fine], u [coarse], coef; adj / adj_scale / adj_e32; nrm / nrm_scale / nrm_e32"""
    def make():
        seed = seed_of("bwd", shape, f)
        g, u = make_tensor(fine(shape, f), seed, grid), make_tensor(shape, seed + 1, grid)
        coef = make_coef(shape[0], shape[4], seed + 2)
        d = {"g": g, "u": u, "coef": coef}
        d["adj"], d["adj_scale"] = R.adjoint_f64(g, f), R.adjoint_scale(g, f)
        d["nrm"] = R.bwd_norm_linear_f64(d["adj"], u, coef, f)
        d["nrm_scale"] = R.bwd_norm_scale(g, u, coef, f, adj_scale=d["adj_scale"])
        d["adj_e32"] = d["nrm_e32"] = 0.0
        for fused in _variants(f):
            adj32 = R.adjoint_f32(g, f, fused)
            d["adj_e32"] = max(d["adj_e32"], R.units(adj32, d["adj"], d["adj_scale"]))
            d["nrm_e32"] = max(d["nrm_e32"], R.units(R.bwd_norm_f32(g, u, coef, f, adj=adj32, fused=fused), d["nrm"], d["nrm_scale"]))
        return d
    return _cached(("bwd", shape, f, grid), make)


def fwd_data(shape, f, grid):
    """-> dict: x; y / y_scale / y_e32; rows / rows_scale / rows_e32 [2] (statistics of the UNROUNDED y, per fine-row group);
    urows / urows_scale / urows_e32 [2] (per coarse row, from x alone); urows_f32 (the restatement's rows, for the totals)"""
    def make():
        x = make_tensor(shape, seed_of("fwd", shape, f), grid)
        d = {"x": x}
        d["y"], d["y_scale"] = R.forward_f64(x, f), R.forward_scale(x, f)
        d["rows"], d["rows_scale"] = R.row_stats_f64(d["y"], f), R.row_stats_scale(d["y"], f)
        d["urows"], d["urows_scale"] = R.u_row_stats_f64(x, f), R.u_row_stats_scale(x, f)
        d["y_e32"], d["rows_e32"], d["urows_e32"] = 0.0, [0.0, 0.0], [0.0, 0.0]
        for fused in _variants(f):
            y32 = R.forward_f32(x, f, fused)
            d["y_e32"] = max(d["y_e32"], R.units(y32, d["y"], d["y_scale"]))
            r32, u32 = R.row_stats_f32(y32, f), R.u_row_stats_f32(x, f, fused)
            for k in (0, 1):
                d["rows_e32"][k] = max(d["rows_e32"][k], R.units(r32[..., k], d["rows"][..., k], d["rows_scale"][..., k]))
                d["urows_e32"][k] = max(d["urows_e32"][k], R.units(u32[..., k], d["urows"][..., k], d["urows_scale"][..., k]))
            if not fused:
                d["urows_f32"] = u32
        return d
    return _cached(("fwd", shape, f, grid), make)
