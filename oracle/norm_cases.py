"""Inputs and the case tables shared by tests/test_norm_cpu.py and tests/test_gpu_norm.py (TEST INFRASTRUCTURE).

Tensors are logical [N, V, C]: seeded randn, channel c scaled by 2^((c % 5) - 2) (a channel mix-up moves an element by a
factor of 2 or more), x plus a per-channel offset of about 0.7 (`offset` of the case: r9 / r9x use 16 / 27 and no zeros, so
|mean| / sigma of a group is 6.8 .. 9.6 / 11.2 .. 15.6 -- a group's sigma is 1.7 .. 2.4 -- and ss / cnt - m^2 cancels
6 .. 8 bits).  grid "16": rounded to values fp16,
bf16 and fp32 all hold exactly (judge.round_common16).  Some x are exactly 0.0 and -0.0 (the ReLU mask `!(x > 0)`);
the last voxel of every sample has |x| >= the channel's mean |x| (and |g| >= mean |g|), so a dropped last voxel moves a sum by
at least 2^23 / V units.  gamma = 1 + 0.3 randn, beta = 0.2 randn (tests/test_gpu_ops.py: test_norm_stats_and_backward).

Geometry columns are what the dispatch queries of csrc/norm.hip must answer: reduction (vec, rows, threads, nblk, vper) for
MODE 0 (norm_stats) and MODE 1 (the backward reduction), apply (vec, threads, grid_x, fast).
"""
import ctypes

import numpy as np

from . import norm_ref as R

EPS = float(np.float32(1e-5))      # the C-ABI takes eps as a float: the kernel adds this value in double
ITEM = {"f32": 4, "f16": 2, "bf16": 2}
ST = {"f32": 0, "f16": 1, "bf16": 2}

# ---------------------------------------------------------------------------------------------------------- reduction
# id: (C, G, N, V, storage types, affine, offset, layout of x, layout of gy, geometry MODE 0, geometry MODE 1)
#   layout: None dense | (Wd, lo): channels [lo, lo + C) of a Wd-channel buffer
_R1 = (4, 32, 256, 2, 257)       # main loop (2 trips of 4 voxels), tail, and uneven blocks 257 + 256
_V1 = (1, 8, 256, 5, 103)        # the same tensor through the scalar kernel
RED = {
    "r1": (32, 4, 2, 513, ("f32",), True, 0.7, None, None, _R1, _R1),
    "r2": (4, 4, 1, 12295, ("f32",), False, 0.7, None, None, (4, 256, 256, 4, 3074), (4, 256, 256, 4, 3074)),
    "r2s": (1, 1, 1, 12295, ("f32",), False, 0.7, None, None, (1, 256, 256, 4, 3074), (1, 256, 256, 4, 3074)),
    "r3": (12, 3, 2, 1365, ("f32",), True, 0.7, None, None, (4, 85, 255, 2, 683), (4, 85, 255, 2, 683)),       # cq = 3
    "r4": (1024, 32, 1, 8209, ("f32",), True, 0.7, None, None, (4, 1, 256, 512, 17), (4, 1, 256, 512, 17)),    # nblk capped; 29 empty blocks
    "r5": (1024, 1024, 1, 37, ("f32",), False, 0.7, (1025, 0), (1025, 0), (1, 1, 1024, 3, 13), (1, 1, 1024, 3, 13)),
    "r6": (257, 1, 2, 50, ("f32",), True, 0.7, None, None, (1, 1, 257, 4, 13), (1, 1, 257, 4, 13)),
    "r7": (32, 32, 2, 513, ("f32",), False, 0.7, (40, 1), None, _V1, _V1),                # x not 16-byte aligned
    "r7g": (32, 32, 2, 513, ("f32",), False, 0.7, None, (33, 0), _R1, _V1),               # gy of odd leading dimension
    "r8": (32, 4, 2, 513, ("f16", "bf16"), True, 0.7, None, None, _R1, _R1),
    "r8w": (32, 4, 2, 513, ("f16", "bf16"), True, 0.7, (40, 4), (40, 4), _R1, _R1),       # 8-byte aligned: still vec 4 (tem_st_align4)
    "r9": (32, 4, 2, 513, ("f32",), True, 16.0, None, None, _R1, _R1),
    "r9x": (32, 4, 2, 513, ("f32",), True, 27.0, None, None, _R1, _R1),
}

# ---------------------------------------------------------------------------------------------------------- apply
# id: (C, G, N, V, storage types, affine, out_amax, layout of gx, geometry (vec, threads, grid_x, fast), in place too)
APP = {
    "a1": (32, 4, 2, 513, ("f32",), True, False, None, (4, 256, 17, 1), False),          # the grid covers the items: one trip
    "a2": (32, 4, 1, 150001, ("f32",), True, False, None, (4, 256, 2048, 1), True),      # two voxels, then for some a third alone
    "a3": (12, 3, 1, 200003, ("f32",), True, False, None, (4, 256, 2048, 0), False),     # two trips, with the q wrap
    "a4": (6, 3, 1, 100003, ("f32",), True, False, None, (1, 256, 2048, 0), False),      # scalar, two trips, with wrap
    "a5": (32, 32, 4, 20011, ("f32",), False, True, None, (4, 1024, 64, 1), False),      # out_amax, fast
    "a6": (12, 3, 3, 30011, ("f32",), True, True, None, (4, 1024, 86, 0), False),        # out_amax, slow path
    "a7": (32, 4, 1, 150001, ("f16", "bf16"), True, False, None, (4, 256, 2048, 1), False),
    "a8": (32, 4, 2, 513, ("f32",), True, False, (40, 4), (4, 256, 17, 1), False),       # gx wider than gy and x
}
# what the table says about the trips of a thread (asserted on the CPU): items / (grid_x * threads)
APP_TRIPS = {"a1": (0.9, 1.0), "a2": (2.0, 3.0), "a3": (1.0, 2.0), "a4": (1.0, 2.0), "a5": (2.0, 3.0), "a6": (1.0, 2.0),
             "a7": (2.0, 3.0), "a8": (0.9, 1.0)}

# ---------------------------------------------------------------------------------------------------------- finalize
# (nblk, cg, threads of the finalize block, note); C = 2 groups of cg channels, N = 2
FIN = [(1, 1, 256), (7, 3, 256), (2048, 1, 256), (2049, 1, 1024), (700, 3, 1024), (16384, 1, 1024), (16385, 1, 1024)]
FIN2 = {"CA": 8, "CB": 24, "cg": 4, "nblkA": 5, "nblkB": 700, "N": 2}
BWD_STAGE = [(nblk, N) for nblk in (1, 300, 5000) for N in (1, 3)]
BWD_STAGE_CG = (8, 4)       # C = 8 channels in 2 groups of 4


def finalize_threads(nblk, cg):
    """csrc/norm.hip: norm_finalize_threads"""
    return 1024 if nblk * cg > 2048 else 256


def grid_of(dtype):
    return "f32" if dtype == "f32" else "16"


def fake_ptr(layout, dtype):
    """a pointer value with the alignment the test's buffers have (only alignment matters to the queries)"""
    lo = layout[1] if layout else 0
    return 0x7F0000001000 + 256 + lo * ITEM[dtype]


def ld_of(layout, C):
    return layout[0] if layout else C


# ---------------------------------------------------------------------------------------------------------- inputs
def _grid(a, grid):
    a = a.astype(np.float32)
    return R.round_common16(a).astype(np.float32) if grid == "16" else a


def _last_voxel_counts(a, grid):
    m = np.abs(a).mean(axis=1)
    last = a[:, -1, :]
    a[:, -1, :] = np.where(np.abs(last) < 1.25 * m, np.where(np.signbit(last), -1.5, 1.5) * m, last)
    a = _grid(a, grid)
    assert (np.abs(a[:, -1, :]) >= np.abs(a).mean(axis=1)).all()
    return a


def make_x(N, V, C, seed, grid="f32", offset=0.7):
    rng = np.random.RandomState(seed)
    c = np.arange(C)
    off = offset * (1.0 + 0.25 * ((c % 3) - 1)) if offset < 1 else offset + 0.175 * ((c % 3) - 1)
    a = rng.randn(N, V, C) * 2.0 ** ((c % 5) - 2) + off
    if offset < 1:                # (2 % zeros in a tensor of mean 16 would be most of its variance)
        flat = a.reshape(-1)
        flat[5::97] = 0.0
        flat[11::101] = -0.0
    return _last_voxel_counts(a, grid)


def make_g(N, V, C, seed, grid="f32"):
    rng = np.random.RandomState(seed)
    a = rng.randn(N, V, C) * 2.0 ** (((np.arange(C) + 2) % 5) - 2)
    return _last_voxel_counts(a, grid)


def make_affine(C, seed, affine=True):
    if not affine:
        return None, None
    rng = np.random.RandomState(seed)
    return (1 + 0.3 * rng.randn(C)).astype(np.float32), (0.2 * rng.randn(C)).astype(np.float32)


def seed_of(name, C, N, V):
    return (sum(map(ord, name[:2])) * 131 + 7 * C + 11 * N + V) % (2 ** 31)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def tensor_data(name, C, G, N, V, affine, offset, grid, spike=None):
    """-> dict: x, g, gamma, beta; sums / sums_scale [N, C, 2]; ref (stats_f64 plus "sums"); mean32, rstd32 (the float32
    statistics the backward is given); bsums / bscale [N, C, 2]; coef [N, C, 4]; dgamma, dbeta.  The same tensors serve the
    cases that share (shape, offset, grid): the id's first two letters seed them."""
    def make():
        seed = seed_of(name, C, N, V)
        x, g = make_x(N, V, C, seed, grid, offset), make_g(N, V, C, seed + 1, grid)
        if spike:                 # one large gradient element: max |gx| is there
            g[spike[0], spike[1], spike[2]] = spike[3]
        gamma, beta = make_affine(C, seed + 2, affine)
        d = {"x": x, "g": g, "gamma": gamma, "beta": beta, "V": V, "G": G}
        d["sums"], d["sums_scale"] = R.channel_sums_f64(x), R.channel_sums_scale(x)
        d["ref"] = R.stats_f64(d["sums"], V, G, gamma, beta, EPS)
        d["ref"]["sums"] = d["sums"]
        d["mean32"], d["rstd32"] = d["ref"]["mean"].astype(np.float32), d["ref"]["rstd"].astype(np.float32)
        d["bsums"], d["bscale"] = R.bwd_sums_f64(g, x, d["mean32"], d["rstd32"]), R.bwd_sums_scale(g, x, d["mean32"], d["rstd32"])
        d["coef"] = R.coef_f64(d["bsums"], V, G, gamma, d["mean32"], d["rstd32"])
        d["dgamma"], d["dbeta"] = R.affine_grads_f64(d["bsums"])
        return d
    return _cached(("t", name[:2], C, G, N, V, affine, offset, grid, spike), make)


def red_data(name, grid):
    C, G, N, V, dtypes, affine, offset = RED[name][:7]
    return tensor_data("r" + str(C), C, G, N, V, affine, offset, grid)


def last_block_elements(name):
    """bool [V, C]: the elements of one sample the LAST block of the apply grid computes (block b takes the items
    i = b threads + t + k grid_x threads; item i is channels [vec (i % cq), + vec) of voxel i / cq, cq = C / vec)"""
    C, G, N, V = APP[name][:4]
    vec, threads, grid_x, fast = APP[name][8]
    cq = C // vec
    i = np.arange(V * cq, dtype=np.int64)
    own = (i % (grid_x * threads)) // threads == grid_x - 1
    return np.repeat(own.reshape(V, cq), vec, axis=1)


def amax_spike(name):
    """(n, v, c, value): an element of the last sample that the last block computes on its last trip"""
    C, G, N, V = APP[name][:4]
    vec = APP[name][8][0]
    m = last_block_elements(name)
    v = int(np.nonzero(m.any(axis=1))[0][-1])
    c = int(np.nonzero(m[v])[0][0]) + (1 if vec == 4 else 0)
    return (N - 1, v, c, 64.0)


def app_data(name, grid):
    C, G, N, V, dtypes, affine, amax = APP[name][:7]
    return tensor_data("a" + str(C), C, G, N, V, affine, 0.7, grid, spike=amax_spike(name) if amax else None)


_E32 = {}


def reduce_e32(d, mode, geom):
    """the restatement's errors for one tensor set, reduction mode and geometry (vec, rows, threads, nblk, vper): the worse
    of the separately rounded and the fused product -> dict sum0, sum1 (and mean, var for MODE 0)"""
    key = (id(d), mode, tuple(geom))
    if key in _E32 and _E32[key][0] is d:
        return _E32[key][1]
    vec, rows, threads, nblk, vper = (int(v) for v in geom)
    x = d["x"]
    out = {}
    for fused in (False, True):
        if mode == 0:
            rows32 = R.partition_sums_f32(x, x, x, rows, nblk, vper, fused)
            e = R.stats_e32(rows32, d["ref"], d["sums_scale"], d["V"], d["G"])
        else:
            rows32 = R.partition_sums_f32(d["g"], d["g"], R.xn_f32(x, d["mean32"], d["rstd32"]), rows, nblk, vper, fused)
            s = R.rows_f64(rows32)
            e = {"sum0": R.units(s[..., 0], d["bsums"][..., 0], d["bscale"][..., 0]),
                 "sum1": R.units(s[..., 1], d["bsums"][..., 1], d["bscale"][..., 1])}
        out = {k: max(v, out.get(k, 0.0)) for k, v in e.items()}
    if len(_E32) >= 8:
        _E32.clear()
    _E32[key] = (d, out)
    return out


# ---------------------------------------------------------------------------------------------------------- synthetic rows
def make_rows(N, nblk, C, seed, V, equal=False):
    """float32 forward rows [N, nblk, C, 2] with ss >= s^2 / V per channel (var >= 0); equal: every x the same (var clamps
    at 0).  Row b stands for V / nblk voxels of mean about 0.7 (2^((c % 5) - 2) sigma)."""
    rng = np.random.RandomState(seed)
    per = V / nblk
    c = np.arange(C)
    if equal:
        s = np.full((N, nblk, C), 0.75 * per)
        ss = np.full((N, nblk, C), 0.5625 * per)
    else:
        sig = 2.0 ** ((c % 5) - 2)
        s = per * (0.7 + sig * rng.randn(N, nblk, C) / np.sqrt(per))
        ss = s * s / per + per * sig * sig * rng.uniform(0.5, 1.5, (N, nblk, C))
    return np.stack([s, ss], axis=-1).astype(np.float32)


def make_bwd_rows(N, nblk, C, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(N, nblk, C, 2) * 2.0 ** ((np.arange(C)[:, None] % 5) - 2) * 8.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- the queries
def _vp(p):
    return p if p is None or isinstance(p, ctypes.c_void_p) else ctypes.c_void_p(int(p))


def reduce_geom(lib, x, x_ld, gy, gy_ld, V, C, st):
    """tem_norm_reduce_geom -> (vec, rows, threads, nblk, vper), or None where the launch would refuse"""
    out = (ctypes.c_int64 * 5)()
    rc = lib.tem_norm_reduce_geom(_vp(x), x_ld, _vp(gy), gy_ld, V, C, st, out)
    return tuple(out) if rc == 0 else None


def apply_geom(lib, gy, gy_ld, x, x_ld, gx, gx_ld, N, V, C, has_amax, st):
    """tem_norm_apply_geom -> (vec, threads, grid_x, fast), or None where the launch would refuse"""
    out = (ctypes.c_int64 * 4)()
    rc = lib.tem_norm_apply_geom(_vp(gy), gy_ld, _vp(x), x_ld, _vp(gx), gx_ld, N, V, C, int(has_amax), st, out)
    return tuple(out) if rc == 0 else None


# ---------------------------------------------------------------------------------------------------------- the judges
def judge_sums(got, ref, scale, e32):
    """got [N, C, 2] (rows merged in float64) -> ratios sum0, sum1"""
    got = np.asarray(got, np.float64)
    return {k: R.ratio_units(got[..., i], ref[..., i], scale[..., i], e32[k]) for i, k in enumerate(("sum0", "sum1"))}


def judge_coef(got, d, e32, dgamma=None, dbeta=None):
    """got: float32 coef [N, C, 4] for the tensors of d (and dgamma, dbeta [C]) -> ratios a, m1, m2r, cmean (0 or infinite:
    coef[3] is the given float32 mean bit for bit), dgamma, dbeta"""
    got = np.asarray(got, np.float64)
    dc, d0, d1 = R.coef_bands(d["coef"], d["bscale"], d["V"], d["G"], d["gamma"], d["rstd32"], e32)
    out = {k: R.ratio_band(got[..., i], d["coef"][..., i], dc[..., i]) for i, k in enumerate(("a", "m1", "m2r"))}
    out["cmean"] = 0.0 if got.shape == d["coef"].shape and np.array_equal(got[..., 3], d["coef"][..., 3]) else float("inf")
    if dgamma is not None:
        bg, bb = R.affine_bands(d["dgamma"], d["dbeta"], d0, d1)
        out["dgamma"], out["dbeta"] = R.ratio_band(dgamma, d["dgamma"], bg), R.ratio_band(dbeta, d["dbeta"], bb)
    return out


def _f64(d):
    """the float64 copies of g and x, made once per tensor set"""
    if "g64" not in d:
        d["g64"], d["x64"] = d["g"].astype(np.float64), d["x"].astype(np.float64)
    return d["g64"], d["x64"]


def gx_end_to_end(d, relu_mask, e32_sums, e32_apply):
    """-> (float64 gx, its absolute band) for the tensors of d"""
    g, x = _f64(d)
    dc, _, _ = R.coef_bands(d["coef"], d["bscale"], d["V"], d["G"], d["gamma"], d["rstd32"], e32_sums)
    return R.apply_f64(g, x, d["coef"], relu_mask), R.gx_band(g, x, d["coef"], dc, e32_apply)


def gx_apply_alone(d, coef32, relu_mask):
    """-> (float64 gx from the float32 coef a coef_out call returned, its scale, e32 of the two float32 evaluations)"""
    g, x = _f64(d)
    ref, scale = R.apply_f64(g, x, coef32, relu_mask), R.apply_scale(g, x, coef32)
    return ref, scale, R.apply_e32(d["g"], d["x"], coef32, relu_mask, ref, scale)
