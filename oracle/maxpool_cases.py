"""Inputs and the case tables shared by tests/test_maxpool_cpu.py and tests/test_gpu_maxpool.py (TEST INFRASTRUCTURE).

x = relu(round(2 randn) / 2) 2^((c % 5) - 2): a post-ReLU tensor on a coarse grid, so that windows are full of exact ties (at 0
and at the maximum) and every value is exact in fp16, bf16 and fp32 -- one float64 reference serves all three storage types.
gy, gskip: upsample_cases.make_tensor on grid "16"; coefficients: upsample_cases.make_coef.

The selector rules the tables are written against (csrc/pool_upsample.hip, include/tem_hip.h):
  forward   VEC8: 16-bit, C % 8 == 0, 16-byte aligned pointers, ld % 8 == 0, 256 % (C / 8) == 0, option pool_vec8 != 0
            VEC4: C % 4 == 0, pointers aligned to 4 elements, ld % 4 == 0;  VEC1 otherwise
            row partials: cq = C / VEC items per voxel, cq <= 256 and 256 % cq == 0 (for C % 4 == 0 judged at VEC = 4)
  backward  the same alignment rules over gy, x, gskip, gx (no 256 % rule); with pool_vec8 >= 2, fy = fx = 2, fz in (1, 2) and
            C <= 2048 the packed-word kernel PACKED16_FZ1 / _FZ2 instead of VEC8
  a block is one output row (n, zo, yo) of 256 threads over Wo cq items: trips = ceil(Wo cq / 256)
  windows of at most 8 voxels take the unrolled form of a kernel, larger ones its loop form
"""
import numpy as np

from . import maxpool_ref as R
from . import upsample_cases as UK

VEC1, VEC4, VEC8, PACKED16_FZ1, PACKED16_FZ2 = 0, 1, 2, 3, 4
PATH_NAME = {0: "vec<1>", 1: "vec<4>", 2: "vec<8>", 3: "packed16<fz1>", 4: "packed16<fz2>"}
VEC_OF = {VEC1: 1, VEC4: 4, VEC8: 8, PACKED16_FZ1: 8, PACKED16_FZ2: 8}
PAD_BYTES = 128                       # oracle/gpu_kit.py: PAD elements of at least 2 bytes in front of a 256-byte aligned buffer


def nwin(f):
    return f[0] * f[1] * f[2]


def form(f):
    return "unrolled" if nwin(f) <= 8 else "loop"


def cq_of(C, path):
    return C // VEC_OF[path]


def trips(shape, f, path):
    return -(-(shape[3] // f[2]) * cq_of(shape[4], path) // 256)


def make_x(shape, seed):
    """float32 [N, D, H, W, C], every value exact in fp16 and bf16"""
    rng = np.random.RandomState(seed)
    a = np.maximum(np.round(2.0 * rng.randn(*shape)) / 2.0, 0.0) * 2.0 ** ((np.arange(shape[-1]) % 5) - 2)
    a = a.astype(np.float32)
    assert np.array_equal(R.round_common16(a), a), "x is exact in every storage type"
    return a


def tie_share(x, f):
    """(share of windows whose maximum is attained more than once, share where in addition the first maximum is not at 0)"""
    w = R.windows(np.asarray(x, np.float64), f)
    m, am = R.pool_f64(x, f)
    tied = (w == m[..., None]).sum(axis=-1) > 1
    return float(tied.mean()), float((tied & (am > 0)).mean())


# ---------------------------------------------------------------------------------------------------------- the tables
MAIN = {"m1": ((2, 2, 2), (2, 4, 6, 8, 32)), "m2": ((1, 2, 2), (1, 3, 8, 140, 32))}
ALL3 = ("f32", "f16", "bf16")
P4_8 = {"f32": VEC4, "f16": VEC8, "bf16": VEC8}
ALL4 = {"f32": VEC4, "f16": VEC4, "bf16": VEC4}
ALL1 = {"f32": VEC1, "f16": VEC1, "bf16": VEC1}

# forward: id: (factor, fine shape, storage types, {type: intended path}, statistics, layout of x, options)
#   statistics: "yes" requested and judged | "no" not requested | "none" tem_maxpool3d_fwd_stat_blocks() == 0 for this C: the
#   query with has_stat names -1 and the launch runs without;  layout of x: None dense | (Wd, lo);  options: those of the
#   library, and "x": the recipe of inputs()
FWD = {
    "m1": ((2, 2, 2), (2, 4, 6, 8, 32), ALL3, P4_8, "yes", None, {}),
    "m2": ((1, 2, 2), (1, 3, 8, 140, 32), ALL3, P4_8, "yes", None, {}),             # 3 trips at cq = 8 (f32), 2 at cq = 4
    "g2": ((1, 2, 2), (1, 3, 8, 140, 32), ALL3, P4_8, "yes", None, {"x": "randn16"}),   # row sums that round (not in the issue's table)
    "g3": ((1, 3, 3), (1, 2, 6, 213, 8), ("f32", "f16"), P4_8, "yes", None, {"x": "randn16"}),  # ... in the loop form, cq = 2 / 1
    "l1": ((3, 3, 3), (1, 3, 6, 9, 8), ("f32", "f16"), P4_8, "no", None, {}),       # the loop form
    "l2": ((1, 3, 3), (1, 2, 6, 9, 8), ("f32", "f16"), P4_8, "no", None, {}),
    "w1": ((1, 1, 1), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, "no", None, {}),       # windows of 1 and 2 voxels
    "w2": ((2, 1, 1), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, "no", None, {}),
    "w3": ((1, 1, 2), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, "no", None, {}),
    "c3": ((2, 2, 2), (1, 2, 4, 6, 3), ("f32", "f16"), ALL1, "none", None, {}),
    "c2": ((2, 2, 2), (1, 2, 4, 6, 2), ("f32", "f16"), ALL1, "yes", None, {}),
    "c20": ((2, 2, 2), (1, 2, 4, 6, 20), ("f32", "f16"), ALL4, "none", None, {}),   # C / 4 = 5 does not divide 256: declined
    "c24": ((2, 2, 2), (1, 2, 4, 6, 24), ("f16",), ALL4, "none", None, {}),         # 256 % (C / 8) != 0: not VEC8
    "c512": ((2, 2, 2), (1, 2, 2, 6, 512), ("f32", "f16"), P4_8, "yes", None, {}),  # cq = 128 / 64: 2 / 4 rows of threads
    "v0": ((2, 2, 2), (2, 4, 6, 8, 32), ("f16",), ALL4, "no", None, {"pool_vec8": 0}),
    "s1": ((2, 2, 2), (2, 4, 6, 8, 32), ("f32", "f16"), P4_8, "no", (64, 32), {}),  # the skip half of a concat buffer
    "s2": ((2, 2, 2), (2, 4, 6, 8, 32), ("f16",), ALL4, "no", (40, 4), {}),         # 8-byte aligned rows
    "s3": ((2, 2, 2), (2, 4, 6, 8, 32), ("f32",), ALL1, "no", (36, 2), {}),
}
FWD_TRIPS = {("m1", "f32"): 1, ("m1", "f16"): 1, ("m2", "f32"): 3, ("m2", "f16"): 2, ("m2", "bf16"): 2, ("c512", "f32"): 2,
             ("c512", "f16"): 1}

# backward variants: (gskip, relu_mask, gcoef, ycoef)
VARIANTS = {"plain": (0, 0, 0, 0), "sm": (1, 1, 0, 0), "smg": (1, 1, 1, 0), "smy": (1, 1, 0, 1), "smb": (1, 1, 1, 1),
            "y": (0, 0, 0, 1),          # ycoef alone: the engine's floor path
            "m": (0, 1, 0, 0)}          # mask alone: at factor (1, 1, 1) the engine's out-layer use
SEVEN = ("plain", "sm", "smg", "smy", "smb", "y")            # ... the seventh is the rows m1r / m2r
TWO = ("plain", "smb")
P16_2 = {"f32": VEC4, "f16": PACKED16_FZ2, "bf16": PACKED16_FZ2}
P16_1 = {"f32": VEC4, "f16": PACKED16_FZ1, "bf16": PACKED16_FZ1}
# backward: id: (factor, fine shape, storage types, {type: intended path}, variants, layout, options)
#   layout: None dense | ("xs", Wd, lo): x and gskip are channels [lo, lo + C) of Wd-channel buffers and gcoef the [:, lo:] view of
#   a [N, Wd, 4] tensor | ("gskip", Wd, lo) | ("gx", Wd, lo)
BWD = {
    "m1": ((2, 2, 2), (2, 4, 6, 8, 32), ALL3, P16_2, SEVEN, None, {}),
    "m2": ((1, 2, 2), (1, 3, 8, 140, 32), ALL3, P16_1, SEVEN, None, {}),
    "m1r": ((1, 1, 1), (2, 4, 6, 8, 32), ALL3, P4_8, ("m",), None, {}),
    "m2r": ((1, 1, 1), (1, 3, 8, 140, 32), ALL3, P4_8, ("m",), None, {}),
    "m1v1": ((2, 2, 2), (2, 4, 6, 8, 32), ("f16", "bf16"), P4_8, TWO, None, {"pool_vec8": 1}),
    "m2v1": ((1, 2, 2), (1, 3, 8, 140, 32), ("f16",), P4_8, TWO, None, {"pool_vec8": 1}),
    "m1v0": ((2, 2, 2), (2, 4, 6, 8, 32), ("f16", "bf16"), ALL4, TWO, None, {"pool_vec8": 0}),
    "l1": ((3, 3, 3), (1, 3, 6, 9, 8), ("f32", "f16", "bf16"), P4_8, TWO, None, {}),
    "l2": ((1, 3, 3), (1, 2, 6, 9, 8), ("f32", "f16"), P4_8, TWO, None, {}),
    "w1": ((1, 1, 1), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, TWO, None, {}),
    "w2": ((2, 1, 1), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, TWO, None, {}),
    "w3": ((1, 1, 2), (1, 4, 3, 6, 8), ("f32", "f16"), P4_8, TWO, None, {}),
    "c3": ((2, 2, 2), (1, 2, 4, 6, 3), ("f32", "f16"), ALL1, TWO, None, {}),
    "c2": ((2, 2, 2), (1, 2, 4, 6, 2), ("f32",), ALL1, TWO, None, {}),
    "c12": ((2, 2, 2), (1, 2, 4, 6, 12), ("f16",), ALL4, TWO, None, {}),
    "c20": ((2, 2, 2), (1, 2, 4, 6, 20), ("f32", "f16"), ALL4, TWO, None, {}),
    "c24": ((2, 2, 2), (1, 2, 4, 6, 24), ("f16",), P16_2, TWO, None, {}),            # cq = 3: i / cq, i % cq of no power of two
    "c512": ((2, 2, 2), (1, 2, 2, 2, 512), ("f32", "f16"), P16_2, TWO, None, {}),    # the staging loop's second trip
    "c2048": ((2, 2, 2), (1, 2, 2, 2, 2048), ("f16",), P16_2, TWO, None, {}),        # 2 C float4 = 64 KB of dynamic LDS
    "c2056": ((2, 2, 2), (1, 2, 2, 2, 2056), ("f16",), P4_8, TWO, None, {}),         # just past the bound
    "s1": ((2, 2, 2), (2, 4, 6, 8, 32), ("f32", "f16"), P16_2, ("sm", "smb"), ("xs", 64, 32), {}),
    "s2": ((2, 2, 2), (2, 4, 6, 8, 32), ("f16",), ALL4, ("sm", "smb"), ("gskip", 40, 4), {}),
    "s3": ((2, 2, 2), (2, 4, 6, 8, 32), ("f32",), ALL1, TWO, ("gx", 36, 2), {}),
}
BIT_IDENTITY = ("m1", "m2")          # 16-bit: pool_vec8 = 2 (packed) and 1 (generic) store the same bits, in every variant
BWD_TRIPS = {("m1", "f32"): 1, ("m2", "f32"): 3, ("m2", "f16"): 2, ("m2v1", "f16"): 2, ("m2r", "f32"): 5, ("m2r", "f16"): 3,
             ("c24", "f16"): 1, ("c512", "f16"): 1, ("c2048", "f16"): 1, ("c2056", "f16"): 2}
TIE_CASES = sorted({(c[1], c[0]) for c in list(FWD.values()) + list(BWD.values()) if nwin(c[0]) >= 4})
TIE_MIN = 0.20


# ---------------------------------------------------------------------------------------------------------- selector rules
def _aligned(lo, Wd, esize, vec):
    """channels [lo, lo + C) of a Wd-channel buffer behind PAD_BYTES: accesses of `vec` elements are aligned"""
    return (PAD_BYTES + lo * esize) % (vec * esize) == 0 and Wd % vec == 0


def expected_path(direction, f, C, dt, tensors, pool_vec8=2):
    """the documented selector rules; tensors: [(Wd, lo)] of every tensor of the launch"""
    esize = 4 if dt == "f32" else 2
    v8 = dt != "f32" and C % 8 == 0 and pool_vec8 and all(_aligned(lo, Wd, 2, 8) for Wd, lo in tensors)
    v4 = C % 4 == 0 and all(_aligned(lo, Wd, esize, 4) for Wd, lo in tensors)
    if direction == "fwd":
        return VEC8 if v8 and 256 % (C // 8) == 0 else VEC4 if v4 else VEC1
    if v8:
        if pool_vec8 >= 2 and f[1] == 2 and f[2] == 2 and f[0] in (1, 2) and C <= 2048:
            return PACKED16_FZ2 if f[0] == 2 else PACKED16_FZ1
        return VEC8
    return VEC4 if v4 else VEC1


def stat_blocks(shape, f):
    """tem_maxpool3d_fwd_stat_blocks as include/tem_hip.h documents it"""
    N, D, H, W, C = shape
    cq = C // 4 if C % 4 == 0 else C
    return 0 if cq > 256 or 256 % cq else (D // f[0]) * (H // f[1])


# ---------------------------------------------------------------------------------------------------------- special values
SPECIAL_F, SPECIAL_SHAPE = (2, 2, 2), (1, 2, 4, 6, 8)
SPECIAL_VARIANTS = ("plain", "sm")


def special_x():
    """the recipe's tensor with planted windows (every channel): -inf throughout; one NaN; two NaNs; all equal and positive;
    zeros of both signs, the first of them negative.  Data values, not faults."""
    x = make_x(SPECIAL_SHAPE, 4242)
    w = R.windows(x, SPECIAL_F).copy()                      # [1, 1, 2, 3, C, 8]
    w[0, 0, 0, 0] = -np.inf
    w[0, 0, 0, 1, :, 3] = np.nan
    w[0, 0, 1, 0, :, 1] = np.nan
    w[0, 0, 1, 0, :, 5] = np.nan
    w[0, 0, 1, 1] = 1.5
    w[0, 0, 0, 2] = np.array([-0.0, 0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0], np.float32)
    return R.unwindows(w, SPECIAL_F).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- shared data
_CACHE = {}


def _cached(key, make):
    """inputs, float64 references, scales and the restatement's errors of one (shape, factor): computed once, shared by the
    storage types and the cases of that shape, left unchanged"""
    if key not in _CACHE:
        if len(_CACHE) >= 24:
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def inputs(shape, f, recipe="ties"):
    """-> dict: x, gy, gskip (float32, exact in every storage type), gcoef, ycoef [N, C, 4]; y, am (float64 maximum, arg-max).
    recipe "randn16": x = relu(upsample_cases.make_tensor on grid "16") -- 8 significant bits on many exponents, so that the
    row sums of the maxima are NOT exact in float32 (those of the tie recipe are)"""
    def make():
        seed = UK.seed_of("maxpool", shape, f)
        x = make_x(shape, seed) if recipe == "ties" else np.maximum(UK.make_tensor(shape, seed, "16"), np.float32(0))
        d = {"x": x, "gy": UK.make_tensor(R.coarse(shape, f), seed + 1, "16"),
             "gskip": UK.make_tensor(shape, seed + 2, "16"), "gcoef": UK.make_coef(shape[0], shape[4], seed + 3),
             "ycoef": UK.make_coef(shape[0], shape[4], seed + 4)}
        d["y"], d["am"] = R.pool_f64(d["x"], f)
        return d
    return _cached(("in", shape, f, recipe), make)


def fwd_rows(shape, f, cq, recipe="ties"):
    """-> dict: rows / rows_scale [N, Do Ho, C, 2], rows_e32 [2] for the path's cq (x is exact in every type, so the stored y
    is the float64 y and its sums are the sums of the stored values)"""
    def make():
        y = inputs(shape, f, recipe)["y"]
        d = {"rows": R.row_stats_f64(y), "rows_scale": R.row_stats_scale(y)}
        d["rows_e32"] = R.row_stats_e32(y, cq, d["rows"], d["rows_scale"])
        return d
    return _cached(("rows", shape, f, cq, recipe), make)


def variant_args(d, variant):
    """-> (gskip, relu_mask, gcoef, ycoef) as bwd_f64 takes them"""
    s, m, g, y = VARIANTS[variant]
    return d["gskip"] if s else None, bool(m), d["gcoef"] if g else None, d["ycoef"] if y else None


def bwd_data(shape, f, variant):
    """-> dict: ref, scale (float64), e32; without coefficients e32 is 0 and the judge is add_exact"""
    def make():
        d = inputs(shape, f)
        gskip, mask, gcoef, ycoef = variant_args(d, variant)
        ref, scale = R.bwd_f64(d["gy"], d["x"], f, gskip, mask, gcoef, ycoef)
        e32 = 0.0
        if gcoef is not None or ycoef is not None:
            e32 = R.bwd_e32(d["gy"], d["x"], f, gskip, mask, gcoef, ycoef, ref, scale)
        return {"ref": ref, "scale": scale, "e32": e32}
    return _cached(("bwd", shape, f, variant), make)
