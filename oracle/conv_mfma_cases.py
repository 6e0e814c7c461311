"""Inputs and the case table shared by tests/test_conv_mfma_cpu.py and tests/test_gpu_conv_mfma.py (TEST INFRASTRUCTURE).

Three input recipes.
  lattice   conv_cases._ints / _quarters / _pow2 as they stand: every value is exact in fp32, fp16 and bf16 and every lo plane of
            every split is zero, so EVERY arithmetic mode must return the float64 value (a 16-bit store: round16 of it).
            Condition: sum |terms| / step < 2^24, asserted for every case by tests/test_conv_mfma_cpu.py.
  split     a lattice whose lo planes are NOT zero: v = hi + lo, hi on the base lattice, lo = +- one power of two below half an
            ulp of every non-zero hi in the mode's element type (0 where hi is 0); no bias, no pre-norm.  The split reproduces
            (hi, lo) exactly, every product the mode keeps is exact and the dropped lo lo is dropped in the model too.
              mode 2 (bf16x3)   x = ints + (+-2^-10), w = quarters + (+-2^-12); step 2^-12; used up to Cin 64 (2^23.5 there)
              mode 4 (fp16x3)   x = ints + (+-2^-13), w = halves + (+-2^-14); the hi hi accumulator has step 2^-1, the cross
                                accumulator (lo planes x 2^12) step 2^-2; the judge is equality with float32(exact): the joining
                                fma rounds once
            Mode 3 (bf16x6) has no split recipe: its third plane needs a second lo level (2^-18 / 2^-20 here) and the six
            terms then span 2^-2 .. 2^-30, past 2^24 steps at every Cin >= 16.  Mode 6 neither: its clamp and the one shared
            accumulator of prescaled terms put the step at 2^-26 of the scaled units.
  random    upsample_cases.make_tensor on the grid every storage type holds and float32 normal weights: judged in units of
            2^-23 x (sum |terms| + |bias|) against MARGIN x max(e32, 1), 16-bit outputs by interval16 (oracle/conv_mfma_ref.py).

The dispatch rules the table is written against (include/tem_hip.h: tem_conv3d_fwd_mfma_path; DESIGN.md "Forward dispatch: one
plan") are restated in expected(); every case names the kernel and the instantiation it is meant for, the rules must agree, and
the library's query must agree with both.  Every tensor of a case is 16-byte aligned with a leading dimension that is a
multiple of 8 (dense, or channels [8, 8 + C) of a buffer 8 channels wider): the alignment branches of the plan are the subject
of tests/test_gpu_conv_layouts.py.
"""
import numpy as np

from . import conv_cases as VK
from . import conv_mfma_ref as M
from . import conv_ref as R
from . import upsample_cases as UK

ZR, ZR_SPLITK, PP, STREAM, PATCH, PATCH_FP32 = 1, 2, 3, 4, 5, 6                # TEM_MFMA_*
NAME = {-1: "refused", 1: "zr", 2: "zr_splitk", 3: "pp", 4: "stream", 5: "patch", 6: "patch_fp32"}
NS, F16, T, KS, EPI, A, B, C, D, E, F = range(11)                              # TEM_MI_*
INST_N = 12
PLAIN, STATS, BWD_SUMS = 1, 2, 3                                               # TEM_MI_EPILOGUE
K333, K133, K111 = VK.K333, VK.K133, VK.K111
NONE, RELU, SIGMOID = R.NONE, R.RELU, R.SIGMOID
ST = {"f32": 0, "f16": 1, "bf16": 2}
PLANES = {1: 2, 2: 2, 3: 3, 4: 2, 5: 1, 6: 2, 7: 1}                            # csrc/conv_arith.h
IS_F16 = {1: 0, 2: 0, 3: 0, 4: 1, 5: 1, 6: 1, 7: 0}
TEAM_MODES = (2, 4, 5, 7)                                                      # modes with a z-reuse / ping-pong instantiation
STREAM_MODES = (2, 3, 5, 7)
DEFAULTS = {"conv_fwd_variant": -1, "zr_wide": 1, "zr_pair": 1, "zr_tile_blocks": 1, "zr_splitk": 1, "fp32_zr": 1,
            "fwd_persistent": -1, "fwd_ksplit_chunks": 0, "conv1x1_stream": 1, "team_min_units": 0}
ZR_KS_FILL = 4                                                                 # csrc/conv_zr.hip: TEM_ZR_KS_FILL


class Case:
    """one forward / data-gradient launch.  shape (N, D, H, W) and cin -> cout of the CALL (a data gradient: the transposed
    operator, packed from the state_dict weights [cin of the call = Cout of the layer]); st: storage type of x, y, ref; wide: x, y
    and ref are channels [8, 8 + C) of buffers 8 channels wider; ybuf: y alone is a channel slice of a wider buffer;
    refnorm / gscaled / sums: the _refnorm / _gscaled variants and TEM_BP_NORM_SUMS (a data gradient behind a norm with SUMS_G
    groups: rows of (sum gy, sum gy xn)); cs: the chunk-stride layout of 16-bit tensors -- the 32-channel chunk k of x (and of y) is
    a dense plane [NV][32] at k * NV * 32 elements, ld 32; opts: library options of the launch"""

    def __init__(self, name, want, shape, cin, cout, k, mode, st="f32", bias=False, norm=False, act=NONE, ref=False, stat=False,
                 amax=False, refnorm=False, gscaled=False, wide=False, ybuf=False, dgrad=False, recipe="lattice", opts=None, inst=None, cs=False, sums=False):
        self.name, self.want, self.shape, self.cin, self.cout, self.k, self.mode, self.st = name, want, tuple(shape), cin, cout, tuple(k), mode, st
        self.bias, self.norm, self.act, self.ref, self.stat, self.amax = bias, norm, act, ref or refnorm, stat, amax
        self.refnorm, self.gscaled, self.wide, self.ybuf, self.dgrad, self.recipe = refnorm, gscaled, wide, ybuf, dgrad, recipe
        self.opts, self.inst, self.cs, self.sums = dict(opts or {}), inst, cs, sums

    @property
    def id(self):
        flags = "".join(ch for ch, on in (("b", self.bias), ("n", self.norm), ("r", self.act == RELU), ("s", self.act == SIGMOID),
                                          ("m", self.ref), ("t", self.stat), ("a", self.amax), ("c", self.refnorm), ("g", self.gscaled),
                                          ("w", self.wide), ("y", self.ybuf), ("d", self.dgrad), ("k", self.cs), ("u", self.sums)) if on)
        return f"{self.name}-m{self.mode}{self.st}-{flags}{'' if self.recipe == 'lattice' else '-' + self.recipe}"

    @property
    def nv(self):
        return int(np.prod(self.shape))

    def lds(self):
        if self.cs:
            return 32, 32, 0
        w = 8 if self.wide else 0
        return self.cin + w, self.cout + (8 if self.wide or self.ybuf else 0), (self.cout + w) if self.ref else 0

    def strides(self):
        """(x_cs, y_cs) in elements"""
        return (self.nv * 32, self.nv * 32) if self.cs else (0, 0)

    def option(self, key):
        return self.opts.get(key, DEFAULTS[key])

    def flops64(self):
        """float64 work of the reference: terms with non-zero planes x the MACs, twice where the judge needs the scale too"""
        nterm = 1 if self.recipe == "lattice" else len(M.TERMS[self.mode])
        inexact = self.recipe == "random" or self.act == SIGMOID
        return (4.0 if inexact else 2.0) * nterm * self.nv * R.ntaps(self.k) * self.cin * self.cout


# ---------------------------------------------------------------------------------------------------------- the rules, restated
def _cdiv(a, b):
    return -(-a // b)


def zr_geometry(c, ncu):
    v = c.option("conv_fwd_variant")
    takes = c.mode in TEAM_MODES or (c.mode == 1 and c.option("fp32_zr") and c.st == "f32")
    takes = takes and (c.st == "f32" or (c.cin % 32 == 0 and c.mode in (5, 7)))
    N, Dd, H, W = c.shape
    if v in (0, 1) or not takes or c.k != K333 or Dd < 4 or c.cin % 16 or c.cout % 32:
        return None
    nZ, nY, nX = _cdiv(Dd, 4), _cdiv(H, 16), _cdiv(W, 8)
    nunits = N * nZ * nY * nX * (c.cout // 32)
    minu = 1 if v == 2 else (c.option("team_min_units") or 2 * ncu)
    pair = bool(c.option("zr_pair")) and c.cout % 64 == 0 and c.st == "f32" and c.mode != 1 and PLANES[c.mode] == 2
    return {"nZ": nZ, "nY": nY, "nX": nX, "nunits": nunits, "ok": nunits >= minu, "pair": pair}


def pp_geometry(c, ncu):
    v = c.option("conv_fwd_variant")
    N, Dd, H, W = c.shape
    if v == 0 or c.mode not in TEAM_MODES or c.st != "f32" or c.k not in (K333, K133) or Dd < 4 or c.cin % 16 or c.cout % 32:
        return None
    CT = 2 if c.cout % 64 == 0 else 1
    nZ, nY, nX = _cdiv(Dd, 4), _cdiv(H, 8), _cdiv(W, 8)
    nunits = N * nZ * nY * nX * (c.cout // (32 * CT))
    if nunits < (1 if v == 1 else (c.option("team_min_units") or 2 * ncu)):
        return None
    return {"CT": CT, "WM": 2 if CT == 2 else 4, "nZ": nZ, "nY": nY, "nX": nX}


def zr_splitk_ks(c, zr, ncu):
    if zr is None or zr["ok"] or not c.option("zr_splitk"):
        return 0
    if c.nv // c.shape[0] * 10 < zr["nZ"] * 4 * zr["nY"] * 16 * zr["nX"] * 8 * ZR_KS_FILL:
        return 0
    nch = c.cin // 16
    for d in range(2, nch // 2 + 1):
        if nch % d == 0 and zr["nunits"] * d >= 2 * ncu and not (c.st != "f32" and (nch // d) % 2):
            return d
    return 0


def splitk_stat_blocks(V, cout):
    cq = cout // 4
    if cout % 4 or cq < 8 or cq > 256 or cq & (cq - 1):
        return 0
    return _cdiv(V, splitk_vb(cout))


def splitk_vb(cout):
    return 4 * (256 // (cout // 4))


def patch_tiling(c):
    N, Dd, H, W = c.shape
    flat = Dd == 1 and c.k[0] == 1
    tz, ty, tx = (1, 16, 16) if flat else (4, 8, 8)
    NR = 2 if c.cout % 64 == 0 else 1
    per = _cdiv(Dd, tz) * _cdiv(H, ty) * _cdiv(W, tx)
    nblk = N * per * (c.cout // (32 * NR))
    nch = c.cin // 16
    ks = 1
    if nblk < 384:
        target = _cdiv(768, nblk)
        ks = max(d for d in range(1, nch + 1) if nch % d == 0 and d <= target)
        mc = c.option("fwd_ksplit_chunks")
        if mc > 0:
            ks = next((d for d in range(ks, nch + 1) if nch % d == 0 and nch // d <= mc), ks)
    return {"flat": flat, "tile": (tz, ty, tx), "NR": NR, "per": per, "ks": ks}


def zr_tile_blocks(c, zr):
    if not c.option("zr_tile_blocks"):
        return 0
    lg = lambda n: 2 if n % 4 == 0 else (1 if n % 2 == 0 else 0)                                # noqa: E731
    return lg(zr["nX"]) | (lg(zr["nY"]) << 4) | (lg(zr["nZ"]) << 8)


def _zr_inst(c, zr, ks):
    i = [0] * INST_N
    one = c.mode in (5, 7)
    if ks:
        wide = one and (c.cin // 16 // ks) % 2 == 0 and bool(c.option("zr_wide") or c.st != "f32")
    else:
        wide = one and c.cin % 32 == 0 and bool(c.option("zr_wide"))
    x32 = xs = 0
    if c.st != "f32":
        ns, wide = 2, True
    elif c.mode == 1:
        ns, wide, x32, xs = 2, False, 1, int(c.option("fp32_zr") == 2)
    elif one:
        ns = 2 if wide else 1
    else:
        ns, wide = 2, False
    i[NS], i[F16], i[T], i[KS] = ns, (int(c.st == "f16") if c.st != "f32" else (0 if c.mode == 1 else IS_F16[c.mode])), ST[c.st], ks or 1
    i[B], i[C], i[D] = int(wide), x32, xs
    i[E] = int(zr["pair"] and ns == 2 and not wide and not x32 and c.st == "f32")
    i[F] = zr_tile_blocks(c, zr)
    if ks:
        i[EPI] = STATS if c.stat else BWD_SUMS if c.sums and splitk_stat_blocks(c.nv // c.shape[0], c.cout) else PLAIN
    else:
        i[A] = 1 if c.stat else 3 if c.refnorm else 2 if c.ref else 0
    return i


def expected(c, ncu=256):
    """-> (kernel, inst, stat_blocks) by the documented rules for a launch with the full workspace"""
    refuse = (-1, [0] * INST_N, 0)
    N, Dd, H, W = c.shape
    V = Dd * H * W
    if c.cin % 16 or c.cout % 32 or (c.st != "f32" and (c.mode not in (5, 7) or ST[c.st] != {5: 1, 7: 2}[c.mode])):
        return refuse
    if (c.gscaled and c.mode != 4) or (c.stat and (c.refnorm or c.gscaled or c.amax)):
        return refuse
    sig = c.act == SIGMOID
    zr, pp = zr_geometry(c, ncu), pp_geometry(c, ncu)
    epi = not sig and not (c.stat and c.ref)
    no_rows = False
    got = None
    if zr and zr["ok"]:
        if epi:
            got = (ZR, _zr_inst(c, zr, 0), 0 if c.ref else zr["nZ"] * zr["nY"] * zr["nX"] * 4)
        elif c.stat:
            return refuse
        no_rows = True
    if got is None and pp:
        if epi:
            i = [0] * INST_N
            i[NS], i[F16], i[T], i[KS], i[A], i[B] = PLANES[c.mode], IS_F16[c.mode], 0, 1, c.k[0], pp["CT"]
            got = (PP, i, 0 if c.ref or no_rows else pp["nZ"] * pp["nY"] * pp["nX"] * pp["WM"])
        elif c.stat:
            return refuse
        no_rows = True
    ks = 0 if pp else zr_splitk_ks(c, zr, ncu)
    if got is None and ks:
        skb = splitk_stat_blocks(V, c.cout)
        if not (c.stat and not skb):
            got = (ZR_SPLITK, _zr_inst(c, zr, ks), skb)
        else:
            no_rows = True
    if got is None:
        if c.k not in (K333, K133, K111):
            return refuse
        t = patch_tiling(c)
        key = {K333: 7, K133: 3, K111: 0}[c.k]
        i = [0] * INST_N
        i[T], i[KS], i[EPI], i[A], i[B], i[C] = ST[c.st], t["ks"], PLAIN if t["ks"] > 1 else 0, key, int(t["flat"]), t["NR"]
        if c.mode == 1:
            if c.stat:
                return refuse
            p = c.option("fwd_persistent")
            i[D] = int(t["NR"] == 2 if p < 0 else p != 0)
            got = (PATCH_FP32, i, 0)
        else:
            blocks = 0 if no_rows or t["ks"] > 1 else t["per"]
            if c.stat and not blocks:
                return refuse
            if (key == 0 and c.option("conv1x1_stream") and c.mode in STREAM_MODES and not c.norm and not c.stat and not sig
                    and c.nv >= 16384):
                i = [0] * INST_N
                i[NS], i[F16], i[T], i[KS], i[A] = (1 if c.st != "f32" else PLANES[c.mode]), \
                    (int(c.st == "f16") if c.st != "f32" else (IS_F16[c.mode] if PLANES[c.mode] == 1 else 0)), ST[c.st], 1, 2 if c.cout >= 64 else 1
                got = (STREAM, i, blocks)
            else:
                i[NS], i[F16], i[D] = (1 if c.st != "f32" else PLANES[c.mode]), (int(c.st == "f16") if c.st != "f32" else IS_F16[c.mode]), int(c.mode == 6)
                got = (PATCH, i, blocks)
    # what only the z-reuse kernel honours
    if c.cs and (got[0] != ZR or c.st == "f32" or c.ref or c.cin % 32 or c.gscaled or c.refnorm):
        return refuse
    if (c.gscaled or c.refnorm) and got[0] != ZR:
        return refuse
    if c.gscaled and (c.bias or c.norm or c.act):
        return refuse
    return got


def stat_geometry(c, kernel, ncu=256):
    """the rows of a launch that writes statistics: ("tile", tile, rows per tile) | ("linear", voxels per row)"""
    if kernel == ZR:
        return ("tile", (4, 16, 8), 4)
    if kernel == PP:
        return ("tile", (4, 8, 8), pp_geometry(c, ncu)["WM"])
    if kernel == ZR_SPLITK:
        return ("linear", splitk_vb(c.cout))
    return ("tile", patch_tiling(c)["tile"], 1)


# ---------------------------------------------------------------------------------------------------------- the table
def _table():
    t = []

    def add(name, want, shape, cin, cout, k, modes, **kw):
        sts = kw.pop("sts", None)
        for mode in modes:
            for st in (sts or ("f32",)):
                t.append(Case(name, want, shape, cin, cout, k, mode, st=st, **kw))

    Z2, P1, P0 = {"conv_fwd_variant": 2}, {"conv_fwd_variant": 1}, {"conv_fwd_variant": 0}
    # ---- z-reuse direct (tile 4 x 16 x 8); conv_fwd_variant 2 lifts the unit minimum
    add("zr_tile", ZR, (1, 4, 16, 8), 16, 32, K333, (2, 4, 5, 7), opts=Z2)
    add("zr_tile", ZR, (1, 4, 16, 8), 16, 32, K333, (2, 4, 5, 7), opts=Z2, dgrad=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4, 5, 7), opts=Z2, bias=True, norm=True, act=RELU, stat=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (1, 2, 4, 5, 7), opts=Z2)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4, 5), opts=Z2, ref=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 7), opts=Z2, ref=True, amax=True, dgrad=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4), opts=Z2, refnorm=True, amax=True, dgrad=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (4,), opts=Z2, gscaled=True, dgrad=True)
    add("zr_rag16", ZR, (2, 5, 17, 9), 32, 64, K333, (5,), sts=("f16",), opts=Z2, bias=True, act=RELU, stat=True)
    add("zr_rag16", ZR, (2, 5, 17, 9), 32, 64, K333, (7,), sts=("bf16",), opts=Z2, bias=True, act=RELU, stat=True)
    add("zr_rag16", ZR, (2, 5, 17, 9), 64, 32, K333, (5,), sts=("f16",), opts=Z2, ref=True, dgrad=True)
    add("zr_rag16", ZR, (2, 5, 17, 9), 64, 32, K333, (7,), sts=("bf16",), opts=Z2, ref=True, dgrad=True)
    add("zr_blk2", ZR, (1, 8, 32, 16), 48, 96, K333, (2, 5, 7), opts=Z2, bias=True)                 # Cin 48: the wide launch falls back
    add("zr_blk4", ZR, (1, 16, 64, 32), 16, 32, K333, (4, 7), opts=Z2)
    add("zr_noblk", ZR, (1, 8, 32, 16), 16, 32, K333, (2,), opts=dict(Z2, zr_tile_blocks=0))
    add("zr_nopair", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4), opts=dict(Z2, zr_pair=0), bias=True)
    add("zr_nowide", ZR, (2, 5, 17, 9), 32, 64, K333, (5, 7), opts=dict(Z2, zr_wide=0), bias=True)
    add("zr_walk", ZR, (2, 16, 48, 48), 16, 128, K333, (2, 5), bias=True, act=RELU, stat=True)      # 576 units on 512 teams: some walk a second unit
    add("zr_fp32", ZR, (2, 5, 17, 9), 32, 64, K333, (1,), opts=Z2, bias=True, norm=True, act=RELU, stat=True)
    add("zr_fp32", ZR, (2, 5, 17, 9), 32, 64, K333, (1,), opts=Z2, ref=True, dgrad=True)
    add("zr_fp32xs", ZR, (2, 5, 17, 9), 32, 64, K333, (1,), opts=dict(Z2, fp32_zr=2), bias=True, act=RELU, stat=True)
    add("zr_fp32off", PATCH_FP32, (2, 5, 17, 9), 32, 64, K333, (1,), opts=dict(Z2, fp32_zr=0), bias=True)
    add("zr_rag", ZR, (2, 5, 17, 9), 32, 64, K333, (1, 5, 7), opts=Z2, refnorm=True, dgrad=True)    # MODE 3 on the exact-fp32 and wide variants
    add("zr_tile", ZR, (1, 4, 16, 8), 16, 32, K333, (2, 5, 7), opts=Z2, refnorm=True, dgrad=True)   # ... unpaired and on one plane
    add("zr_fp32xs", ZR, (2, 5, 17, 9), 32, 64, K333, (1,), opts=dict(Z2, fp32_zr=2))
    add("zr_fp32xs", ZR, (2, 5, 17, 9), 32, 64, K333, (1,), opts=dict(Z2, fp32_zr=2), ref=True, dgrad=True)
    add("zr_wide", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 5), opts=Z2, wide=True, bias=True, ref=True)
    add("zr_split", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4), opts=Z2, recipe="split")
    add("zr_split", ZR, (2, 5, 17, 9), 32, 64, K333, (2, 4), opts=Z2, recipe="split", dgrad=True, ref=True)
    add("zr_rnd", ZR, (2, 5, 17, 9), 32, 64, K333, (1, 2, 4, 5, 7), opts=Z2, bias=True, norm=True, act=RELU, stat=True, recipe="random")
    add("zr_rnd16", ZR, (2, 5, 17, 9), 32, 64, K333, (5,), sts=("f16",), opts=Z2, bias=True, recipe="random")
    add("zr_rnd16", ZR, (2, 5, 17, 9), 32, 64, K333, (7,), sts=("bf16",), opts=Z2, bias=True, recipe="random")
    # ---- z-reuse with split input channels: 64 units, ks 8, slices of two chunks
    SK = (1, 8, 16, 32)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (2, 4, 5, 7, 1), bias=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (2, 5), bias=True, act=RELU, stat=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (2, 7), ref=True, dgrad=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (4,), bias=True, ybuf=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (5,), sts=("f16",), bias=True, act=RELU, stat=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (7,), sts=("bf16",), ref=True, dgrad=True)
    add("zk_odd", ZR_SPLITK, (1, 8, 32, 32), 192, 256, K333, (5, 7), bias=True)                     # slices of three chunks: WIDE off
    add("zk", PATCH, SK, 256, 256, K333, (2, 5), opts={"zr_splitk": 0}, bias=True, ref=True)    # the patch kernel's split-K
    add("zk_rnd", ZR_SPLITK, SK, 256, 256, K333, (5,), bias=True, act=RELU, stat=True, recipe="random")
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (2, 5), wide=True, bias=True, ref=True)
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (2, 5), ref=True, dgrad=True, sums=True)              # the bwd_sums epilogue
    add("zk", ZR_SPLITK, SK, 256, 256, K333, (7,), sts=("bf16",), dgrad=True, sums=True)
    # non-zero lo planes through the two-plane KSPLIT instantiations: mode 4 at Cin 256 (its accumulators stay near 2^14 steps),
    # mode 2 where the rules give split-K at Cin 64 (256 units, ks 2)
    add("zk_split", ZR_SPLITK, SK, 256, 256, K333, (4,), recipe="split")
    add("zk_split", ZR_SPLITK, SK, 256, 256, K333, (4,), recipe="split", dgrad=True, ref=True)
    add("zk_split64", ZR_SPLITK, (1, 16, 64, 64), 64, 64, K333, (2,), recipe="split")
    # the chunk-stride layout of 16-bit tensors (z-reuse direct only)
    add("zr_cs", ZR, (2, 5, 17, 9), 64, 64, K333, (5,), sts=("f16",), opts=Z2, cs=True, bias=True, act=RELU, stat=True)
    add("zr_cs", ZR, (2, 5, 17, 9), 64, 64, K333, (7,), sts=("bf16",), opts=Z2, cs=True, dgrad=True)
    add("zr_cs", ZR, (2, 5, 17, 9), 64, 64, K333, (5,), sts=("f16",), opts=Z2, cs=True, bias=True)
    add("pt_ksc", PATCH, (2, 4, 32, 32), 128, 256, K133, (2, 5), opts=dict(P0, fwd_ksplit_chunks=1), bias=True)   # ks 8 where the heuristic has 4
    # ---- ping-pong (patch 4 x 8 x 8); conv_fwd_variant 1 lifts the unit minimum
    add("pp_patch", PP, (1, 4, 8, 8), 16, 32, K333, (2, 4, 5, 7), opts=P1)
    add("pp_rag", PP, (2, 5, 9, 9), 32, 64, K333, (2, 4, 5, 7), opts=P1, bias=True, norm=True, act=RELU, stat=True)
    add("pp_rag", PP, (2, 5, 9, 9), 32, 96, K333, (2, 5), opts=P1, bias=True, act=RELU, stat=True)
    add("pp_rag", PP, (2, 5, 9, 9), 64, 32, K333, (4, 7), opts=P1, ref=True, dgrad=True)
    add("pp_k133", PP, (2, 5, 9, 9), 32, 64, K133, (2, 4, 5, 7), opts=P1, bias=True, stat=True)
    add("pp_k133", PP, (1, 8, 16, 24), 16, 32, K133, (2, 7), opts=P1, ref=True, dgrad=True)
    add("pp_k133", PP, (2, 5, 9, 9), 32, 32, K133, (4, 5), opts=P1, bias=True)
    add("pp_big", PP, (1, 8, 16, 24), 16, 64, K333, (2, 5), opts=P1, bias=True)
    add("pp_wide", PP, (2, 5, 9, 9), 32, 64, K333, (2, 5), opts=P1, wide=True, bias=True, ref=True)
    add("pp_split", PP, (2, 5, 9, 9), 32, 64, K333, (2, 4), opts=P1, recipe="split")
    add("pp_split", PP, (2, 5, 9, 9), 32, 32, K133, (2, 4), opts=P1, recipe="split", dgrad=True)
    add("pp_rnd", PP, (2, 5, 9, 9), 32, 64, K333, (2, 4, 5, 7), opts=P1, bias=True, norm=True, act=RELU, stat=True, recipe="random")
    # ---- the split-precision patch kernel; conv_fwd_variant 0 forces it
    add("pt_333", PATCH, (2, 3, 9, 11), 16, 32, K333, (2, 3, 4, 5, 6, 7), opts=P0, bias=True, norm=True, act=SIGMOID)
    add("pt_333", PATCH, (2, 3, 9, 11), 32, 64, K333, (2, 3, 4, 5, 6, 7), opts=P0, ref=True, dgrad=True)
    add("pt_133", PATCH, (2, 3, 9, 11), 16, 64, K133, (2, 3, 6), opts=P0, bias=True, act=RELU)
    add("pt_133f", PATCH, (1, 1, 17, 19), 32, 32, K133, (2, 4, 5, 7), opts=P0, bias=True, ref=True)
    add("pt_111", PATCH, (2, 3, 9, 11), 32, 64, K111, (2, 3, 4, 5, 6, 7), bias=True)
    add("pt_111f", PATCH, (1, 1, 17, 19), 16, 32, K111, (2, 6), ref=True, dgrad=True)
    add("pt_16", PATCH, (2, 3, 9, 11), 32, 64, K333, (5,), sts=("f16",), opts=P0, bias=True, ref=True)
    add("pt_16", PATCH, (2, 3, 9, 11), 32, 32, K133, (7,), sts=("bf16",), opts=P0, bias=True, act=RELU)
    add("pt_stat", PATCH, (4, 16, 32, 32), 16, 32, K333, (2, 5), opts=P0, bias=True, act=RELU, stat=True)   # 512 workgroups: no split-K, rows
    add("pt_wide", PATCH, (2, 3, 9, 11), 32, 64, K333, (2, 5), opts=P0, wide=True, bias=True, ref=True)
    add("pt_split", PATCH, (2, 3, 9, 11), 32, 64, K333, (2, 4), opts=P0, recipe="split")
    add("pt_split", PATCH, (1, 1, 17, 19), 32, 32, K133, (2, 4), opts=P0, recipe="split", dgrad=True)
    add("pt_rnd", PATCH, (2, 3, 9, 11), 32, 64, K333, (2, 3, 4, 5, 6, 7), opts=P0, bias=True, norm=True, act=RELU, recipe="random")
    # ---- the exact-fp32 patch kernel
    for pers in (0, 1):
        o = dict(P0, fwd_persistent=pers, fp32_zr=0)
        add(f"pf_333p{pers}", PATCH_FP32, (2, 3, 9, 11), 16, 32, K333, (1,), opts=o, bias=True, norm=True, act=SIGMOID)
        add(f"pf_333p{pers}", PATCH_FP32, (2, 3, 9, 11), 32, 64, K333, (1,), opts=o, ref=True, dgrad=True)
        add(f"pf_133p{pers}", PATCH_FP32, (1, 1, 17, 19), 32, 64, K133, (1,), opts=o, bias=True, ref=True)
        add(f"pf_111p{pers}", PATCH_FP32, (2, 3, 9, 11), 32, 32, K111, (1,), opts=o, bias=True, act=RELU)
    add("pf_133", PATCH_FP32, (2, 3, 9, 11), 32, 64, K133, (1,), bias=True)
    add("pf_111f", PATCH_FP32, (1, 1, 17, 19), 16, 64, K111, (1,), ref=True, dgrad=True)
    add("pf_wide", PATCH_FP32, (2, 3, 9, 11), 32, 64, K333, (1,), opts={"fp32_zr": 0}, wide=True, bias=True, ref=True)
    add("pf_rnd", PATCH_FP32, (2, 3, 9, 11), 32, 64, K333, (1,), opts={"fp32_zr": 0}, bias=True, norm=True, act=RELU, recipe="random")
    # ---- the 1x1 stream: NV >= 16384
    add("st_a", STREAM, (1, 16, 32, 32), 32, 32, K111, (2, 3, 5, 7), bias=True)
    add("st_b", STREAM, (1, 17, 33, 31), 16, 64, K111, (2, 3, 5, 7), ref=True, amax=True, dgrad=True)
    add("st_c", STREAM, (1, 17, 33, 31), 32, 96, K111, (2, 7), bias=True, act=RELU, amax=True)
    add("st_16", STREAM, (1, 17, 33, 31), 32, 64, K111, (5,), sts=("f16",), bias=True, ref=True, amax=True)
    add("st_16", STREAM, (1, 17, 33, 31), 32, 32, K111, (7,), sts=("bf16",), bias=True)
    add("st_16", STREAM, (1, 17, 33, 31), 32, 32, K111, (5,), sts=("f16",), ref=True, dgrad=True)
    add("st_16", STREAM, (1, 17, 33, 31), 32, 64, K111, (7,), sts=("bf16",), bias=True, act=RELU)
    add("st_wide", STREAM, (1, 16, 32, 32), 32, 64, K111, (2, 5), wide=True, bias=True, ref=True)
    add("st_off", PATCH, (1, 16, 32, 32), 32, 32, K111, (2,), opts={"conv1x1_stream": 0}, bias=True)
    add("st_split", STREAM, (1, 16, 32, 32), 32, 64, K111, (2,), recipe="split")
    add("st_rnd", STREAM, (1, 17, 33, 31), 32, 64, K111, (2, 3, 5, 7), bias=True, act=RELU, recipe="random")
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids are unique"
NAMES = sorted({c.name for c in CASES}, key=[c.name for c in CASES].index)


def _req():
    """the instantiations the suite undertakes to reach with lattice cases (DESIGN.md names the ones left out): (kernel, the
    template arguments that name the instantiation)"""
    r = []
    # k_conv_zr<NS, F16, MODE, KSPLIT, WIDE, T, X32, XS, PAIR>: (NS, F16, T, MODE, WIDE, X32, XS, PAIR)
    for mode in (0, 1, 2):
        r += [(ZR, (2, 0, 0, mode, 0, 0, 0, 1)), (ZR, (2, 1, 0, mode, 0, 0, 0, 1))]          # modes 2 / 4, paired (Cout 64)
        r += [(ZR, (2, 1, 0, mode, 1, 0, 0, 0)), (ZR, (2, 0, 0, mode, 1, 0, 0, 0))]          # modes 5 / 7, wide
        r += [(ZR, (2, 0, 0, mode, 0, 1, 0, 0))]                                               # exact fp32
    r += [(ZR, (2, 1, 1, m, 1, 0, 0, 0)) for m in (1, 2)] + [(ZR, (2, 0, 2, m, 1, 0, 0, 0)) for m in (1, 2)]   # 16-bit storage
    r += [(ZR, (2, 1, 1, 0, 1, 0, 0, 0)), (ZR, (2, 0, 2, 0, 1, 0, 0, 0))]                    # ... plain (the chunk-stride cases)
    r += [(ZR, (2, 0, 0, 3, 0, 0, 0, 1)), (ZR, (2, 1, 0, 3, 0, 0, 0, 1))]                    # refnorm
    r += [(ZR, (2, 0, 0, 0, 0, 0, 0, 0)), (ZR, (2, 1, 0, 0, 0, 0, 0, 0))]                    # unpaired (Cout 32 / 96, zr_pair 0)
    r += [(ZR, (1, 1, 0, 0, 0, 0, 0, 0)), (ZR, (1, 0, 0, 0, 0, 0, 0, 0))]                    # one plane, 16 channels per phase
    r += [(ZR, (2, 0, 0, 1, 0, 1, 1, 0)), (ZR, (1, 1, 0, 1, 0, 0, 0, 0))]                    # XS; one plane with statistics
    r += [(ZR, (2, 0, 0, m, 0, 1, 1, 0)) for m in (0, 2)]                                    # XS plain and masked
    r += [(ZR, (1, 0, 0, 3, 0, 0, 0, 0)), (ZR, (1, 1, 0, 3, 0, 0, 0, 0)), (ZR, (2, 0, 0, 3, 0, 0, 0, 0)), (ZR, (2, 0, 0, 3, 0, 1, 0, 0)),
          (ZR, (2, 0, 0, 3, 1, 0, 0, 0)), (ZR, (2, 1, 0, 3, 1, 0, 0, 0))]                     # refnorm: one plane, unpaired, exact fp32, wide
    # ... KSPLIT: (NS, F16, T, WIDE, X32, PAIR, epilogue)
    r += [(ZR_SPLITK, (2, 0, 0, 0, 0, 1, PLAIN)), (ZR_SPLITK, (2, 1, 0, 0, 0, 1, PLAIN)), (ZR_SPLITK, (2, 1, 0, 1, 0, 0, PLAIN)),
          (ZR_SPLITK, (2, 0, 0, 1, 0, 0, PLAIN)), (ZR_SPLITK, (2, 0, 0, 0, 1, 0, PLAIN)), (ZR_SPLITK, (2, 0, 0, 0, 0, 1, STATS)),
          (ZR_SPLITK, (2, 1, 1, 1, 0, 0, STATS)), (ZR_SPLITK, (2, 0, 2, 1, 0, 0, PLAIN)), (ZR_SPLITK, (1, 1, 0, 0, 0, 0, PLAIN)),
          (ZR_SPLITK, (1, 0, 0, 0, 0, 0, PLAIN)), (ZR_SPLITK, (2, 1, 0, 1, 0, 0, STATS)),
          (ZR_SPLITK, (2, 0, 0, 0, 0, 1, BWD_SUMS)), (ZR_SPLITK, (2, 1, 0, 1, 0, 0, BWD_SUMS)), (ZR_SPLITK, (2, 0, 2, 1, 0, 0, BWD_SUMS))]
    # k_conv_pp<KD, .., CT, .., NS, F16>
    r += [(PP, (kd, ct, ns, f)) for kd in (1, 3) for ct in (1, 2) for ns, f in ((2, 0), (2, 1), (1, 1), (1, 0))]      # all 16
    # k_conv_fwd_bfsplit: (key, flat, NR, NS, F16, PS, T)
    r += [(PATCH, (7, 0, nr, ns, f, ps, 0)) for nr in (1, 2) for ns, f, ps in ((2, 0, 0), (3, 0, 0), (2, 1, 0), (1, 1, 0), (2, 1, 1), (1, 0, 0))]
    r += [(PATCH, (7, 0, 2, 1, 1, 0, 1)), (PATCH, (3, 0, 1, 1, 0, 0, 2)), (PATCH, (3, 0, 2, 2, 0, 0, 0)), (PATCH, (3, 0, 2, 3, 0, 0, 0)),
          (PATCH, (3, 0, 2, 2, 1, 1, 0)), (PATCH, (3, 0, 2, 1, 1, 0, 0))]
    r += [(PATCH, (3, 1, 1, ns, f, 0, 0)) for ns, f in ((2, 0), (2, 1), (1, 1), (1, 0))]
    r += [(PATCH, (0, 0, 2, ns, f, ps, 0)) for ns, f, ps in ((2, 0, 0), (3, 0, 0), (2, 1, 0), (1, 1, 0), (2, 1, 1), (1, 0, 0))]
    r += [(PATCH, (0, 1, 1, 2, 0, 0, 0)), (PATCH, (0, 1, 1, 2, 1, 1, 0)), (PATCH, (0, 0, 1, 2, 0, 0, 0))]
    # k_conv_fwd_mfma[_p]: (key, flat, NR, persistent)
    r += [(PATCH_FP32, (7, 0, nr, p)) for nr in (1, 2) for p in (0, 1)] + [(PATCH_FP32, (3, 1, 2, p)) for p in (0, 1)]
    r += [(PATCH_FP32, (0, 0, 1, p)) for p in (0, 1)] + [(PATCH_FP32, (3, 0, 2, 1)), (PATCH_FP32, (0, 1, 2, 1))]
    # k_conv1x1_stream<NS, F16, CT, T>
    r += [(STREAM, (ns, f, ct, 0)) for ct in (1, 2) for ns, f in ((2, 0), (3, 0), (1, 1), (1, 0))]
    r += [(STREAM, (1, 1, ct, 1)) for ct in (1, 2)] + [(STREAM, (1, 0, ct, 2)) for ct in (1, 2)]
    return r


def signature(kernel, i):
    """the template arguments that name the instantiation, from the query's inst"""
    if kernel == ZR:
        return (i[NS], i[F16], i[T], i[A], i[B], i[C], i[D], i[E])
    if kernel == ZR_SPLITK:
        return (i[NS], i[F16], i[T], i[B], i[C], i[E], i[EPI])
    if kernel == PP:
        return (i[A], i[B], i[NS], i[F16])
    if kernel == PATCH:
        return (i[A], i[B], i[C], i[NS], i[F16], i[D], i[T])
    if kernel == PATCH_FP32:
        return (i[A], i[B], i[C], i[D])
    if kernel == STREAM:
        return (i[NS], i[F16], i[A], i[T])
    return ()


REQUIRED = _req()
SUMS_G = 8                                    # groups of the norm a `sums` data gradient lands behind


# ---------------------------------------------------------------------------------------------------------- the library's query
def use_mfma(c):
    return c.mode | (ST[c.st] << 8) | (ST[c.st] << 12)                             # TEM_MFMA_STX | TEM_MFMA_STY


def fwd_ws(lib, c):
    return int(lib.tem_conv3d_fwd_ws(*c.shape, c.cin, c.cout, *c.k, use_mfma(c)))


def query(lib, c, p, ws_bytes=None, bp=None):
    """tem_conv3d_fwd_mfma_path for pointers p: dict x, scale, shift, w, bias, y, ref, amax, coef of ctypes.c_void_p | None ->
    (kernel, inst)"""
    import ctypes
    x_ld, y_ld, ref_ld = c.lds()
    inst = (ctypes.c_int * INST_N)()
    k = lib.tem_conv3d_fwd_mfma_path(p["x"], x_ld, p.get("scale"), p.get("shift"), p["w"], p.get("bias"), p["y"], y_ld, p.get("ref"), ref_ld,
                                     fwd_ws(lib, c) if ws_bytes is None else ws_bytes, *c.shape, c.cin, c.cout, *c.k, c.act, use_mfma(c),
                                     p.get("amax"), p.get("coef"), int(c.stat), *c.strides(), bp, inst)
    return k, list(inst)[:INST_N - 1] + [0]


def byproducts(L, c, p):
    """the TemByproducts of a launch (L: torch_em_amd._lib), or None: out_amax for `amax`, the sums request for `sums`.
    p: dict out_amax, sums_x, sums_mean, sums_rstd, sums_part of addresses (int)"""
    if not (c.amax or c.sums):
        return None
    bp = L.Byproducts()
    if c.amax:
        bp.out_amax = p["out_amax"]
    if c.sums:
        bp.sums_x, bp.sums_x_ld, bp.sums_mean, bp.sums_rstd = p["sums_x"], c.cout, p["sums_mean"], p["sums_rstd"]
        bp.sums_G, bp.sums_part, bp.sums_nblk = SUMS_G, p["sums_part"], splitk_stat_blocks(c.nv // c.shape[0], c.cout)
    return bp


def fake_byproducts(L, c):
    return byproducts(L, c, {k: VK.BASE + VK.PAD * 4 for k in ("out_amax", "sums_x", "sums_mean", "sums_rstd", "sums_part")})


def fake_pointers(c):
    """the addresses a Laid layout of the case's tensors has behind a 256-byte aligned allocation (oracle/gpu_kit.py: PAD)"""
    import ctypes
    es = VK.ESIZE[c.st]
    lo = 8 if c.wide else 0
    P = lambda a: ctypes.c_void_p(a)                                               # noqa: E731
    base = VK.BASE + VK.PAD * 4
    p = {"x": P(VK.BASE + (VK.PAD + lo) * es), "y": P(VK.BASE + (VK.PAD + (8 if c.wide or c.ybuf else 0)) * es), "w": P(base)}
    for key, on in (("scale", c.norm), ("shift", c.norm), ("bias", c.bias), ("amax", c.gscaled), ("coef", c.refnorm)):
        p[key] = P(base) if on else None
    p["ref"] = P(VK.BASE + (VK.PAD + lo) * es) if c.ref else None
    return p


# ---------------------------------------------------------------------------------------------------------- inputs
SPLIT_LO = {2: (2.0 ** -10, 2.0 ** -12), 4: (2.0 ** -13, 2.0 ** -14)}           # mode: (lo of x, lo of w)


def _signs(rng, shape):
    return np.where(rng.rand(*shape) < 0.5, -1.0, 1.0).astype(np.float32)


def inputs(c):
    """-> dict of float32 arrays: x [N, D, H, W, cin], w_sd (the LAYER's state_dict weights: [cout][cin][taps] of a forward,
    [cin][cout][taps] of a data gradient), bias [cout], scale / shift [N, cin], ref [.., cout], coef [N, cout, 4], amax (float:
    max |x| of a gscaled launch); None where absent"""
    rng = np.random.RandomState(UK.seed_of(c.name, c.shape + (c.cin, c.cout), c.k) + 13 * int(c.dgrad))
    sh, nt = c.shape, R.ntaps(c.k)
    wshape = (c.cin, c.cout, nt) if c.dgrad else (c.cout, c.cin, nt)
    if c.recipe in ("lattice", "split"):
        d = {"x": VK._ints(rng, sh + (c.cin,)), "w_sd": VK._quarters(rng, wshape), "bias": VK._quarters(rng, (c.cout,)),
             "scale": VK._pow2(rng, (sh[0], c.cin), signed=False), "shift": VK._quarters(rng, (sh[0], c.cin)),
             "ref": VK._ints(rng, sh + (c.cout,), negzero=0.3), "coef": VK._pow2(rng, (sh[0], c.cout, 4))}
        if c.sums:
            d.update(sums_x=VK._ints(rng, sh + (c.cout,)), sums_mean=VK._quarters(rng, (sh[0], SUMS_G)),
                     sums_rstd=VK._pow2(rng, (sh[0], SUMS_G), signed=False))
        if c.recipe == "split":
            assert not (c.bias or c.norm or c.refnorm) and c.st == "f32"
            lx, lw = SPLIT_LO[c.mode]
            if c.mode == 4:
                d["w_sd"] = (rng.randint(-4, 5, size=wshape) / 2.0).astype(np.float32)          # halves
            d["x"] = (d["x"] + np.where(d["x"] != 0, _signs(rng, d["x"].shape) * np.float32(lx), 0)).astype(np.float32)
            d["w_sd"] = (d["w_sd"] + np.where(d["w_sd"] != 0, _signs(rng, wshape) * np.float32(lw), 0)).astype(np.float32)
    else:
        s = UK.seed_of(c.name, c.shape + (c.cin, c.cout), c.k)
        fan = nt * (c.cout if c.dgrad else c.cin)
        d = {"x": UK.make_tensor(sh + (c.cin,), s, "16"), "w_sd": (rng.randn(*wshape) / np.sqrt(fan)).astype(np.float32),
             "bias": rng.randn(c.cout).astype(np.float32), "scale": rng.uniform(0.5, 2.0, (sh[0], c.cin)).astype(np.float32),
             "shift": (0.5 * rng.randn(sh[0], c.cin)).astype(np.float32), "ref": UK.make_tensor(sh + (c.cout,), s + 1, "16"),
             "coef": UK.make_coef(sh[0], c.cout, s + 3)}
    for key, on in (("bias", c.bias), ("scale", c.norm), ("shift", c.norm), ("ref", c.ref), ("coef", c.refnorm)):
        if not on:
            d[key] = None
    d["amax"] = float(np.abs(d["x"]).max()) if c.gscaled else None
    for key in ("sums_x", "sums_mean", "sums_rstd"):
        d.setdefault(key, None)
    return d


def step(c):
    """the lattice step of a case: the smallest product (per accumulator for mode 4 on the split recipe)"""
    if c.recipe == "split":
        return {2: (2.0 ** -12,), 4: (0.5, 0.25)}[c.mode]
    s = (0.25 if c.norm else 1.0) * 0.25
    if c.refnorm:
        s *= 0.25                                                                    # a lin and (ref - mean) m2r with halves
    return (s,) * 2                     # (a gscaled launch multiplies terms and step by the same power of two)


def model(c, d=None, skip=None, want_mag=True):
    d = d or inputs(c)
    return M.fwd_model(d["x"], d["w_sd"], c.k, c.mode, d["bias"], d["scale"], d["shift"], c.act, d["ref"], c.dgrad, d["coef"], d["amax"], skip,
                       want_mag)


def lattice_bounds(c, d=None):
    """-> [sum |terms| / step per accumulator] of a lattice / split case, before activation and mask.  split: the same upper
    bound per accumulator, or where that is too coarse (mode 2 from Cin 32 on) the sums themselves.
    lattice: an upper bound of them that needs no convolution (M.term_bound: every |x| at its maximum) plus |bias|, and for a
    refnorm epilogue |a| times that plus |m1| + (|ref| + |mean|) |m2r| at their maxima."""
    d = d or inputs(c)
    st = step(c)
    if c.recipe == "split":
        tb = M.term_bound(d["x"], d["w_sd"], c.mode, c.dgrad)
        if all(b / s < 2 ** 24 for b, s in zip(tb, st)):                       # the bound that needs no convolution suffices
            return [b / s for b, s in zip(tb, st)]
        amag = M.abs_sums32(d["x"], d["w_sd"], c.k, c.mode, c.dgrad)           # the sums themselves (float32: 2^-10 accurate)
        return [float(np.max(m)) * 1.001 / s for m, s in zip(amag, st)]
    b = M.term_bound(M.xhat32(d["x"], d["scale"], d["shift"]), d["w_sd"], 1, c.dgrad)[0]          # (a lattice has one plane)
    if c.bias:
        b += float(np.abs(d["bias"]).max())
    if c.refnorm:
        a, m1, m2r, mean = (float(np.abs(d["coef"][..., j]).max()) for j in range(4))
        b = a * b + m1 + (float(np.abs(d["ref"]).max()) + mean) * m2r
    return [b / st[0]]


E32_WORK = 1 << 22                     # the yardstick is evaluated on at most E32_WORK / (cin cout) voxels (at least 64), a fixed subset


def reference(c, d=None, cache=None):
    """-> dict: y, mag (float64; 0 for the exact cases), e32 (random cases and sigmoid outputs; 0 for the exact ones).  cache: a
    dict that keeps the accumulated sums of a layer for the cases that differ only in their epilogue (and, on the lattice, where
    every mode has the same planes, in their mode)"""
    d = d or inputs(c)
    inexact = c.recipe == "random" or c.act == SIGMOID
    pre = None
    if cache is not None and not c.gscaled:
        pm = c.mode if c.recipe != "lattice" or c.mode == 6 else 1               # (mode 6 prescales its planes)
        key = (c.name, c.shape, c.cin, c.cout, c.k, c.dgrad, c.recipe, c.norm, inexact, pm)
        if key not in cache:
            if len(cache) >= 6:
                cache.clear()
            cache[key] = M.accumulate(M.xhat32(d["x"], d["scale"], d["shift"]), d["w_sd"], c.k, pm, c.dgrad, None, inexact)
        pre = cache[key]
    r = M.fwd_model(d["x"], d["w_sd"], c.k, c.mode, d["bias"], d["scale"], d["shift"], c.act, d["ref"], c.dgrad, d["coef"], d["amax"], None,
                    inexact, pre)
    e32 = 0.0
    if inexact:
        sample, n = None, max(64, E32_WORK // (c.cin * c.cout))
        if c.nv > n:
            sample = np.sort(np.random.RandomState(5).choice(c.nv, n, replace=False))
        e32 = M.model_e32(d["x"], d["w_sd"], c.k, c.mode, r["y"], r["mag"], d["bias"], d["scale"], d["shift"], c.act, d["ref"], c.dgrad, sample)
    return {"y": r["y"], "mag": r["mag"], "e32": e32}
