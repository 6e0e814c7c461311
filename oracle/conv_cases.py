"""Inputs and the case tables shared by tests/test_conv_valu_cpu.py and tests/test_gpu_conv_valu.py (TEST INFRASTRUCTURE).

Two input recipes.
  lattice   x, g, ref and the gnorm y are integers in [-4, 4] with a large share of exact zeros (ref and y: some of them -0.0);
            w, bias and shift are integers / 4 in [-2, 2]; scale is 0.5, 1 or 2; the gnorm coefficients are +-0.5, +-1, +-2.
            Every value is exact in fp32, fp16 and bf16 and every term of every sum is a multiple of the case's lattice step, so
            with sum |terms| / step < 2^24 (asserted for every case by tests/test_conv_valu_cpu.py) every partial sum in any
            order, contracted or not, is a float32 number: a float32 kernel returns the float64 value and the judge is
            equality.  A sigmoid output is the one inexact quantity: judged by the units rule.
  random    upsample_cases.make_tensor on the grid every storage type holds (x, g, ref, y) and float32 normal weights, bias
            and coefficients: judged in units of 2^-23 x the per-element scale against MARGIN x max(e32, 1) (oracle/conv_ref.py).

The selector rules the tables are written against (include/tem_hip.h: tem_conv3d_fwd_valu_path, tem_conv3d_wgrad_path) are
restated in expected_fwd() / expected_wgrad(); every case names the kernel it is meant for, the rules must agree, and the
library's query must agree with both.  A tensor is channels [lo, lo + C) of a Wd-channel buffer behind oracle/gpu_kit.py's
PAD sentinels: address() gives the byte address the rules see.
"""
import numpy as np

from . import conv_ref as R
from . import upsample_cases as UK

C1ROWS, CIN1, COUT1, PROJ_R, PROJ, EXPAND, SMALLCOUT, GENERIC = range(8)      # TEM_VALU_*
FWD_NAME = {-1: "refused", 0: "c1rows", 1: "cin1", 2: "cout1", 3: "proj_r", 4: "proj", 5: "expand", 6: "smallcout", 7: "generic"}
WG_GENERIC, WG_CIN1, WG_PROJ = 0, 1, 2                                        # TEM_WGRAD_*
WG_NAME = {-1: "refused", 0: "wgrad_generic", 1: "wgrad_cin1", 2: "proj_wgrad"}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
PAD = 64                                  # oracle/gpu_kit.py
BASE = 1 << 20                            # a 256-byte aligned allocation, as the caching allocator returns them
K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
KSIZES = [(a, b, c) for a in (1, 3) for b in (1, 3) for c in (1, 3)]
FF, FH, FB, HH, BB, HF, BF = (("f32", "f32"), ("f32", "f16"), ("f32", "bf16"), ("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"),
                              ("bf16", "f32"))
NONE, RELU, SIGMOID = R.NONE, R.RELU, R.SIGMOID


def address(dt, lo=0, off=0):
    """the byte address of channel lo of the first voxel of a Laid tensor (off: extra elements)"""
    return BASE + (PAD + lo + off) * ESIZE[dt]


# ---------------------------------------------------------------------------------------------------------- forward table
class Fwd:
    """one forward launch.  shape (N, D, H, W); pair (x type, y / ref type); xlay / ylay / reflay: None dense | (Wd, lo);
    bias_off: floats the bias pointer is moved off its 16-byte boundary; amax: TEM_BP_OUT_AMAX requested"""

    def __init__(self, name, want, shape, cin, cout, k, pair=FF, bias=True, norm=False, act=NONE, ref=False, stat=False, amax=False,
                 xlay=None, ylay=None, reflay=None, bias_off=0, recipe="lattice", inst=None):
        self.name, self.want, self.shape, self.cin, self.cout, self.k, self.pair = name, want, tuple(shape), cin, cout, tuple(k), pair
        self.bias, self.norm, self.act, self.ref, self.stat, self.amax = bias, norm, act, ref, stat, amax
        self.xlay, self.ylay, self.reflay, self.bias_off, self.recipe, self.inst = xlay, ylay, reflay, bias_off, recipe, inst

    @property
    def id(self):
        return (f"{self.name}-{self.pair[0]}.{self.pair[1]}-{'b' if self.bias else ''}{'n' if self.norm else ''}"
                f"{'rs'[self.act - 1] if self.act else ''}{'m' if self.ref else ''}{'t' if self.stat else ''}{'a' if self.amax else ''}"
                f"{'' if self.recipe == 'lattice' else '-rnd'}")

    @property
    def nv(self):
        return int(np.prod(self.shape))

    def lds(self):
        """(x_ld, y_ld, ref_ld)"""
        return ((self.xlay or (self.cin,))[0], (self.ylay or (self.cout,))[0], (self.reflay or (self.cout,))[0] if self.ref else 0)

    def bytes_moved(self):
        x_ld, y_ld, ref_ld = self.lds()
        return self.nv * (x_ld * ESIZE[self.pair[0]] + (y_ld + ref_ld) * ESIZE[self.pair[1]])


def stat_blocks(c):
    """tem_conv3d_fwd_stat_blocks of the first-layer kernels as include/tem_hip.h documents it (0: no rows)"""
    N, D, H, W = c.shape
    cq = c.cout // 4
    if c.cin > 4 or c.cout % 4 or c.cin * c.cout > 128 or cq > 64 or cq & (cq - 1) or c.k not in (K333, K133):
        return 0
    tx = stat_tile(c)[2]
    return -(-D // 4) * -(-H // 8) * -(-W // tx)


def stat_tile(c):
    cp = c.cout // 2
    rows = c.cin == 1 and c.cout % 2 == 0 and 1 <= cp <= 64 and cp & (cp - 1) == 0
    return (4, 8, 32 if rows else 8)


def expected_fwd(c):
    """-> (path, [COUT, NJ, CIN, KD]) by the documented rules, from the addresses and leading dimensions of the launch"""
    dx, dy = c.pair
    x_ld, y_ld, ref_ld = c.lds()
    xa = address(dx, (c.xlay or (0, 0))[1])
    ya = address(dy, (c.ylay or (0, 0))[1])
    ra = address(dy, (c.reflay or (0, 0))[1]) if c.ref else 0
    ba = address("f32", 0, c.bias_off) if c.bias else 0
    cin, cout, k = c.cin, c.cout, c.k
    first = cin <= 4 and cout % 4 == 0 and cin * cout <= 128 and k in (K333, K133)
    if first and not c.ref and y_ld % 4 == 0 and ya % (16 if dy == "f32" else 8) == 0 and ba % 16 == 0:
        if c.stat and not stat_blocks(c):
            return -1, [0, 0, 0, 0]
        return (C1ROWS, [0, 0, 0, k[0]]) if stat_tile(c)[2] == 32 else (CIN1, [0, 0, cin, k[0]])
    if c.stat:
        return -1, [0, 0, 0, 0]
    x16 = x_ld % 4 == 0 and xa % 16 == 0
    if cout == 1 and cin % 16 == 0 and k in (K333, K133) and not c.norm and not c.ref and x16:
        return COUT1, [0, 0, 0, k[0]]
    if k == K111 and not c.norm:
        if cin % 32 == 0 and cout in (1, 2, 3, 4, 6, 8, 12, 16) and not c.ref and x16:
            nj = cin // 32
            nj = nj if nj in (1, 2) or (nj == 4 and cout <= 8) else 0
            return (PROJ_R if nj else PROJ), [cout, nj, 0, 0]
        if cin <= 16 and cout % 4 == 0 and y_ld % 4 == 0 and ya % 16 == 0 and ba % 16 == 0 and (not c.ref or (ref_ld % 4 == 0 and ra % 16 == 0)):
            return EXPAND, [0, 0, 0, 0]
    if k == K111 and cin % 4 == 0 and cout in (1, 2, 3, 4, 8, 12, 16) and x16:
        return SMALLCOUT, [cout, 0, 0, 0]
    return GENERIC, [0, 0, 0, k[0] * 100 + k[1] * 10 + k[2]]


def _variants(base, combos, **kw):
    """`base` (a dict of Fwd arguments) once per (bias, norm, act, stat) of combos; a pre-norm runs with N = 2"""
    out = []
    for bias, norm, act, stat in combos:
        d = dict(base, bias=bias, norm=norm, act=act, stat=stat, **kw)
        if norm and d["shape"][0] == 1:
            d["shape"] = (2,) + tuple(d["shape"][1:])
        out.append(d)
    return out


BN4 = [(1, 0, NONE, 0), (0, 0, NONE, 0), (1, 1, NONE, 0), (0, 1, NONE, 0)]          # with bias and without, with the pre-norm and without
FIRST = [(1, 0, NONE, 0), (0, 0, RELU, 1), (1, 1, RELU, 1), (0, 1, NONE, 0), (1, 1, NONE, 1)]
FIRST_NOSTAT = [(1, 0, NONE, 0), (0, 0, RELU, 0), (1, 1, RELU, 0), (0, 1, NONE, 0)]
ONE = [(1, 0, NONE, 0)]


def _fwd_table():
    t = []

    def add(name, want, shape, cin, cout, k, combos=BN4, pairs=(FF,), **kw):
        """want: the path the case is meant for (of its variants without a pre-norm, where the path declines one)"""
        for pair in pairs:
            for d in _variants(dict(name=name, want=want, shape=shape, cin=cin, cout=cout, k=k, pair=pair), combos, **kw):
                if d["norm"] and want in (COUT1, PROJ_R, PROJ, EXPAND):   # these paths decline a pre-norm: one-thread-per-voxel or generic
                    small = k == K111 and cin % 4 == 0 and cout in (1, 2, 3, 4, 8, 12, 16) and not d.get("xlay")
                    d["want"], d["inst"] = (SMALLCOUT if small else GENERIC), None
                t.append(Fwd(**d))

    # k_conv_fwd_c1rows<3> / <1>
    for cout in (4, 8, 16, 32, 64, 128):
        add(f"c1r_a{cout}", C1ROWS, (1, 3, 5, 11), 1, cout, K333, FIRST, (FF, HH) if cout in (4, 128) else (FF,))
    for cout in (4, 32, 128):
        add(f"c1r_b{cout}", C1ROWS, (2, 5, 9, 41), 1, cout, K333, FIRST, (FF, FH, FB, HH, BB, HF) if cout == 32 else (FF, HH))
    add("c1r_k133", C1ROWS, (2, 3, 9, 35), 1, 8, K133, FIRST, (FF, FB))
    add("c1r_k133w", C1ROWS, (2, 3, 9, 35), 1, 128, K133, FIRST, (FF, HH))
    add("c1r_d1", C1ROWS, (2, 1, 9, 35), 1, 32, K133, FIRST, (FF, HH))
    add("c1r_rnd", C1ROWS, (2, 5, 9, 41), 1, 32, K333, FIRST, (FF, FH, BB), recipe="random")
    # k_conv_fwd_cin1<KD, 3, 3, CIN>
    for cin, cout in ((1, 12), (1, 20), (2, 4), (2, 64), (3, 32), (3, 40), (4, 32)):
        rows = cout // 4 in (1, 8, 16)
        for k in (K333, K133):
            add(f"cin1_{cin}_{cout}_k{k[0]}", CIN1, (2, 5, 9, 11), cin, cout, k, FIRST if rows else FIRST_NOSTAT,
                (FF, HH, FB) if (cin, cout) in ((2, 64), (3, 32)) else (FF,))
    add("cin1_nostat", -1, (2, 5, 9, 11), 1, 12, K333, [(1, 0, NONE, 1)])             # no rows for Cout / 4 = 3: refused
    add("cin1_rnd", CIN1, (2, 5, 9, 11), 3, 32, K333, FIRST, (FF, HH), recipe="random")
    # the fast paths on wide buffers: x, y and ref are channels [8, 8 + C) of buffers 8 channels wider (16-byte aligned in every type)
    add("c1r_wide", C1ROWS, (2, 5, 9, 41), 1, 32, K333, FIRST, (FF, HH), xlay=(9, 8), ylay=(40, 8))
    add("cin1_wide", CIN1, (2, 5, 9, 11), 3, 32, K333, FIRST, (FF, HH), xlay=(11, 8), ylay=(40, 8))
    add("cout1_wide", COUT1, (2, 5, 9, 11), 32, 1, K333, [(1, 0, NONE, 0), (0, 0, NONE, 0)], (FF, HH), xlay=(40, 8), ylay=(9, 8))
    add("projr_wide", PROJ_R, (1, 1, 1, 37), 64, 16, K111, [(1, 0, NONE, 0), (0, 0, SIGMOID, 0)], (FF, HH), xlay=(72, 8), ylay=(24, 8),
        inst=[16, 2, 0, 0])
    add("proj_wide", PROJ, (1, 1, 1, 37), 96, 12, K111, [(1, 0, NONE, 0), (0, 0, SIGMOID, 0)], (FF, HH), xlay=(104, 8), ylay=(20, 8),
        inst=[12, 0, 0, 0])
    add("expand_wide", EXPAND, (1, 1, 1, 37), 12, 32, K111, [(1, 0, NONE, 0), (0, 0, NONE, 0)], (FF, HH), xlay=(20, 8), ylay=(40, 8),
        reflay=(40, 8), ref=True, amax=True)
    # just outside the first-layer kernels
    add("out_4_36", GENERIC, (2, 5, 9, 11), 4, 36, K333)
    add("out_cin5", GENERIC, (2, 5, 9, 11), 5, 8, K333)
    add("out_cout6", GENERIC, (2, 5, 9, 11), 1, 6, K133)
    add("out_yld", GENERIC, (2, 5, 9, 11), 1, 8, K333, ylay=(10, 0))
    add("out_yld_1x1", SMALLCOUT, (2, 1, 1, 37), 4, 8, K111, ylay=(10, 0))
    add("out_bias", GENERIC, (2, 5, 9, 11), 1, 8, K333, [(1, 0, NONE, 0), (1, 1, RELU, 0)], bias_off=1)
    # k_conv_fwd_cout1
    for cin in (16, 32, 48):
        for k in (K333, K133):
            add(f"cout1_{cin}_k{k[0]}", COUT1, (2, 5, 9, 11), cin, 1, k, BN4, (FF, HH, BF) if cin == 32 else (FF, HF))
    add("cout1_rnd", COUT1, (2, 5, 9, 11), 32, 1, K333, [(1, 0, NONE, 0), (0, 0, NONE, 0)], (FF, HH), recipe="random")
    add("cout1_cin8", GENERIC, (2, 5, 9, 11), 8, 1, K333, [(1, 0, NONE, 0)])
    add("cout1_slice", GENERIC, (2, 5, 9, 11), 16, 1, K333, [(1, 0, NONE, 0)], xlay=(20, 1))
    # k_conv1x1_proj_r<CO, NJ>
    PS = [(1, 0, NONE, 0), (0, 0, SIGMOID, 0), (1, 0, SIGMOID, 0), (1, 1, NONE, 0)]
    for nj in (1, 2, 4):
        for co in (1, 2, 3, 4, 6, 8, 12, 16):
            if nj == 4 and co > 8:
                continue
            add(f"projr_{co}_{nj}", PROJ_R, (1, 1, 1, 37), 32 * nj, co, K111, PS, (FF, HH) if co in (8, 16) else (FF,), inst=[co, nj, 0, 0])
    add("projr_2_1_trip2", PROJ_R, (1, 1, 1, 131072 + 37), 32, 2, K111, ONE, inst=[2, 1, 0, 0])
    add("projr_16_2_trip2", PROJ_R, (1, 1, 1, 131072 + 37), 64, 16, K111, ONE, (HF,), inst=[16, 2, 0, 0])   # (fp32 x: 42 MB; fp16 x: 25 MB)
    add("projr_rnd", PROJ_R, (1, 1, 37, 9), 64, 16, K111, [(1, 0, NONE, 0), (1, 0, SIGMOID, 0), (0, 0, SIGMOID, 0)], (FF, HH, FB), recipe="random")
    # k_conv1x1_proj<CO>
    for co in (1, 2, 3, 4, 6, 8, 12, 16):
        add(f"proj_96_{co}", PROJ, (1, 1, 1, 37), 96, co, K111, PS, inst=[co, 0, 0, 0])
    add("proj_128_12", PROJ, (1, 1, 1, 37), 128, 12, K111, PS, (FF, HH), inst=[12, 0, 0, 0])
    add("proj_128_16", PROJ, (1, 1, 1, 37), 128, 16, K111, PS, inst=[16, 0, 0, 0])
    add("proj_160_2", PROJ, (1, 1, 1, 37), 160, 2, K111, PS, inst=[2, 0, 0, 0])
    add("proj_rnd", PROJ, (1, 1, 37, 9), 96, 12, K111, [(1, 0, NONE, 0), (1, 0, SIGMOID, 0)], (FF, HH), recipe="random")
    # k_conv1x1_expand
    for cin in (1, 2, 3, 12, 16):
        for cout in (4, 32):
            add(f"expand_{cin}_{cout}", EXPAND, (1, 1, 1, 37), cin, cout, K111, BN4, (FF, HH) if cin in (2, 16) else (FF,))
            add(f"expand_{cin}_{cout}_ref", EXPAND, (1, 1, 1, 37), cin, cout, K111, [(1, 0, NONE, 0), (0, 0, NONE, 0)],
                (FF, BB) if cin == 2 else (FF,), ref=True, amax=True)
    add("expand_q_carry", EXPAND, (1, 1, 1, 140000), 2, 36, K111, ONE, amax=True)
    add("expand_rnd", EXPAND, (1, 1, 37, 9), 12, 32, K111, [(1, 0, NONE, 0), (0, 0, NONE, 0)], (FF, HH), ref=True, amax=True, recipe="random")
    # k_conv1x1_smallcout<CO>: Cout 4 .. 16 with Cin <= 16 go to the expansion unless a pre-norm is applied
    for cin in (4, 8, 36):
        for co in (1, 2, 3, 4, 8, 12, 16):
            want = EXPAND if cin <= 16 and co % 4 == 0 else SMALLCOUT
            add(f"small_{cin}_{co}", want, (1, 1, 1, 37), cin, co, K111, BN4, (FF, HH) if co == 12 else (FF,))
    add("small_32_2_norm", SMALLCOUT, (2, 1, 1, 37), 32, 2, K111, [(1, 1, NONE, 0), (0, 1, SIGMOID, 0)], (FF, HH))
    add("small_32_2_ref", SMALLCOUT, (2, 1, 1, 37), 32, 2, K111, [(1, 0, NONE, 0), (0, 0, NONE, 0)], (FF, HH), ref=True)
    add("small_rnd", SMALLCOUT, (2, 1, 37, 9), 36, 12, K111, [(1, 1, NONE, 0), (1, 0, RELU, 0)], (FF, HH), ref=True, recipe="random")
    # k_conv_fwd_generic<KD, KH, KW>
    for k in KSIZES:
        kk = "".join(map(str, k))
        add(f"generic_{kk}", GENERIC, (2, 3, 5, 7), 3, 5, k, BN4, (FF, HH) if k in (K333, K111) else (FF,))
        add(f"generic_{kk}_ref", GENERIC, (2, 3, 5, 7), 3, 5, k, [(1, 1, RELU, 0)], ref=True)
        add(f"generic_{kk}_one", GENERIC, (1, 1, 1, 1), 3, 5, k, [(1, 0, NONE, 0), (0, 1, NONE, 0)])
    add("generic_co_carry", GENERIC, (1, 1, 1, 209716), 3, 5, K111, ONE)            # NV Cout = 2^20 + 4: the grid-stride second trip
    add("generic_rnd", GENERIC, (2, 3, 5, 7), 3, 5, K333, [(1, 1, NONE, 0), (1, 0, SIGMOID, 0)], (FF, HH), ref=True, recipe="random")
    return t


FWD = _fwd_table()
FWD_BY_ID = {c.id: c for c in FWD}
assert len(FWD_BY_ID) == len(FWD), "case ids are unique"

# every instantiation and loop trip the table must reach with a lattice case: (path, inst) as the query reports them
FWD_REQUIRED = (
    [(C1ROWS, (0, 0, 0, kd)) for kd in (1, 3)] + [(CIN1, (0, 0, ci, kd)) for ci in (1, 2, 3, 4) for kd in (1, 3)]
    + [(COUT1, (0, 0, 0, kd)) for kd in (1, 3)]
    + [(PROJ_R, (co, nj, 0, 0)) for nj in (1, 2, 4) for co in (1, 2, 3, 4, 6, 8, 12, 16) if not (nj == 4 and co > 8)]
    + [(PROJ, (co, 0, 0, 0)) for co in (1, 2, 3, 4, 6, 8, 12, 16)] + [(EXPAND, (0, 0, 0, 0))]
    + [(SMALLCOUT, (co, 0, 0, 0)) for co in (1, 2, 3, 4, 8, 12, 16)]
    + [(GENERIC, (0, 0, 0, k[0] * 100 + k[1] * 10 + k[2])) for k in KSIZES])


# ---------------------------------------------------------------------------------------------------------- weight gradients
class Wg:
    """one weight-gradient launch.  pair (x type, g / y type); sd: sd_layout; gnorm: tem_conv3d_wgrad_gnorm_st (y and coef);
    xlay / glay / ylay (x, g, the gnorm y): None dense | (Wd, lo)"""

    def __init__(self, name, want, shape, cin, cout, k, pair=FF, sd=0, db=True, norm=False, gnorm=False, xlay=None, glay=None, ylay=None,
                 recipe="lattice"):
        self.name, self.want, self.shape, self.cin, self.cout, self.k, self.pair = name, want, tuple(shape), cin, cout, tuple(k), pair
        self.sd, self.db, self.norm, self.gnorm, self.xlay, self.glay, self.ylay, self.recipe = sd, db, norm, gnorm, xlay, glay, ylay, recipe

    @property
    def id(self):
        return (f"{self.name}-{self.pair[0]}.{self.pair[1]}-sd{self.sd}{'b' if self.db else ''}{'n' if self.norm else ''}"
                f"{'g' if self.gnorm else ''}{'' if self.recipe == 'lattice' else '-rnd'}")

    @property
    def nv(self):
        return int(np.prod(self.shape))

    def bytes_moved(self):
        g_ld = (self.glay or (self.cout,))[0] + ((self.ylay or (self.cout,))[0] if self.gnorm else 0)
        return self.nv * ((self.xlay or (self.cin,))[0] * ESIZE[self.pair[0]] + g_ld * ESIZE[self.pair[1]])


def proj_wgrad_takes(cin, cout):
    nj = cin // 32
    return cin % 32 == 0 and cin <= 128 and nj != 3 and nj * cout <= 32 and cout in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)


def expected_wgrad(c):
    cq = c.cout // 4
    x_ld = (c.xlay or (c.cin,))[0]
    xa = address(c.pair[0], (c.xlay or (0, 0))[1])
    rows16 = lambda lay: (lay or (c.cout,))[0] % 4 == 0 and address(c.pair[1], (lay or (0, 0))[1]) % 16 == 0      # noqa: E731
    if (1 <= c.cin <= 4 and c.cout % 4 == 0 and cq <= 16 and cq & (cq - 1) == 0 and c.k in (K333, K133) and rows16(c.glay)
            and not (c.gnorm and not rows16(c.ylay))):           # (the coefficients are aligned in every case of the table)
        return WG_CIN1
    if c.gnorm:
        return -1
    if c.k == K111 and proj_wgrad_takes(c.cin, c.cout) and not c.norm and x_ld % 4 == 0 and xa % 16 == 0:
        return WG_PROJ
    return WG_GENERIC


def _wg_table():
    t = []

    def add(name, want, shape, cin, cout, k, combos, pairs=(FF,), **kw):
        for pair in pairs:
            for sd, db, norm in combos:
                t.append(Wg(name, want, shape if not (norm and shape[0] == 1) else (2,) + tuple(shape[1:]), cin, cout, k, pair, sd, db, norm, **kw))

    W4 = [(0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1)]
    W2 = [(0, 1, 0), (1, 0, 1)]
    for cout in (4, 8, 16, 32, 64):
        for cin in (1, 2, 3, 4):
            for k in (K333, K133):
                full = cout in (4, 64) and cin in (1, 3)
                add(f"wc1_{cin}_{cout}_k{k[0]}", WG_CIN1, (2, 5, 9, 11), cin, cout, k, W4 if full else W2, (FF, HH, FB, HF) if full else (FF,))
                add(f"wc1_{cin}_{cout}_k{k[0]}", WG_CIN1, (2, 5, 9, 11), cin, cout, k, W2, (FF, HH, BB) if full else (FF, HH), gnorm=True)
    add("wc1_two_patches", WG_CIN1, (1, 4, 264, 256), 1, 4, K333, [(1, 1, 0)], (FF,))            # 1056 patches on 1024 workgroups
    add("wc1_two_patches", WG_CIN1, (1, 4, 264, 256), 1, 4, K333, [(1, 1, 0)], (FF,), gnorm=True)
    # x, g and y as channels [8, 8 + C) of buffers 8 channels wider (16-byte aligned in every storage type)
    add("wc1_wide", WG_CIN1, (2, 5, 9, 11), 3, 64, K333, W2, (FF, HH), xlay=(11, 8), glay=(72, 8))
    add("wc1_wide", WG_CIN1, (2, 5, 9, 11), 3, 64, K333, W2, (FF, HH), xlay=(11, 8), glay=(72, 8), ylay=(72, 8), gnorm=True)
    add("wc1_rnd", WG_CIN1, (2, 5, 9, 11), 3, 64, K333, [(1, 1, 0), (0, 1, 1)], (FF, HH), recipe="random")
    add("wc1_rnd", WG_CIN1, (2, 5, 9, 11), 1, 4, K133, [(1, 1, 1)], (FF, HH), gnorm=True, recipe="random")
    for nj in (1, 2, 4):
        for co in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32):
            if proj_wgrad_takes(32 * nj, co):
                add(f"pw_{co}_{nj}", WG_PROJ, (1, 1, 1, 37), 32 * nj, co, K111, [(0, 1, 0), (1, 0, 0)], (FF, HH) if co in (2, 32) else (FF,))
    add("pw_2_1_trip2", WG_PROJ, (1, 1, 1, 32768 + 37), 32, 2, K111, [(1, 1, 0)])
    add("pw_8_4_trip2", WG_PROJ, (1, 1, 1, 32768 + 37), 128, 8, K111, [(1, 1, 0)])
    add("pw_wide", WG_PROJ, (1, 1, 1, 37), 64, 12, K111, [(0, 1, 0), (1, 0, 0)], (FF, HH), xlay=(72, 8), glay=(20, 8))
    add("pw_rnd", WG_PROJ, (1, 1, 37, 9), 64, 12, K111, [(1, 1, 0)], (FF, HH), recipe="random")
    add("pw_out_96", WG_GENERIC, (1, 1, 1, 37), 96, 2, K111, [(1, 1, 0)])
    add("pw_out_norm", WG_GENERIC, (2, 1, 1, 37), 32, 2, K111, [(1, 1, 1)])
    add("pw_out_64_24", WG_GENERIC, (1, 1, 1, 37), 64, 24, K111, [(1, 1, 0)])
    for k in KSIZES:
        add("wgen_" + "".join(map(str, k)), WG_GENERIC, (2, 5, 9, 31), 3, 5, k, W4 if k in (K333, K111) else W2, (FF, HH) if k == K333 else (FF,))
    add("wgen_20_20", WG_GENERIC, (2, 1, 10, 10), 20, 20, K111, W2)                               # more than 256 pairs
    add("wgen_1_300", WG_GENERIC, (2, 1, 10, 10), 1, 300, K111, W2)                               # more than 256 columns
    add("wgen_rnd", WG_GENERIC, (2, 5, 9, 31), 3, 5, K333, [(1, 1, 1)], (FF, HH), recipe="random")
    return t


WG = _wg_table()
WG_BY_ID = {c.id: c for c in WG}
assert len(WG_BY_ID) == len(WG), "case ids are unique"

# tem_conv1x1_out_bwd_st: (Cin, Cout, pair, recipe): all 8 <CO, NJ>
OUT_BWD = [(32 * nj, co, pair, "lattice") for nj in (1, 2) for co in (1, 2, 3, 4) for pair in ((FF, HF, HH) if co in (2, 3) else (FF,))]
OUT_BWD += [(64, 2, FF, "random"), (32, 4, BB, "random")]
OUT_BWD_NV = 37 * 3


# ---------------------------------------------------------------------------------------------------------- inputs
def _ints(rng, shape, lo=-4, hi=4, zeros=0.4, negzero=0.0):
    a = rng.randint(lo, hi + 1, size=shape).astype(np.float32)
    a[rng.rand(*shape) < zeros] = 0.0
    if negzero:
        a[(a == 0) & (rng.rand(*shape) < negzero)] = -0.0
    return a


def _quarters(rng, shape):
    return (rng.randint(-8, 9, size=shape) / 4.0).astype(np.float32)


def _pow2(rng, shape, signed=True):
    a = np.array([0.5, 1.0, 2.0], np.float32)[rng.randint(0, 3, size=shape)]
    return a * np.where(rng.rand(*shape) < 0.5, -1, 1).astype(np.float32) if signed else a


def _seed(c):
    return UK.seed_of(c.name, c.shape + (c.cin, c.cout), c.k)


def fwd_inputs(c):
    """-> dict of float32 arrays: x [N, D, H, W, Cin], w [taps, Cin, Cout], bias, scale, shift [N, Cin], ref (None where absent)"""
    rng = np.random.RandomState(_seed(c))
    sh, nt = c.shape, R.ntaps(c.k)
    if c.recipe == "lattice":
        d = {"x": _ints(rng, sh + (c.cin,)), "w": _quarters(rng, (nt, c.cin, c.cout)), "bias": _quarters(rng, (c.cout,)),
             "scale": _pow2(rng, (sh[0], c.cin), signed=False), "shift": _quarters(rng, (sh[0], c.cin)),
             "ref": _ints(rng, sh + (c.cout,), negzero=0.3)}
    else:
        s = _seed(c)
        d = {"x": UK.make_tensor(sh + (c.cin,), s, "16"), "w": (rng.randn(nt, c.cin, c.cout) / np.sqrt(nt * c.cin)).astype(np.float32),
             "bias": rng.randn(c.cout).astype(np.float32), "scale": rng.uniform(0.5, 2.0, (sh[0], c.cin)).astype(np.float32),
             "shift": (0.5 * rng.randn(sh[0], c.cin)).astype(np.float32), "ref": UK.make_tensor(sh + (c.cout,), s + 1, "16")}
    for key, on in (("bias", c.bias), ("scale", c.norm), ("shift", c.norm), ("ref", c.ref)):
        if not on:
            d[key] = None
    return d


def fwd_step(c):
    """the lattice step of a forward case: x (or x scale + shift: quarters) times w (quarters)"""
    return (0.25 if c.norm else 1.0) * 0.25


def fwd_reference(c, d=None):
    """-> dict: y, mag (float64), e32 (random cases and sigmoid outputs; 0 for the exact ones)"""
    d = d or fwd_inputs(c)
    y, mag = R.fwd_f64(d["x"], d["w"], c.k, d["bias"], d["scale"], d["shift"], c.act, d["ref"])
    e32 = 0.0
    if c.recipe != "lattice" or c.act == SIGMOID:
        e32 = R.fwd_e32(d["x"], d["w"], c.k, y, mag, d["bias"], d["scale"], d["shift"], c.act, d["ref"])
    return {"y": y, "mag": mag, "e32": e32}


def fwd_lattice_bound(c, d=None):
    d = d or fwd_inputs(c)
    _, mag = R.fwd_f64(d["x"], d["w"], c.k, d["bias"], d["scale"], d["shift"], NONE, None)
    return R.lattice_bound(mag, fwd_step(c))


def wg_inputs(c):
    rng = np.random.RandomState(_seed(c) + 7)
    sh = c.shape
    if c.recipe == "lattice":
        d = {"x": _ints(rng, sh + (c.cin,)), "g": _ints(rng, sh + (c.cout,)), "scale": _pow2(rng, (sh[0], c.cin), signed=False),
             "shift": _quarters(rng, (sh[0], c.cin)), "y": _ints(rng, sh + (c.cout,), negzero=0.3), "coef": _pow2(rng, (sh[0], c.cout, 4))}
    else:
        s = _seed(c)
        d = {"x": UK.make_tensor(sh + (c.cin,), s, "16"), "g": UK.make_tensor(sh + (c.cout,), s + 1, "16"),
             "scale": rng.uniform(0.5, 2.0, (sh[0], c.cin)).astype(np.float32), "shift": (0.5 * rng.randn(sh[0], c.cin)).astype(np.float32),
             "y": UK.make_tensor(sh + (c.cout,), s + 2, "16"), "coef": UK.make_coef(sh[0], c.cout, s + 3)}
    for key, on in (("scale", c.norm), ("shift", c.norm), ("y", c.gnorm), ("coef", c.gnorm)):
        if not on:
            d[key] = None
    return d


def wg_step(c):
    """x (or quarters) times g (or a g - m1 - (y - mean) m2r: quarters)"""
    return (0.25 if c.norm else 1.0) * (0.25 if c.gnorm else 1.0)


def wg_reference(c, d=None):
    """-> dict: dw [taps, Cin, Cout], db, mag, dbmag (float64), e32 (dw, db)"""
    d = d or wg_inputs(c)
    if c.gnorm:
        dw, db, mag, dbmag = R.wgrad_gnorm_f64(d["x"], d["g"], d["y"], d["coef"], c.k, d["scale"], d["shift"])
    else:
        dw, db, mag, dbmag = R.wgrad_f64(d["x"], d["g"], c.k, d["scale"], d["shift"])
    e32 = (0.0, 0.0)
    if c.recipe != "lattice":
        es = []
        for fused in (False, True):
            g = R.gnorm_f32(d["g"], d["y"], d["coef"], fused) if c.gnorm else d["g"]
            a, b = R.wgrad_f32(d["x"], g, c.k, d["scale"], d["shift"], fused)
            es.append((R.units(a, dw, mag), R.units(b, db, dbmag)))
        e32 = (max(e[0] for e in es), max(e[1] for e in es))
    return {"dw": dw, "db": db, "mag": mag, "dbmag": dbmag, "e32": e32}


def out_bwd_inputs(cin, cout, recipe):
    """x holds 0, -0.0 and negative values (the ReLU mask), w [Cout][Cin]"""
    rng = np.random.RandomState(1000 + 37 * cin + cout)
    sh = (1, 1, 1, OUT_BWD_NV)
    if recipe == "lattice":
        return {"x": _ints(rng, sh + (cin,), negzero=0.3), "g": _ints(rng, sh + (cout,)), "w": _quarters(rng, (cout, cin))}
    x = UK.make_tensor(sh + (cin,), 77 + cin, "16")
    x[rng.rand(*x.shape) < 0.2] = 0.0
    return {"x": x, "g": UK.make_tensor(sh + (cout,), 78 + cout, "16"), "w": (rng.randn(cout, cin) / np.sqrt(cout)).astype(np.float32)}
