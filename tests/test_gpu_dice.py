"""GPU: every kernel of csrc/dice.hip on every dispatch path, op by op through the C ABI, against the float64 references of
oracle/dice_ref.py (which tests/test_dice_cpu.py pins to torch float64 autograd and to the reference-made fixtures, and
whose judge it tests on deliberately wrong outputs).

Rule (oracle/judge.py).  Errors are counted in units of 2^-23 times a per-quantity scale: a sum column
against the column's own float64 value (every term is non-negative), a gradient element against
|gout| (w_dice (|ca t| + |cb p|) s + |w_bce| b) [m] (oracle/dice_ref.py: grad_scale), after an absolute allowance of 2^-126
(sigmoid(-90) is a float32 subnormal).  On the same inputs the test evaluates the numpy float32 restatement (one rounding
per operation -- a reference, not the code under test) and takes its worst figure e32; the kernel must stay within
MARGIN * max(e32, 1), the MARGIN of 4 of oracle/judge.py.  EVERY sum column and EVERY gradient element is judged.  The restatement stays at <= 1.9
units for the sums and <= 2.8 for the gradients on the small shapes (asserted on the CPU; 2.9 over the 5e5 elements of the
grid-cap cases, and up to 7.2 for its pairwise float32 sums of the 5 million terms of the clamped case), so the bound has
room for the reference.  No allowance for the kernels' fp32 chains was needed: a thread sums at most 11 terms before the wave reduction
(8 by construction, 11 in the clamped cases), the partial rows are added in double.
The coefficients of the gradient cases are the float32-rounded oracle ones: a one-step error without drift.

Observed on the MI355X (profiles/dice_op_errors.txt): worst kernel error / max(e32, 1) = 2.39 (OBSERVED_WORST_RATIO below:
sum t^2 of k_dice_partial<true>; gradients at most 1.23, k_dice_finalize 0.82 units of 2^-23 |value|).

What a sum check cannot see: one voxel among the 5 million terms of the clamped case N = 512 is 2e-7 of a column, below
4 units; every other case has at most 4e5 terms per column and the anchors of oracle/dice_cases.py (terms of order 1 at the
last voxel and at the start of the last 256-voxel tile of every row), so a dropped tail is 10 units or more there.

Every case prints the kernel it is meant to reach (with -s): `expect_sums_path` / `expect_grad_path` restate the dispatch
conditions of dice_sums_impl / dice_grad_impl from the strides and pointers the test passes, and the case tables name the
intended kernel, so a layout that silently takes another path fails.  At V = 1 a NCDHW tensor has channel stride 1 and IS
channels-last; those rows print the path the strides select.
The C ABI sees (N, C, V) and strides only; the ranks (N, C) ... (N, C, D, H, W) appear in the end-to-end class tests.
k_dice_finalize takes the first channel on ties of max / min (torch.max documents no order); the scores here are distinct.

No test provokes a device fault: every tensor's extent is asserted against its buffer before a launch, the unused channels
of wide buffers hold NaN (a neighbour's value cannot go unnoticed), outputs sit between sentinels that must survive.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import dice_ref as R
from oracle import gpu_kit as kit
from oracle import loss_ref
from oracle.dice_cases import FLAG_SETS, coefficients, flag_name, gout_variant, make_inputs
from oracle.gpu_kit import lib as _lib, ops as _ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = R.MARGIN
OBSERVED_WORST_RATIO = 2.39      # informational (profiles/dice_op_errors.txt); the assertions use MARGIN
SENT = 12345.0                   # the sentinel around every output
f32 = np.float32


LEDGER = kit.Ledger("DICE_ERR")
_note = LEDGER.note
_print_worst = LEDGER.summary_fixture()
# select the one-voxel-per-thread kernels (1, the default) or the (channel, voxel) kernels (0) for one test
dice_vox_option = kit.option_fixture("dice_vox")


# ------------------------------------------------------------------------------------------ tensors the test lays out itself
class Laid:
    """A logical float32 [N, C, V] array inside a device buffer the test owns.  kind "ncv": channel-first, W >= C planes per
    sample; "cl": channels-last with pitch W >= C.  `off` floats precede the tensor (pointer alignment); everything that is
    not an element of the tensor holds `fill`."""

    def __init__(self, arr, kind="ncv", W=None, off=0, fill=float("nan")):
        N, C, V = arr.shape
        W = W or C
        assert W >= C and kind in ("ncv", "cl")
        self.kind, self.W, self.shape, self.fill = kind, W, (N, C, V), fill
        self.s = (W * V, V, 1) if kind == "ncv" else (V * W, 1, W)
        self.off = off
        self.buf = torch.full((off + N * W * V + 8,), fill, dtype=torch.float32, device=DEV)
        self._check()
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))

    def _check(self):
        N, C, V = self.shape
        last = self.off + (N - 1) * self.s[0] + (C - 1) * self.s[1] + (V - 1) * self.s[2]
        assert 0 <= self.off and last < self.buf.numel(), "the tensor leaves its buffer"

    @property
    def view(self):
        return torch.as_strided(self.buf, self.shape, self.s, self.off)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def channels(self, lo, C):
        """channels [lo, lo + C) of this tensor, in place"""
        assert 0 <= lo and lo + C <= self.shape[1]
        sub = object.__new__(Laid)
        sub.kind, sub.W, sub.fill, sub.buf, sub.s = self.kind, self.W, self.fill, self.buf, self.s
        sub.shape, sub.off = (self.shape[0], C, self.shape[2]), self.off + lo * self.s[1]
        sub._check()
        return sub

    def host(self):
        return self.view.cpu().numpy().copy()

    def untouched_outside(self):
        """consumes the tensor: True if every float of the buffer that is not an element still holds `fill`"""
        self.view.fill_(self.fill)
        return bool((self.buf == self.fill).all())


def _wide(arr, W, lo):
    """arr as channels [lo, lo + C) of a W-channel array whose other channels are NaN"""
    N, C, V = arr.shape
    out = np.full((N, W, V), np.nan, f32)
    out[:, lo:lo + C] = arr
    return out


def lay_prediction(p, spec):
    """spec: "ncv" | "cl" | ("cl", W, lo)"""
    if isinstance(spec, str):
        return Laid(p, spec)
    kind, W, lo = spec
    return Laid(_wide(p, W, lo), kind).channels(lo, p.shape[1])


def lay_target(t, m, spec):
    """spec "ncv" | "cl": target and mask in two buffers of the same layout; "pair": the target is the first half of a 2C-channel
    tensor and the mask the other half (what ApplyAndRemoveMask splits).  -> (T, M); M is None without a mask"""
    C = t.shape[1]
    if spec == "pair":
        both = Laid(np.concatenate([t, m if m is not None else np.full_like(t, np.nan)], 1), "ncv")
        return both.channels(0, C), (both.channels(C, C) if m is not None else None)
    return Laid(t, spec), (Laid(m, spec) if m is not None else None)


def expect_sums_path(vox, C, P):
    sn, sc, sv = P.s
    cfast = sc == 1
    if C <= 16 and vox:
        if cfast and C % 4 == 0 and sn % 4 == 0 and sv % 4 == 0 and P.ptr % 16 == 0:
            return "partial_vox<4>"
        if cfast and C == 2 and sn % 2 == 0 and sv == 2 and P.ptr % 8 == 0:
            return "partial_vox<2>"
        return "partial_vox<1>"
    return "partial<true>" if cfast else "partial<false>"


def expect_grad_path(vox, C, P, G):
    (psn, psc, psv), (gsn, gsc, gsv) = P.s, G.s
    if C <= 16 and vox:
        cl = psc == 1 and gsc == 1
        if cl and C % 4 == 0 and psn % 4 == 0 and psv % 4 == 0 and gsn % 4 == 0 and gsv % 4 == 0 and \
                P.ptr % 16 == 0 and G.ptr % 16 == 0:
            return "grad_vox<4>"
        if cl and C == 2 and psv == 2 and gsv == 2 and psn % 2 == 0 and gsn % 2 == 0 and P.ptr % 8 == 0 and G.ptr % 8 == 0:
            return "grad_vox<2>"
        return "grad_vox<1>"
    return "grad<true>" if psc == 1 else "grad<false>"


def _vp(x):
    return None if x is None else ctypes.c_void_p(x if isinstance(x, int) else x.ptr)


def launch_sums(P, T, M, flags):
    """-> double [C, 3 | 4] from tem_dice_sums (flags 0) or tem_dice_sums2; the rows around the output and the floats behind
    the workspace must survive"""
    lib, ops = _lib().load(), _ops()
    N, C, V = P.shape
    ncol = 4 if flags & R.BCE else 3
    nws = lib.tem_dice_ws(N, V, C)
    ws = torch.full((nws // 4 + 64,), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((C + 2, ncol), SENT, dtype=torch.float64, device=DEV)
    stream = ops._stream(ws)
    if flags == 0:
        rc = lib.tem_dice_sums(_vp(P), *P.s, _vp(T), *T.s, _vp(M), N, C, V, out[1].data_ptr(), ws.data_ptr(), nws, stream)
    else:
        assert M is None
        rc = lib.tem_dice_sums2(_vp(P), *P.s, _vp(T), *T.s, N, C, V, out[1].data_ptr(), ws.data_ptr(), nws, flags, stream)
    _lib().check(rc, "tem_dice_sums")
    assert bool((ws[nws // 4:] == SENT).all()), "wrote behind the workspace"
    assert bool((out[0] == SENT).all()) and bool((out[-1] == SENT).all()), "wrote around the sums"
    return out[1:-1].cpu().numpy()


def launch_grad(P, T, M, ca, cb, gout, per_channel, G, flags, wd, wb):
    """tem_dice_grad (flags 0) or tem_dice_grad2 into G (pre-filled with NaN by the caller)"""
    lib, ops = _lib().load(), _ops()
    N, C, V = P.shape
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, f32)).to(DEV) for a in (ca, cb, gout)]
    p_ = [None if d is None else d.data_ptr() for d in dev]
    stream = ops._stream(G.buf)
    if flags == 0:
        rc = lib.tem_dice_grad(_vp(P), *P.s, _vp(T), *T.s, _vp(M), p_[0], p_[1], p_[2], int(per_channel), _vp(G), *G.s,
                               N, C, V, stream)
    else:
        assert M is None
        rc = lib.tem_dice_grad2(_vp(P), *P.s, _vp(T), *T.s, p_[0], p_[1], p_[2], int(per_channel), _vp(G), *G.s, N, C, V,
                                flags, float(wd), float(wb), stream)
    _lib().check(rc, "tem_dice_grad")
    torch.cuda.synchronize()
    return G.host()


# ------------------------------------------------------------------------------------------ the path tables
V_ALL = (1, 63, 255, 256, 257, 2047, 2049, 5 * 2048 + 257)
V_TWO = (257, 2049)
V_WIDE = (63, 257)
# (name, intended kernel family with dice_vox = 1, prediction layout, C, voxel counts)
PATHS = [
    ("cl4", "vox<4>", "cl", 4, V_ALL),
    ("cl12", "vox<4>", "cl", 12, V_TWO),
    ("cl16", "vox<4>", "cl", 16, V_TWO),
    ("cl8[4:8]", "vox<4>", ("cl", 8, 4), 4, V_TWO),
    ("cl2", "vox<2>", "cl", 2, V_ALL),
    ("ncv1", "vox<1>", "ncv", 1, V_TWO),
    ("ncv2", "vox<1>", "ncv", 2, V_TWO),
    ("ncv3", "vox<1>", "ncv", 3, V_ALL),
    ("ncv12", "vox<1>", "ncv", 12, V_TWO),
    ("cl1", "vox<1>", "cl", 1, V_TWO),
    ("cl3", "vox<1>", "cl", 3, V_TWO),
    ("cl6", "vox<1>", "cl", 6, V_TWO),
    ("cl8[2:6]", "vox<1>", ("cl", 8, 2), 4, V_TWO),      # pointer % 16 == 8: must not take the vector path
    ("cl4[0:2]", "vox<1>", ("cl", 4, 0), 2, V_TWO),      # p_sv = 4: not the float2 path
    ("cl17", "<true>", "cl", 17, V_ALL),
    ("cl20", "<true>", "cl", 20, V_TWO),
    ("cl100", "<true>", "cl", 100, V_TWO),
    ("cl256", "<true>", "cl", 256, V_WIDE),
    ("cl300", "<true>", "cl", 300, V_WIDE),
    ("ncv17", "<false>", "ncv", 17, V_ALL),
    ("ncv100", "<false>", "ncv", 100, V_TWO),
]
TARGETS = ("ncv", "cl", "pair")
CASES = [(name, fam, spec, C, V, TARGETS[(i + j) % 3]) for i, (name, fam, spec, C, vs) in enumerate(PATHS)
         for j, V in enumerate(vs)]
IDS = [f"{c[0]}-V{c[4]}-t_{c[5]}" for c in CASES]
VARIANTS = [(0, False), (0, True), (R.LOGITS, False), (R.BCE, False), (R.LOGITS | R.BCE, False)]   # (flags, masked)


def _intended(kernel, fam, vox, C, spec):
    if C <= 16 and vox:
        return f"{kernel}_{fam}" if fam.startswith("vox") else None
    cl = spec == "cl" or isinstance(spec, tuple)
    return f"{kernel}{'<true>' if cl else '<false>'}"


def _check_path(kernel, got_path, fam, vox, C, spec, V):
    want = _intended(kernel, fam, vox, C, spec)
    assert V == 1 or want is None or got_path == want, f"meant for k_dice_{want}, the strides select k_dice_{got_path}"


def _seed(name, V, flags):
    return (sum(map(ord, name)) * 131 + V * 7 + flags) % (2 ** 31)


_INPUTS = {}


def _case_data(name, N, C, V, flags, masked):
    """inputs, float64 reference and the restatement's error of one (case, variant): computed once, shared, left unchanged"""
    key = (name, N, C, V, flags, masked)
    if key not in _INPUTS:
        if len(_INPUTS) > 8:
            _INPUTS.clear()
        p, t, m = make_inputs(N, C, V, _seed(name, V, flags), bool(flags & R.LOGITS), soft=bool((V + C + flags) & 1),
                              masked=masked)
        ref = R.dice_sums_f64(p, t, m, flags)
        e32 = R.sums_units(R.dice_sums_f32(p, t, m, flags), ref)
        _INPUTS[key] = (p, t, m, ref, e32)
    return _INPUTS[key]


def _judge_sums(tag, path, got, ref, e32):
    ek = R.sums_units(got, ref)
    names = ("pt", "pp", "tt", "bce")
    print(f"DICE_ERR {tag} -> k_dice_{path} " + " ".join(f"{names[k]}: kernel {ek[k]:.2f} f32 {e32[k]:.2f}"
                                                          for k in range(len(ek))))
    for k in range(len(ek)):
        _note(path, "sum " + names[k], ek[k], e32[k])
    for k in range(len(ek)):
        assert R.within(ek[k], e32[k]), \
            f"{tag}: column {names[k]} is {ek[k]:.2f} units from float64, plain fp32 arithmetic {e32[k]:.2f}"


# ------------------------------------------------------------------------------------------ sums
def _run_sums_case(set_vox, name, fam, spec, C, N, V, tspec, variants=VARIANTS):
    for flags, masked in variants:
        p, t, m, ref, e32 = _case_data(name, N, C, V, flags, masked)
        P = lay_prediction(p, spec)
        T, M = lay_target(t, m, tspec)
        for vox in (1, 0):
            set_vox(vox)
            path = expect_sums_path(vox, C, P)
            _check_path("partial", path, fam, vox, C, spec, V)
            got = launch_sums(P, T, M, flags)
            _judge_sums(f"sums {name} N={N} V={V} t={tspec} {flag_name(flags, masked)} dice_vox={vox}", path, got, ref, e32)
            again = launch_sums(P, T, M, flags)
            assert np.array_equal(got.view(np.int64), again.view(np.int64)), "a repeated launch is bit-identical"
        assert np.array_equal(P.host(), p) and np.array_equal(T.host(), t), "prediction and target are inputs"


@pytest.mark.parametrize("name,fam,spec,C,V,tspec", CASES, ids=IDS)
def test_sums_against_float64(name, fam, spec, C, V, tspec, dice_vox_option):
    _run_sums_case(dice_vox_option, name, fam, spec, C, 3 if V < 300 else 2, V, tspec)


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_sums_clamped_grid_n512(flags, dice_vox_option):
    """N = 512: DICE_MAX_BLOCKS / N = 4 workgroups per sample where V = 5 * 2048 + 3 asks for 6 (11 with dice_vox = 0);
    k_dice_reduce adds 2048 partial rows.  One case per member of the family."""
    N, C, V = 512, 2, 5 * 2048 + 3
    assert -(-V // 2048) > 2048 // N and -(-V // (128 * 8)) > 2048 // N
    _run_sums_case(dice_vox_option, "clamp512", "vox<2>", "cl", C, N, V, "ncv", variants=[(flags, False)])


def test_sums_clamped_grid_n64_c20(dice_vox_option):
    """C = 20: 12 voxel rows per workgroup, V = 3845 asks for 41 workgroups per sample, 32 are allowed"""
    N, C, V = 64, 20, 3845
    assert -(-V // ((256 // C) * 8)) > 2048 // N
    _run_sums_case(dice_vox_option, "clamp64", "<true>", "cl", C, N, V, "pair",
                   variants=[(0, True), (R.LOGITS | R.BCE, False)])


# ------------------------------------------------------------------------------------------ finalize
def _finalize_sums(C, ncol, dead, seed):
    """hand-made sums with well separated scores; dead: "none" | "one" | "all" channels with den < eps = 1e-7 (the flat
    mode's pooled den too, for "all")"""
    rng = np.random.RandomState(seed)
    order = rng.permutation(C)
    s = np.zeros((C, ncol))
    s[:, 0] = 10.0 * (order + 1) / (C + 1)
    s[:, 1] = 10.0 + rng.uniform(0, 0.01, C)
    s[:, 2] = 10.0 + rng.uniform(0, 0.01, C)
    if ncol == 4:
        s[:, 3] = rng.uniform(1, 1000, C)
    rows = {"none": [], "one": [C // 2], "all": list(range(C))}[dead]
    for c in rows:
        s[c, :3] = np.array([1e-9 * (order[c] + 1) / (C + 1), 2e-8, 3e-8]) / C
    return s


@pytest.mark.parametrize("C", [1, 3, 12, 300])
def test_finalize_against_float64(C):
    lib, ops = _lib().load(), _ops()
    worst = 0.0
    for ncol in (3, 4):
        for dead in ("none", "one", "all"):
            sums = _finalize_sums(C, ncol, dead, 7 * C + ncol)
            sd = torch.from_numpy(sums).to(DEV)
            for channelwise, reduce in [(1, r) for r in ("none", "sum", "mean", "max", "min")] + [(0, "sum")]:
                for invert in (0, 1):
                    ref = R.dice_finalize_f64(sums, 1e-7, bool(channelwise), bool(invert), reduce)
                    if dead != "none" and channelwise:
                        assert (ref[2] == 0).sum() >= (1 if dead == "one" else C)
                    bufs = [torch.full((C + 2,), SENT, dtype=torch.float32, device=DEV) for _ in range(3)]
                    ptrs = [b[1:].data_ptr() for b in bufs]
                    stream = ops._stream(sd)
                    if ncol == 3:
                        rc = lib.tem_dice_finalize(sd.data_ptr(), C, 1e-7, channelwise, invert, R.REDUCE[reduce], *ptrs, stream)
                    else:
                        rc = lib.tem_dice_finalize2(sd.data_ptr(), ncol, C, 1e-7, channelwise, invert, R.REDUCE[reduce], *ptrs,
                                                    stream)
                    _lib().check(rc, "tem_dice_finalize")
                    got = [b.cpu().numpy() for b in bufs]
                    n_out = ref[0].size
                    what = (C, ncol, dead, channelwise, reduce, invert)
                    for k, (g, r, n) in enumerate(zip(got, ref, (n_out, C, C))):
                        assert g[0] == SENT and (g[1 + n:] == SENT).all(), ("wrote around its output", what, k)
                        u = R.finalize_units(g[1:1 + n], r)
                        worst = max(worst, u)
                        assert u <= 1.0, f"{what} {'out ca cb'.split()[k]}: {u:.3f} units of 2^-23 |value|"
                    assert np.array_equal(sd.cpu().numpy(), sums)
    print(f"DICE_ERR finalize C={C}: worst {worst:.3f} units of 2^-23 |value| (out, ca, cb; every mode)")
    _note("finalize", "out/ca/cb", worst, 0.0)


# ------------------------------------------------------------------------------------------ gradient
def _lay_gradient(shape, gspec):
    """gspec: "ncv" | "cl" | ("cl", W) pitched | ("cl+2",) dense channels-last two floats past the alignment"""
    nan = np.full(shape, np.nan, f32)
    if gspec == ("cl+2",):
        return Laid(nan, "cl", off=2, fill=SENT)
    if isinstance(gspec, tuple):
        return Laid(nan, gspec[0], W=gspec[1], fill=SENT)
    return Laid(nan, gspec, fill=SENT)


def _run_grad_case(set_vox, name, fam, spec, C, N, V, tspec, gspec, variants, want=None, gkind0=0):
    for k, (flags, masked) in enumerate(variants):
        p, t, m, _, _ = _case_data(name, N, C, V, flags, masked)
        ca, cb = coefficients(p, t, m, flags)
        wd, wb = (f32(0.75), f32(2.0 / p.size)) if flags & R.BCE else (f32(1.0), f32(0.0))
        gout, per = gout_variant((gkind0 + k) % 3, C, V)
        args = (p, t, m, ca, cb, gout, per, flags, wd, wb)
        ref = R.dice_grad_f64(*args)
        scale = R.grad_scale(p, t, m, ca, cb, gout, flags, wd, wb)
        r32 = R.dice_grad_f32(*args)
        e32 = R.grad_units(r32, ref, scale)
        P = lay_prediction(p, spec)
        T, M = lay_target(t, m, tspec)
        for vox in (1, 0):
            set_vox(vox)
            G = _lay_gradient(p.shape, gspec)
            path = expect_grad_path(vox, C, P, G)
            if want is not None:
                assert path == want[vox], f"meant for k_dice_{want[vox]}, the strides select k_dice_{path}"
            elif gspec == spec or (isinstance(spec, tuple) and gspec == "cl"):
                _check_path("grad", path, fam, vox, C, spec, V)
            got = launch_grad(P, T, M, ca, cb, gout, per, G, flags, wd, wb)
            tag = (f"grad {name} N={N} V={V} t={tspec} g={gspec} {flag_name(flags, masked)} "
                   f"gout={'null scalar per-channel'.split()[(gkind0 + k) % 3]} dice_vox={vox}")
            assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} elements were never written"
            assert G.untouched_outside(), f"{tag}: wrote outside the gradient's elements"
            ek = R.grad_units(got, ref, scale)
            print(f"DICE_ERR {tag} -> k_dice_{path} g: kernel {ek:.2f} f32 {e32:.2f}")
            _note(path, "grad " + flag_name(flags, masked), ek, e32)
            assert R.within(ek, e32), f"{tag}: {ek:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"
            if masked:
                assert not got[m == 0].any(), "exactly zero outside the mask"
            if C >= 2:                                          # the channel with ca = cb = 0
                if not flags & R.BCE:
                    assert not got[:, -1].any(), "ca = cb = 0: exactly zero"
                elif not flags & R.LOGITS:                      # every operation of the cross-entropy part is correctly
                    assert np.array_equal(got[:, -1], r32[:, -1]), "ca = cb = 0: exactly the cross-entropy part"   # rounded
        assert np.array_equal(P.host(), p) and np.array_equal(T.host(), t), "prediction and target are inputs"


GRAD_V = {V_ALL: (1, 63, 257, 2049), V_TWO: (257,), V_WIDE: (63,)}
GRAD_CASES = [(name, fam, spec, C, V, TARGETS[(i + j + 1) % 3]) for i, (name, fam, spec, C, vs) in enumerate(PATHS)
              for j, V in enumerate(GRAD_V[vs])]
GRAD_IDS = [f"{c[0]}-V{c[4]}-t_{c[5]}" for c in GRAD_CASES]


@pytest.mark.parametrize("name,fam,spec,C,V,tspec", GRAD_CASES, ids=GRAD_IDS)
def test_grad_against_float64(name, fam, spec, C, V, tspec, dice_vox_option):
    """the gradient in the prediction's own layout, dense (g_sv = C for channels-last, also for a sliced prediction)"""
    gspec = "ncv" if spec == "ncv" else "cl"
    _run_grad_case(dice_vox_option, name, fam, spec, C, 3 if V < 300 else 2, V, tspec, gspec, VARIANTS,
                   gkind0=GRAD_IDS.index(f"{name}-V{V}-t_{tspec}"))


@pytest.mark.parametrize("name,spec,C,gspec,want", [
    ("pitch16", "cl", 12, ("cl", 16), {1: "grad_vox<4>", 0: "grad<true>"}),          # g_sv = 16 for C = 12: still float4
    ("goff2", "cl", 4, ("cl+2",), {1: "grad_vox<1>", 0: "grad<true>"}),              # gradient pointer % 16 == 8
    ("pitch4c2", "cl", 2, ("cl", 4), {1: "grad_vox<1>", 0: "grad<true>"}),            # g_sv = 4 for C = 2: not float2
    ("ncvgrad", "cl", 4, "ncv", {1: "grad_vox<1>", 0: "grad<true>"}),                # NCDHW gradient of a channels-last p
    ("ncvgrad20", "cl", 20, "ncv", {1: "grad<true>", 0: "grad<true>"}),
    ("clgrad3", "ncv", 3, "cl", {1: "grad_vox<1>", 0: "grad<false>"}),               # and the other way round
])
def test_grad_pitches_and_fallbacks(name, spec, C, gspec, want, dice_vox_option):
    for V, tspec in ((257, "pair"), (2049, "cl")):
        _run_grad_case(dice_vox_option, name, None, spec, C, 2, V, tspec, gspec, VARIANTS, want=want, gkind0=V)


@pytest.mark.parametrize("name,spec,C,V,want", [
    ("cap2048", "cl", 20, 26215, {1: "grad<true>", 0: "grad<true>"}),                # 524300 items > 2048 * 256
    ("cap2048n", "ncv", 20, 26215, {1: "grad<false>", 0: "grad<false>"}),
    ("cap4096", "cl", 2, 4096 * 256 + 257, {1: "grad_vox<2>", 0: "grad<true>"}),     # the vox grid wraps (and 2048 * 256 * 4)
])
def test_grad_grid_caps(name, spec, C, V, want, dice_vox_option):
    assert C * V > 2048 * 256 and (C > 16 or V > 4096 * 256)
    _run_grad_case(dice_vox_option, name, None, spec, C, 1, V, "ncv", spec, [(0, True), (R.LOGITS | R.BCE, False)],
                   want=want, gkind0=1)


# ------------------------------------------------------------------------------------------ the classes, end to end
SHAPES = {2: (2, 2, 5, 6, 7), 4: (2, 4, 9, 11), 12: (2, 12, 77), 20: (1, 20, 3, 5, 7)}


def _as_layout(x, layout):
    """x (CPU, [N, C, *spatial]) on the device as NCDHW, channels-last, or channels [4, 4 + C) of a channels-last buffer of C + 8 channels (16-byte
    aligned: the float4 kernels for C = 4 and 12)"""
    nd = x.dim()
    to_phys, from_phys = (0, *range(2, nd), 1), (0, nd - 1, *range(1, nd - 1))
    if layout == "ncdhw":
        return x.to(DEV).contiguous()
    phys = x.permute(*to_phys).contiguous().to(DEV)
    if layout == "cl":
        return phys.permute(*from_phys)
    C = x.shape[1]
    wide = torch.full(phys.shape[:-1] + (C + 8,), float("nan"), device=DEV)
    wide[..., 4:4 + C] = phys
    return wide[..., 4:4 + C].permute(*from_phys)


def _family_reference(kind, x64, t64, alpha, beta):
    import torch.nn.functional as F
    if kind == "dice":
        return loss_ref.dice_loss(x64, t64)
    if kind == "dice_logits":
        return loss_ref.dice_loss(torch.sigmoid(x64), t64)
    if kind == "bce_dice":
        return alpha * loss_ref.dice_loss(x64, t64) + beta * F.binary_cross_entropy(x64, t64)
    if kind == "bce_dice_logits":
        return alpha * loss_ref.dice_loss(torch.sigmoid(x64), t64) + beta * F.binary_cross_entropy_with_logits(x64, t64)
    return loss_ref.masked_dice_loss(x64, t64)


@pytest.mark.parametrize("layout", ["ncdhw", "cl", "cl_slice"])
@pytest.mark.parametrize("C", [2, 4, 12, 20])
def test_loss_classes_against_float64_autograd(C, layout, dice_vox_option):
    """value within 3e-6 max(1, |ref|), gradient within 2e-5 of its maximum (the tolerances tests/test_gpu_ops.py holds these
    classes to); exactly zero outside the mask; the gradient comes back in the prediction's memory format.  C = 4 has an
    integer-typed target."""
    from torch_em_amd.loss import (ApplyAndRemoveMask, BCEDiceLoss, BCEDiceLossWithLogits, DiceLoss, DiceLossWithLogits,
                                   LossWrapper)
    shape = SHAPES[C]
    g = torch.Generator().manual_seed(100 + C)
    probs = torch.rand(shape, generator=g) * 0.96 + 0.02
    logits = torch.randn(shape, generator=g) * 2
    tbin = (torch.rand(shape, generator=g) < 0.5)
    target = tbin.to(torch.int64) if C == 4 else (tbin.float() if C == 2 else torch.rand(shape, generator=g))
    mask = (torch.rand(shape, generator=g) >= 0.3).float()
    members = [("dice", DiceLoss(), probs), ("dice_logits", DiceLossWithLogits(), logits),
               ("bce_dice", BCEDiceLoss(alpha=0.7, beta=1.3), probs),
               ("bce_dice_logits", BCEDiceLossWithLogits(alpha=1.5, beta=0.25), logits),
               ("masked", LossWrapper(DiceLoss(), ApplyAndRemoveMask("multiply")), probs)]
    for kind, loss, x in members:
        tt = torch.cat([target.float(), mask], 1) if kind == "masked" else target
        x64 = x.double().requires_grad_(True)
        a, b = getattr(loss, "alpha", 1.0), getattr(loss, "beta", 0.0)
        ref = _family_reference(kind, x64, tt.double(), a, b)
        ref_grad, = torch.autograd.grad(ref, x64)
        for vox in (1, 0):
            dice_vox_option(vox)
            xd = _as_layout(x, layout).requires_grad_(True)
            val = loss(xd, tt.to(DEV))
            grad, = torch.autograd.grad(val, xd)
            what = (kind, C, layout, vox)
            got, want = float(val.detach()), float(ref.detach())
            assert abs(got - want) <= 3e-6 * max(1.0, abs(want)), (what, got, want)
            err = rel_err(grad.cpu(), ref_grad)
            print(f"DICE_ERR class {kind} C={C} {layout} rank={len(shape)} dice_vox={vox}: value {got:.7f} "
                  f"(float64 {want:.7f}) gradient rel_err {err:.2e}")
            assert err < 2e-5, what
            assert grad.shape == xd.shape
            if layout == "ncdhw":
                assert grad.is_contiguous(), what
            else:
                nd = grad.dim()
                assert grad.stride(1) == 1 and grad.permute(0, *range(2, nd), 1).is_contiguous(), what
            if kind == "masked":
                assert float(grad.cpu()[mask == 0].abs().max()) == 0.0 and float(grad.cpu()[mask == 1].abs().max()) > 0


def test_loss_classes_on_two_dimensional_input(dice_vox_option):
    """rank (N, C): one voxel per sample"""
    from torch_em_amd.loss import BCEDiceLossWithLogits, DiceLoss
    g = torch.Generator().manual_seed(5)
    x, t = torch.rand(5, 4, generator=g) * 0.96 + 0.02, torch.rand(5, 4, generator=g)
    for kind, loss, inp in (("dice", DiceLoss(), x), ("bce_dice_logits", BCEDiceLossWithLogits(), x * 4 - 2)):
        x64 = inp.double().requires_grad_(True)
        ref = _family_reference(kind, x64, t.double(), 1.0, 1.0)
        ref_grad, = torch.autograd.grad(ref, x64)
        for vox in (1, 0):
            dice_vox_option(vox)
            xd = inp.to(DEV).requires_grad_(True)
            val = loss(xd, t.to(DEV))
            grad, = torch.autograd.grad(val, xd)
            got, want = float(val.detach()), float(ref.detach())
            assert abs(got - want) <= 3e-6 * max(1.0, abs(want)), (kind, vox, got, want)
            assert rel_err(grad.cpu(), ref_grad) < 2e-5 and grad.is_contiguous()
