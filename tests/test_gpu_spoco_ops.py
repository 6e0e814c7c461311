"""GPU: every C-ABI entry point of csrc/spoco.hip on every dispatch path, op by op, against the float64 references of
oracle/spoco_op_ref.py (which tests/test_spoco_cpu.py pins to torch float64 autograd and to the goldens, and whose judge it
tests on deliberately wrong outputs).  Inputs and the census that proves the path: oracle/spoco_cases.py.

Rule (oracle/judge.py).  Errors are counted in units of 2^-23 times a per-element scale
(oracle/spoco_op_ref.py: the sum of the absolute values of an element's terms, a difference a - b formed in fp32 counting as
|a| + |b|, a term through exp(x) as exp(x) (1 + |x|)).  On the same inputs the test evaluates the numpy float32 restatement
(one rounding per operation -- a reference, not the code under test) and takes its worst figure e32; the kernel must stay
within MARGIN * max(e32, 1), the MARGIN of 4 of oracle/judge.py.  EVERY element of EVERY output is judged.  Exact quantities (label range, counts,
chunk counts, indices, every gradient element an op must not touch, the stride padding, the sentinels) are compared exactly.

Derived allowance, not fitted to an observed error: means, S and dpush are 64-bit fixed-point sums with 2^-28 resolution;
each add rounds by at most 2^-29, so a slot gets `adds * 2^-29`, scaled as the output is (/ count for the means,
* 2 / (n_bg (C - 1)) for dpush).  `adds` is the census: one per voxel of a mixed or tail wave, one per uniform wave (dpush:
one per wave that holds a background voxel, at most).
No allowance for the kernels' serial fp32 chains was needed: a thread adds at most 2 terms of a streaming sum before the
block reduction (`capped`), C - 1 <= 8 push terms per voxel, A <= 64 consistency terms per voxel (typical error sqrt(A) / 2
units of a sum of positive terms, observed below 1), and the block partials are added in double.

Gradient ops add to a tensor the test fills first (start_grad: random, a quarter of the increment's root mean square); the
result is judged against `start + float64 increment` with the scale `|start| + the increment's scale`.

What a sum check cannot see: the anchors of oracle/spoco_cases.py make a dropped last voxel cost 100 units or more in the
means, S and dpush of every case and 29 or more in the push value (tests/test_spoco_cpu.py: test_a_dropped_last_voxel_costs_many_units), but
the pull VALUE sees it only by 7 units in `capped` and not at all in `global` (one voxel is 2e-8 of that sum); S and the
means carry the check there.

Every op is called twice and must return bit-identical outputs (the file promises "no floating-point atomics").
The test owns every buffer: extents are asserted against the buffers before a launch, stride padding and a spare channel
plane hold NaN (inputs) or a sentinel (outputs), outputs and the workspace -- exactly tem_spoco_ws bytes -- sit between
sentinels that must survive.  Labels are always in [0, C); no case provokes a fault.
Rows of dmu that belong to an EMPTY label (V = 1 only) are 0 / 0 by the formula and are never read; they are not judged.

Observed on the MI355X (profiles/spoco_op_errors.txt): worst kernel error / max(e32, 1) = 1.40 (OBSERVED_WORST_RATIO below: dreg
of tem_spoco_means_terms, 1.73 units where the restatement has 1.24); every other quantity at or below 1.25 units.  Without
its fixed-point allowance dpush is 1.68 units off (0.52 with it), the means 0.40, S 0.17: the 2^-28 resolution shows in dpush,
whose sums are scaled by 2 / (n_bg (C - 1)), and is nowhere the limiting error.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gpu_kit as kit
from oracle import spoco_cases as K
from oracle import spoco_op_ref as R
from oracle.gpu_kit import lib as _lib, ops as _ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = R.MARGIN
OBSERVED_WORST_RATIO = 1.40      # informational: dreg of tem_spoco_means_terms (profiles/spoco_op_errors.txt); the assertions use MARGIN
SENT = 12345.0
G = 64                           # guard floats around every buffer (keeps 256-byte alignment)
f32, f64 = np.float32, np.float64


LEDGER = kit.Ledger("SPOCO_ERR")
_note = LEDGER.note
_print_worst = LEDGER.summary_fixture(left_out=lambda q: q.endswith("no allow."))      # those rows are for the record


def _raw(entry, key, got, ref, scale):
    """for the record: a fixed-point output's units WITHOUT its allowance"""
    _note(entry, key + " no allow.", R.units(got[key], ref[key], scale[key]), 0.0)


def _verdict(entry, tag, j):
    """print, record and assert one judged call: j = {quantity: (kernel units, e32, ok)}"""
    print(f"SPOCO_ERR {entry} {tag}: " + " ".join(f"{k}: kernel {v[0]:.2f} f32 {v[1]:.2f}" for k, v in j.items()))
    for k, (ek, e32, ok) in j.items():
        _note(entry, k, ek, e32)
    for k, (ek, e32, ok) in j.items():
        assert ok, f"{entry} {tag}: {k} is {ek:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"


# ------------------------------------------------------------------------------------------ buffers the test lays out itself
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Planes:
    """A logical float32 [E, V] array as E planes of stride cs = V + pad inside a device buffer the test owns; one spare
    plane and everything else hold `fill`."""

    def __init__(self, arr, pad=0, fill=float("nan")):
        E, V = arr.shape
        self.E, self.V, self.cs = E, V, V + pad
        self.buf = torch.full((G + (E + 1) * self.cs + G,), fill, dtype=torch.float32, device=DEV)
        assert self.cs >= V and G + (E - 1) * self.cs + V <= self.buf.numel() - G, "the tensor leaves its buffer"
        self.view = torch.as_strided(self.buf, (E, V), (self.cs, 1), G)
        self.view.copy_(torch.from_numpy(np.array(arr, f32)))
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        torch.as_strided(self.inside, (E, V), (self.cs, 1), G).fill_(True)
        self.snap = self.buf.clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * G)

    def host(self):
        return self.view.cpu().numpy().copy()

    def outside_untouched(self):
        return bool(torch.equal(_bits(self.buf)[~self.inside], _bits(self.snap)[~self.inside]))

    def unchanged(self):
        return bool(torch.equal(_bits(self.buf), _bits(self.snap)))


class Out:
    """n elements between two guards of G sentinels"""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + 2 * G,), 12345, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + G * self.buf.element_size())

    def host(self, shape=None):
        assert bool((self.buf[:G] == 12345).all()) and bool((self.buf[G + self.n:] == 12345).all()), "wrote around an output"
        a = self.buf[G:G + self.n].cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)


class Ws:
    """exactly tem_spoco_ws(C, E, V, nz, A, K) bytes, and a guard behind them"""

    def __init__(self, C, E, V, nz=1, A=1, Kn=1):
        self.n = int(_lib().load().tem_spoco_ws(int(C), int(E), int(V), int(nz), int(A), int(Kn)))
        self.buf = torch.full((self.n + 256,), 0xA5, dtype=torch.uint8, device=DEV)

    @property
    def args(self):
        return ctypes.c_void_p(self.buf.data_ptr()), self.n

    def floats(self, n):
        return self.buf[:4 * n].view(torch.float32).cpu().numpy().copy()

    def check(self):
        assert bool((self.buf[self.n:] == 0xA5).all()), "wrote behind the workspace"


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype, order="C")).to(DEV)       # a C-ordered copy: the case data is read-only


def call(name, *args):
    lib = _lib()
    lib.check(getattr(lib.load(), name)(*args), name)


def stream():
    return _ops()._stream(torch.empty(1, device=DEV))


def start_grad(inc, seed):
    """the tensor a gradient op adds to: random, a quarter of the increment's root mean square, so that the rounding of
    `grad + increment` does not drown an error of the increment (an input choice; no tolerance depends on it)"""
    nzv = np.asarray(inc, f64)[np.asarray(inc) != 0]
    s = float(np.sqrt((nzv * nzv).mean())) if nzv.size else 1.0
    return (0.25 * s * np.random.RandomState(seed).randn(*np.shape(inc))).astype(f32)


def twice(fn):
    """run an op twice on fresh outputs: bit-identical, and return the first"""
    a, b = fn(), fn()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{k}: a repeated launch is not bit-identical"
    return a


# ------------------------------------------------------------------------------------------ label range, zero count / select
@pytest.mark.parametrize("V", [1, 255, 1024, 1025, 262144 + 37])
def test_label_range_and_zero_ops_exact(V):
    rng = np.random.RandomState(V % 1000)
    p = _ops()._p
    ws = Ws(1, 1, V)
    second = 262144 + 5 if V > 262144 else V // 2        # a wave only the second grid-stride iteration reaches
    print(f"SPOCO_PATH label ops V={V}: grid={K.grid_1d(V, R.SP_MAXB)} twice={V > 262144} chunks={-(-V // 1024)}")
    for lo_at, hi_at in ((0, V - 1), (V - 1, 0), (second, min(second + 1, V - 1))):
        lbl = rng.randint(-3, 6, V).astype(np.int64)      # negative labels appear
        lbl[hi_at] = 9
        lbl[lo_at] = -7                                    # (V = 1: the one voxel is both)
        ld = dev(lbl)

        def run():
            out = Out(2, torch.int64)
            call("tem_label_range", p(ld), V, out.ptr, *ws.args, stream())
            return {"minmax": out.host()}
        got = twice(run)
        ws.check()
        assert R.exact(got["minmax"], R.label_range(lbl)["minmax"]), (got, lo_at, hi_at)
    lbl = (rng.uniform(size=V) > 0.3).astype(np.int64) * rng.randint(-2, 5, V)
    lbl[V - 1] = 0                                       # the last rank hits the last voxel
    ld = dev(lbl)
    ref = R.zero_count(lbl)
    nch = ref["chunk_counts"].size
    cc = Out(nch, torch.int32)

    def run_count():
        tot = Out(1, torch.int64)
        call("tem_zero_count", p(ld), V, cc.ptr, tot.ptr, stream())
        return {"chunk_counts": cc.host(), "total": tot.host()}
    got = twice(run_count)
    assert R.exact(got["chunk_counts"], ref["chunk_counts"]) and R.exact(got["total"], ref["total"])
    n0 = int(ref["total"][0])
    ranks = sorted({0, n0 - 1, n0 // 2, min(7, n0 - 1), int(ref["chunk_counts"][:65].sum()) % n0})
    rd = dev(np.array(ranks, np.int64))

    def run_sel():
        idx = Out(len(ranks), torch.int64)
        call("tem_zero_select", p(ld), V, cc.ptr, p(rd), len(ranks), idx.ptr, stream())
        return {"idx": idx.host()}
    got = twice(run_sel)
    want = R.zero_select(lbl, ranks)
    assert R.exact(got["idx"], want["idx"]), (got, want)
    assert want["idx"][-1] == V - 1
    assert np.array_equal(ld.cpu().numpy(), lbl), "the labels are an input"


# ------------------------------------------------------------------------------------------ cluster means and pull
ALL = K.expand()


def _path_line(cid, d, want):
    line = K.check_path(d["census"], want)
    print(f"SPOCO_PATH {cid}: {line}")
    return d["census"]


@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", ALL, ids=[c[0] for c in ALL])
def test_cluster_means_and_pull_against_float64(cid, name, E, C, V, plan, pad, want):
    d = K.case_data(name, E, C, V, plan)
    cen = _path_line(cid, d, want)
    p = _ops()._p
    lbl, emb = d["lbl"], d["emb"]
    P, ld = Planes(emb, pad), dev(lbl)
    assert lbl.min() >= 0 and lbl.max() < C and ld.numel() == V
    ws = Ws(C, E, V)

    def run_means():
        m, c = Out(C * E), Out(C)
        call("tem_spoco_cluster_means", P.ptr, P.cs, p(ld), V, E, C, m.ptr, c.ptr, *ws.args, stream())
        return {"means": m.host((C, E)), "counts": c.host()}
    got = twice(run_means)
    ws.check()
    ref, r32, sc = R.cluster_means(emb, lbl, C), R.cluster_means_f32(emb, lbl, C), R.cluster_means_scale(emb, lbl, C)
    j = R.judge(got, ref, r32, sc, R.cluster_means_allow(cen["adds"], cen["counts"]))
    _raw("tem_spoco_cluster_means", "means", got, ref, sc)
    _verdict("tem_spoco_cluster_means", cid, j)
    assert not got["means"][cen["counts"] == 0].any(), "an empty label has mean 0"

    means, counts = d["means"], d["counts"]
    md, cd = dev(means), dev(counts)

    def run_pull():
        v, s = Out(1), Out(C * E)
        call("tem_spoco_pull", P.ptr, P.cs, p(ld), V, E, C, p(md), p(cd), K.DELTA_VAR, v.ptr, s.ptr, *ws.args, stream())
        return {"value": v.host(), "S": s.host((C, E))}
    got = twice(run_pull)
    ws.check()
    safe = np.maximum(counts, 1)                         # an empty label has no voxel: its count is never read
    a = (emb, lbl, C, means, safe, K.DELTA_VAR)
    ref, sc = R.pull(*a), R.pull_scale(*a)
    j = R.judge(got, ref, R.pull_f32(*a), sc, R.pull_allow(cen["adds"]))
    _raw("tem_spoco_pull", "S", got, ref, sc)
    _verdict("tem_spoco_pull", cid, j)
    assert P.unchanged() and np.array_equal(ld.cpu().numpy(), lbl), "embeddings and labels are inputs"


# ------------------------------------------------------------------------------------------ push and the embedding gradient
PUSH = K.expand(("tiny", "waves", "em16", "em32", "capped"))
WEIGHTS = dict(n_inst=4.0, w_var=0.9, w_dist=0.7, w_reg=0.01, w_push=0.6)


def _embed_grad_case(tag, emb, lbl, C, pad, means, counts, S, ddist, dreg, dpush, variants):
    """variants: [(accumulate, with_dpush)]"""
    p = _ops()._p
    E, V = emb.shape
    P, ld = Planes(emb, pad), dev(lbl)
    md, cd, Sd, ddd, drd, dpd = (dev(a, f32) for a in (means, counts, S, ddist, dreg, dpush))
    ws = Ws(C, E, V)
    w = WEIGHTS
    rows = counts > 0
    for acc, with_dp in variants:
        a = (emb, lbl, C, means, np.maximum(counts, 1), S, ddist, dreg, dpush if with_dp else None, K.DELTA_VAR,
             w["n_inst"], w["w_var"], w["w_dist"], w["w_reg"], w["w_push"])
        ref, r32, sc = R.embed_grad(*a), R.embed_grad_f32(*a), R.embed_grad_scale(*a)
        g0 = start_grad(ref["g"], V % 997)

        def run():
            Gd = Planes(g0, pad, fill=SENT)
            call("tem_spoco_embed_grad", P.ptr, P.cs, p(ld), V, E, C, p(md), p(cd), p(Sd), p(ddd), p(drd),
                 p(dpd) if with_dp else None, K.DELTA_VAR, w["n_inst"], w["w_var"], w["w_dist"], w["w_reg"], w["w_push"],
                 Gd.ptr, Gd.cs, acc, *ws.args, stream())
            torch.cuda.synchronize()
            assert Gd.outside_untouched(), "wrote into the gradient's stride padding"
            return {"dmu": ws.floats(C * E).reshape(C, E)[rows], "g": Gd.host()}
        got = twice(run)
        ws.check()
        for o in (ref, r32, sc):
            o["dmu"] = o["dmu"][rows]
        if acc:
            ref["g"], r32["g"], sc["g"] = ref["g"] + g0, (r32["g"] + g0).astype(f32), sc["g"] + np.abs(g0)
        _verdict("tem_spoco_embed_grad", f"{tag} accumulate={acc} dpush={'set' if with_dp else 'NULL'}", R.judge(got, ref, r32, sc))
    assert P.unchanged(), "the embeddings are an input"


@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", PUSH, ids=[c[0] for c in PUSH])
def test_push_and_embed_grad_against_float64(cid, name, E, C, V, plan, pad, want):
    d = K.case_data(name, E, C, V, plan)
    cen = _path_line(cid, d, want)
    print(f"SPOCO_PATH {cid}: push skips {cen['no_bg_waves']} waves without background, works on {cen['bg_waves']}; "
          f"embed_grad grid={cen['grid_grad']} twice={cen['twice_grad']}")
    p = _ops()._p
    lbl, emb, means, counts = d["lbl"], d["emb"], d["means"], d["counts"]
    assert counts[0] > 0 and lbl.min() >= 0 and lbl.max() < C
    P, ld, md, cd = Planes(emb, pad), dev(lbl), dev(means), dev(counts)
    ws = Ws(C, E, V)
    gs = 0.75
    a = (emb, lbl, C, means, counts, K.DELTA_DIST, gs)
    ref, r32, sc = R.push(*a), R.push_f32(*a), R.push_scale(*a)
    g0 = start_grad(ref["ginc"], V % 991)
    allow = R.push_allow(cen["bg_waves"], C, counts)
    fg = lbl != 0
    for with_grad in (False, True):
        def run():
            v, dp = Out(1), Out(C * E)
            Gd = Planes(g0, pad, fill=SENT)
            call("tem_spoco_push", P.ptr, P.cs, p(ld), V, E, C, p(md), p(cd), K.DELTA_DIST, v.ptr, gs,
                 Gd.ptr if with_grad else None, Gd.cs, dp.ptr, *ws.args, stream())
            torch.cuda.synchronize()
            assert Gd.outside_untouched(), "wrote into the gradient's stride padding"
            return {"value": v.host(), "dpush": dp.host((C, E)), "after": Gd.host()}
        got = twice(run)
        ws.check()
        after = got.pop("after")
        if with_grad:
            assert R.untouched(g0, after, fg), "push changed the gradient of a voxel that is not background"
            ref_a, r32_a = dict(ref, ginc=ref["ginc"] + g0), dict(r32, ginc=(r32["ginc"] + g0).astype(f32))
            sc_a = dict(sc, ginc=sc["ginc"] + np.abs(g0) * ~fg)
            j = R.judge(dict(got, ginc=after), ref_a, r32_a, sc_a, allow)
        else:
            assert R.untouched(g0, after, np.ones(V, bool)), "grad = NULL: nothing is written"
            keys = {k: v for k, v in sc.items() if k != "ginc"}
            j = R.judge(got, ref, r32, keys, allow)
        _raw("tem_spoco_push", "dpush", got, ref, sc)
        _verdict("tem_spoco_push", f"{cid} grad={'set' if with_grad else 'NULL'}", j)
        assert not got["dpush"][0].any(), "the background mean gets no push"
    assert P.unchanged(), "the embeddings are an input"
    S = R.pull(emb, lbl, C, means, np.maximum(counts, 1), K.DELTA_VAR)["S"].astype(f32)
    mt = R.means_terms(means, K.DELTA_DIST, 1)
    variants = [(0, False), (1, True)] if name == "capped" else [(0, False), (1, True), (0, True), (1, False)]
    _embed_grad_case(cid, emb, lbl, C, pad, means, counts, S, mt["ddist"].astype(f32), mt["dreg"].astype(f32),
                     ref["dpush"].astype(f32), variants)


def test_embed_grad_grid_cap():
    """V = 524288 + 101: the grid of k_embed_grad stops at 2048 blocks and 101 threads run a second iteration"""
    V, E, C = 524288 + 101, 3, 6
    lbl = K.make_labels(V, C, "UUUSRBUU", 1)
    cen = K.census(lbl, E, C, V)
    assert cen["grid_grad"] == 2048 and cen["twice_grad"]
    print(f"SPOCO_PATH embed_grad cap V={V}: grid={cen['grid_grad']} twice={cen['twice_grad']} EM={cen['EM']}")
    emb = K.make_embeddings(E, V, 11)
    cm = R.cluster_means(emb, lbl, C)
    means, counts = cm["means"].astype(f32), cm["counts"].astype(f32)
    S = R.pull(emb, lbl, C, means, counts, K.DELTA_VAR)["S"].astype(f32)
    mt = R.means_terms(means, K.DELTA_DIST, 1)
    _embed_grad_case("cap2048", emb, lbl, C, 0, means, counts, S, mt["ddist"].astype(f32), mt["dreg"].astype(f32),
                     np.zeros((C, E), f32), [(1, False)])


# ------------------------------------------------------------------------------------------ means terms
@pytest.mark.parametrize("C", [1, 2, 3, 65, 130])
def test_means_terms_against_float64(C):
    p = _ops()._p
    print(f"SPOCO_PATH means_terms C={C}: lanes stride over j {-(-C // 64)} times")
    for E in (3, 16, 32):
        mu = K.means_case(C, E, 5 * C + E)
        md = dev(mu)
        ws = Ws(C, E, 1)
        for iz in (0, 1):
            def run():
                v, dd, dr = Out(2), Out(C * E), Out(C * E)
                call("tem_spoco_means_terms", p(md), C, E, K.DELTA_DIST, iz, v.ptr, dd.ptr, dr.ptr, *ws.args, stream())
                return {"values": v.host(), "ddist": dd.host((C, E)), "dreg": dr.host((C, E))}
            got = twice(run)
            ws.check()
            a = (mu, K.DELTA_DIST, iz)
            j = R.judge(got, R.means_terms(*a), R.means_terms_f32(*a), R.means_terms_scale(*a))
            _verdict("tem_spoco_means_terms", f"C={C} E={E} ignore_zero={iz}", j)
            if C == 1 or (iz and C == 2):
                assert got["values"][0] == 0 and not got["ddist"].any(), "the inactive cases"
            if C >= 6:
                assert not got["dreg"][5].any(), "a zero-norm mean has no regulariser gradient"


# ------------------------------------------------------------------------------------------ instance Dice
@pytest.mark.parametrize("nz,sl", K.IDICE)
def test_instance_dice_against_float64(nz, sl):
    p = _ops()._p
    V = nz * sl
    per = -(-sl // R.SP_NCH)
    for C, E in [(1, 3), (2, 8), (9, 9), (10, 16), (18, 17)]:
        lbl, emb = K.volume(nz, sl, C, E, C + sl)
        mu = R.cluster_means(emb, lbl, C)["means"].astype(f32)
        print(f"SPOCO_PATH instance_dice nz={nz} slice={sl} C={C} E={E}: EM={K.census(lbl, E, C, V)['EM']} "
              f"tiles={-(-(C - 1) // R.SP_IT)} empty chunks={max(R.SP_NCH - -(-sl // per), 0)}")
        P, ld, md = Planes(emb, 24 if C == 9 else 0), dev(lbl), dev(mu)
        ws = Ws(C, E, V, nz)

        def run():
            v = Out(1)
            call("tem_spoco_instance_dice", P.ptr, P.cs, p(ld), V, nz, E, C, p(md), float(K.TWO_SIGMA), 1e-7, v.ptr,
                 *ws.args, stream())
            return {"value": v.host()}
        got = twice(run)
        ws.check()
        a = (emb, lbl, nz, C, mu, K.TWO_SIGMA, 1e-7)
        if C == 1:
            assert got["value"][0] == 0.0
            continue
        j = R.judge(got, R.instance_dice(*a), R.instance_dice_f32(*a), R.instance_dice_scale(*a))
        _verdict("tem_spoco_instance_dice", f"nz={nz} slice={sl} C={C} E={E}", j)
        assert P.unchanged()


# ------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize("nz,sl,E,A,pad", [c + (0,) for c in K.CONS] + [K.CONS[0] + (24,)])
def test_consistency_against_float64(nz, sl, E, A, pad):
    p = _ops()._p
    V = nz * sl
    q, k, idx, far = K.cons_inputs(nz, sl, E, A, A + sl)
    assert 0 <= idx.min() and idx.max() < V and A <= R.SP_MAXA
    iters = -(-(-(-sl // R.SP_NCH)) // 256)
    print(f"SPOCO_PATH consistency nz={nz} slice={sl} E={E} A={A} cs=V+{pad}: EM={8 if E <= 8 else 16 if E <= 16 else 32} "
          f"terms per thread={A * iters} eps-branch slice={far} duplicate anchor={len(set(idx.tolist())) < A}")
    Q, Kd, idd = Planes(q, pad), Planes(k, pad), dev(idx)
    ws = Ws(1, E, V, nz, A)
    gs = 0.5
    a = (q, k, nz, idx, K.TWO_SIGMA, 1e-7, gs)
    ref, r32, sc = R.consistency(*a), R.consistency_f32(*a), R.consistency_scale(*a)
    g0 = start_grad(ref["ginc"], A)
    for with_grad in (False, True):
        def run():
            v = Out(1)
            Gd = Planes(g0, pad, fill=SENT)
            call("tem_spoco_consistency", Q.ptr, Kd.ptr, Q.cs, V, nz, E, p(idd), A, float(K.TWO_SIGMA), 1e-7, v.ptr, gs,
                 Gd.ptr if with_grad else None, Gd.cs, *ws.args, stream())
            torch.cuda.synchronize()
            assert Gd.outside_untouched(), "wrote into the gradient's stride padding"
            return {"value": v.host(), "after": Gd.host()}
        got = twice(run)
        ws.check()
        after = got.pop("after")
        if with_grad:
            j = R.judge(dict(got, ginc=after), dict(ref, ginc=ref["ginc"] + g0), dict(r32, ginc=(r32["ginc"] + g0).astype(f32)),
                        dict(sc, ginc=sc["ginc"] + np.abs(g0)))
            if far is not None:                          # the d <= eps branch: the gradient is exactly 0
                s = slice(far * sl, (far + 1) * sl)
                assert R.untouched(g0[:, s], after[:, s], np.ones(sl, bool)), "the underflowed slice must keep its gradient"
        else:
            assert R.untouched(g0, after, np.ones(V, bool)), "grad_q = NULL: nothing is written"
            j = R.judge(got, ref, r32, {"value": sc["value"]})
        _verdict("tem_spoco_consistency", f"nz={nz} slice={sl} E={E} A={A} cs+{pad} grad={'set' if with_grad else 'NULL'}", j)
    if far is not None:                                  # ... and its term exactly 1: the value without it is 1 lower
        rest = np.delete(np.arange(V), np.arange(far * sl, (far + 1) * sl))
        sub = R.consistency(q[:, rest], k[:, rest], nz - 1, np.searchsorted(rest, idx), K.TWO_SIGMA, 1e-7, gs)
        assert abs(ref["value"][0] - sub["value"][0] - 1.0) < 1e-12
    assert Q.unchanged() and Kd.unchanged(), "the embeddings are inputs"


# ------------------------------------------------------------------------------------------ affinity side loss
@pytest.mark.parametrize("shape,Kn", K.AFF)
def test_affinity_side_against_float64(shape, Kn):
    p = _ops()._p
    E = 3 if Kn != 32 else 9
    zero_only = (shape, Kn) == K.AFF[-1]
    emb, lbl, offs = K.aff_inputs(shape, Kn, E, Kn + shape[2], zero_only)
    V = int(np.prod(shape))
    assert offs.shape == (Kn, 3) and Kn <= R.SP_MAXK
    beyond = [tuple(o) for o in offs if any(abs(int(o[i])) >= shape[i] and o[i] for i in range(3))]
    print(f"SPOCO_PATH affinity shape={shape} K={Kn} E={E}: grid={K.grid_1d(V, R.SP_MAXB)} offsets at or beyond the extent "
          f"{len(beyond)} zero-offset-only={zero_only}")
    P, ld = Planes(emb, 24 if Kn == 8 else 0), dev(lbl)
    ws = Ws(1, E, V, 1, 1, Kn)
    oarr = (ctypes.c_int * (3 * Kn))(*[int(x) for x in offs.reshape(-1)])
    gs = 0.5
    a = (emb, lbl, shape, offs, K.DELTA_DIST, 1e-7, gs)
    ref, r32, sc = R.affinity_side(*a), R.affinity_side_f32(*a), R.affinity_side_scale(*a)
    g0 = start_grad(ref["ginc"], Kn)
    for with_grad in (False, True):
        def run():
            v = Out(1)
            Gd = Planes(g0, P.cs - V, fill=SENT)
            call("tem_affinity_side", P.ptr, P.cs, p(ld), *shape, E, oarr, Kn, K.DELTA_DIST, 1e-7, v.ptr, gs,
                 Gd.ptr if with_grad else None, Gd.cs, *ws.args, stream())
            torch.cuda.synchronize()
            assert Gd.outside_untouched(), "wrote into the gradient's stride padding"
            return {"value": v.host(), "after": Gd.host()}
        got = twice(run)
        ws.check()
        after = got.pop("after")
        if zero_only:
            assert got["value"][0] == 1.0 and R.untouched(g0, after, np.ones(V, bool)), "n = d = 0: loss 1, gradient 0"
        if with_grad:
            j = R.judge(dict(got, ginc=after), dict(ref, ginc=ref["ginc"] + g0), dict(r32, ginc=(r32["ginc"] + g0).astype(f32)),
                        dict(sc, ginc=sc["ginc"] + np.abs(g0)))
        else:
            assert R.untouched(g0, after, np.ones(V, bool)), "grad = NULL: nothing is written"
            j = R.judge(got, ref, r32, {"value": sc["value"]})
        _verdict("tem_affinity_side", f"shape={shape} K={Kn} grad={'set' if with_grad else 'NULL'}", j)
    assert P.unchanged(), "the embeddings are an input"


def test_affinity_side_value_grid_cap():
    """(1, 1, V) with V = 262144 + 101: k_aff_sums runs SP_MAXB blocks and 101 threads a second iteration"""
    p = _ops()._p
    V, E, Kn = 262144 + 101, 3, 2
    shape = (1, 1, V)
    assert K.grid_1d(V, R.SP_MAXB) == R.SP_MAXB and V > R.SP_MAXB * 256
    print(f"SPOCO_PATH affinity cap V={V}: grid={R.SP_MAXB} twice=True")
    rng = np.random.RandomState(4)
    emb = (0.8 * rng.randn(E, V)).astype(f32)
    lbl = np.repeat(rng.randint(0, 4, -(-V // 3)), 3)[:V].astype(np.int64)
    emb[:, V - 1] = emb[:, V - 2] + 1.0                  # the last pair: a term of order 1 behind the cap
    lbl[V - 1] = lbl[V - 2] + 1
    offs = np.array([(0, 0, 1), (0, 0, -5)], np.int32)
    P, ld = Planes(emb), dev(lbl)
    ws = Ws(1, E, V, 1, 1, Kn)
    oarr = (ctypes.c_int * (3 * Kn))(*[int(x) for x in offs.reshape(-1)])

    def run():
        v = Out(1)
        call("tem_affinity_side", P.ptr, P.cs, p(ld), *shape, E, oarr, Kn, K.DELTA_DIST, 1e-7, v.ptr, 1.0, None, V,
             *ws.args, stream())
        return {"value": v.host()}
    got = twice(run)
    ws.check()
    a = (emb, lbl, shape, offs, K.DELTA_DIST, 1e-7, 1.0)
    kw = dict(want_grad=False)
    sc = R.affinity_side_scale(*a, **kw)
    j = R.judge(got, R.affinity_side(*a, **kw), R.affinity_side_f32(*a, **kw), {"value": sc["value"]})
    _verdict("tem_affinity_side", f"cap V={V} K={Kn} grad=NULL", j)
