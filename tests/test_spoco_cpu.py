"""CPU: the float64 references, the float32 restatements, the case census and the judge of the SPOCO op-by-op suite
(oracle/spoco_op_ref.py, oracle/spoco_cases.py), which tests/test_gpu_spoco_ops.py holds the kernels of csrc/spoco.hip to.

  * every float64 reference is pinned to oracle/spoco_ref.py under torch float64 autograd, per term and per gradient, at
    rtol 1e-10 (plus 1e-12 of the quantity's largest element: the two sum in different orders), and, composed, to the
    g6g / g6h goldens (the only ones that carry a quantity of a single code path: loss and gradient of ContrastiveLoss);
  * each case's census equals the path the case table names;
  * the float32 restatement stays under a cap, in units of 2^-23 x scale, for every quantity.  Measured here:
    means 0.73, pull value 0.16 / S 0.21, means_terms values 0.81 / ddist 0.54 / dreg 1.45, instance Dice 0.75, push value
    0.11 / gradient 0.43 / dpush 0.39, embed_grad dmu 1.78 / g 1.23, consistency value 0.04 / gradient 1.33, affinity value
    0.06 / gradient 0.41 (printed as SPOCO_E32_SUMMARY with -s).  The caps below are these rounded up to the next integer;
  * the judge rejects ten deliberately wrong outputs built from the reference, and accepts the restatement.
"""
import os

import numpy as np
import pytest
import torch

from oracle import spoco_cases as K
from oracle import spoco_op_ref as R
from oracle import spoco_ref
from oracle.loss_ref import dice_score

f32, f64 = np.float32, np.float64
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SMALL = [c for c in K.expand(("tiny", "waves", "em16", "em32")) if c[6] == K.CASES[c[1]][4][0]]   # layouts are GPU business
IDS = [c[0] for c in SMALL]
CAPS = {"means": 1, "pull.value": 1, "pull.S": 1, "mt.values": 1, "mt.ddist": 1, "mt.dreg": 2, "idice.value": 1,
        "push.value": 1, "push.ginc": 1, "push.dpush": 1, "eg.dmu": 2, "eg.g": 2, "cons.value": 1, "cons.ginc": 2,
        "aff.value": 1, "aff.ginc": 1}
W = dict(n_inst=4.0, w_var=0.9, w_dist=0.7, w_reg=0.01, w_push=0.6)


MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    print("\nSPOCO_E32_SUMMARY " + " ".join(f"{k} {v:.2f}" for k, v in sorted(MEASURED.items())))


def cap(key, ek):
    MEASURED[key] = max(MEASURED.get(key, 0.0), ek)
    assert ek <= CAPS[key], f"the float32 restatement of {key} is {ek:.2f} units from float64, cap {CAPS[key]}"


def close(got, want, what):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape, what
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * max(float(np.abs(want).max()), 1e-300), err_msg=what)


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, f64).copy()).requires_grad_(grad)


# ------------------------------------------------------------------------------------------ pins to torch float64 autograd
@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", SMALL, ids=IDS)
def test_segment_ops_match_torch_float64(cid, name, E, C, V, plan, pad, want):
    d = K.case_data(name, E, C, V, plan)
    lbl, emb = d["lbl"], d["emb"]
    tl = torch.from_numpy(lbl.copy())
    cm = R.cluster_means(emb, lbl, C)
    close(cm["means"], spoco_ref.cluster_means(t64(emb), tl, C).numpy(), "cluster means")
    assert np.array_equal(cm["counts"], np.bincount(lbl, minlength=C))
    occ = np.nonzero(d["counts"] > 0)[0]                 # V = 1 leaves label 1 empty: mean 0, count 0, and no pull term
    if occ.size < C:
        assert not cm["means"][d["counts"] == 0].any()
    # pull: value and S = -count/2 d value / d mu, the means a leaf
    mu = t64(d["means"], True)
    safe = np.maximum(d["counts"], 1)
    val = spoco_ref.variance_term(mu, t64(emb), tl, t64(safe), K.DELTA_VAR, False) * C
    val.sum().backward()
    p = R.pull(emb, lbl, C, d["means"], safe, K.DELTA_VAR)
    close(p["value"], val.detach().numpy(), "pull value")
    close(p["S"], -0.5 * safe[:, None] * mu.grad.numpy(), "pull S")
    # push: value, d / d emb on the background, d / d means
    mu, te = t64(d["means"], True), t64(emb, True)
    val = spoco_ref.unlabeled_push(mu, te, tl, K.DELTA_DIST)
    val.backward()
    q = R.push(emb, lbl, C, d["means"], d["counts"], K.DELTA_DIST, 0.75)
    close(q["value"], [val.item()], "push value")
    close(q["ginc"], float(f32(0.75)) * te.grad.numpy(), "push gradient")
    close(q["dpush"], mu.grad.numpy(), "dpush")
    assert not q["ginc"][:, lbl != 0].any() and not q["dpush"][0].any()


@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", [c for c in SMALL if c[4] > 1], ids=[i for i, c in zip(IDS, SMALL) if c[4] > 1])
def test_embed_grad_chain_matches_torch_float64(cid, name, E, C, V, plan, pad, want):
    """embed_grad + the direct push gradient = autograd of the whole objective through the means"""
    d = K.case_data(name, E, C, V, plan)
    lbl, emb = d["lbl"], d["emb"]
    tl, te = torch.from_numpy(lbl.copy()), t64(emb, True)
    means = spoco_ref.cluster_means(te, tl, C)
    cnt = t64(d["counts"])
    wv, wd, wr, wp, ni = (float(f32(W[k])) for k in ("w_var", "w_dist", "w_reg", "w_push", "n_inst"))
    obj = wv * spoco_ref.variance_term(means, te, tl, cnt, K.DELTA_VAR, False).sum() * C / ni + \
        wd * spoco_ref.distance_term(means, K.DELTA_DIST, True) + wr * spoco_ref.regularizer_term(means) + \
        wp * spoco_ref.unlabeled_push(means, te, tl, K.DELTA_DIST)
    obj.backward()
    m64 = R.cluster_means(emb, lbl, C)
    mu, cn = m64["means"], m64["counts"]
    p = R.pull(emb, lbl, C, mu, cn, K.DELTA_VAR)
    mt = R.means_terms(mu, K.DELTA_DIST, 1)
    ps = R.push(emb, lbl, C, mu, cn, K.DELTA_DIST, wp)
    eg = R.embed_grad(emb, lbl, C, mu, cn, p["S"], mt["ddist"], mt["dreg"], ps["dpush"], K.DELTA_VAR, ni, wv, wd, wr, wp)
    close(eg["g"] + ps["ginc"], te.grad.numpy(), "embedding gradient")
    e0 = R.embed_grad(emb, lbl, C, mu, cn, p["S"], mt["ddist"], mt["dreg"], None, K.DELTA_VAR, ni, wv, wd, wr, 0.0)
    e1 = R.embed_grad(emb, lbl, C, mu, cn, p["S"], mt["ddist"], mt["dreg"], 0 * ps["dpush"], K.DELTA_VAR, ni, wv, wd, wr, wp)
    assert np.array_equal(e0["g"], e1["g"]), "dpush NULL = a zero dpush"


MT = [(C, E, iz) for C in (1, 2, 3, 65, 130) for E in (3, 16, 32) for iz in (0, 1)]


@pytest.mark.parametrize("C,E,iz", MT)
def test_means_terms_match_torch_float64(C, E, iz):
    mu = K.means_case(C, E, 5 * C + E)
    if C >= 10:
        d = np.linalg.norm(mu.astype(f64)[:, None] - mu.astype(f64)[None], axis=2)
        assert d[1, 2] == 0 and d[0, 4] == 0 and not mu[5].any()
        assert 0 < 2 * K.DELTA_DIST - d[6, 7] < 1e-4 and 0 < d[8, 9] - 2 * K.DELTA_DIST < 1e-4
    t = t64(mu, True)
    dist = spoco_ref.distance_term(t, K.DELTA_DIST, bool(iz))
    reg = spoco_ref.regularizer_term(t)
    got = R.means_terms(mu, K.DELTA_DIST, iz)
    close(got["values"], [float(dist.detach()) if torch.is_tensor(dist) else dist, float(reg.detach())], "values")
    gd = torch.autograd.grad(dist, t)[0].numpy() if torch.is_tensor(dist) else np.zeros((C, E))
    close(got["ddist"], gd, "ddist")
    close(got["dreg"], torch.autograd.grad(reg, t)[0].numpy(), "dreg")
    if C >= 6:
        assert not got["dreg"][5].any()
    if C == 1 or (iz and C == 2):
        assert got["values"][0] == 0 and not got["ddist"].any()                                   # the inactive cases
    if iz and C >= 5:
        assert got["values"][0] >= 2 * 4 * K.DELTA_DIST ** 2 / ((C - 1) * (C - 2))                   # + 4 delta^2, both orders
    sc = R.means_terms_scale(mu, K.DELTA_DIST, iz)
    j = R.judge(R.means_terms_f32(mu, K.DELTA_DIST, iz), got, R.means_terms_f32(mu, K.DELTA_DIST, iz), sc)
    for k, (ek, _, ok) in j.items():
        assert ok
        cap("mt." + k, ek)


@pytest.mark.parametrize("nz,sl", K.IDICE)
@pytest.mark.parametrize("C,E", [(1, 3), (2, 8), (9, 9), (10, 16), (18, 17)])
def test_instance_dice_matches_torch_float64(nz, sl, C, E):
    lbl, emb = K.volume(nz, sl, C, E, C + sl)
    mu = R.cluster_means(emb, lbl, C)["means"].astype(f32)
    got = R.instance_dice(emb, lbl, nz, C, mu, K.TWO_SIGMA, 1e-7)
    ts = float(f32(K.TWO_SIGMA))
    e = t64(emb).reshape(E, nz, sl).movedim(0, -1)
    vals = [dice_score(spoco_ref.pmap(e, t64(mu[i]), ts)[None], t64(lbl.reshape(nz, sl) == i)[None], invert=True)
            for i in range(1, C)]
    close(got["value"], [float(torch.stack(vals).mean()) if vals else 0.0], "instance dice")
    r32 = R.instance_dice_f32(emb, lbl, nz, C, mu, K.TWO_SIGMA, 1e-7)
    if C > 1:
        ek = R.units(r32["value"], got["value"], R.instance_dice_scale(emb, lbl, nz, C, mu, K.TWO_SIGMA, 1e-7)["value"])
        cap("idice.value", ek)


@pytest.mark.parametrize("nz,sl,E,A", K.CONS)
def test_consistency_matches_torch_float64(nz, sl, E, A):
    q, k, idx, far = K.cons_inputs(nz, sl, E, A, A + sl)
    ts = float(f32(K.TWO_SIGMA))
    tq = t64(q, True)
    val = spoco_ref.consistency_term(tq.reshape(E, nz, sl), t64(k).reshape(E, nz, sl), torch.ones(nz, sl, dtype=torch.int32),
                                     ts, A, 0.0, anchors=[int(i) for i in idx])
    val.backward()
    got = R.consistency(q, k, nz, idx, K.TWO_SIGMA, 1e-7, 0.5)
    close(got["value"], [val.item()], "consistency value")
    close(got["ginc"], float(f32(0.5)) * tq.grad.numpy(), "consistency gradient")
    r32 = R.consistency_f32(q, k, nz, idx, K.TWO_SIGMA, 1e-7, 0.5)
    if far is not None:                                  # the d <= eps branch: the term is exactly 1, the gradient exactly 0
        assert not r32["ginc"][:, far * sl:(far + 1) * sl].any()
        one = R.consistency(q[:, far * sl:(far + 1) * sl], k[:, far * sl:(far + 1) * sl], 1, [0], K.TWO_SIGMA, 1e-7, 0.5)
        assert one["value"][0] < nz                      # (sanity: a slice of its own is not 1)
        rest = np.delete(np.arange(nz * sl), np.arange(far * sl, (far + 1) * sl))
        sub = R.consistency(q[:, rest], k[:, rest], nz - 1, np.searchsorted(rest, idx), K.TWO_SIGMA, 1e-7, 0.5)
        assert got["value"][0] == sub["value"][0] + 1.0 or abs(got["value"][0] - sub["value"][0] - 1.0) < 1e-12
    j = R.judge(r32, got, r32, R.consistency_scale(q, k, nz, idx, K.TWO_SIGMA, 1e-7, 0.5))
    for kk, (ek, _, ok) in j.items():
        assert ok
        cap("cons." + kk, ek)


@pytest.mark.parametrize("shape,Kn", K.AFF)
def test_affinity_side_matches_torch_float64(shape, Kn):
    E = 3 if Kn != 32 else 9
    zero_only = (shape, Kn) == K.AFF[-1]
    emb, lbl, offs = K.aff_inputs(shape, Kn, E, Kn + shape[2], zero_only)
    te = t64(emb, True)
    val = spoco_ref.affinity_side_loss(te.reshape(1, E, *shape), torch.from_numpy(lbl).reshape(1, 1, *shape),
                                       [list(map(int, o)) for o in offs], float(f32(K.DELTA_DIST)))
    val.backward()
    got = R.affinity_side(emb, lbl, shape, offs, K.DELTA_DIST, 1e-7, 0.5)
    close(got["value"], [val.item()], "affinity value")
    close(got["ginc"], float(f32(0.5)) * te.grad.numpy(), "affinity gradient")
    r32 = R.affinity_side_f32(emb, lbl, shape, offs, K.DELTA_DIST, 1e-7, 0.5)
    if zero_only:                                        # n = d = 0: the loss is exactly 1 and the gradient exactly 0
        assert got["value"][0] == 1.0 and r32["value"][0] == 1.0 and not got["ginc"].any() and not r32["ginc"].any()
    j = R.judge(r32, got, r32, R.affinity_side_scale(emb, lbl, shape, offs, K.DELTA_DIST, 1e-7, 0.5))
    for kk, (ek, _, ok) in j.items():
        assert ok
        cap("aff." + kk, ek)


def test_label_ops_match_torch():
    rng = np.random.RandomState(3)
    for V in (1, 255, 1024, 1025, 70001):
        lbl = rng.randint(-3, 4, V).astype(np.int64)
        t = torch.from_numpy(lbl)
        assert R.label_range(lbl)["minmax"].tolist() == [int(t.min()), int(t.max())]
        zc = R.zero_count(lbl)
        nzr = torch.nonzero(t == 0)[:, 0].numpy()
        assert zc["total"][0] == nzr.size and zc["chunk_counts"].sum() == nzr.size and zc["chunk_counts"].size == -(-V // 1024)
        assert zc["chunk_counts"][0] == (lbl[:1024] == 0).sum()
        if nzr.size:
            ranks = [0, nzr.size - 1, nzr.size // 2]
            assert np.array_equal(R.zero_select(lbl, ranks)["idx"], nzr[ranks])


@pytest.mark.parametrize("name,N,alpha,beta,gamma", [("g6g_contrastive_2d", 3, 1.0, 0.7, 0.01), ("g6h_contrastive_3d", 2, 1.0, 0.7, 0.01)])
def test_composed_ops_match_contrastive_goldens(name, N, alpha, beta, gamma):
    """ContrastiveLoss(delta_var 0.5, delta_dist 1.5): cluster_means -> pull -> means_terms -> embed_grad, per sample"""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    total, grads = 0.0, []
    for b in range(N):
        emb, lbl = g["emb"][b].reshape(g["emb"].shape[1], -1), g["target"][b, 0].reshape(-1)
        C = int(lbl.max()) + 1
        assert np.array_equal(np.unique(lbl), np.arange(C))
        cm = R.cluster_means(emb, lbl, C)
        p = R.pull(emb, lbl, C, cm["means"], cm["counts"], 0.5)
        mt = R.means_terms(cm["means"], 1.5, 0)
        total += alpha * p["value"][0] / C + beta * mt["values"][0] + gamma * mt["values"][1]
        grads.append(R.embed_grad(emb, lbl, C, cm["means"], cm["counts"], p["S"], mt["ddist"], mt["dreg"], None, 0.5, C,
                                  alpha / N, beta / N, gamma / N, 0.0)["g"].reshape(g["emb"].shape[1:]))
    np.testing.assert_allclose(total / N, g["loss"][0], rtol=2e-6)
    # embed_grad rounds its weights to float32 as the C ABI does: 1 / 3 costs 3e-8
    assert np.linalg.norm(np.stack(grads) - g["grad"]) / np.linalg.norm(g["grad"]) < 2e-6


# ------------------------------------------------------------------------------------------ the cases and their census
@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", K.expand(), ids=[c[0] for c in K.expand()])
def test_census_equals_named_path(cid, name, E, C, V, plan, pad, want):
    lbl = K.make_labels(V, C, plan, 7)
    cen = K.census(lbl, E, C, V)
    print(cid, "->", K.check_path(cen, want))
    cnt = np.bincount(lbl, minlength=C)
    assert lbl.min() == 0 and lbl.max() < C and (V < C or (cnt > 0).all()), "every id occurs"
    assert cen["adds"].sum() == cen["uniform"] + 64 * cen["mixed"] + V % 64
    assert all(lbl[v] == 0 for v in K.anchors(V))
    if V >= 64 and C >= 4:
        u = C - 2
        assert cnt[u] % 64 == 0 and cen["adds"][u] == cnt[u] // 64, "label C - 2 is counted by += 64 only"
        if V % 64:
            where = np.nonzero(lbl == C - 1)[0]
            assert where.size and where.min() >= V // 64 * 64, "label C - 1 lives only in the tail"
    if name == "global":
        assert C * (E + 1) == 6600 > 6144
    if name == "capped":
        assert cen["grid"] * 256 == 262144 < V and cen["iters"] == 2


def test_census_of_the_embed_grad_cap():
    V = 524288 + 101
    cen = K.census(K.make_labels(V, 6, "UUUSRBUU", 1), 3, 6, V)
    assert cen["grid_grad"] == 2048 and cen["twice_grad"] and cen["twice"]


@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", SMALL, ids=IDS)
def test_anchors_contribute_order_one(cid, name, E, C, V, plan, pad, want):
    d = K.case_data(name, E, C, V, plan)
    for v in K.anchors(V):
        e = d["emb"][:, v].astype(f64)
        assert V == 1 or np.linalg.norm(e - d["means"][0]) >= K.DELTA_VAR + 1.0, "the pull anchor (V = 1: the voxel is its mean)"
        if (d["counts"][1:] > 0).any():
            dist = np.linalg.norm(e[None] - d["means"][1:][d["counts"][1:] > 0], axis=1)
            assert K.DELTA_DIST - dist.min() >= 0.5, "the push anchor"


ONE_PER_LAYOUT = [c for c in K.expand() if c[6] == K.CASES[c[1]][4][0] and c[4] > 1]


@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", ONE_PER_LAYOUT, ids=[c[0] for c in ONE_PER_LAYOUT])
def test_a_dropped_last_voxel_costs_many_units(cid, name, E, C, V, plan, pad, want):
    """What the anchors buy, in units of the judge (the kernel is allowed 4 where the restatement stays below 1): the means,
    S and dpush lose at least 25 times that (100 units) in every case, the push value at least 5 times (29 units in `capped`).  The pull VALUE sees the voxel only where a label's
    share of the sum is large enough: >= 100 units in the small cases, 7 in `capped` (one voxel among 33000 of its label),
    and nothing in `global` (2e-8 of the sum of 200 labels' terms at E = 32) -- there S and the means carry the check."""
    d = K.case_data(name, E, C, V, plan)
    lbl, emb, cen = d["lbl"], d["emb"], d["census"]
    safe = np.maximum(d["counts"], 1)
    keep = np.arange(V) != V - 1
    a = (emb, lbl, C, d["means"], safe, K.DELTA_VAR)
    ref, sc = R.pull(*a), R.pull_scale(*a)
    cut = R.pull(emb[:, keep], lbl[keep], C, d["means"], safe, K.DELTA_VAR)
    uv = R.units(cut["value"], ref["value"], sc["value"])
    us = R.units(cut["S"], ref["S"], sc["S"], R.pull_allow(cen["adds"])["S"])
    cm, scm = R.cluster_means(emb, lbl, C), R.cluster_means_scale(emb, lbl, C)
    short = (R._seg_sum(emb[:, keep].astype(f64), lbl[keep], C, f64) / safe).T
    um = R.units(short, cm["means"], scm["means"], R.cluster_means_allow(cen["adds"], d["counts"])["means"])
    print(f"SPOCO_DROP {cid}: pull value {uv:.0f} S {us:.0f} means {um:.0f}")
    assert us >= 25 * R.MARGIN and um >= 25 * R.MARGIN
    assert uv >= {"capped": 1.5, "global": 0.0}.get(name, 25.0) * R.MARGIN
    if name != "global":
        b = (emb, lbl, C, d["means"], d["counts"], K.DELTA_DIST, 0.75)
        pr, ps = R.push(*b), R.push_scale(*b)
        pc = R.push(emb[:, keep], lbl[keep], C, d["means"], d["counts"], K.DELTA_DIST, 0.75)
        up = R.units(pc["value"], pr["value"], ps["value"])
        ud = R.units(pc["dpush"], pr["dpush"], ps["dpush"], R.push_allow(cen["bg_waves"], C, d["counts"])["dpush"])
        print(f"SPOCO_DROP {cid}: push value {up:.0f} dpush {ud:.0f}")
        assert up >= 5 * R.MARGIN and ud >= 25 * R.MARGIN


# ------------------------------------------------------------------------------------------ the restatement's level
@pytest.mark.parametrize("cid,name,E,C,V,plan,pad,want", SMALL, ids=IDS)
def test_float32_restatement_stays_under_its_caps(cid, name, E, C, V, plan, pad, want):
    d = K.case_data(name, E, C, V, plan)
    lbl, emb, mu, cn = d["lbl"], d["emb"], d["means"], np.maximum(d["counts"], 1)
    seen = {}

    def level(prefix, f64fn, f32fn, scfn, *a):
        ref, r32, sc = f64fn(*a), f32fn(*a), scfn(*a)
        for k, (ek, _, ok) in R.judge(r32, ref, r32, sc).items():
            key = "means" if k == "means" else f"{prefix}.{k}"
            if key in CAPS:
                seen[key] = ek
                cap(key, ek)
        return ref

    level("cm", R.cluster_means, R.cluster_means_f32, R.cluster_means_scale, emb, lbl, C)
    p = level("pull", R.pull, R.pull_f32, R.pull_scale, emb, lbl, C, mu, cn, K.DELTA_VAR)
    ps = level("push", R.push, R.push_f32, R.push_scale, emb, lbl, C, mu, d["counts"], K.DELTA_DIST, 0.75)
    mt = R.means_terms(mu, K.DELTA_DIST, 1)
    if V > 1:
        args = (emb, lbl, C, mu, cn, p["S"].astype(f32), mt["ddist"].astype(f32), mt["dreg"].astype(f32),
                ps["dpush"].astype(f32), K.DELTA_VAR, W["n_inst"], W["w_var"], W["w_dist"], W["w_reg"], W["w_push"])
        level("eg", R.embed_grad, R.embed_grad_f32, R.embed_grad_scale, *args)
    print("SPOCO_E32", cid, " ".join(f"{k} {v:.2f}" for k, v in seen.items()))


# ------------------------------------------------------------------------------------------ the judge rejects wrong outputs
def _waves():
    _, name, E, C, V, plan, pad, want = K.expand(("waves",))[0]
    return K.case_data(name, E, C, V, plan), E, C, V


def _rejects(j):
    return not all(ok for _, _, ok in j.values())


def _cm_judge(got, d, E, C, V):
    ref = R.cluster_means(d["emb"], d["lbl"], C)
    r32 = R.cluster_means_f32(d["emb"], d["lbl"], C)
    return R.judge(got, ref, r32, R.cluster_means_scale(d["emb"], d["lbl"], C),
                   R.cluster_means_allow(d["census"]["adds"], d["counts"]))


def test_judge_accepts_the_restatement_and_rejects_a_dropped_last_voxel():
    d, E, C, V = _waves()
    assert not _rejects(_cm_judge(R.cluster_means_f32(d["emb"], d["lbl"], C), d, E, C, V))
    lbl2 = d["lbl"][:-1]
    wrong = R.cluster_means_f32(d["emb"][:, :-1], lbl2, C)
    wrong["counts"] = R.cluster_means(d["emb"], d["lbl"], C)["counts"].astype(f32)      # even with the right count
    wrong["means"] = (wrong["means"] * (np.bincount(lbl2, minlength=C) / d["counts"])[:, None]).astype(f32)
    assert _rejects(_cm_judge(wrong, d, E, C, V))
    args = (d["emb"], d["lbl"], C, d["means"], d["counts"], K.DELTA_VAR)
    ref, r32, sc = R.pull(*args), R.pull_f32(*args), R.pull_scale(*args)
    al = R.pull_allow(d["census"]["adds"])
    assert not _rejects(R.judge(r32, ref, r32, sc, al))
    keep = np.arange(V) != V - 1
    cut = R.pull(d["emb"][:, keep], d["lbl"][keep], C, d["means"], d["counts"], K.DELTA_VAR)
    j = R.judge(cut, ref, r32, sc, al)
    assert not j["value"][2] and not j["S"][2], "a dropped tail voxel shows in the value and in S_0"
    assert j["value"][0] >= 10 * R.MARGIN, "and by a wide margin"


def test_judge_rejects_a_dropped_uniform_wave_and_a_low_count():
    d, E, C, V = _waves()
    lbl, emb = d["lbl"], d["emb"].astype(f64)
    full = lbl[:V // 64 * 64].reshape(-1, 64)
    w = int(np.nonzero((full == full[:, :1]).all(1) & (full[:, 0] == C - 2))[0][0])
    l = C - 2
    ref = R.cluster_means(emb, lbl, C)
    wrong = {k: v.copy() for k, v in ref.items()}
    wrong["means"][l] -= emb[:, 64 * w:64 * w + 64].sum(1) / ref["counts"][l]
    assert _rejects(_cm_judge(wrong, d, E, C, V))
    low = {k: v.copy() for k, v in ref.items()}
    k = int((full[(full == full[:, :1]).all(1)][:, 0] == l).sum())
    low["counts"][l] -= k                                       # count += 63 per uniform wave
    low["means"][l] *= ref["counts"][l] / low["counts"][l]
    j = _cm_judge(low, d, E, C, V)
    assert not j["counts"][2] and not j["means"][2]


def test_judge_rejects_swapped_channels():
    d, E, C, V = _waves()
    wrong = R.cluster_means(d["emb"], d["lbl"], C)
    wrong["means"] = wrong["means"][:, [1, 0] + list(range(2, E))]
    assert not _cm_judge(wrong, d, E, C, V)["means"][2]


def test_judge_rejects_push_gradient_errors():
    d, E, C, V = _waves()
    args = (d["emb"], d["lbl"], C, d["means"], d["counts"], K.DELTA_DIST, 0.75)
    ref, r32, sc = R.push(*args), R.push_f32(*args), R.push_scale(*args)
    al = R.push_allow(d["census"]["bg_waves"], C, d["counts"])
    assert not _rejects(R.judge(r32, ref, r32, sc, al))
    bg = np.nonzero((d["lbl"] == 0) & (np.abs(ref["ginc"]).sum(0) > 0))[0]
    wrong = {k: v.copy() for k, v in ref.items()}
    wrong["ginc"][:, bg[len(bg) // 2]] = 0                     # one background voxel's gradient missing
    assert not R.judge(wrong, ref, r32, sc, al)["ginc"][2]
    before = (1.2 * np.random.RandomState(1).randn(E, V)).astype(f32)
    after = (before + ref["ginc"].astype(f32)).astype(f32)
    fg = d["lbl"] != 0
    assert R.untouched(before, after, fg)
    v = int(np.nonzero(fg)[0][3])
    after[1, v] = np.nextafter(after[1, v], f32(np.inf))        # a non-background voxel changed by one ulp
    assert not R.untouched(before, after, fg)


def test_judge_rejects_anchor_errors_of_the_consistency_gradient():
    nz, sl, E, A = K.CONS[0]
    q, k, idx, _ = K.cons_inputs(nz, sl, E, A, A + sl)
    assert idx[1] == idx[2] and idx[0] == 0 and idx[1] == nz * sl - 1
    args = (q, k, nz, idx, K.TWO_SIGMA, 1e-7, 0.5)
    ref, r32, sc = R.consistency(*args), R.consistency_f32(*args), R.consistency_scale(*args)
    assert not _rejects(R.judge(r32, ref, r32, sc))
    wrong = {k_: v.copy() for k_, v in ref.items()}
    wrong["ginc"][:, idx[3]] *= 0.5                            # half of one anchor voxel's gradient
    assert not R.judge(wrong, ref, r32, sc)["ginc"][2]
    # the duplicate anchor counted once
    once = R.consistency(q, k, nz, np.delete(idx, 2), K.TWO_SIGMA, 1e-7, 0.5)
    assert _rejects(R.judge(once, ref, r32, sc))
    dup = {k_: v.copy() for k_, v in ref.items()}
    dup["ginc"][:, idx[1]] = once["ginc"][:, idx[1]]           # only the scatter to the doubled voxel is short
    assert not R.judge(dup, ref, r32, sc)["ginc"][2]


def test_judge_rejects_a_missing_anchor_scatter():
    """the gradient with every anchor voxel's scattered part left out: each voxel keeps only its own terms"""
    nz, sl, E, A = K.CONS[0]
    q, k, idx, _ = K.cons_inputs(nz, sl, E, A, A + sl)
    args = (q, k, nz, idx, K.TWO_SIGMA, 1e-7, 0.5)
    ref, r32, sc = R.consistency(*args), R.consistency_f32(*args), R.consistency_scale(*args)
    wrong = R.consistency(*args, scatter=False)
    other = np.setdiff1d(np.arange(nz * sl), idx)
    assert np.array_equal(wrong["ginc"][:, other], ref["ginc"][:, other]) and wrong["value"] == ref["value"]
    assert not R.judge(wrong, ref, r32, sc)["ginc"][2]


def test_judge_rejects_an_index_off_by_one_and_a_nonzero_dreg_of_the_zero_row():
    lbl = np.random.RandomState(2).randint(0, 3, 3000).astype(np.int64)
    ref = R.zero_select(lbl, [0, 5, 100])
    wrong = {"idx": ref["idx"] + np.array([0, 0, 1])}
    assert not R.judge(wrong, ref, None, {"idx": None})["idx"][2] and R.judge(ref, ref, None, {"idx": None})["idx"][2]
    mu = K.means_case(10, 3, 1)
    a = (mu, K.DELTA_DIST, 1)
    ref, r32, sc = R.means_terms(*a), R.means_terms_f32(*a), R.means_terms_scale(*a)
    assert not _rejects(R.judge(r32, ref, r32, sc))
    wrong = {k: v.copy() for k, v in ref.items()}
    wrong["dreg"][5, 0] = 1e-30
    assert not R.judge(wrong, ref, r32, sc)["dreg"][2]
