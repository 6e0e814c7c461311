"""Inputs that reach every dispatch path of csrc/spoco.hip, and a census that proves it (TEST INFRASTRUCTURE; shared by
tests/test_spoco_cpu.py and tests/test_gpu_spoco_ops.py).

make_labels(V, C, plan) builds a label row wave by wave (64 voxels): `plan` is a string over U S R B, repeated over the full
waves.
  U  uniform, one label          S  split into two labels at lane 1, 32 or 63 (in turn)
  R  a label per voxel           B  all background (label 0)
and a tail of V % 64 voxels of one label.  Every id in [0, C) occurs when V >= C.  With full waves and C >= 4, label C - 2
lives ONLY in U waves (its count comes only from `+= 64`) and, with a tail, label C - 1 lives ONLY in the tail.
The LAST voxel of the volume and the first voxel of its last wave are ANCHORS: label 0, embedding (delta_var + 1.2, 0, ...),
which is >= delta_var + 1 from the background mean (the pull) and inside delta_dist of every foreground mean (the push) for
the DELTA_VAR / DELTA_DIST below; tests/test_spoco_cpu.py asserts both.  A dropped tail then costs terms of order 1.

census(lbl, E, C, V) restates the dispatch conditions of tem_spoco_cluster_means / _pull / _push / _embed_grad from the
arguments a test passes; CASES names the path each case is meant to reach and `check_path` fails a case that takes another.
"""
import numpy as np

from . import spoco_op_ref as R

f32 = np.float32
DELTA_VAR, DELTA_DIST = 0.5, 2.5
TWO_SIGMA = DELTA_VAR * DELTA_VAR / -np.log(0.9)
SPLITS = (1, 32, 63)


def make_labels(V, C, plan, seed=0):
    rng = np.random.RandomState(seed)
    nw, tail = V // 64, V % 64
    lbl = np.zeros(V, np.int64)
    if nw == 0:                                           # a tail-only volume: the ids in turn, background first and last
        lbl[:] = np.arange(V) * C // max(V, 1)
        lbl[-1] = 0
        return lbl
    special = C >= 4
    u_only = C - 2 if special else None
    t_only = C - 1 if special and tail else None
    free = [l for l in range(1, C) if l not in (u_only, t_only)] or [0]
    kinds = [plan[w % len(plan)] for w in range(nw)]
    assert not special or "U" in kinds
    todo = list(free)                                     # ids still to place: R waves take them first
    ui, si = 0, 0
    first_u = True
    for w, kd in enumerate(kinds):
        s = slice(64 * w, 64 * w + 64)
        if kd == "B":
            lbl[s] = 0
        elif kd == "U":
            lbl[s] = u_only if (first_u and special) else free[ui % len(free)]
            ui += 0 if (first_u and special) else 1
            first_u = False
        elif kd == "S":
            a, b = free[si % len(free)], free[(si + 1) % len(free)] if len(free) > 1 else 0
            lbl[s] = a
            lbl[64 * w + SPLITS[si % 3]:64 * w + 64] = b
            si += 1
        else:
            row = rng.choice(free, 64)
            k = min(len(todo), 64)
            row[:k] = todo[:k]
            del todo[:k]
            lbl[s] = rng.permutation(row)
    if tail:
        lbl[64 * nw:] = t_only if t_only is not None else free[0]
    for v in anchors(V):
        lbl[v] = 0
    return lbl


def anchors(V):
    return sorted({V - 1, 64 * ((V - 1) // 64)})


def make_embeddings(E, V, seed):
    """1.2 randn with the anchor voxels planted"""
    e = (1.2 * np.random.RandomState(seed).randn(E, V)).astype(f32)
    for v in anchors(V):
        e[:, v] = 0.0
        e[0, v] = DELTA_VAR + 1.2
    return e


def grid_1d(V, cap):
    return int(min(max(-(-V // 256), 1), cap))


def census(lbl, E, C, V):
    lbl = np.asarray(lbl).reshape(-1)
    assert lbl.size == V and lbl.min() >= 0 and lbl.max() < C
    nw, tail = V // 64, V % 64
    full = lbl[:nw * 64].reshape(nw, 64)
    uni = (full == full[:, :1]).all(1) if nw else np.zeros(0, bool)
    adds = np.bincount(full[uni][:, 0], minlength=C) + np.bincount(full[~uni].reshape(-1), minlength=C) + \
        np.bincount(lbl[nw * 64:], minlength=C)
    waves = -(-V // 64)
    pad = np.ones(waves * 64, bool)
    pad[:V] = lbl != 0
    nb, nbg = grid_1d(V, R.SP_MAXB), grid_1d(V, 2048)
    return {
        "EM": 8 if E <= 8 else (16 if E <= 16 else 32),
        "use_lds": C * (E + 1) * 8 <= 48 * 1024,
        "grid": nb, "twice": waves * 64 > nb * 256, "iters": -(-waves * 64 // (nb * 256)),
        "grid_grad": nbg, "twice_grad": V > nbg * 256,
        "uniform": int(uni.sum()), "mixed": int((~uni).sum()), "tail": int(tail > 0),
        "background": int((uni & (full[:, 0] == 0)).sum()) if nw else 0,
        "no_bg_waves": int(pad.reshape(waves, 64).all(1).sum()),          # waves k_push skips
        "bg_waves": int((~pad.reshape(waves, 64).all(1)).sum()),
        "adds": adds.astype(np.int64),                                     # fixed-point adds per label and channel
        "counts": np.bincount(lbl, minlength=C),
    }


def check_path(cen, want):
    """want: {key: value | "some" | "none"}; a case that silently takes another path fails"""
    for k, v in want.items():
        got = cen[k]
        ok = got > 0 if v == "some" else (got == 0 if v == "none" else got == v)
        assert ok, f"meant to reach {k} = {v}, the arguments select {k} = {got}"
    return " ".join(f"{k}={cen[k]}" for k in ("EM", "use_lds", "grid", "iters", "uniform", "mixed", "tail", "background"))


# name: (E list, C, V list, plan, pad list (cs = gcs = V + pad), the path it is meant to reach)
CASES = {
    "tiny": ((3,), 2, (1, 37), "U", (0,),
             dict(EM=8, use_lds=True, twice=False, uniform="none", mixed="none", tail=1)),
    "waves": ((3, 8), 5, (64 * 12 + 37,), "USRBUSRBSSRU", (0, 24),
              dict(EM=8, use_lds=True, twice=False, uniform="some", mixed="some", tail=1, background="some")),
    "em16": ((9, 16), 9, (64 * 16,), "USRBUSRRSSRUBRSU", (24,),
             dict(EM=16, use_lds=True, twice=False, uniform="some", mixed="some", tail=0, background="some")),
    "em32": ((17, 32), 9, (64 * 16 + 5,), "USRBUSRRSSRUBRSU", (0,),
             dict(EM=32, use_lds=True, twice=False, uniform="some", mixed="some", tail=1, background="some")),
    "global": ((32,), 200, (64 * 260 + 5,), "RRRRUSBU", (0,),
               dict(EM=32, use_lds=False, twice=False, uniform="some", mixed="some", tail=1, background="some")),
    "capped": ((3,), 6, (262144 + 64 * 3 + 37,), "UUUSRBUU", (0,),
               dict(EM=8, use_lds=True, grid=R.SP_MAXB, twice=True, iters=2, uniform="some", mixed="some", tail=1,
                    background="some")),
}


def expand(names=None):
    """-> [(id, name, E, C, V, plan, pad, want)]"""
    out = []
    for name, (Es, C, Vs, plan, pads, want) in CASES.items():
        if names is not None and name not in names:
            continue
        for E in Es:
            for V in Vs:
                for pad in pads:
                    out.append((f"{name}-E{E}-V{V}-cs+{pad}", name, E, C, V, plan, pad, want))
    return out


_CACHE = {}


def case_data(name, E, C, V, plan):
    """labels, embeddings, the census and the float32-rounded float64 oracle values that feed the later ops (a one-step
    error without drift); computed once, shared, left unchanged"""
    key = (name, E, C, V)
    if key not in _CACHE:
        if len(_CACHE) > 6:
            _CACHE.clear()
        seed = sum(map(ord, name)) * 31 + E
        lbl = make_labels(V, C, plan, seed)
        emb = make_embeddings(E, V, seed + 1)
        cm = R.cluster_means(emb, lbl, C)
        means, counts = cm["means"].astype(f32), cm["counts"].astype(f32)
        d = dict(lbl=lbl, emb=emb, census=census(lbl, E, C, V), means=means, counts=counts)
        for a in (lbl, emb, means, counts):
            a.setflags(write=False)
        _CACHE[key] = d
    return _CACHE[key]


def means_case(C, E, seed):
    """[C, E] float32 means with the planted edges: two coincident foreground means, a foreground mean equal to mean 0, an
    all-zero row, a pair just inside and a pair just outside 2 delta_dist (as far as C has rows for them)"""
    rng = np.random.RandomState(seed)
    mu = (1.5 * rng.randn(C, E)).astype(f32)
    if C >= 3:
        mu[2] = mu[1]                                     # coincident foreground pair
    if C >= 5:
        mu[4] = mu[0]                                     # a foreground mean on the background mean
    if C >= 6:
        mu[5] = 0.0                                       # zero norm
    for a, b, fac in ((6, 7, 1.0 - 2e-6), (8, 9, 1.0 + 2e-6)):
        if C > b:
            u = rng.randn(E)
            mu[b] = (mu[a].astype(np.float64) + u / np.linalg.norm(u) * 2.0 * DELTA_DIST * fac).astype(f32)
    return mu


def far_slice(e, nz, z, idx, dist=40.0):
    """move slice z of e [E, V] at least `dist` away from every anchor embedding (the anchors are outside the slice)"""
    V = e.shape[1]
    sl = V // nz
    assert all(not (z * sl <= i < (z + 1) * sl) for i in idx)
    e = e.copy()
    e[0, z * sl:(z + 1) * sl] = np.abs(e[0]).max() + dist + np.abs(e[0, z * sl:(z + 1) * sl])
    return e


# ------------------------------------------------------------------------------------------ inputs of the volume ops
IDICE = [(1, 805), (5, 3), (4, 64 * 3 + 7)]


def volume(nz, sl, C, E, seed):
    """-> (labels [nz * sl], embeddings [E, nz * sl]) of the instance Dice cases"""
    V = nz * sl
    rng = np.random.RandomState(seed)
    lbl = rng.randint(0, C, V).astype(np.int64)
    lbl[:min(C, V)] = np.arange(min(C, V))               # every id that fits occurs ...
    if C > 2 and nz > 1:
        lbl[:sl][lbl[:sl] == C - 1] = 0                  # ... and one label is absent from slice 0
        lbl[sl] = C - 1
    emb = (1.2 * rng.randn(E, V)).astype(f32)
    return lbl, emb


def cons_inputs(nz, sl, E, A, seed):
    """-> (q, k [E, V], anchor voxel indices [A], far): the anchors hold voxel 0, the last voxel and (A >= 3) one voxel twice;
    with nz >= 3, slice `far` holds no anchor and lies >= 40 from all of them in q and in k (both pmaps underflow)"""
    V = nz * sl
    rng = np.random.RandomState(seed)
    q = (1.2 * rng.randn(E, V)).astype(f32)
    k = (q + 0.3 * rng.randn(E, V)).astype(f32)
    far = nz - 2 if nz >= 3 else None                    # a slice with no anchor, far from all of them
    pool = [v for v in range(V) if far is None or not (far * sl <= v < (far + 1) * sl)]
    idx = [0, V - 1 if far != nz - 1 else pool[-1]] + [pool[i] for i in rng.randint(0, len(pool), max(A - 2, 0))]
    idx = idx[:A]
    if A >= 3:
        idx[2] = idx[1]                                  # the same voxel drawn twice
    idx = np.array(idx, np.int64)
    if far is not None:
        q, k = far_slice(q, nz, far, idx), far_slice(k, nz, far, idx)
    return q, k, idx, far


CONS = [(1, 805, 3, 9), (6, 5, 9, 1), (3, 64 * 9, 17, 64), (6, 5, 3, 9)]


OFFS = [(0, 0, 0), (0, 1, 0), (0, 0, -1), (1, 0, 0), (-1, -1, 1), (0, 9, 0), (0, 0, 11), (0, -12, 3), (0, 5, -80),
        (2, -3, 4), (-3, 0, 0), (0, 40, 0), (0, 0, 48), (1, 39, -47), (0, 2, 2), (0, -2, 5), (0, 7, -7), (1, 1, 1)]
AFF = [((1, 9, 11), 8), ((3, 5, 7), 32), ((1, 1, 70), 8), ((2, 40, 48), 1), ((1, 9, 11), 1)]


def aff_inputs(shape, Kn, E, seed, zero_only=False):
    """-> (embeddings, labels in runs of 3, offsets int32 [Kn, 3] from OFFS: 0, +-1, equal to and beyond the extents, mixed
    signs; z offsets 0 for D = 1); zero_only: the zero offset alone"""
    V = int(np.prod(shape))
    rng = np.random.RandomState(seed)
    lbl = np.repeat(rng.randint(0, 4, -(-V // 3)), 3)[:V].astype(np.int64)
    emb = (0.8 * rng.randn(E, V)).astype(f32)
    offs = [(0, 0, 0)] if zero_only else [OFFS[(i + (0 if Kn > 1 else 1)) % len(OFFS)] for i in range(Kn)]
    if shape[0] == 1:
        offs = [(0, o[1], o[2]) for o in offs]
    return emb, lbl, np.array(offs, np.int32)
