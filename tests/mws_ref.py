"""The numpy oracle of the mutex watershed (TEST INFRASTRUCTURE; numpy only).

The contract (DESIGN.md "Mutex watershed"): nodes = the voxels inside the mask; edge (c, v) joins v and u = v + offsets[c]
when u is inside the sample, both ends are inside the mask and edge_valid[c, v] is set; its id is c * V + v.  The priority is
p = 1 - aff (float32) for the n_attractive leading channels and p = aff for the others, -0.0 tied with 0.0; edges are taken
by p descending, ties by the lower id.  An attractive edge merges its clusters unless they are one or mutually exclusive
(the union inherits the mutexes); a repulsive edge between two clusters makes them mutually exclusive.  Labels: 0 outside
the mask, else 1..n in raster order of each cluster's first voxel.

  edges        the existing edges of one sample -> (channel, v, u), in ascending id order
  priorities   p per edge, float32
  keys         the 64-bit key of the contract: ordered uint32 of p << 32 | 0xffffffff - id; the larger key goes first
  sequential   (a) Kruskal with mutex constraints: a stable descending sort, union-find, mutex sets
  schedule     (b) the rounds of csrc/mws.hip, simulated: mutex set / pick / veto / commit (R1-R3) / flatten
               -> (labels, rounds that did work)
  np_mutex_watershed_segmentation   the public function restated on top of (a) and watershed_ref.np_size_filter

Every function takes ONE sample: aff [C, *spatial] with 2 or 3 spatial axes; labels come back as int64 in the spatial shape."""
import numpy as np

OPEN, MUTEX, DEAD = 1, 2, 0


def _prep(aff, offsets, mask, edge_valid):
    aff = np.asarray(aff, dtype=np.float32)
    shape = aff.shape[1:]
    s3 = (1,) * (3 - len(shape)) + tuple(shape)
    C, V = aff.shape[0], int(np.prod(s3))
    offs = [(0,) * (3 - len(o)) + tuple(int(x) for x in o) for o in offsets]
    assert len(offs) == C and all(len(o) == 3 for o in offs)
    m = np.ones(V, bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    ev = np.ones((C, V), bool) if edge_valid is None else np.asarray(edge_valid, bool).reshape(C, V)
    assert m.size == V
    return aff.reshape(C, V), offs, m, ev, s3, shape


def edges(s3, offs, m, ev):
    """-> (c, v, u) int64 arrays of the existing edges, ascending in the id c * V + v"""
    D, H, W = s3
    V = D * H * W
    z, y, x = (a.ravel() for a in np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"))
    cs, vs, us = [], [], []
    for c, (dz, dy, dx) in enumerate(offs):
        zz, yy, xx = z + dz, y + dy, x + dx
        ok = (zz >= 0) & (zz < D) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        u = np.where(ok, (zz * H + yy) * W + xx, 0)
        ok &= m & m[u] & ev[c]
        v = np.flatnonzero(ok)
        cs.append(np.full(v.size, c, np.int64))
        vs.append(v)
        us.append(u[v])
    assert len(offs) * V < 2 ** 32 - 1
    return np.concatenate(cs), np.concatenate(vs), np.concatenate(us)


def priorities(aff, c, v, n_attractive):
    a = aff[c, v]
    return (np.where(c < n_attractive, np.float32(1) - a, a) + np.float32(0)).astype(np.float32)


def keys(p, ids):
    b = np.asarray(p, np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(b & np.uint64(0x80000000), b ^ np.uint64(0xffffffff), b | np.uint64(0x80000000))
    return (o << np.uint64(32)) | (np.uint64(0xffffffff) - ids.astype(np.uint64))


def _number(root, m, shape):
    """roots (the smallest voxel of each cluster) -> 1..n in ascending order of the root, 0 outside the mask"""
    ids = np.unique(root[m])
    return np.where(m, np.searchsorted(ids, root) + 1, 0).astype(np.int64).reshape(shape)


def sequential(aff, offsets, n_attractive, mask=None, edge_valid=None):
    aff, offs, m, ev, s3, shape = _prep(aff, offsets, mask, edge_valid)
    V = aff.shape[1]
    c, v, u = edges(s3, offs, m, ev)
    p = priorities(aff, c, v, n_attractive)
    by = np.argsort(-p, kind="stable")            # descending, ties by the lower id (the arrays ascend in the id)
    assert np.array_equal(by, np.argsort(~keys(p, c * V + v), kind="stable")), "the 64-bit key orders the edges the same way"
    par = np.arange(V)
    mut = {}

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for ce, a, b in zip(c[by].tolist(), v[by].tolist(), u[by].tolist()):
        a, b = find(a), find(b)
        if a == b:
            continue
        if ce >= n_attractive:
            mut.setdefault(a, set()).add(b)
            mut.setdefault(b, set()).add(a)
            continue
        if b in mut.get(a, ()):
            continue
        r, s = min(a, b), max(a, b)               # the root of a cluster is its smallest voxel
        par[s] = r
        for t in mut.pop(s, ()):
            mut[t].discard(s)
            mut[t].add(r)
            mut.setdefault(r, set()).add(t)
    root = np.array([find(x) for x in range(V)])
    return _number(root, m, shape)


def schedule(aff, offsets, n_attractive, mask=None, edge_valid=None, mutual_only=False, partners=True):
    """the kernel's rounds, one after the other -> (labels, rounds that did work).  mutual_only: the schedule without R1's
    and R3's head start (a repulsive edge commits only when both ends picked it, hooks only by R2): slower, the same result.
    partners=False: R3 only for roots without any mutex (no veto pass): slower as well, the same result"""
    aff, offs, m, ev, s3, shape = _prep(aff, offsets, mask, edge_valid)
    V = aff.shape[1]
    c, v, u = edges(s3, offs, m, ev)
    key = keys(priorities(aff, c, v, n_attractive), c * V + v)
    slot = {int(k): i for i, k in enumerate(key.tolist())}
    assert len(slot) == key.size, "keys are pairwise distinct"
    state = np.full(key.size, OPEN, np.uint8)
    comp = np.arange(V)
    rounds = 0
    while True:
        # 1. the mutex set of this round and the roots that have a mutex
        mx = state == MUTEX
        ra, rb = comp[v[mx]], comp[u[mx]]
        assert (ra != rb).all(), "mutually exclusive clusters never merge"
        pairs = np.unique(np.minimum(ra, rb) * V + np.maximum(ra, rb))
        pairset = set(pairs.tolist())
        has = np.zeros(V, bool)
        has[ra] = True
        has[rb] = True
        # 2. pick
        op = np.flatnonzero(state == OPEN)
        A, B = comp[v[op]], comp[u[op]]
        gone = (A == B) | np.isin(np.minimum(A, B) * V + np.maximum(A, B), pairs)
        state[op[gone]] = DEAD
        op, A, B = op[~gone], A[~gone], B[~gone]
        if op.size == 0:
            break
        rounds += 1
        assert rounds <= key.size + 1
        best = np.zeros(V, np.uint64)
        np.maximum.at(best, A, key[op])
        np.maximum.at(best, B, key[op])
        # 3. commit.  veto: a root whose best edge is attractive and leads to a cluster that is NOT mutually exclusive with
        # every one of the root's own mutex partners (found edge by edge: each mutex edge asks for both of its ends)
        veto = np.zeros(V, bool) if partners else has.copy()
        for x, y in ((ra, rb), (rb, ra)) if partners else ():
            k = best[x]
            live = np.flatnonzero(k != 0)
            for i in live.tolist():
                e = slot[int(k[i])]
                if c[e] >= n_attractive:
                    continue
                p, q = int(comp[v[e]]), int(comp[u[e]])
                far = q if p == x[i] else p
                lo, hi = min(far, int(y[i])), max(far, int(y[i]))
                if far == y[i] or lo * V + hi not in pairset:
                    veto[x[i]] = True
        nxt = comp.copy()
        for a in np.flatnonzero(best).tolist():
            e = slot[int(best[a])]
            x, y = int(comp[v[e]]), int(comp[u[e]])
            b = y if x == a else x
            assert a in (x, y) and a != b
            if c[e] >= n_attractive:
                if not mutual_only or best[b] == best[a]:
                    state[e] = MUTEX                              # R1
            elif best[b] == best[a]:
                state[e] = DEAD                                   # R2: the larger root hooks to the smaller
                if a > b:
                    nxt[a] = b
            elif not veto[a] and not mutual_only:
                nxt[a] = b                                        # R3
        # 4. flatten, commit
        while True:
            up = nxt[nxt]
            if np.array_equal(up, nxt):
                break
            nxt = up
        comp = nxt[comp]
    first = np.full(V, V, np.int64)                               # the smallest voxel of each cluster
    np.minimum.at(first, comp, np.arange(V))
    return _number(first[comp], m, shape), rounds


def grid_edge_valid(shape, offsets, n_attractive, strides):
    """the grid rule of the subsampling helper: attractive channels whole, a repulsive edge where every coordinate is a
    multiple of its stride -> bool [C, *shape]"""
    ev = np.zeros((len(offsets),) + tuple(shape), bool)
    ev[:n_attractive] = True
    ev[(slice(n_attractive, None),) + tuple(slice(None, None, int(s)) for s in strides)] = True
    return ev


def np_mutex_watershed_segmentation(foreground, affinities, offsets, edge_valid, min_size=50, threshold=0.5):
    """mutex_watershed_segmentation behind its draw: `edge_valid` is what the subsampling helper returned"""
    import watershed_ref as R
    fg = np.asarray(foreground, np.float32)
    aff = np.asarray(affinities, np.float32)
    seg = sequential(aff, offsets, fg.ndim, fg >= np.float32(threshold), edge_valid)
    return R.np_size_filter(seg, min_size, aff, True)
