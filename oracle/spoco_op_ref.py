"""Float64 references of the SPOCO loss kernels (csrc/spoco.hip), one per C-ABI entry point (TEST INFRASTRUCTURE, see
oracle/__init__.py).

Written from the formulas of include/tem_hip.h and of oracle/spoco_ref.py; plain numpy, no code shared with the kernels.
tests/test_spoco_cpu.py pins the float64 functions to torch float64 autograd over oracle/spoco_ref.py and to the g6* goldens
and tests the judge on deliberately wrong outputs; tests/test_gpu_spoco_ops.py judges the kernels with them.

Embeddings are LOGICAL arrays [E, V] (whatever channel stride the kernel reads), labels int64 [V] in [0, C).

Every op is ONE function `op(..., dt)`: dt = numpy.float64 is the reference; dt = numpy.float32 is the float32 restatement
(`*_f32`): the same formula with every array and constant in float32, one rounding per operation, sums in numpy's pairwise
order.  It is a yardstick for the error level of plain fp32 arithmetic, not a copy of the kernel's order.  Each returns a
dict: exactly the quantities the call writes.  `*_scale` returns a dict with the same keys: the per-element scale of the
judge, or None for a quantity that must be exact.

The scale rule.  An element's scale is the float64 sum of the absolute values of its terms.  Every difference a - b the
kernel forms in fp32 counts as |a| + |b|: e - mu (so a distance d has the scale ds = |(|e| + |mu|)|_2 >= d), d - delta_var,
delta_dist - d, 2 delta - d (scale delta + ds).  A square h^2 of such a difference counts as 2 h hs; a product counts as the
sum over its factors of (the factor's scale x the other factors).  A term through exp(x) counts as exp(x) (1 + |x|) with
|x| taken from ds.  A hinge whose float64 argument lies within NEAR of zero (relative to its scale) counts as open in the
scale: the fp32 distance may fall on either side.

  units(got, ref, scale, allow)   worst |got - ref| over EVERY element in units of 2^-23 x scale, after the absolute
                                  allowances `allow` (fixed point, below) and TINY = 2^-126 (an exp that underflows in fp32
                                  is 1e-290 in float64)
  fix_allow(adds)                 adds x 2^-29: each fixed-point add rounds to the nearest 2^-28
  within(ek, e32)                 ek <= MARGIN * max(e32, 1)                          (units, within, MARGIN: oracle/judge.py)
"""
import numpy as np

from . import judge as J

f64, f32 = np.float64, np.float32
NEAR = 2.0 ** -20
ZCH = 1024                      # voxels per chunk of tem_zero_count
SP_NCH, SP_IT, SP_MAXA, SP_MAXK, SP_MAXB = 8, 8, 64, 32, 1024


# ------------------------------------------------------------------------------------------------------- the judge
# oracle/judge.py under the names the tests use; the absolute allowances: `allow` per element (fixed point) and TINY
TINY, MARGIN, within, band = J.TINY, J.MARGIN, J.within, J.band


def units(got, ref, scale, allow=0.0):
    return J.units(got, ref, scale, allow=allow, tiny=TINY)


def fix_allow(adds):
    return np.asarray(adds, f64) * 2.0 ** -29


def exact(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.shape == ref.shape and got.dtype.kind == ref.dtype.kind and bool(np.array_equal(got, ref))


def untouched(before, after, mask):
    """True if every element of the [E, V] array whose voxel is in `mask` [V] is bit-identical afterwards"""
    b, a = (np.ascontiguousarray(np.asarray(x, f32)[:, np.asarray(mask, bool)]).view(np.uint32) for x in (before, after))
    return b.shape == a.shape and bool(np.array_equal(b, a))


def judge(got, ref, r32, scale, allow=None):
    """-> {key: (kernel units, e32 units, ok)}; an exact quantity (scale None) has units 0 / inf.  allow: {key: absolute}"""
    out = {}
    for k, sc in scale.items():
        if sc is None:
            ok = exact(got[k], ref[k])
            out[k] = (0.0 if ok else float("inf"), 0.0, ok)
            continue
        ek = units(got[k], ref[k], sc, 0.0 if allow is None or k not in allow else allow[k])
        e32 = units(r32[k], ref[k], sc)
        out[k] = (ek, e32, within(ek, e32))
    return out


# ------------------------------------------------------------------------------------------------------- helpers
def _seg_sum(vals, lbl, C, dt):
    """sum of vals [..., V] over the voxels of each label -> [..., C]; pairwise within a label"""
    order = np.argsort(lbl, kind="stable")
    b = np.searchsorted(lbl[order], np.arange(C + 1))
    sv = np.ascontiguousarray(vals[..., order])
    out = np.zeros(vals.shape[:-1] + (C,), dt)
    for l in range(C):
        if b[l + 1] > b[l]:
            out[..., l] = sv[..., b[l]:b[l + 1]].sum(-1, dtype=dt)
    return out


def _dist(df, dt):
    return np.sqrt((df * df).sum(0, dtype=dt))


def _dscale(a, b):
    """the scale of |a - b|_2: |(|a| + |b|)|_2"""
    s = np.abs(a) + np.abs(b)
    return np.sqrt((s * s).sum(0))


def _ratio(a, b, dt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, dt(1)), dt(0)).astype(dt)


def _lbl(lbl):
    return np.ascontiguousarray(np.asarray(lbl, np.int64).reshape(-1))


def _ev(emb, dt):
    e = np.asarray(emb)
    return np.ascontiguousarray(e.reshape(e.shape[0], -1)).astype(dt)


# ------------------------------------------------------------------------------------------------------- exact ops
def label_range(lbl):
    lbl = _lbl(lbl)
    return {"minmax": np.array([lbl.min(), lbl.max()], np.int64)}


def zero_count(lbl):
    z = _lbl(lbl) == 0
    n = -(-z.size // ZCH)
    pad = np.zeros(n * ZCH, bool)
    pad[:z.size] = z
    return {"chunk_counts": pad.reshape(n, ZCH).sum(1).astype(np.int32), "total": np.array([z.sum()], np.int64)}


def zero_select(lbl, ranks):
    return {"idx": np.nonzero(_lbl(lbl) == 0)[0][np.asarray(ranks, np.int64)].astype(np.int64)}


# ------------------------------------------------------------------------------------------------------- cluster means
def cluster_means(emb, lbl, C, dt=f64):
    e, lbl = _ev(emb, dt), _lbl(lbl)
    cnt = np.bincount(lbl, minlength=C).astype(dt)
    return {"means": (_seg_sum(e, lbl, C, dt) / np.maximum(cnt, dt(1))).T.astype(dt), "counts": cnt}


def cluster_means_scale(emb, lbl, C):
    e, lbl = _ev(emb, f64), _lbl(lbl)
    cnt = np.bincount(lbl, minlength=C).astype(f64)
    return {"means": (_seg_sum(np.abs(e), lbl, C, f64) / np.maximum(cnt, 1.0)).T, "counts": None}


def cluster_means_allow(adds, counts):
    """adds [C] fixed-point adds per label (oracle/spoco_cases.py: census), scaled as the mean is"""
    return {"means": (fix_allow(adds) / np.maximum(np.asarray(counts, f64), 1.0))[:, None]}


# ------------------------------------------------------------------------------------------------------- pull
def pull(emb, lbl, C, means, counts, delta_var, dt=f64, scale=False):
    e, lbl = _ev(emb, dt), _lbl(lbl)
    mu, cnt, dv = np.asarray(means).astype(dt)[lbl].T, np.asarray(counts).astype(dt)[lbl], dt(delta_var)
    df = e - mu
    d = _dist(df, dt)
    h = np.maximum(d - dv, dt(0))
    if not scale:
        return {"value": np.array([(h * h / cnt).sum(dtype=dt)], dt), "S": _seg_sum(df * _ratio(h, d, dt), lbl, C, dt).T}
    ds = _dscale(e, mu)
    hs = ds + abs(dv)
    on = (d - dv) > -NEAR * hs
    s_terms = np.where(on, (hs * np.abs(df) + h * (np.abs(e) + np.abs(mu))) / np.where(d > 0, d, 1.0), 0.0)
    return {"value": np.array([(2.0 * h * hs / cnt).sum()]), "S": _seg_sum(s_terms, lbl, C, f64).T}


def pull_scale(emb, lbl, C, means, counts, delta_var):
    return pull(emb, lbl, C, means, counts, delta_var, f64, True)


def pull_allow(adds):
    return {"S": fix_allow(adds)[:, None]}


# ------------------------------------------------------------------------------------------------------- means terms
def means_terms(means, delta_dist, ignore_zero, dt=f64, scale=False):
    mu = np.asarray(means).astype(dt)
    C, E = mu.shape
    dd = dt(delta_dist)
    Cn = C - 1 if ignore_zero else C
    active = C > 1 and not (ignore_zero and C == 2)
    nrm = np.sqrt((mu * mu).sum(1, dtype=dt))
    reg = (nrm / dt(C)).sum(dtype=dt)
    dreg = _ratio(mu, (nrm * dt(C))[:, None] * np.ones_like(mu), dt)
    val, ddist = dt(0), np.zeros((C, E), dt)
    sval, sdd = 0.0, np.zeros((C, E))
    if active:
        Z = dt(Cn * (Cn - 1))
        df = mu[:, None, :] - mu[None, :, :]                       # [i, j, e] = mu_i - mu_j
        d = np.sqrt((df * df).sum(2, dtype=dt))
        off = ~np.eye(C, dtype=bool)
        bgp = np.zeros((C, C), bool)
        if ignore_zero:
            bgp[0, :] = bgp[:, 0] = True
        h = np.where(off & ~bgp, np.maximum(dt(2) * dd - d, dt(0)), dt(0)).astype(dt)
        terms = h * h + np.where(off & bgp & (d == 0), dt(4) * dd * dd, dt(0)).astype(dt)
        val = terms.sum(dtype=dt) / Z
        cf = -dt(4) * _ratio(h, d * Z, dt)
        ddist = (cf[:, :, None] * df).sum(1, dtype=dt)
        if scale:
            am = np.abs(mu)
            sm = am[:, None, :] + am[None, :, :]
            ds = np.sqrt((sm * sm).sum(2))
            hs = 2.0 * dd + ds
            on = off & ~bgp & ((2.0 * dd - d) > -NEAR * hs) & (d > 0)
            sval = ((2.0 * h * hs).sum() + np.where(off & bgp & (d == 0), 4.0 * dd * dd, 0.0).sum()) / Z
            w = np.where(on, 4.0 / (np.where(d > 0, d, 1.0) * Z), 0.0)
            sdd = (w[:, :, None] * (hs[:, :, None] * np.abs(df) + h[:, :, None] * sm)).sum(1)
    if scale:
        return {"values": np.array([sval, reg]), "ddist": sdd, "dreg": np.abs(dreg)}
    return {"values": np.array([val, reg], dt), "ddist": ddist.astype(dt), "dreg": dreg}


def means_terms_scale(means, delta_dist, ignore_zero):
    return means_terms(means, delta_dist, ignore_zero, f64, True)


# ------------------------------------------------------------------------------------------------------- instance Dice
def _pmap(e, anchor, inv, dt, scale=False):
    """exp(-|e - a|^2 * inv) for e [E, V], a [E] -> [V]; with scale: (p, p (1 + |x| from the scale of the distance))"""
    df = e - anchor[:, None]
    d = _dist(df, dt)
    with np.errstate(under="ignore"):
        p = np.exp(-(d * d) * inv).astype(dt)
    if not scale:
        return p
    ds = _dscale(e, anchor[:, None] * np.ones_like(e))
    return p, p * (1.0 + ds * ds * inv)


def _eps(eps, dt):
    """the C ABI carries eps as a float; the kernels compare in double"""
    return dt(f32(eps))


def _dice_rows(num, den, eps, dt):
    return dt(1) - dt(2) * (num / np.maximum(den, _eps(eps, dt)))


def instance_dice(emb, lbl, nz, C, means, two_sigma, eps, dt=f64, scale=False):
    e, lbl, mu = _ev(emb, dt), _lbl(lbl), np.asarray(means).astype(dt)
    inv = dt(1) / dt(f32(two_sigma))
    tot, stot = dt(0), 0.0
    L = lbl.reshape(nz, -1)
    for i in range(1, C):
        m = (L == i).astype(dt)
        if scale:
            p, ps = _pmap(e, mu[i], inv, dt, True)
            p, ps = p.reshape(nz, -1), ps.reshape(nz, -1)
            num, den = (p * m).sum(1), (p * p).sum(1) + m.sum(1)
            ns, dns = (ps * m).sum(1), (2.0 * p * ps).sum(1) + m.sum(1)
            cd = np.maximum(den, _eps(eps, dt))
            stot += (1.0 + 2.0 * (ns / cd + num * dns / (cd * cd))).sum()
            continue
        p = _pmap(e, mu[i], inv, dt).reshape(nz, -1)
        num, den = (p * m).sum(1, dtype=dt), (p * p).sum(1, dtype=dt) + m.sum(1, dtype=dt)
        tot = tot + _dice_rows(num, den, eps, dt).sum(dtype=dt)
    if scale:
        return {"value": np.array([stot / max(C - 1, 1)])}
    return {"value": np.array([tot / dt(C - 1) if C > 1 else dt(0)], dt)}


def instance_dice_scale(emb, lbl, nz, C, means, two_sigma, eps):
    return instance_dice(emb, lbl, nz, C, means, two_sigma, eps, f64, True)


# ------------------------------------------------------------------------------------------------------- unlabeled push
def push(emb, lbl, C, means, counts, delta_dist, grad_scale, dt=f64, scale=False):
    """value; ginc [E, V]: the increment to grad (zero off the background); dpush [C, E]"""
    e, lbl, mu = _ev(emb, dt), _lbl(lbl), np.asarray(means).astype(dt)
    E, V = e.shape
    bg = np.nonzero(lbl == 0)[0]
    eb = e[:, bg]
    dd, gs = dt(delta_dist), dt(f32(grad_scale))
    norm = dt(1) / (dt(np.asarray(counts).reshape(-1)[0]) * dt(C - 1))
    vsum, gb, dpush = dt(0), np.zeros_like(eb), np.zeros((C, E), dt)
    for i in range(1, C):
        m = mu[i][:, None]
        df = eb - m
        d = _dist(df, dt)
        t = np.maximum(dd - d, dt(0))
        if scale:
            ts = dd + _dscale(eb, m * np.ones_like(eb))
            on = ((dd - d) > -NEAR * ts) & (d > 0)
            u = np.where(on, (ts * np.abs(df) + t * (np.abs(eb) + np.abs(m))) / np.where(d > 0, d, 1.0), 0.0)
            vsum = vsum + (2.0 * t * ts).sum()
        else:
            u = df * _ratio(t, d, dt)
            vsum = vsum + (t * t).sum(dtype=dt)
        gb = gb + u if scale else gb - u
        dpush[i] = u.sum(1, dtype=dt)
    ginc = np.zeros((E, V), dt)
    ginc[:, bg] = gs * dt(2) * norm * gb if not scale else abs(gs) * 2.0 * norm * gb
    return {"value": np.array([vsum * norm], dt), "ginc": ginc, "dpush": (dt(2) * norm * dpush).astype(dt)}


def push_scale(emb, lbl, C, means, counts, delta_dist, grad_scale):
    return push(emb, lbl, C, means, counts, delta_dist, grad_scale, f64, True)


def push_allow(bg_waves, C, counts):
    """one fixed-point add per wave that holds a background voxel, at most, into each slot of dpush; scaled by 2 norm"""
    norm = 1.0 / (float(np.asarray(counts).reshape(-1)[0]) * (C - 1))
    return {"dpush": fix_allow(bg_waves) * 2.0 * norm}


# ------------------------------------------------------------------------------------------------------- embedding gradient
def embed_grad(emb, lbl, C, means, counts, S, ddist, dreg, dpush, delta_var, n_inst, w_var, w_dist, w_reg, w_push,
               dt=f64, scale=False):
    """dmu [C, E] (pre-divided by the label size; rows of empty labels are 0/0 and never read) and g [E, V]: the value
    written (accumulate 0) or added (accumulate 1)"""
    e, lbl = _ev(emb, dt), _lbl(lbl)
    mu_all, cnt_all = np.asarray(means).astype(dt), np.asarray(counts).astype(dt)
    S, ddist, dreg = (np.asarray(a).astype(dt) for a in (S, ddist, dreg))
    ni, wv, wd, wr, wp, dv = (dt(f32(x)) for x in (n_inst, w_var, w_dist, w_reg, w_push, delta_var))
    cn = cnt_all[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        if scale:
            g = np.abs(wv * 2.0 / (ni * cn) * S) + np.abs(wd * ddist) + np.abs(wr * dreg)
            if dpush is not None:
                g = g + np.abs(wp * np.asarray(dpush, f64))
        else:
            g = -wv * dt(2) / (ni * cn) * S + wd * ddist + wr * dreg
            if dpush is not None:
                g = wp * np.asarray(dpush).astype(dt) + g
        dmu = (g / cn).astype(dt)
    mu, cnt = mu_all[lbl].T, cnt_all[lbl]
    df = e - mu
    d = _dist(df, dt)
    h = np.maximum(d - dv, dt(0))
    cvar = wv / ni
    if scale:
        hs = _dscale(e, mu) + abs(dv)
        on = ((d - dv) > -NEAR * hs) & (d > 0)
        gv = np.where(on, np.abs(cvar) * 2.0 / (cnt * np.where(d > 0, d, 1.0)) *
                      (hs * np.abs(df) + h * (np.abs(e) + np.abs(mu))), 0.0) + dmu[lbl].T
        return {"dmu": dmu, "g": gv}
    sc = np.where(h > 0, cvar * dt(2) * h / (cnt * np.where(d > 0, d, dt(1))), dt(0)).astype(dt)
    return {"dmu": dmu, "g": (sc * df + dmu[lbl].T).astype(dt)}


def embed_grad_scale(*a):
    return embed_grad(*a, f64, True)


# ------------------------------------------------------------------------------------------------------- consistency
def consistency(eq, ek, nz, idx, two_sigma, eps, grad_scale, dt=f64, scale=False, scatter=True):
    """value and ginc [E, V]: the increment to grad_q, the anchor voxels included (a voxel drawn twice counts twice).
    scatter=False leaves the anchor voxels' part out: a deliberately WRONG gradient for the tests of the judge"""
    q, k, idx = _ev(eq, dt), _ev(ek, dt), np.asarray(idx, np.int64)
    E, V = q.shape
    sl = V // nz
    inv, gs = dt(1) / dt(f32(two_sigma)), dt(f32(grad_scale))
    A = idx.size
    pq, pk, pqs, pks = (np.empty((A, V), dt if j < 2 else f64) for j in range(4))
    for a in range(A):
        if scale:
            pq[a], pqs[a] = _pmap(q, q[:, idx[a]], inv, dt, True)
            pk[a], pks[a] = _pmap(k, k[:, idx[a]], inv, dt, True)
        else:
            pq[a], pk[a] = _pmap(q, q[:, idx[a]], inv, dt), _pmap(k, k[:, idx[a]], inv, dt)
    r = lambda x: x.reshape(A, nz, sl)
    with np.errstate(under="ignore"):
        n = r(pq * pk).sum((0, 2), dtype=dt)
        den = r(pq * pq).sum((0, 2), dtype=dt) + r(pk * pk).sum((0, 2), dtype=dt)
    big = den > _eps(eps, dt)
    cd = np.maximum(den, _eps(eps, dt))
    c_k = (dt(-2) / cd).astype(dt)
    c_q = np.where(big, dt(4) * n / (cd * cd), dt(0)).astype(dt)
    ck_v, cq_v = np.repeat(c_k, sl), np.repeat(c_q, sl)
    ginc = np.zeros((E, V), dt)
    if scale:
        ns = r(pqs * pk + pq * pks).sum((0, 2))
        dns = r(2.0 * pq * pqs + 2.0 * pk * pks).sum((0, 2))
        sval = (1.0 + 2.0 * (ns / cd + n * dns / (cd * cd))).sum()
        for a in range(A):
            cf = abs(gs) * (np.abs(ck_v) * pk[a] + cq_v * pq[a]) * pq[a] * (2.0 * inv) * \
                (1.0 + (pqs[a] / np.maximum(pq[a], TINY) - 1.0) + (pks[a] / np.maximum(pk[a], TINY) - 1.0))
            gv = cf * (np.abs(q) + np.abs(q[:, idx[a]])[:, None])
            ginc += gv
            ginc[:, idx[a]] += gv.sum(1)
        return {"value": np.array([sval]), "ginc": ginc}
    with np.errstate(under="ignore"):
        for a in range(A):
            cf = gs * (ck_v * pk[a] + cq_v * pq[a]) * pq[a] * (dt(-2) * inv)
            gv = (cf * (q - q[:, idx[a]][:, None])).astype(dt)
            ginc += gv
            if scatter:
                ginc[:, idx[a]] -= gv.sum(1, dtype=dt)
    return {"value": np.array([_dice_rows(n, den, eps, dt).sum(dtype=dt)], dt), "ginc": ginc}


def consistency_scale(eq, ek, nz, idx, two_sigma, eps, grad_scale):
    return consistency(eq, ek, nz, idx, two_sigma, eps, grad_scale, f64, True)


# ------------------------------------------------------------------------------------------------------- affinity side loss
def _partner(D, H, W, off):
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    pz, py, px = (np.clip(c + o, 0, n - 1) for c, o, n in ((z, off[0], D), (y, off[1], H), (x, off[2], W)))
    return ((pz * H + py) * W + px).reshape(-1)


def affinity_side(emb, lbl, shape, offsets, delta, eps, grad_scale, dt=f64, scale=False, want_grad=True):
    """value and ginc [E, V]: both roles of a voxel (first of its own pair, partner of the pairs that clamp or shift onto it)"""
    e, lbl = _ev(emb, dt), _lbl(lbl)
    D, H, W = shape
    E, V = e.shape
    assert V == D * H * W
    dl, gs = dt(f32(delta)), dt(f32(grad_scale))
    tot, stot = dt(0), 0.0
    ginc = np.zeros((E, V), dt)
    for off in np.asarray(offsets, np.int64).reshape(-1, 3):
        p = _partner(D, H, W, off)
        ep = e[:, p]
        df = e - ep
        d = _dist(df, dt)
        sv = np.maximum((dt(2) * dl - d) / (dt(2) * dl), dt(0))
        a = dt(1) - sv * sv
        t = (lbl != lbl[p]).astype(dt)
        n, dn = (a * t).sum(dtype=dt), (a * a).sum(dtype=dt) + t.sum(dtype=dt)
        cd = max(dn, _eps(eps, dt))
        c_t, c_a = dt(-2) / cd, (dt(4) * n / (cd * cd) if dn > _eps(eps, dt) else dt(0))
        rd = np.where(d > 0, d, dt(1))
        if scale:
            svs = (2.0 * dl + _dscale(e, ep)) / (2.0 * dl)
            a_s = 1.0 + 2.0 * sv * svs
            ns, dns = (t * a_s).sum(), (2.0 * a * a_s).sum() + t.sum()
            stot += 1.0 + 2.0 * (ns / cd + n * dns / (cd * cd))
            if want_grad:
                on = (d > 0) & ((2.0 * dl - d) > -NEAR * 2.0 * dl * svs)
                g = np.where(on, abs(gs) / (dl * rd) * ((abs(c_t) * t + c_a * a_s) * sv * (np.abs(e) + np.abs(ep)) +
                                                       (abs(c_t) * t + c_a * a) * svs * np.abs(df)), 0.0)
                ginc += g
                for c in range(E):
                    np.add.at(ginc[c], p, g[c])
            continue
        tot = tot + (dt(1) - dt(2) * (n / cd))
        if want_grad:
            cf = np.where((sv > 0) & (d > 0), gs * (c_t * t + c_a * a) * sv / (dl * rd), dt(0)).astype(dt)
            g = (cf * df).astype(dt)
            ginc += g
            for c in range(E):
                np.subtract.at(ginc[c], p, g[c])
    if scale:
        return {"value": np.array([stot]), "ginc": ginc}
    return {"value": np.array([tot], dt), "ginc": ginc}


def affinity_side_scale(emb, lbl, shape, offsets, delta, eps, grad_scale, want_grad=True):
    return affinity_side(emb, lbl, shape, offsets, delta, eps, grad_scale, f64, True, want_grad)


# ------------------------------------------------------------------------------------------------------- float32 restatements
def _as32(fn):
    def g(*a, **kw):
        return fn(*a, dt=f32, **kw)
    g.__name__ = fn.__name__ + "_f32"
    g.__doc__ = f"the float32 restatement of {fn.__name__}: every array and constant in float32, one rounding per operation"
    return g


cluster_means_f32, pull_f32, means_terms_f32, instance_dice_f32 = map(_as32, (cluster_means, pull, means_terms, instance_dice))
push_f32, embed_grad_f32, consistency_f32, affinity_side_f32 = map(_as32, (push, embed_grad, consistency, affinity_side))
