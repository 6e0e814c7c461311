"""The random stream of the device noise transforms, in numpy (the CPU oracle of csrc/rawaug.hip; DESIGN.md, "The stream of
the raw noise transforms", is the specification both follow).

Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (i & 0xffffffff, i >> 32, row, round): the words of element
`i` of row `row` are a pure function of (seed, row, i, round).  `normal_from_words` and `poisson_from_words` turn words into
samples in float32 (what the kernels compute, up to the accuracy of the device's logf / cospif / lgammaf) or in float64 (the
reference the device results are judged against); one text serves both precisions.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
INVERSION_BELOW = 10.0     # lam < 10: inversion; lam >= 10: transformed rejection (numpy's threshold)
INVERSION_STEPS = 80       # bound of the sequential search
PTRS_ROUNDS = 64           # bound of the rejection loop; then rint(lam)


def philox4x32(counter, key):
    """Philox4x32-10.  counter: four integers or integer arrays (broadcast against each other), key: two; every value is
    taken modulo 2^32.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(v).astype(np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & MASK for v in key)
    m0, m1, mask, s32 = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]          # 32 x 32 -> 64 bit: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(v.astype(np.uint32) for v in c)


def words(seed: int, row, i, rnd=0):
    """w0..w3 of element(s) `i` of row(s) `row` at redraw `rnd` under the 64-bit `seed`"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.asarray(i).astype(np.uint64)
    return philox4x32((i & np.uint64(MASK), i >> np.uint64(32), row, rnd), (seed & MASK, seed >> 32))


def uniform_oc(w, dtype=np.float64):
    """u in (0, 1]: ((w >> 8) + 1) * 2^-24 (exact in float32)"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(dtype) + dtype(1)) * dtype(2.0 ** -24)


def uniform_co(w, dtype=np.float64):
    """u in [0, 1): (w >> 8) * 2^-24 (exact in float32)"""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)


def normal_from_words(w0, w1, dtype=np.float64):
    """Box-Muller, cosine branch: sqrt(-2 log u1) * cospi(2 u2), u1 = u_(0,1](w0), u2 = u_[0,1)(w1).  2 * u2 is exact, and
    the argument is brought into (-1, 1] exactly before it meets pi."""
    dtype = np.dtype(dtype).type
    u1, t = uniform_oc(w0, dtype), dtype(2) * uniform_co(w1, dtype)
    t = np.where(t > dtype(1), t - dtype(2), t)
    return (np.sqrt(dtype(-2) * np.log(u1)) * np.cos(dtype(np.pi) * t)).astype(dtype)


_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def lgamma(x, dtype=np.float64):
    """log Gamma, evaluated in double and rounded to `dtype`"""
    return np.asarray(_lgamma(np.asarray(x, dtype=np.float64)), dtype=np.float64).astype(dtype)


def field_words(seed: int, row, i):
    """-> words(rnd, sel): (w0, w1) of the flat elements `sel` (None: all) of the field (row, i) at redraw `rnd`"""
    row, i = np.broadcast_arrays(np.asarray(row, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
    row, i = row.ravel(), i.ravel()

    def draw(rnd, sel=None):
        w = words(seed, row if sel is None else row[sel], i if sel is None else i[sel], rnd)
        return w[0], w[1]
    return draw


def _inversion(lam, u, dtype):
    """sequential search from k = 0 with at most INVERSION_STEPS steps"""
    p = np.exp(-lam)
    s = p.copy()
    k = np.zeros(lam.shape, dtype=np.int64)
    live = np.nonzero(u >= s)[0]
    for step in range(1, INVERSION_STEPS + 1):
        if live.size == 0:
            break
        k[live] = step
        p[live] = p[live] * lam[live] / dtype(step)
        s[live] = s[live] + p[live]
        live = live[u[live] >= s[live]]
    return k


def _ptrs(lam, draw, sel, dtype, lgamma_dtype):
    """Hoermann's transformed rejection (PTRS) over a shrinking set of undecided elements"""
    slam, loglam = np.sqrt(lam), np.log(lam)
    b = dtype(0.931) + dtype(2.53) * slam
    a = dtype(-0.059) + dtype(0.02483) * b
    inv_alpha = dtype(1.1239) + dtype(1.1328) / (b - dtype(3.4))
    vr = dtype(0.9277) - dtype(3.6224) / (b - dtype(2))
    out = np.rint(lam).astype(np.int64)      # what is left after PTRS_ROUNDS
    todo = np.arange(lam.size)
    for rnd in range(PTRS_ROUNDS):
        if todo.size == 0:
            break
        w0, w1 = draw(rnd, sel[todo])
        la, bb, aa = lam[todo], b[todo], a[todo]
        U = uniform_co(w0, dtype) - dtype(0.5)
        V = uniform_oc(w1, dtype)
        us = dtype(0.5) - np.abs(U)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            kf = np.floor((dtype(2) * aa / us + bb) * U + la + dtype(0.43))
            fast = (us >= dtype(0.07)) & (V <= vr[todo])
            reject = ~fast & ((kf < 0) | ((us < dtype(0.013)) & (V > us)))
            slow = np.nonzero(~fast & ~reject)[0]
            lhs = np.log(V[slow]) + np.log(inv_alpha[todo][slow]) - np.log(aa[slow] / (us[slow] * us[slow]) + bb[slow])
            rhs = -la[slow] + kf[slow] * loglam[todo][slow] - lgamma(kf[slow] + 1, lgamma_dtype).astype(dtype)
        accept = fast.copy()
        accept[slow] = lhs <= rhs
        out[todo[accept]] = kf[accept].astype(np.int64)
        todo = todo[~accept]
    return out


def poisson_from_words(lam, draw, dtype=np.float64, lgamma_dtype=None):
    """Poisson counts (int64, the shape of `lam`) with mean `lam` from the words `draw(rnd, sel)` delivers (`field_words`).
    lam == 0: 0; lam < 10: inversion on u_[0,1)(w0) of redraw 0; lam >= 10: PTRS, redraw r using U = u_[0,1)(w0) - 0.5 and
    V = u_(0,1](w1).  All arithmetic in `dtype`; `lgamma_dtype`: the precision log Gamma is rounded to (default: dtype)."""
    dtype = np.dtype(dtype).type
    lgamma_dtype = dtype if lgamma_dtype is None else np.dtype(lgamma_dtype).type
    shape = np.shape(lam)
    lam = np.asarray(lam).astype(dtype).ravel()
    out = np.zeros(lam.shape, dtype=np.int64)
    small = np.nonzero((lam > 0) & (lam < dtype(INVERSION_BELOW)))[0]
    if small.size:
        out[small] = _inversion(lam[small], uniform_co(draw(0, small)[0], dtype), dtype)
    big = np.nonzero(lam >= dtype(INVERSION_BELOW))[0]
    if big.size:
        out[big] = _ptrs(lam[big], draw, big, dtype, lgamma_dtype)
    return out.reshape(shape)
