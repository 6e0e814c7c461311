// cldice.hip -- soft skeletonisation and the clDice score (reference loss/cldice.py:25-108), forward and backward.
//
//   erode(x)  = min over the axis lines: 3-D min(min(p_z, p_y), p_x), 2-D min(p_y, p_x); p_a = min of the 3-voxel line
//               along axis a; out-of-volume neighbours are ignored
//   dilate(x) = max over the 3x3x3 (3x3) window; out-of-volume neighbours are ignored
//   e_0 = x, e_{j+1} = erode(e_j), delta_j = relu(e_j - dilate(e_{j+1})) for j = 0..K (open(e_j) = dilate(e_{j+1}): one
//   erosion per round serves the erosion chain and the opening), skel_0 = delta_0,
//   skel_j = skel_{j-1} + relu(delta_j - skel_{j-1} * delta_j)          (multiply, then subtract: never contracted)
//
// Forward: ONE launch per round (k_cld_step).  A block owns an 8x8x32 (2-D: 16x32) tile of one (n, c) volume, stages e_j
// with a 2-voxel halo in LDS (fp32; +inf outside the volume), computes e_{j+1} on the tile + 1 halo (-inf outside), the
// 3x3 (h, w) maxima, then per output the maximum over d, delta and the skeleton update.  Reads e_j (+halo) and skel,
// writes e_{j+1} and skel: 16 B / voxel / round.  Round 0 reads the caller's tensor through (sn, sc, sv) strides (NDHWC
// predictions and NCDHW targets alike, also a channel-sliced view); its outputs and every later round are planar
// [N][C][D][H][W].  Interior loads and all planar stores are 16-byte vectors along W when W % 4 == 0.
// Arithmetic is single-rounded IEEE fp32 in the order written above, so the skeleton equals a torch-op restatement bit
// for bit.  Inputs are assumed finite: NaN propagation is out of scope (min / max drop NaNs here, torch propagates them).
//
// Backward (upstream d/d skel_K -> d/d x), rounds in reverse, all in GATHER form -- every voxel recomputes which
// neighbours selected it and sums their contributions in a fixed order; no floating-point atomics, bitwise
// reproducible.  Per round j, three launches:
//   point  (k_cld_step, a backward mode): recomputes delta_j from e_j, reads skel_{j-1} and the upstream gs_j; writes
//          h_j = -(d / d delta_j) * [delta_j > 0]  (the gradient arriving at dilate(e_{j+1}); -h_j goes to e_j directly)
//          and gs_{j-1}
//   dilate (k_cld_dilate_bwd): G_{j+1}[v] = A_{j+1}[v] + sum over the window u of v of h_j[u] * [argmax window(u) == v]
//   erode  (k_cld_erode_bwd):  A_j[v] = -h_j[v] + sum over axes a and u in the line of v of
//                              G_{j+1}[u] * w_a(u) * [argmin line_a(u) == v];  A_0 is d/d x, written with x's strides
// The routing is recomputed from the saved e_j, never stored as indices.  Tie rules are PyTorch's:
//   pools     first extremum in (d, h, w) scan order (strict comparison while scanning)
//   min(a, b) the smaller operand takes the gradient, on equality each takes half: 3-D all equal -> p_z 1/4, p_y 1/4,
//             p_x 1/2; 2-D 1/2, 1/2 (2-D is its own instantiation, not 3-D with D = 1)
//   relu      passes iff its argument is > 0
// Saved for the backward (the builder's choice: saved, not recomputed): e_1..e_{K+1} and skel_0..skel_{K-1}, i.e.
// (2K + 1) * 4 B / voxel (K = 5: 44 B / voxel, 369 MB for a 2x2x128^3 prediction); recomputing the skel_j instead would
// save K * 4 B / voxel for one more forward sweep.  Backward scratch: 4 planar tensors (gs, h, two G / A buffers).
//
// clDice score: one pass for the four sums (sum skel_x*t, sum skel_x, sum skel_t*x, sum skel_t; per-block double
// partials in a fixed grid, summed in block order) and a one-thread finalise on the device (no host sync).
#include <float.h>
#include <math.h>

#include "tem_common.h"

namespace {

enum { CLD_ROUND0 = 0, CLD_ROUND = 1, CLD_ERODE = 2, CLD_OPEN = 3, CLD_DILATE = 4, CLD_BWD_POINT0 = 5, CLD_BWD_POINT = 6 };

struct CldGeo {
    int N, C, D, H, W;
    int tz, ty, tx;   // tiles per axis
};

template <int NDIM>
struct CldTile {
    static constexpr int TD = NDIM == 3 ? 8 : 1, TH = NDIM == 3 ? 8 : 16, TW = 32;
};

// the tile with a halo of R voxels (no halo along d in 2-D)
template <int NDIM, int R>
struct CldReg {
    using T = CldTile<NDIM>;
    static constexpr int OD = NDIM == 3 ? R : 0;
    static constexpr int RD = T::TD + 2 * OD, RH = T::TH + 2 * R, RW = T::TW + 2 * R;
    static constexpr int SIZE = RD * RH * RW;
    __device__ static __forceinline__ int at(int d, int h, int w) { return (d * RH + h) * RW + w; }
};

struct CldBlock {
    int n, c, z0, y0, x0;
};

template <int NDIM>
__device__ __forceinline__ CldBlock cld_block(const CldGeo& g) {
    using T = CldTile<NDIM>;
    int b = blockIdx.x;
    CldBlock B;
    B.x0 = (b % g.tx) * T::TW, b /= g.tx;
    B.y0 = (b % g.ty) * T::TH, b /= g.ty;
    B.z0 = (b % g.tz) * T::TD, b /= g.tz;
    B.c = b % g.C, B.n = b / g.C;
    return B;
}

// stage the tile + halo R of one (n, c) volume (element (z, y, x) at base[((z*H + y)*W + x) * sv]) in LDS; `fill` outside
// the volume.  vec: sv == 1 and every row start x0 + 4k is 16-byte aligned (checked on the host)
template <int NDIM, int R>
__device__ __forceinline__ void cld_stage(float* __restrict__ lds, const float* __restrict__ base, int64_t sv, int vec,
                                          const CldBlock& B, const CldGeo& g, float fill) {
    using G = CldReg<NDIM, R>;
    constexpr int NV4 = G::T::TW / 4, IPR = NV4 + 2 * R;
    for (int i = threadIdx.x; i < G::RD * G::RH * IPR; i += 256) {
        const int row = i / IPR, k = i - row * IPR;
        const int rd = row / G::RH, rh = row - rd * G::RH;
        const int z = B.z0 + rd - G::OD, y = B.y0 + rh - R;
        const bool rowok = (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H;
        const float* src = base + (rowok ? ((int64_t)z * g.H + y) * g.W * sv : 0);
        float* dst = lds + (rd * G::RH + rh) * G::RW;
        if (k < NV4) {
            const int x = B.x0 + 4 * k;
            float4 v = make_float4(fill, fill, fill, fill);
            if (rowok) {
                if (vec && x + 3 < g.W) {
                    v = *reinterpret_cast<const float4*>(src + x);
                } else {
                    if (x < g.W) v.x = src[(int64_t)x * sv];
                    if (x + 1 < g.W) v.y = src[(int64_t)(x + 1) * sv];
                    if (x + 2 < g.W) v.z = src[(int64_t)(x + 2) * sv];
                    if (x + 3 < g.W) v.w = src[(int64_t)(x + 3) * sv];
                }
            }
            dst[R + 4 * k] = v.x, dst[R + 4 * k + 1] = v.y, dst[R + 4 * k + 2] = v.z, dst[R + 4 * k + 3] = v.w;
        } else {
            const int hk = k - NV4;
            const int rw = hk < R ? hk : G::T::TW + hk;
            const int x = B.x0 + rw - R;
            dst[rw] = (rowok && (unsigned)x < (unsigned)g.W) ? src[(int64_t)x * sv] : fill;
        }
    }
}

// 4 consecutive planar values at off (x..x+3 of a row of width W); lanes past the row end read as 0 / are not stored
__device__ __forceinline__ float4 cld_ld4(const float* p, int64_t off, int nvalid, bool vec) {
    if (vec && nvalid >= 4) return *reinterpret_cast<const float4*>(p + off);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nvalid > 0) v.x = p[off];
    if (nvalid > 1) v.y = p[off + 1];
    if (nvalid > 2) v.z = p[off + 2];
    if (nvalid > 3) v.w = p[off + 3];
    return v;
}
__device__ __forceinline__ void cld_st4(float* p, int64_t off, int nvalid, bool vec, float4 v) {
    if (vec && nvalid >= 4) {
        *reinterpret_cast<float4*>(p + off) = v;
        return;
    }
    if (nvalid > 0) p[off] = v.x;
    if (nvalid > 1) p[off + 1] = v.y;
    if (nvalid > 2) p[off + 2] = v.z;
    if (nvalid > 3) p[off + 3] = v.w;
}

// skel + relu(delta - skel * delta): multiply, subtract, add, each rounded once (no FMA contraction)
__device__ __forceinline__ float cld_skel_pre(float s, float d) {
#pragma clang fp contract(off)
    const float m = s * d;
    return d - m;
}
__device__ __forceinline__ float cld_skel_update(float s, float d) { return s + fmaxf(cld_skel_pre(s, d), 0.f); }

// One round of the skeleton recurrence, the stand-alone erode / open / dilate, and the pointwise part of the backward
// (which needs the same delta_j).  e: strided input; a_in, b_in, e_next, out, out2: planar.
//   ROUND0      e_next = erode(e), out = delta                         ROUND  a_in = skel, out = skel'
//   ERODE       e_next = erode(e)        OPEN  out = dilate(erode(e))    DILATE out = dilate(e)
//   BWD_POINT0  b_in = gs: out = h                                      BWD_POINT a_in = skel_{j-1}, b_in = gs: out = h, out2 = gs'
template <int NDIM>
__global__ __launch_bounds__(256) void k_cld_step(const float* __restrict__ e, int64_t sn, int64_t sc, int64_t sv, int vec_in,
                                                  const float* a_in, const float* b_in, float* __restrict__ e_next,
                                                  float* out, float* out2, CldGeo g, int mode, int vec_out) {
    using T = CldTile<NDIM>;
    using G2 = CldReg<NDIM, 2>;
    using G1 = CldReg<NDIM, 1>;
    constexpr int CD = G1::RD;   // planes of the (h, w)-maxima
    __shared__ float A[G2::SIZE];
    __shared__ float Bm[G1::SIZE];
    __shared__ float Cm[CD * T::TH * T::TW];
    const CldBlock B = cld_block<NDIM>(g);
    const float* base = e + B.n * sn + B.c * sc;
    cld_stage<NDIM, 2>(A, base, sv, vec_in, B, g, mode == CLD_DILATE ? -INFINITY : INFINITY);
    __syncthreads();
    // e_{j+1} on the tile + 1 halo; -inf outside the volume (ignored by the dilation)
    for (int i = threadIdx.x; i < G1::SIZE; i += 256) {
        const int rd = i / (G1::RH * G1::RW), r2 = i - rd * (G1::RH * G1::RW);
        const int rh = r2 / G1::RW, rw = r2 - rh * G1::RW;
        const int z = B.z0 + rd - G1::OD, y = B.y0 + rh - 1, x = B.x0 + rw - 1;
        const int ad = rd + (G2::OD - G1::OD), ah = rh + 1, aw = rw + 1;
        float v = -INFINITY;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W) {
            const float c = A[G2::at(ad, ah, aw)];
            if (mode == CLD_DILATE) {
                v = c;
            } else {
                const float py = fminf(fminf(A[G2::at(ad, ah - 1, aw)], c), A[G2::at(ad, ah + 1, aw)]);
                const float px = fminf(fminf(A[G2::at(ad, ah, aw - 1)], c), A[G2::at(ad, ah, aw + 1)]);
                if (NDIM == 3) {
                    const float pz = fminf(fminf(A[G2::at(ad - 1, ah, aw)], c), A[G2::at(ad + 1, ah, aw)]);
                    v = fminf(fminf(pz, py), px);
                } else {
                    v = fminf(py, px);
                }
            }
        }
        Bm[i] = v;
    }
    __syncthreads();
    if (mode != CLD_ERODE) {
        for (int i = threadIdx.x; i < CD * T::TH * T::TW; i += 256) {
            const int rd = i / (T::TH * T::TW), r2 = i - rd * (T::TH * T::TW);
            const int h = r2 / T::TW, w = r2 - h * T::TW;
            float m = -INFINITY;
#pragma unroll
            for (int dh = 0; dh < 3; ++dh)
#pragma unroll
                for (int dw = 0; dw < 3; ++dw) m = fmaxf(m, Bm[G1::at(rd, h + dh, w + dw)]);
            Cm[i] = m;
        }
        __syncthreads();
    }
    constexpr int NW4 = T::TW / 4;
    for (int i = threadIdx.x; i < T::TD * T::TH * NW4; i += 256) {
        const int d = i / (T::TH * NW4), r2 = i - d * (T::TH * NW4);
        const int h = r2 / NW4, w = (r2 - h * NW4) * 4;
        const int z = B.z0 + d, y = B.y0 + h, x = B.x0 + w;
        if (z >= g.D || y >= g.H || x >= g.W) continue;
        const int nvalid = g.W - x;
        const int64_t off = (((int64_t)(B.n * g.C + B.c) * g.D + z) * g.H + y) * g.W + x;
        float en[4], dil[4], ec[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            en[k] = Bm[G1::at(d + G1::OD, h + 1, w + k + 1)];
            ec[k] = A[G2::at(d + G2::OD, h + 2, w + k + 2)];
            float m = Cm[((d + G1::OD) * T::TH + h) * T::TW + w + k];
            if (NDIM == 3) m = fmaxf(fmaxf(Cm[(d * T::TH + h) * T::TW + w + k], m), Cm[((d + 2) * T::TH + h) * T::TW + w + k]);
            dil[k] = m;
        }
        if (e_next && mode <= CLD_ERODE) cld_st4(e_next, off, nvalid, vec_out, make_float4(en[0], en[1], en[2], en[3]));
        if (mode == CLD_ERODE) continue;
        if (mode == CLD_OPEN || mode == CLD_DILATE) {
            cld_st4(out, off, nvalid, vec_out, make_float4(dil[0], dil[1], dil[2], dil[3]));
            continue;
        }
        float pre[4];   // e_j - open(e_j): delta_j = relu(pre)
#pragma unroll
        for (int k = 0; k < 4; ++k) pre[k] = ec[k] - dil[k];
        float o[4], o2[4];
        if (mode == CLD_ROUND0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = fmaxf(pre[k], 0.f);
        } else if (mode == CLD_ROUND) {
            const float4 s4 = cld_ld4(a_in, off, nvalid, vec_out);
            const float s[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = cld_skel_update(s[k], fmaxf(pre[k], 0.f));
        } else if (mode == CLD_BWD_POINT0) {
            const float4 g4 = cld_ld4(b_in, off, nvalid, vec_out);
            const float gs[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = pre[k] > 0.f ? -gs[k] : 0.f;
        } else {   // CLD_BWD_POINT
            const float4 s4 = cld_ld4(a_in, off, nvalid, vec_out);
            const float4 g4 = cld_ld4(b_in, off, nvalid, vec_out);
            const float s[4] = {s4.x, s4.y, s4.z, s4.w}, gs[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dl = fmaxf(pre[k], 0.f);
                const float gr = cld_skel_pre(s[k], dl) > 0.f ? gs[k] : 0.f;   // through relu(delta - skel*delta)
                const float gd = gr - gr * s[k];
                o[k] = pre[k] > 0.f ? -gd : 0.f;
                o2[k] = gs[k] - gr * dl;
            }
            cld_st4(out2, off, nvalid, vec_out, make_float4(o2[0], o2[1], o2[2], o2[3]));
        }
        cld_st4(out, off, nvalid, vec_out, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// backward of y = dilate(e): out[v] = add[v] + sum_{u in window(v)} h[u] * [first maximum of window(u) is v]
template <int NDIM>
__global__ __launch_bounds__(256) void k_cld_dilate_bwd(const float* __restrict__ e, int64_t sn, int64_t sc, int64_t sv, int vec_in,
                                                        const float* __restrict__ h, const float* add, float* out,
                                                        CldGeo g, int vec_out) {
    using T = CldTile<NDIM>;
    using G2 = CldReg<NDIM, 2>;
    using G1 = CldReg<NDIM, 1>;
    __shared__ float A[G2::SIZE];
    __shared__ float Hm[G1::SIZE];
    __shared__ int Im[G1::SIZE];
    const CldBlock B = cld_block<NDIM>(g);
    cld_stage<NDIM, 2>(A, e + B.n * sn + B.c * sc, sv, vec_in, B, g, -INFINITY);
    cld_stage<NDIM, 1>(Hm, h + (int64_t)(B.n * g.C + B.c) * g.D * g.H * g.W, 1, vec_out, B, g, 0.f);
    __syncthreads();
    constexpr int ND = NDIM == 3 ? 3 : 1;
    for (int i = threadIdx.x; i < G1::SIZE; i += 256) {
        const int rd = i / (G1::RH * G1::RW), r2 = i - rd * (G1::RH * G1::RW);
        const int rh = r2 / G1::RW, rw = r2 - rh * G1::RW;
        const int z = B.z0 + rd - G1::OD, y = B.y0 + rh - 1, x = B.x0 + rw - 1;
        int idx = -1;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W) {
            float best = -INFINITY;   // finite inputs: the first in-volume voxel always beats it
#pragma unroll
            for (int dz = 0; dz < ND; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float v = A[G2::at(rd + dz, rh + dy, rw + dx)];   // region-1 (rd, rh, rw) = region-2 + 1
                        if (v > best) best = v, idx = (dz * 3 + dy) * 3 + dx;
                    }
        }
        Im[i] = idx;
    }
    __syncthreads();
    constexpr int NW4 = T::TW / 4;
    for (int i = threadIdx.x; i < T::TD * T::TH * NW4; i += 256) {
        const int d = i / (T::TH * NW4), r2 = i - d * (T::TH * NW4);
        const int hh = r2 / NW4, w = (r2 - hh * NW4) * 4;
        const int z = B.z0 + d, y = B.y0 + hh, x = B.x0 + w;
        if (z >= g.D || y >= g.H || x >= g.W) continue;
        const int nvalid = g.W - x;
        const int64_t off = (((int64_t)(B.n * g.C + B.c) * g.D + z) * g.H + y) * g.W + x;
        float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (add) a4 = cld_ld4(add, off, nvalid, vec_out);
        float acc[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int oz = 0; oz < ND; ++oz)
#pragma unroll
                for (int oy = 0; oy < 3; ++oy)
#pragma unroll
                    for (int ox = 0; ox < 3; ++ox) {
                        // u = v + (oz, oy, ox) - 1; v sits at window(u) position 2 - o
                        const int u = G1::at(d + oz, hh + oy, w + k + ox);
                        const int kv = ((ND - 1 - oz) * 3 + (2 - oy)) * 3 + (2 - ox);
                        if (Im[u] == kv) acc[k] += Hm[u];
                    }
        cld_st4(out, off, nvalid, vec_out, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

// routing of e' = erode(e) at one voxel: bits 0-1 / 2-3 / 4-5 the position (0, 1, 2) of the first minimum of the z / y / x
// line, bits 6-8 / 9-11 / 12-14 four times the share (0, 1/4, 1/2, 1) of p_z / p_y / p_x in min(min(p_z, p_y), p_x)
template <int NDIM, typename G2>
__device__ __forceinline__ int cld_erode_code(const float* A, int ad, int ah, int aw) {
    const float c = A[G2::at(ad, ah, aw)];
    auto line = [&](float m, float p, int& pos) {
        float best = m;
        pos = 0;
        if (c < best) best = c, pos = 1;
        if (p < best) best = p, pos = 2;
        return best;
    };
    int posz = 1, posy, posx;
    const float py = line(A[G2::at(ad, ah - 1, aw)], A[G2::at(ad, ah + 1, aw)], posy);
    const float px = line(A[G2::at(ad, ah, aw - 1)], A[G2::at(ad, ah, aw + 1)], posx);
    int wz = 0, wy = 4, wx;
    float m1 = py;
    if (NDIM == 3) {
        const float pz = line(A[G2::at(ad - 1, ah, aw)], A[G2::at(ad + 1, ah, aw)], posz);
        wz = pz < py ? 4 : (pz > py ? 0 : 2);
        wy = 4 - wz;
        m1 = fminf(pz, py);
    }
    if (m1 < px) {
        wx = 0;
    } else if (m1 > px) {
        wx = 4, wz = 0, wy = 0;
    } else {
        wx = 2, wz >>= 1, wy >>= 1;
    }
    return posz | (posy << 2) | (posx << 4) | (wz << 6) | (wy << 9) | (wx << 12);
}

// backward of e' = erode(e): out[v] = -h[v] + cdir * direct[v] + sum over axes a (z, y, x) and u = v-1_a, v, v+1_a of
// g[u] * w_a(u) * [first minimum of line_a(u) is v]; out has strides (on, oc, ov); h, direct may be null
template <int NDIM>
__global__ __launch_bounds__(256) void k_cld_erode_bwd(const float* __restrict__ e, int64_t sn, int64_t sc, int64_t sv, int vec_in,
                                                       const float* __restrict__ gin, const float* __restrict__ h,
                                                       const float* __restrict__ direct, const float* __restrict__ coef,
                                                       const float* __restrict__ gout, float* __restrict__ out, int64_t on,
                                                       int64_t oc, int64_t ov, CldGeo g, int vec_pl) {
    using T = CldTile<NDIM>;
    using G2 = CldReg<NDIM, 2>;
    using G1 = CldReg<NDIM, 1>;
    __shared__ float A[G2::SIZE];
    __shared__ float Gm[G1::SIZE];
    __shared__ int Km[G1::SIZE];
    const CldBlock B = cld_block<NDIM>(g);
    cld_stage<NDIM, 2>(A, e + B.n * sn + B.c * sc, sv, vec_in, B, g, INFINITY);
    cld_stage<NDIM, 1>(Gm, gin + (int64_t)(B.n * g.C + B.c) * g.D * g.H * g.W, 1, vec_pl, B, g, 0.f);
    __syncthreads();
    for (int i = threadIdx.x; i < G1::SIZE; i += 256) {
        const int rd = i / (G1::RH * G1::RW), r2 = i - rd * (G1::RH * G1::RW);
        const int rh = r2 / G1::RW, rw = r2 - rh * G1::RW;
        const int z = B.z0 + rd - G1::OD, y = B.y0 + rh - 1, x = B.x0 + rw - 1;
        int code = 0;   // outside the volume: no share for anybody
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W)
            code = cld_erode_code<NDIM, G2>(A, rd + (G2::OD - G1::OD), rh + 1, rw + 1);
        Km[i] = code;
    }
    __syncthreads();
    const float cdir = direct ? coef[2] * gout[0] : 0.f;
    constexpr int NW4 = T::TW / 4;
    for (int i = threadIdx.x; i < T::TD * T::TH * NW4; i += 256) {
        const int d = i / (T::TH * NW4), r2 = i - d * (T::TH * NW4);
        const int hh = r2 / NW4, w = (r2 - hh * NW4) * 4;
        const int z = B.z0 + d, y = B.y0 + hh, x = B.x0 + w;
        if (z >= g.D || y >= g.H || x >= g.W) continue;
        const int nvalid = g.W - x;
        const int64_t off = (((int64_t)(B.n * g.C + B.c) * g.D + z) * g.H + y) * g.W + x;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int rd = d + G1::OD, rh = hh + 1, rw = w + k + 1;
            float s = 0.f;
#pragma unroll
            for (int o = 0; o < 3; ++o) {   // u = v + o - 1 along the axis; v is at line position 2 - o
                if (NDIM == 3) {
                    const int u = G1::at(rd + o - 1, rh, rw), code = Km[u];
                    if ((code & 3) == 2 - o) s += Gm[u] * (0.25f * (float)((code >> 6) & 7));
                }
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const int u = G1::at(rd, rh + o - 1, rw), code = Km[u];
                if (((code >> 2) & 3) == 2 - o) s += Gm[u] * (0.25f * (float)((code >> 9) & 7));
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const int u = G1::at(rd, rh, rw + o - 1), code = Km[u];
                if (((code >> 4) & 3) == 2 - o) s += Gm[u] * (0.25f * (float)((code >> 12) & 7));
            }
            acc[k] = s;
        }
        if (h) {
            const float4 h4 = cld_ld4(h, off, nvalid, vec_pl);
            acc[0] -= h4.x, acc[1] -= h4.y, acc[2] -= h4.z, acc[3] -= h4.w;
        }
        if (direct) {
            const float4 d4 = cld_ld4(direct, off, nvalid, vec_pl);
            acc[0] += cdir * d4.x, acc[1] += cdir * d4.y, acc[2] += cdir * d4.z, acc[3] += cdir * d4.w;
        }
        const int64_t v0 = ((int64_t)z * g.H + y) * g.W + x;
        float* o = out + B.n * on + B.c * oc;
        if (ov == 1 && vec_pl && (on & 3) == 0 && (oc & 3) == 0 && nvalid >= 4) {
            *reinterpret_cast<float4*>(o + v0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nvalid) o[(v0 + k) * ov] = acc[k];
        }
    }
}

// ---- clDice score ---------------------------------------------------------------------------------------------------
#define CLD_BLOCKS 1024

__global__ __launch_bounds__(256) void k_cld_sums(const float* __restrict__ sx, const float* __restrict__ st,
                                                  const float* __restrict__ x, int64_t x_sn, int64_t x_sc, int64_t x_sv,
                                                  const float* __restrict__ t, int64_t t_sn, int64_t t_sc, int64_t t_sv,
                                                  int C, int64_t V, int64_t total, double* __restrict__ part) {
    __shared__ double sh[4][4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)CLD_BLOCKS * 256) {
        const int64_t nc = i / V, v = i - nc * V;
        const int64_t n = nc / C, c = nc - n * C;
        const float a = sx[i], b = st[i];
        acc[0] += (double)(a * t[n * t_sn + c * t_sc + v * t_sv]);   // fp32 product like the reference, double sum
        acc[1] += (double)a;
        acc[2] += (double)(b * x[n * x_sn + c * x_sc + v * x_sv]);
        acc[3] += (double)b;
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = tem_wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        part[(int64_t)blockIdx.x * 4 + threadIdx.x] =
            ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// t_prec = A / max(B, eps), t_sens = Cc / max(Dd, eps), score = 2 t_prec t_sens / max(t_prec + t_sens, eps)
// (loss/cldice.py:101-106); clamp(min=eps) passes its gradient iff the argument is >= eps.
// coef: d out / d skel_x = coef[0] * t + coef[1]; d out / d x (direct) = coef[2] * skel_t
__global__ void k_cld_finalize(const double* __restrict__ part, double eps, int invert, double* __restrict__ sums,
                               float* __restrict__ outv, float* __restrict__ coef) {
    __shared__ double s[4];
    if (threadIdx.x < 4) {
        double a = 0.0;
        for (int b = 0; b < CLD_BLOCKS; ++b) a += part[(int64_t)b * 4 + threadIdx.x];
        s[threadIdx.x] = a;
        sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double A = s[0], Bs = s[1], Cs = s[2], Ds = s[3];
    const double Bc = Bs < eps ? eps : Bs, Dc = Ds < eps ? eps : Ds;
    const double tp = A / Bc, ts = Cs / Dc;
    const double S = tp + ts, Sc = S < eps ? eps : S;
    const double score = 2.0 * tp * ts / Sc;
    const double dS = S >= eps ? -2.0 * tp * ts / (Sc * Sc) : 0.0;
    const double sgn = invert ? -1.0 : 1.0;
    const double dtp = sgn * (2.0 * ts / Sc + dS), dts = sgn * (2.0 * tp / Sc + dS);
    outv[0] = (float)(invert ? 1.0 - score : score);
    coef[0] = (float)(dtp / Bc);
    coef[1] = (float)(Bs >= eps ? -dtp * A / (Bc * Bc) : 0.0);
    coef[2] = (float)(dts / Dc);
    coef[3] = 0.f;
}

// upstream gradient of the prediction's skeleton: gs = gout * (coef[0] * t + coef[1]), planar
__global__ __launch_bounds__(256) void k_cld_seed(const float* __restrict__ t, int64_t t_sn, int64_t t_sc, int64_t t_sv,
                                                  const float* __restrict__ coef, const float* __restrict__ gout,
                                                  float* __restrict__ gs, int C, int64_t V, int64_t total) {
    const float ca = coef[0] * gout[0], cb = coef[1] * gout[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t nc = i / V, v = i - nc * V;
        const int64_t n = nc / C, c = nc - n * C;
        gs[i] = ca * t[n * t_sn + c * t_sc + v * t_sv] + cb;
    }
}

bool cld_geo(CldGeo& g, int N, int C, int D, int H, int W, int ndim) {
    if (!(ndim == 2 || ndim == 3) || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || (ndim == 2 && D != 1)) return false;
    g.N = N, g.C = C, g.D = D, g.H = H, g.W = W;
    const int td = ndim == 3 ? CldTile<3>::TD : 1, th = ndim == 3 ? CldTile<3>::TH : CldTile<2>::TH;
    g.tz = (int)tem_cdiv(D, td), g.ty = (int)tem_cdiv(H, th), g.tx = (int)tem_cdiv(W, 32);
    const int64_t blocks = (int64_t)N * C * g.tz * g.ty * g.tx;
    return blocks < INT_MAX && (int64_t)N * C * D * H * W < ((int64_t)1 << 40);
}
int cld_grid(const CldGeo& g) { return g.N * g.C * g.tz * g.ty * g.tx; }
// 16-byte vector access along W: planar tensors need W % 4 == 0 and an aligned base; a strided one also sv == 1 and
// aligned plane starts
int cld_vec_planar(const CldGeo& g, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    auto ok = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return g.W % 4 == 0 && ok(a) && ok(b) && ok(c) && ok(d);
}
int cld_vec_strided(const CldGeo& g, const void* p, int64_t sn, int64_t sc, int64_t sv) {
    return g.W % 4 == 0 && sv == 1 && ((uintptr_t)p & 15) == 0 && sn % 4 == 0 && sc % 4 == 0;
}

}   // namespace

// what: 0 reduction partials of tem_cldice_sums; 1 erosion ping-pong of a forward that saves nothing (2 planar tensors);
// 2 the tensors a forward saves for the backward (e_1..e_{K+1}, skel_0..skel_{K-1}); 3 backward scratch (4 planar tensors)
extern "C" int64_t tem_cldice_ws(int N, int C, int64_t V, int num_iter, int what) {
    const int64_t t = (int64_t)N * C * V * (int64_t)sizeof(float);
    switch (what) {
        case 0: return (int64_t)CLD_BLOCKS * 4 * sizeof(double);
        case 1: return 2 * t;
        case 2: return (2 * (int64_t)num_iter + 1) * t;
        case 3: return 4 * t;
        default: return -1;
    }
}

extern "C" int tem_cldice_step(const float* e, int64_t sn, int64_t sc, int64_t sv, const float* a_in, const float* b_in,
                               float* e_next, float* out, float* out2, int N, int C, int D, int H, int W, int ndim,
                               int mode, tem_stream_t stream) {
    CldGeo g;
    TEM_REQUIRE(cld_geo(g, N, C, D, H, W, ndim), "tem_cldice_step: bad shape (ndim 2 needs D == 1)");
    TEM_REQUIRE(e, "tem_cldice_step: null input");
    TEM_REQUIRE(mode >= CLD_ROUND0 && mode <= CLD_BWD_POINT, "tem_cldice_step: unknown mode %d", mode);
    TEM_REQUIRE(mode == CLD_ERODE ? e_next != nullptr : out != nullptr, "tem_cldice_step: null output");
    TEM_REQUIRE((mode != CLD_ROUND && mode != CLD_BWD_POINT) || a_in, "tem_cldice_step: the mode needs skel (a_in)");
    TEM_REQUIRE((mode != CLD_BWD_POINT0 && mode != CLD_BWD_POINT) || b_in, "tem_cldice_step: the mode needs the upstream (b_in)");
    TEM_REQUIRE(mode != CLD_BWD_POINT || out2, "tem_cldice_step: the mode needs out2");
    TEM_REQUIRE(e_next != e && out != e, "tem_cldice_step: the input is read with a halo; it cannot be an output");
    const int vin = cld_vec_strided(g, e, sn, sc, sv), vout = cld_vec_planar(g, a_in, b_in, e_next, out) && ((uintptr_t)out2 & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (ndim == 3)
        hipLaunchKernelGGL(k_cld_step<3>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, a_in, b_in, e_next, out,
                           out2, g, mode, vout);
    else
        hipLaunchKernelGGL(k_cld_step<2>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, a_in, b_in, e_next, out,
                           out2, g, mode, vout);
    TEM_CHECK_LAUNCH("tem_cldice_step");
    return TEM_OK;
}

extern "C" int tem_cldice_dilate_bwd(const float* e, int64_t sn, int64_t sc, int64_t sv, const float* h, const float* add,
                                     float* out, int N, int C, int D, int H, int W, int ndim, tem_stream_t stream) {
    CldGeo g;
    TEM_REQUIRE(cld_geo(g, N, C, D, H, W, ndim), "tem_cldice_dilate_bwd: bad shape (ndim 2 needs D == 1)");
    TEM_REQUIRE(e && h && out, "tem_cldice_dilate_bwd: null pointer");
    TEM_REQUIRE(out != h && out != e, "tem_cldice_dilate_bwd: e and h are read with a halo; they cannot be the output");
    const int vin = cld_vec_strided(g, e, sn, sc, sv), vout = cld_vec_planar(g, h, add, out);
    hipStream_t st = (hipStream_t)stream;
    if (ndim == 3)
        hipLaunchKernelGGL(k_cld_dilate_bwd<3>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, h, add, out, g, vout);
    else
        hipLaunchKernelGGL(k_cld_dilate_bwd<2>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, h, add, out, g, vout);
    TEM_CHECK_LAUNCH("tem_cldice_dilate_bwd");
    return TEM_OK;
}

extern "C" int tem_cldice_erode_bwd(const float* e, int64_t sn, int64_t sc, int64_t sv, const float* gin, const float* h,
                                    const float* direct, const float* coef, const float* gout, float* out, int64_t on,
                                    int64_t oc, int64_t ov, int N, int C, int D, int H, int W, int ndim,
                                    tem_stream_t stream) {
    CldGeo g;
    TEM_REQUIRE(cld_geo(g, N, C, D, H, W, ndim), "tem_cldice_erode_bwd: bad shape (ndim 2 needs D == 1)");
    TEM_REQUIRE(e && gin && out, "tem_cldice_erode_bwd: null pointer");
    TEM_REQUIRE(!direct || (coef && gout), "tem_cldice_erode_bwd: the direct term needs coef and gout");
    TEM_REQUIRE(out != gin && out != e, "tem_cldice_erode_bwd: e and g are read with a halo; they cannot be the output");
    const int vin = cld_vec_strided(g, e, sn, sc, sv), vpl = cld_vec_planar(g, gin, h, direct, ov == 1 ? out : nullptr);
    hipStream_t st = (hipStream_t)stream;
    if (ndim == 3)
        hipLaunchKernelGGL(k_cld_erode_bwd<3>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, gin, h, direct, coef,
                           gout, out, on, oc, ov, g, vpl);
    else
        hipLaunchKernelGGL(k_cld_erode_bwd<2>, dim3(cld_grid(g)), dim3(256), 0, st, e, sn, sc, sv, vin, gin, h, direct, coef,
                           gout, out, on, oc, ov, g, vpl);
    TEM_CHECK_LAUNCH("tem_cldice_erode_bwd");
    return TEM_OK;
}

extern "C" int tem_cldice_sums(const float* skel_x, const float* skel_t, const float* x, int64_t x_sn, int64_t x_sc,
                               int64_t x_sv, const float* t, int64_t t_sn, int64_t t_sc, int64_t t_sv, int N, int C,
                               int64_t V, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(skel_x && skel_t && x && t && ws, "tem_cldice_sums: null pointer");
    TEM_REQUIRE(N > 0 && C > 0 && V > 0, "tem_cldice_sums: bad shape");
    if (ws_bytes < tem_cldice_ws(N, C, V, 0, 0)) {
        tem_set_error("tem_cldice_sums: workspace too small");
        return TEM_EWS;
    }
    hipLaunchKernelGGL(k_cld_sums, dim3(CLD_BLOCKS), dim3(256), 0, (hipStream_t)stream, skel_x, skel_t, x, x_sn, x_sc, x_sv,
                       t, t_sn, t_sc, t_sv, C, V, (int64_t)N * C * V, (double*)ws);
    TEM_CHECK_LAUNCH("tem_cldice_sums");
    return TEM_OK;
}

extern "C" int tem_cldice_finalize(const void* ws, double eps, int invert, double* sums, float* out, float* coef,
                                   tem_stream_t stream) {
    TEM_REQUIRE(ws && sums && out && coef, "tem_cldice_finalize: null pointer");
    TEM_REQUIRE(eps >= 0.0, "tem_cldice_finalize: eps must not be negative");
    hipLaunchKernelGGL(k_cld_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, eps, invert, sums, out,
                       coef);
    TEM_CHECK_LAUNCH("tem_cldice_finalize");
    return TEM_OK;
}

extern "C" int tem_cldice_grad(const float* t, int64_t t_sn, int64_t t_sc, int64_t t_sv, const float* coef,
                               const float* gout, float* gs, int N, int C, int64_t V, tem_stream_t stream) {
    TEM_REQUIRE(t && coef && gout && gs, "tem_cldice_grad: null pointer");
    TEM_REQUIRE(N > 0 && C > 0 && V > 0, "tem_cldice_grad: bad shape");
    const int64_t total = (int64_t)N * C * V;
    hipLaunchKernelGGL(k_cld_seed, dim3(tem_grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, t, t_sn, t_sc, t_sv,
                       coef, gout, gs, C, V, total);
    TEM_CHECK_LAUNCH("tem_cldice_grad");
    return TEM_OK;
}
