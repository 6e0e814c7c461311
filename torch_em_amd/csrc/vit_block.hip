// vit_block.hip -- what a SAM transformer block needs besides attention and its four linears (DESIGN.md "Transformer block";
// model/vit.py: Block): LayerNorm fused with the window partition, un-partition + crop + residual add fused with the second
// LayerNorm, bias + exact GELU, each forward and backward.
//
// Row kernels.  A token is a row of C channels (C % 8 == 0, C <= TEM_VB_MAX_C).  One wave owns one token; lane l owns the
// 8-channel chunks l + 64 j, j < NCH = ceil(C / 512) (a template parameter: the row never indexes registers dynamically), the
// last chunk predicated where C / 8 is no multiple of 64.  The row lives in registers as fp32: mean = one wave sum / C,
// variance = the wave sum of (x - mean)^2 over the same registers / C (never E[x^2] - mean^2), rstd = 1 / sqrt(var + eps), and
// the normalised row is written from those registers.  A workgroup is 4 waves on 4 consecutive tokens.
//   k_ln_win_fwd        over the B Hp Wp destination tokens of the window tensor [B nWh nWw][ws][ws][C] (Hp = ceil(H / ws) ws):
//                       a token inside H x W reads its source row, normalises it, stores mean and rstd (fp32 [B][H][W]) when
//                       asked; a token of the padding stores +0.0 (SAM pads AFTER the norm).  Every byte written once.
//   k_win_merge_ln_fwd  over the B H W source tokens: x1 = shortcut + y[window token], stored rounded; xn = LN(x1) from the
//                       fp32 sum BEFORE that rounding; mean, rstd of x1.  Pad tokens of y are never read.
//   k_ln_win_bwd        over source tokens: gh = g gamma, dx = rstd (gh - mean_c(gh) - xhat mean_c(gh xhat)), xhat = (x - mean) rstd
//                       recomputed; g is read at the token's window position, gradients of pad tokens are dropped.
//   k_win_merge_ln_bwd  over destination tokens: t = dx1 + LNbwd(dxn) formed once, stored as dshortcut (source position) and as
//                       dy (window position); a pad token stores +0.0 into dy.  xhat comes from the STORED x1.
// Parameter gradients ride in the backward kernels: a lane owns fixed channels, so dgamma[c] += g xhat and dbeta[c] += g are
// lane-private registers.  A workgroup walks a slab of TEM_VB_SLAB = 32 tokens (wave w the tokens 4 i + w of it), its waves are
// added in wave order through LDS (waves 1..3 write, wave 0 adds: 3 x 2 x 512 NCH floats = 12 NCH KB), and one [2][C] fp32 partial a
// workgroup goes to the workspace; k_col_sum adds the partials in index order.  32 tokens: the partials cost 2 C floats per
// 32 rows (8 % of one fp16 pass over the rows) and ViT-B's 4096 tokens still give 128 workgroups.
//
// k_bias_gelu_fwd / _bwd: [M][C4], C4 % 8 == 0.  Thread l of a workgroup owns chunk l + 256 j of a row -- its bias chunk and, in
// the backward, its bias-gradient sums are registers -- and workgroups stride over rows.  y = 0.5 z (1 + erf(z / sqrt 2)),
// z = h + b; dh = dy (Phi(z) + z phi(z)) recomputed from h and b.  The backward runs ceil(M / TEM_VB_GELU_ROWS) workgroups (at
// most 1024), each leaves one [C4] partial, k_col_sum adds them.
// No atomics, no memset: same input, same bits.  16-bit roundings besides the final store: none, except that
// k_win_merge_ln_bwd computes xhat from the stored (once rounded) x1.
#include "tem_common.h"
#include <type_traits>

#define VB_GELU_MAX_WG 1024
typedef _Float16 vb_h2 __attribute__((ext_vector_type(2)));
typedef __bf16 vb_b2 __attribute__((ext_vector_type(2)));

struct VbGeom {
    int H, W, ws, Wp, nWw, nW;   // nW = windows of one image; ws == 0: Wp = W, no windows
    int64_t nsrc, ndst;          // B H W, B Hp Wp
};

// destination (window-layout) token -> source token, -1 in the padding
__device__ __forceinline__ int64_t vb_dst_to_src(const VbGeom& g, int64_t d) {
    if (g.ws == 0) return d;
    const int ww2 = g.ws * g.ws;
    const int64_t win = d / ww2;
    const int r = (int)(d - win * ww2), i = r / g.ws, j = r - i * g.ws;
    const int64_t b = win / g.nW;
    const int wr = (int)(win - b * g.nW), wh = wr / g.nWw, ww = wr - wh * g.nWw;
    const int h = wh * g.ws + i, w = ww * g.ws + j;
    return (h < g.H && w < g.W) ? (b * g.H + h) * g.W + w : -1;
}
__device__ __forceinline__ int64_t vb_src_to_dst(const VbGeom& g, int64_t s) {
    if (g.ws == 0) return s;
    const int hw = g.H * g.W;
    const int64_t b = s / hw;
    const int r = (int)(s - b * hw), h = r / g.W, w = r - h * g.W;
    const int wh = h / g.ws, i = h - wh * g.ws, ww = w / g.ws, j = w - ww * g.ws;
    return ((b * g.nW + wh * g.nWw + ww) * g.ws + i) * g.ws + j;
}

// 8 consecutive elements (p 16-byte aligned for 16-bit types, 32 for float: two 16-byte accesses) <-> 8 floats
template <typename T>
__device__ __forceinline__ void vb_ld8(const T* p, float* v) {
    if constexpr (std::is_same<T, float>::value) {
        const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
        const uint4 u = *(const uint4*)p;
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (std::is_same<T, _Float16>::value) {
                const vb_h2 h = __builtin_bit_cast(vb_h2, w[k]);
                v[2 * k] = (float)h.x, v[2 * k + 1] = (float)h.y;
            } else {
                v[2 * k] = __builtin_bit_cast(float, w[k] << 16), v[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
            }
        }
    }
}
template <typename T>
__device__ __forceinline__ void vb_st8(T* p, const float* v) {   // one rounding to nearest even
    if constexpr (std::is_same<T, float>::value) {
        *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (std::is_same<T, _Float16>::value) {
                const vb_h2 h = {(_Float16)v[2 * k], (_Float16)v[2 * k + 1]};
                w[k] = __builtin_bit_cast(unsigned, h);
            } else {
                const vb_b2 h = {(__bf16)v[2 * k], (__bf16)v[2 * k + 1]};
                w[k] = __builtin_bit_cast(unsigned, h);
            }
        }
        *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
    }
}
template <typename T>
__device__ __forceinline__ void vb_st8_zero(T* p) {   // +0.0 in every bit
    *(uint4*)p = make_uint4(0, 0, 0, 0);
    if constexpr (std::is_same<T, float>::value) *(uint4*)(p + 4) = make_uint4(0, 0, 0, 0);
}

// the lane's chunks of a row; chunk j is live in every lane for j < NCH - 1, the last one where lane + 64 j < nch
#define VB_LIVE(j) ((j) < NCH - 1 || lane + 64 * (j) < nch)
template <typename T, int NCH>
__device__ __forceinline__ void vb_load_row(const T* row, int lane, int nch, float (&v)[NCH][8]) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (VB_LIVE(j)) {
            vb_ld8<T>(row + 8 * (lane + 64 * j), v[j]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
        }
    }
}
template <typename T, int NCH>
__device__ __forceinline__ void vb_store_row(T* row, int lane, int nch, const float (&v)[NCH][8]) {
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        if (VB_LIVE(j)) vb_st8<T>(row + 8 * (lane + 64 * j), v[j]);
}
template <typename T, int NCH>
__device__ __forceinline__ void vb_zero_row(T* row, int lane, int nch) {
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        if (VB_LIVE(j)) vb_st8_zero<T>(row + 8 * (lane + 64 * j));
}
template <int NCH>
__device__ __forceinline__ float vb_row_sum(const float (&v)[NCH][8]) {   // dead chunks hold zeros
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[j][e];
    return tem_wave_sum(s);
}
__device__ __forceinline__ int vb_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// v (the fp32 row, dead chunks zero) -> LN(v) gamma + beta in place; mean and rstd returned
template <typename T, int NCH>
__device__ __forceinline__ void vb_normalise(float (&v)[NCH][8], const T* gamma, const T* beta, int lane, int nch, int C, float eps,
                                             float& mean, float& rstd) {
    mean = vb_row_sum<NCH>(v) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[j][e] = VB_LIVE(j) ? v[j][e] - mean : 0.f;
            q += v[j][e] * v[j][e];
        }
    rstd = 1.f / sqrtf(tem_wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        if (VB_LIVE(j)) {
            float ga[8], be[8];
            vb_ld8<T>(gamma + 8 * (lane + 64 * j), ga);
            vb_ld8<T>(beta + 8 * (lane + 64 * j), be);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = v[j][e] * rstd * ga[e] + be[e];
        }
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_ln_win_fwd(const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                    T* __restrict__ xw, float* __restrict__ mean, float* __restrict__ rstd, VbGeom g, int C,
                                                    float eps) {
    const int lane = tem_lane(), nch = C >> 3;
    const int64_t d = (int64_t)blockIdx.x * 4 + vb_wave();
    if (d >= g.ndst) return;
    const int64_t s = vb_dst_to_src(g, d);
    if (s < 0) {
        vb_zero_row<T, NCH>(xw + d * C, lane, nch);
        return;
    }
    float v[NCH][8], m, r;
    vb_load_row<T, NCH>(x + s * C, lane, nch, v);
    vb_normalise<T, NCH>(v, gamma, beta, lane, nch, C, eps, m, r);
    vb_store_row<T, NCH>(xw + d * C, lane, nch, v);
    if (mean && lane == 0) mean[s] = m, rstd[s] = r;
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_win_merge_ln_fwd(const T* __restrict__ y, const T* __restrict__ shortcut, const T* __restrict__ gamma,
                                                          const T* __restrict__ beta, T* __restrict__ x1, T* __restrict__ xn,
                                                          float* __restrict__ mean, float* __restrict__ rstd, VbGeom g, int C, float eps) {
    const int lane = tem_lane(), nch = C >> 3;
    const int64_t s = (int64_t)blockIdx.x * 4 + vb_wave();
    if (s >= g.nsrc) return;
    const int64_t d = vb_src_to_dst(g, s);
    float v[NCH][8], a[NCH][8], m, r;
    vb_load_row<T, NCH>(shortcut + s * C, lane, nch, v);
    vb_load_row<T, NCH>(y + d * C, lane, nch, a);
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] += a[j][e];
    vb_store_row<T, NCH>(x1 + s * C, lane, nch, v);
    vb_normalise<T, NCH>(v, gamma, beta, lane, nch, C, eps, m, r);
    vb_store_row<T, NCH>(xn + s * C, lane, nch, v);
    if (mean && lane == 0) mean[s] = m, rstd[s] = r;
}

// x (the row) and gr (its incoming gradient) -> gr = rstd (gh - mean_c(gh) - xhat mean_c(gh xhat)); dg += g xhat, db += g
template <int NCH>
__device__ __forceinline__ void vb_ln_bwd_row(float (&x)[NCH][8], float (&gr)[NCH][8], const float (&gam)[NCH][8], float (&dg)[NCH][8],
                                              float (&db)[NCH][8], int lane, int nch, int C, float m, float r) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = VB_LIVE(j) ? (x[j][e] - m) * r : 0.f, gg = gr[j][e];
            x[j][e] = xh;
            dg[j][e] += gg * xh;
            db[j][e] += gg;
            const float gh = gg * gam[j][e];
            gr[j][e] = gh;
            s1 += gh;
            s2 += gh * xh;
        }
    const float m1 = tem_wave_sum(s1) / (float)C, m2 = tem_wave_sum(s2) / (float)C;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) gr[j][e] = r * (gr[j][e] - m1 - x[j][e] * m2);
}

// the workgroup's four (dg, db) pairs, wave 0 + wave 1 + wave 2 + wave 3, to part[blockIdx.x][2][C]
template <int NCH>
__device__ __forceinline__ void vb_commit_partials(float (&dg)[NCH][8], float (&db)[NCH][8], float (*red)[2][NCH * 512], float* part, int lane,
                                                   int nch, int C, int wv) {
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (VB_LIVE(j)) {
                float* a = &red[wv - 1][0][8 * (lane + 64 * j)];
                float* b = &red[wv - 1][1][8 * (lane + 64 * j)];
                *(float4*)a = make_float4(dg[j][0], dg[j][1], dg[j][2], dg[j][3]);
                *(float4*)(a + 4) = make_float4(dg[j][4], dg[j][5], dg[j][6], dg[j][7]);
                *(float4*)b = make_float4(db[j][0], db[j][1], db[j][2], db[j][3]);
                *(float4*)(b + 4) = make_float4(db[j][4], db[j][5], db[j][6], db[j][7]);
            }
    }
    __syncthreads();
    if (wv != 0) return;
    float* out = part + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        if (VB_LIVE(j)) {
            const int c = 8 * (lane + 64 * j);
#pragma unroll
            for (int w = 0; w < 3; ++w)
#pragma unroll
                for (int e = 0; e < 8; ++e) dg[j][e] += red[w][0][c + e], db[j][e] += red[w][1][c + e];
            *(float4*)(out + c) = make_float4(dg[j][0], dg[j][1], dg[j][2], dg[j][3]);
            *(float4*)(out + c + 4) = make_float4(dg[j][4], dg[j][5], dg[j][6], dg[j][7]);
            *(float4*)(out + C + c) = make_float4(db[j][0], db[j][1], db[j][2], db[j][3]);
            *(float4*)(out + C + c + 4) = make_float4(db[j][4], db[j][5], db[j][6], db[j][7]);
        }
}

template <typename T, int NCH>
__device__ __forceinline__ void vb_load_gamma(const T* gamma, int lane, int nch, float (&gam)[NCH][8], float (&dg)[NCH][8], float (&db)[NCH][8]) {
    vb_load_row<T, NCH>(gamma, lane, nch, gam);
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) dg[j][e] = 0.f, db[j][e] = 0.f;
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_ln_win_bwd(const T* __restrict__ gw, const T* __restrict__ x, const T* __restrict__ gamma,
                                                    const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ dx,
                                                    float* __restrict__ part, VbGeom g, int C) {
    __shared__ __attribute__((aligned(16))) float red[3][2][NCH * 512];
    const int lane = tem_lane(), nch = C >> 3, wv = vb_wave();
    float gam[NCH][8], dg[NCH][8], db[NCH][8];
    vb_load_gamma<T, NCH>(gamma, lane, nch, gam, dg, db);
    const int64_t t0 = (int64_t)blockIdx.x * TEM_VB_SLAB;
    for (int i = 0; i < TEM_VB_SLAB / 4; ++i) {
        const int64_t s = t0 + 4 * i + wv;   // wave uniform
        if (s >= g.nsrc) break;
        float xr[NCH][8], gr[NCH][8];
        vb_load_row<T, NCH>(x + s * C, lane, nch, xr);
        vb_load_row<T, NCH>(gw + vb_src_to_dst(g, s) * C, lane, nch, gr);
        vb_ln_bwd_row<NCH>(xr, gr, gam, dg, db, lane, nch, C, mean[s], rstd[s]);
        vb_store_row<T, NCH>(dx + s * C, lane, nch, gr);
    }
    vb_commit_partials<NCH>(dg, db, red, part, lane, nch, C, wv);
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_win_merge_ln_bwd(const T* __restrict__ dx1, const T* __restrict__ dxn, const T* __restrict__ x1,
                                                          const T* __restrict__ gamma, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, T* __restrict__ dy, T* __restrict__ dshortcut,
                                                          float* __restrict__ part, VbGeom g, int C) {
    __shared__ __attribute__((aligned(16))) float red[3][2][NCH * 512];
    const int lane = tem_lane(), nch = C >> 3, wv = vb_wave();
    float gam[NCH][8], dg[NCH][8], db[NCH][8];
    vb_load_gamma<T, NCH>(gamma, lane, nch, gam, dg, db);
    const int64_t t0 = (int64_t)blockIdx.x * TEM_VB_SLAB;
    for (int i = 0; i < TEM_VB_SLAB / 4; ++i) {
        const int64_t d = t0 + 4 * i + wv;   // wave uniform
        if (d >= g.ndst) break;
        const int64_t s = vb_dst_to_src(g, d);
        if (s < 0) {
            vb_zero_row<T, NCH>(dy + d * C, lane, nch);
            continue;
        }
        float xr[NCH][8], gr[NCH][8], g1[NCH][8];
        vb_load_row<T, NCH>(x1 + s * C, lane, nch, xr);
        vb_load_row<T, NCH>(dxn + s * C, lane, nch, gr);
        vb_load_row<T, NCH>(dx1 + s * C, lane, nch, g1);
        vb_ln_bwd_row<NCH>(xr, gr, gam, dg, db, lane, nch, C, mean[s], rstd[s]);
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) gr[j][e] += g1[j][e];
        vb_store_row<T, NCH>(dshortcut + s * C, lane, nch, gr);
        vb_store_row<T, NCH>(dy + d * C, lane, nch, gr);
    }
    vb_commit_partials<NCH>(dg, db, red, part, lane, nch, C, wv);
}

// out[c] = part[0][c] + part[1][c] + ... in index order; columns < split go to out_a, the others to out_b
__global__ __launch_bounds__(256) void k_col_sum(const float* __restrict__ part, int nrows, int ncols, int split, float* __restrict__ out_a,
                                                 float* __restrict__ out_b) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    float s = 0.f;
    int r = 0;
    for (; r + 16 <= nrows; r += 16) {   // 16 loads in flight, added in index order
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part[(int64_t)(r + u) * ncols + c];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; r < nrows; ++r) s += part[(int64_t)r * ncols + c];
    if (c < split) out_a[c] = s;
    else out_b[c - split] = s;
}

// ---- bias + GELU
__device__ __forceinline__ float vb_erf_part(float z) { return erff(z * 0.70710678118654752f); }

template <typename T>
__global__ __launch_bounds__(256) void k_bias_gelu_fwd(const T* __restrict__ h, const T* __restrict__ bias, T* __restrict__ y, int64_t M, int C4) {
    const int nch = C4 >> 3;
    for (int ch = threadIdx.x; ch < nch; ch += 256) {
        float b[8];
        vb_ld8<T>(bias + 8 * ch, b);
        for (int64_t r = blockIdx.x; r < M; r += gridDim.x) {
            float v[8];
            vb_ld8<T>(h + r * C4 + 8 * ch, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float z = v[e] + b[e];
                v[e] = 0.5f * z * (1.f + vb_erf_part(z));
            }
            vb_st8<T>(y + r * C4 + 8 * ch, v);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bias_gelu_bwd(const T* __restrict__ dy, const T* __restrict__ h, const T* __restrict__ bias,
                                                       T* __restrict__ dh, float* __restrict__ part, int64_t M, int C4) {
    const int nch = C4 >> 3;
    for (int ch = threadIdx.x; ch < nch; ch += 256) {
        float b[8], acc[8];
        vb_ld8<T>(bias + 8 * ch, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int64_t r = blockIdx.x; r < M; r += gridDim.x) {
            float v[8], gy[8];
            vb_ld8<T>(h + r * C4 + 8 * ch, v);
            vb_ld8<T>(dy + r * C4 + 8 * ch, gy);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float z = v[e] + b[e];
                const float Phi = 0.5f * (1.f + vb_erf_part(z)), phi = expf(-0.5f * z * z) * 0.39894228040143268f;
                v[e] = gy[e] * (Phi + z * phi);
                acc[e] += v[e];
            }
            vb_st8<T>(dh + r * C4 + 8 * ch, v);
        }
        float* out = part + (int64_t)blockIdx.x * C4 + 8 * ch;
        *(float4*)out = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *(float4*)(out + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int vb_gelu_wgs(int64_t M) {
    const int64_t n = tem_cdiv(M, TEM_VB_GELU_ROWS);
    return (int)(n > VB_GELU_MAX_WG ? VB_GELU_MAX_WG : n);
}

static int vb_geom(const char* who, int64_t B, int H, int W, int C, int ws, VbGeom* g) {
    TEM_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: B, H, W, C must be positive", who);
    TEM_REQUIRE(C % 8 == 0, "%s: C = %d is no multiple of 8", who, C);
    TEM_REQUIRE(C <= TEM_VB_MAX_C, "%s: C = %d exceeds %d", who, C, TEM_VB_MAX_C);
    TEM_REQUIRE(ws >= 0, "%s: negative window size %d", who, ws);
    TEM_REQUIRE(H <= 32768 && W <= 32768 && ws <= 32768, "%s: H, W and the window size are at most 32768", who);
    const int64_t nWh = ws ? tem_cdiv(H, ws) : 1, nWw = ws ? tem_cdiv(W, ws) : 1;
    const int64_t Hp = ws ? nWh * ws : H, Wp = ws ? nWw * ws : W;
    TEM_REQUIRE(B * Hp * Wp <= 0x7fffffffLL, "%s: %lld tokens exceed 2^31 - 1", who, (long long)(B * Hp * Wp));
    g->H = H, g->W = W, g->ws = ws, g->Wp = (int)Wp, g->nWw = (int)nWw, g->nW = (int)(nWh * nWw);
    g->nsrc = B * H * W, g->ndst = B * Hp * Wp;
    return TEM_OK;
}

extern "C" int64_t tem_vit_block_ws(int op, int64_t B, int H, int W, int C, int ws) {
    const char* who = "tem_vit_block_ws";
    if (op == TEM_VB_BIAS_GELU_BWD) {
        if (B <= 0 || C <= 0 || C % 8 != 0) {
            tem_set_error("%s: M = %lld rows of C4 = %d (M > 0, C4 a positive multiple of 8)", who, (long long)B, C);
            return -1;
        }
        return (int64_t)vb_gelu_wgs(B) * C * 4;
    }
    if (op != TEM_VB_LN_WINDOWS_BWD && op != TEM_VB_WINDOW_MERGE_BWD) {
        tem_set_error("%s: unknown operation %d", who, op);
        return -1;
    }
    VbGeom g;
    if (vb_geom(who, B, H, W, C, ws, &g) != TEM_OK) return -1;
    return tem_cdiv(op == TEM_VB_LN_WINDOWS_BWD ? g.nsrc : g.ndst, TEM_VB_SLAB) * 2 * C * 4;
}

static int vb_check_ptrs(const char* who, int n, const void* const* ptrs, const char* const* names) {
    for (int i = 0; i < n; ++i) TEM_REQUIRE(ptrs[i], "%s: null pointer (%s)", who, names[i]);
    for (int i = 0; i < n; ++i) TEM_REQUIRE(((uintptr_t)ptrs[i] & 15u) == 0, "%s: %s must be 16-byte aligned", who, names[i]);
    return TEM_OK;
}
static int vb_check_st(const char* who, int st) {
    TEM_REQUIRE(st == TEM_ST_F32 || st == TEM_ST_F16 || st == TEM_ST_BF16, "%s: unknown storage type %d", who, st);
    return TEM_OK;
}
static int vb_check_ws(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
    TEM_REQUIRE(ws && ((uintptr_t)ws & 15u) == 0, "%s: a 16-byte aligned workspace is needed", who);
    if (ws_bytes < need) {
        tem_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)need);
        return TEM_EWS;
    }
    return TEM_OK;
}

// F(T-tag, NCH-tag) with the storage type and the chunk count as template arguments
#define VB_DISPATCH_NCH(T, C, CALL)                     \
    do {                                                \
        switch (((C) + 511) / 512) {                    \
            case 1: CALL(T, 1); break;                  \
            case 2: CALL(T, 2); break;                  \
            case 3: CALL(T, 3); break;                  \
            default: CALL(T, 4); break;                 \
        }                                               \
    } while (0)
#define VB_DISPATCH(st, C, CALL)                                      \
    do {                                                              \
        if ((st) == TEM_ST_F32) VB_DISPATCH_NCH(float, C, CALL);      \
        else if ((st) == TEM_ST_F16) VB_DISPATCH_NCH(_Float16, C, CALL); \
        else VB_DISPATCH_NCH(__bf16, C, CALL);                        \
    } while (0)

static int vb_col_sum(const char* who, const float* part, int64_t nrows, int ncols, int split, float* a, float* b, hipStream_t s) {
    hipLaunchKernelGGL(k_col_sum, dim3((unsigned)tem_cdiv(ncols, 256)), dim3(256), 0, s, part, (int)nrows, ncols, split, a, b);
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

extern "C" int tem_ln_windows_fwd(const void* x, const void* gamma, const void* beta, void* xw, float* mean, float* rstd, int B, int H, int W,
                                  int C, int ws, float eps, int st, tem_stream_t stream) {
    const char* who = "tem_ln_windows_fwd";
    const void* ptrs[4] = {x, gamma, beta, xw};
    const char* names[4] = {"x", "gamma", "beta", "xw"};
    TEM_TRY(vb_check_ptrs(who, 4, ptrs, names));
    TEM_REQUIRE((mean != nullptr) == (rstd != nullptr), "%s: mean and rstd come as a pair", who);
    VbGeom g;
    TEM_TRY(vb_geom(who, B, H, W, C, ws, &g));
    TEM_TRY(vb_check_st(who, st));
    TEM_REQUIRE(eps == eps && eps >= 0.f, "%s: eps must be non-negative", who);
    const dim3 grid((unsigned)tem_cdiv(g.ndst, 4));
#define VB_CALL(T, N) \
    hipLaunchKernelGGL((k_ln_win_fwd<T, N>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)gamma, (const T*)beta, (T*)xw, mean, rstd, g, C, eps)
    VB_DISPATCH(st, C, VB_CALL);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

extern "C" int tem_window_merge_ln_fwd(const void* y, const void* shortcut, const void* gamma, const void* beta, void* x1, void* xn, float* mean,
                                       float* rstd, int B, int H, int W, int C, int ws, float eps, int st, tem_stream_t stream) {
    const char* who = "tem_window_merge_ln_fwd";
    const void* ptrs[6] = {y, shortcut, gamma, beta, x1, xn};
    const char* names[6] = {"y", "shortcut", "gamma", "beta", "x1", "xn"};
    TEM_TRY(vb_check_ptrs(who, 6, ptrs, names));
    TEM_REQUIRE((mean != nullptr) == (rstd != nullptr), "%s: mean and rstd come as a pair", who);
    VbGeom g;
    TEM_TRY(vb_geom(who, B, H, W, C, ws, &g));
    TEM_TRY(vb_check_st(who, st));
    TEM_REQUIRE(eps == eps && eps >= 0.f, "%s: eps must be non-negative", who);
    const dim3 grid((unsigned)tem_cdiv(g.nsrc, 4));
#define VB_CALL(T, N)                                                                                                                    \
    hipLaunchKernelGGL((k_win_merge_ln_fwd<T, N>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)y, (const T*)shortcut, (const T*)gamma, \
                       (const T*)beta, (T*)x1, (T*)xn, mean, rstd, g, C, eps)
    VB_DISPATCH(st, C, VB_CALL);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

extern "C" int tem_ln_windows_bwd(const void* g_win, const void* x, const void* gamma, const float* mean, const float* rstd, void* dx,
                                  float* dgamma, float* dbeta, int B, int H, int W, int C, int ws, int st, void* wsp, int64_t ws_bytes,
                                  tem_stream_t stream) {
    const char* who = "tem_ln_windows_bwd";
    const void* ptrs[8] = {g_win, x, gamma, mean, rstd, dx, dgamma, dbeta};
    const char* names[8] = {"g", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta"};
    TEM_TRY(vb_check_ptrs(who, 8, ptrs, names));
    VbGeom g;
    TEM_TRY(vb_geom(who, B, H, W, C, ws, &g));
    TEM_TRY(vb_check_st(who, st));
    TEM_TRY(vb_check_ws(who, wsp, ws_bytes, tem_vit_block_ws(TEM_VB_LN_WINDOWS_BWD, B, H, W, C, ws)));
    const int64_t nwg = tem_cdiv(g.nsrc, TEM_VB_SLAB);
    float* part = (float*)wsp;
#define VB_CALL(T, N)                                                                                                                        \
    hipLaunchKernelGGL((k_ln_win_bwd<T, N>), dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const T*)g_win, (const T*)x, (const T*)gamma, \
                       mean, rstd, (T*)dx, part, g, C)
    VB_DISPATCH(st, C, VB_CALL);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return vb_col_sum(who, part, nwg, 2 * C, C, dgamma, dbeta, (hipStream_t)stream);
}

extern "C" int tem_window_merge_ln_bwd(const void* dx1, const void* dxn, const void* x1, const void* gamma, const float* mean, const float* rstd,
                                       void* dy, void* dshortcut, float* dgamma, float* dbeta, int B, int H, int W, int C, int ws, int st,
                                       void* wsp, int64_t ws_bytes, tem_stream_t stream) {
    const char* who = "tem_window_merge_ln_bwd";
    const void* ptrs[10] = {dx1, dxn, x1, gamma, mean, rstd, dy, dshortcut, dgamma, dbeta};
    const char* names[10] = {"dx1", "dxn", "x1", "gamma", "mean", "rstd", "dy", "dshortcut", "dgamma", "dbeta"};
    TEM_TRY(vb_check_ptrs(who, 10, ptrs, names));
    VbGeom g;
    TEM_TRY(vb_geom(who, B, H, W, C, ws, &g));
    TEM_TRY(vb_check_st(who, st));
    TEM_TRY(vb_check_ws(who, wsp, ws_bytes, tem_vit_block_ws(TEM_VB_WINDOW_MERGE_BWD, B, H, W, C, ws)));
    const int64_t nwg = tem_cdiv(g.ndst, TEM_VB_SLAB);
    float* part = (float*)wsp;
#define VB_CALL(T, N)                                                                                                                     \
    hipLaunchKernelGGL((k_win_merge_ln_bwd<T, N>), dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const T*)dx1, (const T*)dxn,       \
                       (const T*)x1, (const T*)gamma, mean, rstd, (T*)dy, (T*)dshortcut, part, g, C)
    VB_DISPATCH(st, C, VB_CALL);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return vb_col_sum(who, part, nwg, 2 * C, C, dgamma, dbeta, (hipStream_t)stream);
}

static int vb_gelu_dims(const char* who, int64_t M, int C4, int st) {
    TEM_REQUIRE(M > 0 && C4 > 0, "%s: M and C4 must be positive", who);
    TEM_REQUIRE(C4 % 8 == 0, "%s: C4 = %d is no multiple of 8", who, C4);
    return vb_check_st(who, st);
}

extern "C" int tem_bias_gelu_fwd(const void* h, const void* bias, void* y, int64_t M, int C4, int st, tem_stream_t stream) {
    const char* who = "tem_bias_gelu_fwd";
    const void* ptrs[3] = {h, bias, y};
    const char* names[3] = {"h", "bias", "y"};
    TEM_TRY(vb_check_ptrs(who, 3, ptrs, names));
    TEM_TRY(vb_gelu_dims(who, M, C4, st));
    const dim3 grid((unsigned)(M < 2048 ? M : 2048));
#define VB_CALL(T) hipLaunchKernelGGL((k_bias_gelu_fwd<T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)h, (const T*)bias, (T*)y, M, C4)
    if (st == TEM_ST_F32) VB_CALL(float);
    else if (st == TEM_ST_F16) VB_CALL(_Float16);
    else VB_CALL(__bf16);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

extern "C" int tem_bias_gelu_bwd(const void* dy, const void* h, const void* bias, void* dh, float* dbias, int64_t M, int C4, int st, void* wsp,
                                 int64_t ws_bytes, tem_stream_t stream) {
    const char* who = "tem_bias_gelu_bwd";
    const void* ptrs[5] = {dy, h, bias, dh, dbias};
    const char* names[5] = {"dy", "h", "bias", "dh", "dbias"};
    TEM_TRY(vb_check_ptrs(who, 5, ptrs, names));
    TEM_TRY(vb_gelu_dims(who, M, C4, st));
    TEM_TRY(vb_check_ws(who, wsp, ws_bytes, tem_vit_block_ws(TEM_VB_BIAS_GELU_BWD, M, 1, 1, C4, 0)));
    const int nwg = vb_gelu_wgs(M);
    float* part = (float*)wsp;
#define VB_CALL(T) \
    hipLaunchKernelGGL((k_bias_gelu_bwd<T>), dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)h, (const T*)bias, (T*)dh, part, M, C4)
    if (st == TEM_ST_F32) VB_CALL(float);
    else if (st == TEM_ST_F16) VB_CALL(_Float16);
    else VB_CALL(__bf16);
#undef VB_CALL
    TEM_CHECK_LAUNCH(who);
    return vb_col_sum(who, part, nwg, C4, C4, dbias, nullptr, (hipStream_t)stream);
}
