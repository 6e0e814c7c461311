// attention_bwd.hip -- the gradients of attention.hip (DESIGN.md "Attention", part "Backward").  With L[i] the log-sum-exp of
// logit row i (stored by k_attn_fwd built with its LSE flag: tem_attention_fwd_ex) and dO the incoming gradient:
//
//   P[i][j] = exp(S[i][j] - L[i])      delta[i] = dO[i] . O[i]      dP[i][j] = dO[i] . v[j]      dS[i][j] = P[i][j] (dP[i][j] - delta[i])
//   dV[j] = sum_i P[i][j] dO[i]        dK[j] = scale sum_i dS[i][j] q[i]
//   dBh[i][x] = sum_{j: hj = x} dS[i][j]    dBw[i][y] = sum_{j: wj = y} dS[i][j]            (adjoint of the bias pre-pass, [N][H + W])
//   dQ[i] = scale sum_j dS[i][j] k[j] + sum_x dBh[i][x] Rh[hi - x + H-1] + sum_y dBw[i][y] Rw[wi - y + W-1]
//   dRh[r] = sum_{b, a} sum_{i, x: hi - x + H-1 = r} dBh[i][x] q[i]                            dRw likewise
//
// S, P, dP and dS never reach global memory.  Six launches with table gradients (four without tables), the two big ones on the forward's 32x32 MFMA layout (attention.hip's header:
// the stationary token is the accumulator COLUMN = lane & 31, a lane holds 16 streamed tokens of each 32-token block, token
// = 8 (r / 4) + 4 (lane / 32) + r % 4 of register r, and accumulator registers rounded once ARE the B operand of the next product):
//   k_attn_bwd_prep     delta, an fp32 fma chain in channel order; the bias pre-pass k_attn_relpos runs again into the workspace
//   k_attn_bwd_kv       key-stationary: a workgroup of 4 waves owns 128 keys, wave w 32 of them with its K and V rows in registers
//                       as B operands for the whole march.  Query tiles (64 queries, 32 for fp32) stream through LDS: Q and dO
//                       rows, each staged twice from ONE global load -- key-major rows for the 16-byte A fragments of
//                       S = Q K^T and dP = dO V^T, 192-byte rows for the transposing reads (ds_read_b64_tr_b16) that give the A
//                       operands of dV^T += dO^T P and dK^T += Q^T dS -- plus their L, delta and bias rows.  The lane's own
//                       (hj, wj) are constants of the kernel.  scale multiplies the fp32 accumulator of dK once, at the end.
//   k_attn_bwd_q        query-stationary, the forward's structure: Q and dO rows in registers, L and delta per-lane scalars,
//                       K tiles (both layouts) and V tiles (rows) through LDS: S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T -
//                       delta), dQ^T += K^T dS^T.  dB accumulates in LDS, one fp32 row of (H + W) | 1 floats a LANE (lanes l and
//                       l ^ 32 hold disjoint keys of one query), the two rows of a query are added half 0 + half 1 after the
//                       march and go to the workspace; the epilogue adds the table part of dQ from them in fp32 and rounds dQ once.
//   k_attn_relpos_bwd   table gradients: partial sums per (batch, head) -- one workgroup a table row, its terms dealt to NG
//                       thread groups in a fixed pattern and added in group order -- then k_attn_relpos_bwd_sum over (batch, head).
// Masking: a key column >= N gets -inf before the exponent (P = 0 exactly) and its K and V rows are zeros, as in the forward.
// A padded QUERY row of k_attn_bwd_kv contributes exact zeros: its Q and dO rows, L, delta and bias row are staged as ZEROS
// and its P is replaced by the constant 0 (a select, not a product), so dS = 0 (0 - 0); never 0 x garbage.  Padded keys of the
// kv kernel and padded queries of the q kernel compute on zeros with P forced to 0 / finite values and are not stored.
// 16-bit roundings on an element's path, besides its one final store (tests/test_gpu_attention_bwd.py builds its band from
// this count): dV -- P (1).  dK, dQ -- dS as the MFMA operand (1), the stored O inside delta (1); P inside dS stays fp32.
// dRh, dRw -- the stored O inside delta (1): dB is summed from the fp32 dS BEFORE it is packed, and stays fp32 to the end.
// No atomics anywhere: same input, same bits.
#include "attention.h"

#define AT_BWD_NW4_MAX_HW 29    // k_attn_bwd_q with tables: 4 waves while tiles + 384 rows of (H + W) | 1 floats stay within 80 KB,
#define AT_BWD_NW2_MAX_HW 167   // 2 waves while tiles + 192 rows fit the 160 KB, 1 wave (96 rows) up to TEM_ATTN_BWD_MAX_HW

struct AtBwdArgs {
    const void *q, *k, *v, *dout;
    void *dq, *dk, *dv;
    int64_t qs[3], ks[3], vs[3], dos[3], dqs[3], dks[3], dvs[3];   // element strides of (batch, head, token); unit stride along D
    const float *lse, *delta;                                      // [B][nH][N]
    const float* bias;                                             // [B][nH][N][H + W] of k_attn_relpos, or NULL
    float* dbias;                                                  // the same shape: dB
    const void *rel_h, *rel_w;
    int nH, N, H, W;
    float scale;
};

template <typename T, int D>
struct AtBwdLds {
    typedef AtLds<T, D> L;
    static constexpr int BN = AtTile<T>::BN;
    static constexpr int Q_TILES = BN * (2 * L::KS + L::VS);    // k_attn_bwd_q: K rows | V rows | K for transposing reads
    static constexpr int KV_TILES = 2 * BN * (L::KS + L::VS);   // k_attn_bwd_kv: Q rows | dO rows | Q, dO for transposing reads
};

// One tile of BN token rows from global into LDS: `rows` key-major with the K stride (or NULL), `tr` with the V stride and
// zeros in channels D .. DP (or NULL); rows >= N are zeros.  One 16-byte global load serves both copies.
template <typename T, int D, int NTHR>
__device__ __forceinline__ void at_stage(const T* base, int64_t stride, int r0, int N, unsigned char* rows, unsigned char* tr, int tid) {
    typedef AtLds<T, D> L;
    constexpr int BN = AtTile<T>::BN, EPC = 16 / (int)sizeof(T), CHK = D / EPC, CHV = L::DP / EPC, KS = L::KS, VS = L::VS;
    for (int idx = tid; idx < BN * CHV; idx += NTHR) {
        const int r = idx / CHV, ch = idx - r * CHV, j = r0 + r;
        const uint4 val = (j < N && ch < CHK) ? *(const uint4*)(base + (int64_t)j * stride + ch * EPC) : make_uint4(0, 0, 0, 0);
        if (tr) *(uint4*)(tr + r * VS + ch * 16) = val;
        if (rows && ch < CHK) {
            if constexpr (L::F32) {   // rows of D + 2 floats are 8-byte aligned
                *(uint2*)(rows + r * KS + ch * 16) = make_uint2(val.x, val.y);
                *(uint2*)(rows + r * KS + ch * 16 + 8) = make_uint2(val.z, val.w);
            } else {
                *(uint4*)(rows + r * KS + ch * 16) = val;
            }
        }
    }
}

// acc[t] = A B^T for the NT 32-row blocks of a tile: A = the tile's rows from LDS (K stride), B = the lane's stationary row in registers
template <typename T, int D>
__device__ __forceinline__ void at_rows_x_regs(const unsigned char* rows, const uint4* bf, const float* bf32, int l32, int h,
                                               at_fx16* acc) {
    typedef AtLds<T, D> L;
    constexpr int NT = AtTile<T>::NT, KS = L::KS, NQ = L::F32 ? D / 2 : D / 16;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        if constexpr (L::F32) {
#pragma unroll
            for (int st = 0; st < NQ; ++st) {
                const float af = *(const float*)(rows + (32 * t + l32) * KS + (2 * st + h) * 4);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf32[st], acc[t], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int st = 0; st < NQ; ++st) {
                const uint4 af = *(const uint4*)(rows + (32 * t + l32) * KS + st * 32 + h * 16);
                acc[t] = at_mfma16<T>(af, bf[st], acc[t]);
            }
        }
    }
}

// o[cb] += X^T w: X = the tile in the V-stride layout (transposing reads), w = accumulator registers of the first products: the k
// slots are the streamed tokens the lane holds (attention.hip, second product)
template <typename T, int D>
__device__ __forceinline__ void at_tr_x_acc(const unsigned char* tr, const at_fx16* w, int l32, int h, int v_lane, at_fx16* o) {
    typedef AtLds<T, D> L;
    constexpr int NT = AtTile<T>::NT, NCB = L::DP / 32, VS = L::VS;
    if constexpr (L::F32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tok = 8 * (r >> 2) + 4 * h + (r & 3);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const float xf = *(const float*)(tr + tok * VS + (cb * 32 + l32) * 4);
                o[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xf, w[0][r], o[cb], 0, 0, 0);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {   // a K = 16 step: registers 8 s2 .. 8 s2 + 7 = tokens 16 s2 + 4 h + (0..3), + 8
                const uint4 pf = make_uint4(at_pk<T>(w[t][8 * s2 + 0], w[t][8 * s2 + 1]), at_pk<T>(w[t][8 * s2 + 2], w[t][8 * s2 + 3]),
                                            at_pk<T>(w[t][8 * s2 + 4], w[t][8 * s2 + 5]), at_pk<T>(w[t][8 * s2 + 6], w[t][8 * s2 + 7]));
                const unsigned char* xb = tr + (32 * t + 16 * s2) * VS + v_lane;
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const uint2 x0 = at_tr_read(xb + cb * 64), x1 = at_tr_read(xb + cb * 64 + 8 * VS);
                    o[cb] = at_mfma16<T>(make_uint4(x0.x, x0.y, x1.x, x1.y), pf, o[cb]);
                }
            }
    }
}

template <typename T>
__device__ __forceinline__ float at_exp(float x) {   // the forward's exponentials: expf for fp32 tensors, v_exp_f32 for 16-bit ones
    if constexpr (std::is_same<T, float>::value) return expf(x);
    else return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
}

// the lane's stationary row as the B operand of the first products: 16-bit: 8 channels a step; fp32: 1 a step; zeros past N
template <typename T, int D>
__device__ __forceinline__ void at_load_regs(const T* base, int64_t stride, int tok, int N, int h, uint4* bf, float* bf32) {
    constexpr bool F32 = std::is_same<T, float>::value;
    constexpr int NQ = F32 ? D / 2 : D / 16;
    if constexpr (F32) {
#pragma unroll
        for (int st = 0; st < NQ; ++st) bf32[st] = tok < N ? (float)base[(int64_t)tok * stride + 2 * st + h] : 0.f;
    } else {
#pragma unroll
        for (int st = 0; st < NQ; ++st)
            bf[st] = tok < N ? *(const uint4*)(base + (int64_t)tok * stride + 16 * st + 8 * h) : make_uint4(0, 0, 0, 0);
    }
}

// the lane's column of NCB transposed accumulators (rows = channels) to its token's row, `mul` applied in fp32, one rounding
template <typename T, int D>
__device__ __forceinline__ void at_store_col(T* row, const at_fx16* o, float mul, int h) {
    constexpr int NCB = AtLds<T, D>::DP / 32;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = cb * 32 + 8 * g + 4 * h;   // 4 consecutive channels: registers 4 g .. 4 g + 3
            if (c >= D) continue;
            const float y0 = o[cb][4 * g] * mul, y1 = o[cb][4 * g + 1] * mul, y2 = o[cb][4 * g + 2] * mul, y3 = o[cb][4 * g + 3] * mul;
            if constexpr (std::is_same<T, float>::value)
                *(float4*)(row + c) = make_float4(y0, y1, y2, y3);
            else
                *(uint2*)(row + c) = make_uint2(at_pk<T>(y0, y1), at_pk<T>(y2, y3));
        }
}

// ---- delta[b][a][i] = sum_c dO[i][c] O[i][c]: one thread a row, fp32 fma chain in channel order
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_bwd_prep(const T* __restrict__ o, int64_t os0, int64_t os1, int64_t os2, const T* __restrict__ dout,
                                                       int64_t ds0, int64_t ds1, int64_t ds2, int nH, int N, int64_t total,
                                                       float* __restrict__ delta) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int i = (int)(idx % N);
        const int64_t bh = idx / N, bb = bh / nH, hd = bh % nH;
        const T* op = o + bb * os0 + hd * os1 + (int64_t)i * os2;
        const T* gp = dout + bb * ds0 + hd * ds1 + (int64_t)i * ds2;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
            const float4 x = at_ld4<T>(gp + c), y = at_ld4<T>(op + c);
            acc = fmaf(x.x, y.x, acc);
            acc = fmaf(x.y, y.y, acc);
            acc = fmaf(x.z, y.z, acc);
            acc = fmaf(x.w, y.w, acc);
        }
        delta[idx] = acc;
    }
}

// ---- key-stationary: grid (key tiles of 128, B nH), 256 threads, dynamic LDS = Q | dO | Q^T-read | dO^T-read | L | delta | bias rows
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_bwd_kv(AtBwdArgs a) {
    typedef AtLds<T, D> L;
    constexpr bool F32 = L::F32;
    constexpr int NT = AtTile<T>::NT, BM = AtTile<T>::BN, NCB = L::DP / 32, KS = L::KS, VS = L::VS;
    constexpr int NQ = F32 ? D / 2 : D / 16, NW = 4, NTHR = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char at_lds[];
    unsigned char* ldsQ = at_lds;
    unsigned char* ldsG = ldsQ + BM * KS;
    unsigned char* ldsQt = ldsG + BM * KS;
    unsigned char* ldsGt = ldsQt + BM * VS;
    float* ldsL = (float*)(at_lds + AtBwdLds<T, D>::KV_TILES);
    float* ldsDl = ldsL + BM;
    float* ldsB = ldsDl + BM;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, bb = bh / a.nH, hd = bh - bb * a.nH;
    const int N = a.N, H = a.H, W = a.W, HW = H + W, RS = HW | 1;
    const int k0 = blockIdx.x * (32 * NW);
    const int kj = k0 + 32 * wv + l32;                                 // this lane's key
    const bool wave_live = k0 + 32 * wv < N;                           // wave uniform
    const bool key_live = kj < N;
    const int hj = key_live ? kj / W : 0, wj = key_live ? kj - hj * W : 0;
    const T* qp = (const T*)a.q + bb * a.qs[0] + hd * a.qs[1];
    const T* gp = (const T*)a.dout + bb * a.dos[0] + hd * a.dos[1];
    const bool has_bias = a.bias != nullptr;                           // workgroup uniform
    const float* lp = a.lse + (int64_t)bh * N;
    const float* dlp = a.delta + (int64_t)bh * N;

    uint4 kf[F32 ? 1 : NQ], vf[F32 ? 1 : NQ];
    float kf32[F32 ? NQ : 1], vf32[F32 ? NQ : 1];
    at_load_regs<T, D>((const T*)a.k + bb * a.ks[0] + hd * a.ks[1], a.ks[2], kj, N, h, kf, kf32);
    at_load_regs<T, D>((const T*)a.v + bb * a.vs[0] + hd * a.vs[1], a.vs[2], kj, N, h, vf, vf32);

    at_fx16 dk[NCB], dv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[cb][r] = 0.f, dv[cb][r] = 0.f;
    const int p16 = lane & 15;
    const int v_lane = (4 * h + (p16 >> 2)) * VS + ((lane >> 4) & 1) * 32 + (p16 & 3) * 8;   // transposing-read address of this lane

    for (int i0 = 0; i0 < N; i0 += BM) {
        __syncthreads();   // the previous tile has been read
        at_stage<T, D, NTHR>(qp, a.qs[2], i0, N, ldsQ, ldsQt, tid);
        at_stage<T, D, NTHR>(gp, a.dos[2], i0, N, ldsG, ldsGt, tid);
        if (tid < BM) {
            const bool live = i0 + tid < N;
            ldsL[tid] = live ? lp[i0 + tid] : 0.f;
            ldsDl[tid] = live ? dlp[i0 + tid] : 0.f;
        }
        if (has_bias) {   // rows i0 .. i0 + BM of the pre-pass result are contiguous
            const float* bp = a.bias + ((int64_t)bh * N + i0) * HW;
            const int valid = (N - i0 < BM ? N - i0 : BM) * HW;
            for (int idx = tid; idx < BM * HW; idx += NTHR) {
                const int r = idx / HW;
                ldsB[r * RS + (idx - r * HW)] = idx < valid ? bp[idx] : 0.f;
            }
        }
        __syncthreads();
        if (!wave_live) continue;   // a wave without a stored key keeps the barriers only

        // ---- S = Q K^T, dP = dO V^T: rows = queries, column = this lane's key
        at_fx16 s[NT], dp[NT];
        at_rows_x_regs<T, D>(ldsQ, kf, kf32, l32, h, s);
        at_rows_x_regs<T, D>(ldsG, vf, vf32, l32, h, dp);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int iq = 32 * t + 8 * (r >> 2) + 4 * h + (r & 3);   // the query of register r, within the tile
                float x = s[t][r] * a.scale;
                if (has_bias) x += ldsB[iq * RS + hj] + ldsB[iq * RS + H + wj];
                const float e = at_exp<T>(x - ldsL[iq]);
                const float p = (key_live && i0 + iq < N) ? e : 0.f;      // padded rows and columns: the constant 0
                s[t][r] = p;
                dp[t][r] = p * (dp[t][r] - ldsDl[iq]);
            }
        // ---- dV^T += dO^T P, dK^T += Q^T dS: rows = channels, column = this lane's key
        at_tr_x_acc<T, D>(ldsGt, s, l32, h, v_lane, dv);
        at_tr_x_acc<T, D>(ldsQt, dp, l32, h, v_lane, dk);
    }

    if (!key_live) return;
    at_store_col<T, D>((T*)a.dk + bb * a.dks[0] + hd * a.dks[1] + (int64_t)kj * a.dks[2], dk, a.scale, h);
    at_store_col<T, D>((T*)a.dv + bb * a.dvs[0] + hd * a.dvs[1] + (int64_t)kj * a.dvs[2], dv, 1.f, h);
}

// ---- query-stationary: grid (query tiles of 32 NW, B nH), 64 NW threads, dynamic LDS = K | V | K^T-read | bias rows | dB rows
template <typename T, int D, int NW>
__global__ __launch_bounds__(64 * NW) void k_attn_bwd_q(AtBwdArgs a) {
    typedef AtLds<T, D> L;
    constexpr bool F32 = L::F32;
    constexpr int NT = AtTile<T>::NT, BN = AtTile<T>::BN, NCB = L::DP / 32, KS = L::KS, VS = L::VS;
    constexpr int NQ = F32 ? D / 2 : D / 16, NTHR = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char at_lds[];
    unsigned char* ldsK = at_lds;
    unsigned char* ldsV = ldsK + BN * KS;
    unsigned char* ldsKt = ldsV + BN * KS;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, bb = bh / a.nH, hd = bh - bb * a.nH;
    const int N = a.N, H = a.H, W = a.W, HW = H + W, RS = HW | 1;
    const int q0 = blockIdx.x * (32 * NW);
    const int qi = q0 + 32 * wv + l32;                                 // this lane's query
    const bool wave_live = q0 + 32 * wv < N;                           // wave uniform
    const T* kp = (const T*)a.k + bb * a.ks[0] + hd * a.ks[1];
    const T* vp = (const T*)a.v + bb * a.vs[0] + hd * a.vs[1];
    const bool has_bias = a.bias != nullptr;                           // workgroup uniform
    float* ldsB = (float*)(at_lds + AtBwdLds<T, D>::Q_TILES);          // 32 NW bias rows
    float* ldsDB = ldsB + 32 * NW * RS;                                // 64 NW rows of dB: row 64 wv + lane

    if (has_bias) {
        const float* bp = a.bias + ((int64_t)bh * N + q0) * HW;
        const int valid = (N - q0 < 32 * NW ? N - q0 : 32 * NW) * HW;
        for (int idx = tid; idx < 32 * NW * HW; idx += NTHR) {
            const int r = idx / HW;
            ldsB[r * RS + (idx - r * HW)] = idx < valid ? bp[idx] : 0.f;
        }
        for (int idx = tid; idx < 64 * NW * RS; idx += NTHR) ldsDB[idx] = 0.f;
    }

    uint4 qf[F32 ? 1 : NQ], gf[F32 ? 1 : NQ];
    float qf32[F32 ? NQ : 1], gf32[F32 ? NQ : 1];
    at_load_regs<T, D>((const T*)a.q + bb * a.qs[0] + hd * a.qs[1], a.qs[2], qi, N, h, qf, qf32);
    at_load_regs<T, D>((const T*)a.dout + bb * a.dos[0] + hd * a.dos[1], a.dos[2], qi, N, h, gf, gf32);
    const float Lq = qi < N ? a.lse[(int64_t)bh * N + qi] : 0.f;
    const float dl = qi < N ? a.delta[(int64_t)bh * N + qi] : 0.f;

    at_fx16 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
    const float NEG_INF = -__builtin_inff();
    const float inv_w = 1.f / (float)W;
    const float* brow = ldsB + (32 * wv + l32) * RS;
    float* dbrow = ldsDB + (64 * wv + lane) * RS;
    const int p16 = lane & 15;
    const int v_lane = (4 * h + (p16 >> 2)) * VS + ((lane >> 4) & 1) * 32 + (p16 & 3) * 8;   // transposing-read address of this lane

    for (int j0 = 0; j0 < N; j0 += BN) {
        __syncthreads();   // the previous tile has been read (first trip: the bias and dB rows are in place)
        at_stage<T, D, NTHR>(kp, a.ks[2], j0, N, ldsK, ldsKt, tid);
        at_stage<T, D, NTHR>(vp, a.vs[2], j0, N, ldsV, nullptr, tid);
        __syncthreads();
        if (!wave_live) continue;   // a wave without a stored row keeps the barriers only

        // ---- S^T = K Q^T, dP^T = V dO^T: rows = keys, column = this lane's query
        at_fx16 s[NT], dp[NT];
        at_rows_x_regs<T, D>(ldsK, qf, qf32, l32, h, s);
        at_rows_x_regs<T, D>(ldsV, gf, gf32, l32, h, dp);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int jb = j0 + 32 * t + 8 * g + 4 * h;            // 4 consecutive keys: registers 4 g .. 4 g + 3
                int hj = 0, wj = 0;
                if (has_bias) {   // jb / W by a float product: (jb + 0.5) / W is at least 1 / 512 away from an integer
                    hj = (int)(((float)jb + 0.5f) * inv_w);
                    wj = jb - hj * W;
                }
                float hacc = 0.f;                                      // dBh of the grid row the group is in
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float x = NEG_INF;
                    if (jb + u < N) {
                        x = s[t][4 * g + u] * a.scale;
                        if (has_bias) x += brow[hj] + brow[H + wj];
                    }
                    const float p = at_exp<T>(x - Lq);                 // masked key: exp(-inf) = 0; its dP is 0 (V row of zeros)
                    const float ds = p * (dp[t][4 * g + u] - dl);
                    dp[t][4 * g + u] = ds;
                    if (has_bias) {
                        if (jb + u < N) {
                            hacc += ds;
                            dbrow[H + wj] += ds;
                        }
                        if (++wj == W) {
                            if (hj < H) dbrow[hj] += hacc;
                            hacc = 0.f;
                            wj = 0;
                            ++hj;
                        }
                    }
                }
                if (has_bias && hj < H) dbrow[hj] += hacc;
            }
        // ---- dQ^T += K^T dS^T: rows = channels, column = this lane's query
        at_tr_x_acc<T, D>(ldsKt, dp, l32, h, v_lane, o);
    }

    if (has_bias) {   // the two rows of a query, half 0 + half 1, into the first and into the workspace
        __syncthreads();
        if (wave_live) {
            float* w0 = ldsDB + 64 * wv * RS;
            for (int idx = lane; idx < 32 * HW; idx += 64) {
                const int r = idx / HW, x = idx - r * HW;
                const float sum = w0[r * RS + x] + w0[(r + 32) * RS + x];
                w0[r * RS + x] = sum;
                if (q0 + 32 * wv + r < N) a.dbias[((int64_t)bh * N + q0 + 32 * wv + r) * HW + x] = sum;
            }
        }
        __syncthreads();
    }
    if (!wave_live || qi >= N) return;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] *= a.scale;
    if (has_bias) {   // the table part of dQ: sum_x dBh[x] Rh[hi - x + H-1] + sum_y dBw[y] Rw[wi - y + W-1], fp32
        const float* drow = ldsDB + (64 * wv + l32) * RS;
        const int hi = qi / W, wi = qi - hi * W;
        for (int x = 0; x < HW; ++x) {
            const float d = drow[x];
            const T* rp = x < H ? (const T*)a.rel_h + (int64_t)(hi - x + H - 1) * D : (const T*)a.rel_w + (int64_t)(wi - (x - H) + W - 1) * D;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = cb * 32 + 8 * g + 4 * h;
                    if (c >= D) continue;
                    const float4 t4 = at_ld4<T>(rp + c);
                    o[cb][4 * g] = fmaf(d, t4.x, o[cb][4 * g]);
                    o[cb][4 * g + 1] = fmaf(d, t4.y, o[cb][4 * g + 1]);
                    o[cb][4 * g + 2] = fmaf(d, t4.z, o[cb][4 * g + 2]);
                    o[cb][4 * g + 3] = fmaf(d, t4.w, o[cb][4 * g + 3]);
                }
        }
    }
    at_store_col<T, D>((T*)a.dq + bb * a.dqs[0] + hd * a.dqs[1] + (int64_t)qi * a.dqs[2], o, 1.f, h);
}

// ---- table gradients, stage 1: part[b a][r][c] = sum over the (i, x) of table row r of dB[i][x] q[i][c]; grid (2H-1 + 2W-1, B nH).
// A thread owns 4 channels; the terms of the row are dealt to the NG thread groups (term t to group t % NG), each group adds
// its terms in order, the groups are added in order.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_relpos_bwd(const T* __restrict__ q, int64_t qs0, int64_t qs1, int64_t qs2, const float* __restrict__ db,
                                                         int nH, int N, int H, int W, float* __restrict__ part) {
    constexpr int C4 = D / 4, NG = 256 / C4;
    __shared__ float4 red[NG * C4];
    const int tid = threadIdx.x, cg = tid % C4, grp = tid / C4;
    const int r = blockIdx.x, bh = blockIdx.y, HW = H + W;
    const T* qp = q + (bh / nH) * qs0 + (bh % nH) * qs1;
    const float* dbp = db + (int64_t)bh * N * HW;
    const bool hpart = r < 2 * H - 1;
    const int dd = hpart ? r - (H - 1) : r - (2 * H - 1) - (W - 1);    // hi - x, or wi - y
    const int lo = dd > 0 ? dd : 0, cnt = (hpart ? H : W) - (dd > 0 ? dd : -dd);   // the query coordinates lo .. lo + cnt - 1
    const int nterms = cnt * (hpart ? W : H);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (grp < NG) {
        for (int t = grp; t < nterms; t += NG) {
            int i, col;
            if (hpart) {
                const int hi = lo + t / W;
                i = hi * W + t % W, col = hi - dd;
            } else {
                const int wi = lo + t % cnt;
                i = (t / cnt) * W + wi, col = H + wi - dd;
            }
            const float d = dbp[(int64_t)i * HW + col];
            const float4 q4 = at_ld4<T>(qp + (int64_t)i * qs2 + 4 * cg);
            acc.x = fmaf(d, q4.x, acc.x);
            acc.y = fmaf(d, q4.y, acc.y);
            acc.z = fmaf(d, q4.z, acc.z);
            acc.w = fmaf(d, q4.w, acc.w);
        }
        red[grp * C4 + cg] = acc;
    }
    __syncthreads();
    if (tid < C4) {
        float4 s = red[tid];
        for (int g = 1; g < NG; ++g) {
            const float4 x = red[g * C4 + tid];
            s.x += x.x, s.y += x.y, s.z += x.z, s.w += x.w;
        }
        float* pp = part + ((int64_t)bh * gridDim.x + r) * D + 4 * tid;   // 4-byte aligned only: the partials follow delta
        pp[0] = s.x, pp[1] = s.y, pp[2] = s.z, pp[3] = s.w;
    }
}

// ---- stage 2: the sum over (batch, head) in index order; rows 0 .. 2H-2 go to drel_h, the rest to drel_w
__global__ __launch_bounds__(256) void k_attn_relpos_bwd_sum(const float* __restrict__ part, int BH, int per, int split, float* __restrict__ drh,
                                                             float* __restrict__ drw) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= per) return;
    float s = 0.f;
    for (int b = 0; b < BH; ++b) s += part[(int64_t)b * per + idx];
    if (idx < split) drh[idx] = s;
    else drw[idx - split] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static int at_bwd_check_dims(const char* who, int B, int nH, int H, int W, int D) {
    TEM_TRY(at_check_dims(who, B, nH, H, W, D));
    TEM_REQUIRE(H + W <= TEM_ATTN_BWD_MAX_HW, "%s: grid %d x %d exceeds H + W = %d of the backward", who, H, W, TEM_ATTN_BWD_MAX_HW);
    return TEM_OK;
}

extern "C" int64_t tem_attention_bwd_ws(int B, int nH, int H, int W, int D, int has_rel_pos) {
    if (at_bwd_check_dims("tem_attention_bwd_ws", B, nH, H, W, D) != TEM_OK) return -1;
    const int64_t BH = (int64_t)B * nH, N = (int64_t)H * W;
    const int64_t delta = BH * N * 4;
    if (!has_rel_pos) return delta;
    return 2 * BH * N * (H + W) * 4 + delta + BH * (2 * H - 1 + 2 * W - 1) * D * 4;
}

template <typename K>
static int at_bwd_lds(const char* who, K kern, size_t lds) {
    TEM_REQUIRE(lds <= AT_LDS_MAX, "%s: %zu bytes of LDS needed, %d available", who, lds, AT_LDS_MAX);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            tem_set_error("%s: cannot reserve %zu bytes of LDS: %s", who, lds, hipGetErrorString(e));
            return TEM_ELAUNCH;
        }
    }
    return TEM_OK;
}

template <typename T, int D, int NW>
static int at_launch_bwd_q(const AtBwdArgs& a, int B, hipStream_t stream) {
    const char* who = "tem_attention_bwd (k_attn_bwd_q)";
    const size_t lds = AtBwdLds<T, D>::Q_TILES + (a.bias ? (size_t)96 * NW * at_bias_stride(a.H, a.W) * 4 : 0);
    TEM_TRY(at_bwd_lds(who, k_attn_bwd_q<T, D, NW>, lds));
    hipLaunchKernelGGL((k_attn_bwd_q<T, D, NW>), dim3((unsigned)tem_cdiv(a.N, 32 * NW), (unsigned)(B * a.nH)), dim3(64 * NW), lds, stream, a);
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

template <typename T, int D>
static int at_bwd_run(AtBwdArgs a, const void* out, const int64_t* os, int B, float* drel_h, float* drel_w, float* ws, hipStream_t stream) {
    const int64_t BH = (int64_t)B * a.nH, rows = BH * a.N, nb = a.rel_h ? rows * (a.H + a.W) : 0;
    float* bias = ws;            // workspace: bias | dB | delta | table-gradient partials
    float* dbias = ws + nb;
    float* delta = ws + 2 * nb;
    float* part = delta + rows;
    hipLaunchKernelGGL((k_attn_bwd_prep<T, D>), dim3(tem_grid_1d(rows, 256, 256 * 16)), dim3(256), 0, stream, (const T*)out, os[0], os[1], os[2],
                       (const T*)a.dout, a.dos[0], a.dos[1], a.dos[2], a.nH, a.N, rows, delta);
    TEM_CHECK_LAUNCH("tem_attention_bwd (k_attn_bwd_prep)");
    a.delta = delta;
    a.bias = nullptr, a.dbias = nullptr;
    if (a.rel_h) {
        hipLaunchKernelGGL((k_attn_relpos<T, D>), dim3(tem_grid_1d(nb, 256, 256 * 16)), dim3(256), 0, stream, (const T*)a.q, a.qs[0], a.qs[1],
                           a.qs[2], (const T*)a.rel_h, (const T*)a.rel_w, a.nH, a.N, a.H, a.W, nb, bias);
        TEM_CHECK_LAUNCH("tem_attention_bwd (bias pre-pass)");
        a.bias = bias, a.dbias = dbias;
    }
    {
        const char* who = "tem_attention_bwd (k_attn_bwd_kv)";
        const size_t lds = AtBwdLds<T, D>::KV_TILES + (size_t)AtTile<T>::BN * 4 * (2 + (a.bias ? at_bias_stride(a.H, a.W) : 0));
        TEM_TRY(at_bwd_lds(who, k_attn_bwd_kv<T, D>, lds));
        hipLaunchKernelGGL((k_attn_bwd_kv<T, D>), dim3((unsigned)tem_cdiv(a.N, 128), (unsigned)BH), dim3(256), lds, stream, a);
        TEM_CHECK_LAUNCH(who);
    }
    if (!a.bias || a.H + a.W <= AT_BWD_NW4_MAX_HW) TEM_TRY((at_launch_bwd_q<T, D, 4>(a, B, stream)));
    else if (a.H + a.W <= AT_BWD_NW2_MAX_HW) TEM_TRY((at_launch_bwd_q<T, D, 2>(a, B, stream)));
    else TEM_TRY((at_launch_bwd_q<T, D, 1>(a, B, stream)));
    if (a.rel_h && drel_h) {
        const int NR = 2 * a.H - 1 + 2 * a.W - 1;
        hipLaunchKernelGGL((k_attn_relpos_bwd<T, D>), dim3((unsigned)NR, (unsigned)BH), dim3(256), 0, stream, (const T*)a.q, a.qs[0], a.qs[1],
                           a.qs[2], dbias, a.nH, a.N, a.H, a.W, part);
        TEM_CHECK_LAUNCH("tem_attention_bwd (k_attn_relpos_bwd)");
        hipLaunchKernelGGL(k_attn_relpos_bwd_sum, dim3((unsigned)tem_cdiv((int64_t)NR * D, 256)), dim3(256), 0, stream, part, (int)BH, NR * D,
                           (2 * a.H - 1) * D, drel_h, drel_w);
        TEM_CHECK_LAUNCH("tem_attention_bwd (k_attn_relpos_bwd_sum)");
    }
    return TEM_OK;
}

template <typename T>
static int at_bwd_run_d(const AtBwdArgs& a, const void* out, const int64_t* os, int B, int D, float* drel_h, float* drel_w, float* ws,
                        hipStream_t stream) {
    return D == 64 ? at_bwd_run<T, 64>(a, out, os, B, drel_h, drel_w, ws, stream) : at_bwd_run<T, 80>(a, out, os, B, drel_h, drel_w, ws, stream);
}

extern "C" int tem_attention_bwd(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                 const int64_t* v_strides, const void* out, const int64_t* out_strides, const void* dout,
                                 const int64_t* dout_strides, const float* lse, const void* rel_h, const void* rel_w, void* dq,
                                 const int64_t* dq_strides, void* dk, const int64_t* dk_strides, void* dv, const int64_t* dv_strides,
                                 float* drel_h, float* drel_w, int B, int nH, int H, int W, int D, float scale, int st, void* ws,
                                 int64_t ws_bytes, tem_stream_t stream) {
    const char* who = "tem_attention_bwd";
    TEM_REQUIRE(q && k && v && out && dout && lse && dq && dk && dv && q_strides && k_strides && v_strides && out_strides && dout_strides &&
                    dq_strides && dk_strides && dv_strides,
                "%s: null pointer", who);
    TEM_TRY(at_bwd_check_dims(who, B, nH, H, W, D));
    TEM_REQUIRE(st == TEM_ST_F32 || st == TEM_ST_F16 || st == TEM_ST_BF16, "%s: unknown storage type %d", who, st);
    TEM_REQUIRE((rel_h != nullptr) == (rel_w != nullptr), "%s: the relative-position tables come as a pair", who);
    TEM_REQUIRE((drel_h != nullptr) == (drel_w != nullptr), "%s: the table gradients come as a pair", who);
    TEM_REQUIRE(!drel_h || rel_h, "%s: table gradients asked for without tables", who);
    TEM_REQUIRE(scale == scale && scale - scale == 0.f, "%s: scale must be finite", who);
    const int vec = st == TEM_ST_F32 ? 4 : 8;   // elements of 16 bytes
    const void* ptrs[8] = {q, k, v, out, dout, dq, dk, dv};
    const int64_t* strides[8] = {q_strides, k_strides, v_strides, out_strides, dout_strides, dq_strides, dk_strides, dv_strides};
    const char* names[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
    AtBwdArgs a;
    int64_t os[3];
    int64_t* dst[8] = {a.qs, a.ks, a.vs, os, a.dos, a.dqs, a.dks, a.dvs};
    for (int t = 0; t < 8; ++t) {
        TEM_REQUIRE(strides[t][3] == 1, "%s: %s must have unit stride along D (got %lld)", who, names[t], (long long)strides[t][3]);
        TEM_REQUIRE(((uintptr_t)ptrs[t] & 15u) == 0, "%s: %s must be 16-byte aligned", who, names[t]);
        for (int d = 0; d < 3; ++d) {
            TEM_REQUIRE(strides[t][d] >= 0 && strides[t][d] % vec == 0, "%s: stride %lld of %s is negative or no multiple of %d elements", who,
                        (long long)strides[t][d], names[t], vec);
            dst[t][d] = strides[t][d];
        }
        TEM_REQUIRE(t < 5 || strides[t][2] >= D, "%s: %s rows overlap (token stride %lld < D)", who, names[t], (long long)strides[t][2]);
    }
    TEM_REQUIRE(((uintptr_t)lse & 3u) == 0, "%s: lse must be 4-byte aligned", who);
    if (rel_h) TEM_REQUIRE((((uintptr_t)rel_h | (uintptr_t)rel_w) & 15u) == 0, "%s: the tables must be 16-byte aligned", who);
    if (drel_h) TEM_REQUIRE((((uintptr_t)drel_h | (uintptr_t)drel_w) & 15u) == 0, "%s: the table gradients must be 16-byte aligned", who);
    const int64_t need = tem_attention_bwd_ws(B, nH, H, W, D, rel_h != nullptr);
    TEM_REQUIRE(ws && ((uintptr_t)ws & 15u) == 0, "%s: a 16-byte aligned workspace is needed", who);
    if (ws_bytes < need) {
        tem_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)need);
        return TEM_EWS;
    }
    a.q = q, a.k = k, a.v = v, a.dout = dout, a.dq = dq, a.dk = dk, a.dv = dv;
    a.lse = lse, a.delta = nullptr, a.bias = nullptr, a.dbias = nullptr;
    a.rel_h = rel_h, a.rel_w = rel_w;
    a.nH = nH, a.N = H * W, a.H = H, a.W = W, a.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    if (st == TEM_ST_F32) return at_bwd_run_d<float>(a, out, os, B, D, drel_h, drel_w, (float*)ws, s);
    if (st == TEM_ST_F16) return at_bwd_run_d<_Float16>(a, out, os, B, D, drel_h, drel_w, (float*)ws, s);
    return at_bwd_run_d<__bf16>(a, out, os, B, D, drel_h, drel_w, (float*)ws, s);
}
