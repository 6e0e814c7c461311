// attention.hip -- fused multi-head self-attention over a 2-D token grid with SAM's decomposed relative-position bias
// (segment_anything's Attention + add_decomposed_rel_pos, equal query and key grids; DESIGN.md "Attention").
//
//   S[i][j] = scale * q_i . k_j + q_i . Rh[hi - hj + H-1] + q_i . Rw[wi - wj + W-1]      P = softmax_j(S)      O = P V
//
// S and P never reach global memory.  A workgroup of NW waves owns 32 NW queries of one (batch, head); wave w owns 32 of
// them for the whole march over the key tiles (BN = 64 keys, 32 for fp32 tensors).  Both products run TRANSPOSED on the
// 32x32 MFMAs, so that the query is the COLUMN (= lane & 31) of every accumulator:
//   S^T = K Q^T   A = a K row from LDS (16 bytes of 8 channels a lane), B = the wave's Q rows, loaded ONCE into registers
//   O^T = V^T P^T A = V^T, B = P^T
// A lane then holds, for ITS query, 16 keys of each 32-key block (key = 8 (r / 4) + 4 (lane / 32) + r % 4 of accumulator
// register r): the row maximum and the row sum are in-lane reductions plus ONE exchange with lane ^ 32, the running maximum,
// the running sum and the rescale factor of the O^T accumulators are per-lane scalars, and the accumulator registers of P --
// rounded once to the 16-bit type -- ARE the B operand of the second product: its k index is a summation index, so slot
// (lane / 32, e) of a K = 16 step is simply DEFINED as the key the lane already holds there, and V^T is read to match.
// No LDS round trip for P, no cross-lane traffic but the one exchange.
//   K tile in LDS: key-major rows of D elements as they come from global, padded to 2 D + 16 bytes: the 16-byte fragment
//                  reads of 16 consecutive rows cover the 64 banks once (fp32: rows of D + 2 floats, b32 reads of 32 rows x 2
//                  channels cover them once).
//   V tile in LDS: key-major rows too, 192 bytes apart (channels D .. 96 of a D = 80 row are zeros).  V^T fragments are
//                  ds_read_b64_tr_b16: a 16-lane group reads 4 keys x 16 channels and gets them transposed, 4 keys of ONE
//                  channel a lane; the 32 lanes of a half-wave address 4 rows x 64 bytes, 192-byte rows put those on
//                  disjoint 16-bank windows (fp32: plain b32 reads, rows of DP + 8 floats put the two lane halves -- 4 keys
//                  apart -- on opposite bank halves).  The transpose costs nothing on the write side: staging is a 16-byte copy.
//   bias in LDS:   the workgroup's 32 NW rows of the pre-pass result [H + W] (k_attn_relpos), staged once, row stride odd.
// Masking: a key column >= N gets -inf before the maximum, so it contributes exp(-inf) = 0 exactly; its K and V rows are
// ZEROS in LDS (0 x garbage could be NaN); the maximum used in the exponent is replaced by 0 while it is still -inf, so a
// fully masked tile gives exp(-inf - 0) = 0, never -inf - (-inf); query rows >= N compute on zeros and are not stored.
// No atomics anywhere: same input, same bits.  The gradients are attention_bwd.hip; what both files share is attention.h.
#include "attention.h"

// ---- the streaming-softmax kernel: grid (query tiles, B nH), 64 NW threads, dynamic LDS = K tile | V tile | bias rows
// LSE (compile time): also store L[i] = m + log(sum) of every logit row, fp32 [B][nH][N], for the backward (attention_bwd.hip);
// without the flag the kernel is instruction for instruction the one it was (profiles/attention_fwd_asm_equal.txt).
template <typename T, int D, int NW, bool LSE>
__global__ __launch_bounds__(64 * NW) void k_attn_fwd(AtArgs a) {
    typedef AtLds<T, D> L;
    constexpr bool F32 = L::F32;
    constexpr int NT = AtTile<T>::NT, BN = AtTile<T>::BN, NCB = L::DP / 32, KS = L::KS, VS = L::VS;
    constexpr int ES = (int)sizeof(T), EPC = 16 / ES;                  // elements of a 16-byte chunk
    constexpr int CHK = D / EPC, CHV = L::DP / EPC;                    // chunks of a K row / of a padded V row
    constexpr int NQ = F32 ? D / 2 : D / 16;                           // MFMA steps of S^T = registers (uint4 / float) of Q
    constexpr int NTHR = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char at_lds[];
    unsigned char* ldsK = at_lds;
    unsigned char* ldsV = at_lds + BN * KS;
    float* ldsB = (float*)(at_lds + L::KV);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int bh = blockIdx.y, bb = bh / a.nH, hd = bh - bb * a.nH;
    const int N = a.N, H = a.H, W = a.W;
    const int q0 = blockIdx.x * (32 * NW);
    const int qi = q0 + 32 * wv + l32;                                 // this lane's query
    const bool wave_live = q0 + 32 * wv < N;                           // wave uniform
    const T* qp = (const T*)a.q + bb * a.qs[0] + hd * a.qs[1];
    const T* kp = (const T*)a.k + bb * a.ks[0] + hd * a.ks[1];
    const T* vp = (const T*)a.v + bb * a.vs[0] + hd * a.vs[1];
    const bool has_bias = a.bias != nullptr;                           // workgroup uniform
    const int RS = (H + W) | 1;

    if (has_bias) {   // rows q0 .. q0 + 32 NW of the pre-pass result are contiguous: one coalesced sweep
        const int HW = H + W;
        const float* bp = a.bias + ((int64_t)bh * N + q0) * HW;
        const int valid = (N - q0 < 32 * NW ? N - q0 : 32 * NW) * HW;
        for (int idx = tid; idx < 32 * NW * HW; idx += NTHR) {
            const int r = idx / HW;
            ldsB[r * RS + (idx - r * HW)] = idx < valid ? bp[idx] : 0.f;
        }
    }

    // the wave's Q rows as the B operand: lane = query, registers = channels (16-bit: 8 a step; fp32: 1 a step)
    uint4 qf[F32 ? 1 : NQ];
    float qf32[F32 ? NQ : 1];
    if constexpr (F32) {
#pragma unroll
        for (int st = 0; st < NQ; ++st) qf32[st] = qi < N ? (float)qp[(int64_t)qi * a.qs[2] + 2 * st + h] : 0.f;
    } else {
#pragma unroll
        for (int st = 0; st < NQ; ++st)
            qf[st] = qi < N ? *(const uint4*)(qp + (int64_t)qi * a.qs[2] + 16 * st + 8 * h) : make_uint4(0, 0, 0, 0);
    }

    at_fx16 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, lsum = 0.f;                                     // running maximum (both lane halves agree), this lane's part of the sum
    const float inv_w = 1.f / (float)W;
    const float* brow = ldsB + (32 * wv + l32) * RS;
    const int p16 = lane & 15;
    const int v_lane = (4 * h + (p16 >> 2)) * VS + ((lane >> 4) & 1) * 32 + (p16 & 3) * 8;   // transposing-read address of this lane

    for (int j0 = 0; j0 < N; j0 += BN) {
        __syncthreads();   // the previous tile has been read (first trip: orders nothing that matters)
        for (int idx = tid; idx < BN * CHK; idx += NTHR) {
            const int r = idx / CHK, ch = idx - r * CHK, j = j0 + r;
            const uint4 val = j < N ? *(const uint4*)(kp + (int64_t)j * a.ks[2] + ch * EPC) : make_uint4(0, 0, 0, 0);
            if constexpr (F32) {   // rows of D + 2 floats are 8-byte aligned
                *(uint2*)(ldsK + r * KS + ch * 16) = make_uint2(val.x, val.y);
                *(uint2*)(ldsK + r * KS + ch * 16 + 8) = make_uint2(val.z, val.w);
            } else {
                *(uint4*)(ldsK + r * KS + ch * 16) = val;
            }
        }
        for (int idx = tid; idx < BN * CHV; idx += NTHR) {
            const int r = idx / CHV, ch = idx - r * CHV, j = j0 + r;
            const uint4 val = (j < N && ch < CHK) ? *(const uint4*)(vp + (int64_t)j * a.vs[2] + ch * EPC) : make_uint4(0, 0, 0, 0);
            *(uint4*)(ldsV + r * VS + ch * 16) = val;
        }
        __syncthreads();
        if (!wave_live) continue;   // a wave without a stored row keeps the barriers only

        // ---- S^T = K Q^T: rows = keys, column = this lane's query
        at_fx16 s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
            if constexpr (F32) {
#pragma unroll
                for (int st = 0; st < NQ; ++st) {
                    const float kf = *(const float*)(ldsK + l32 * KS + (2 * st + h) * 4);
                    s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf, qf32[st], s[t], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int st = 0; st < NQ; ++st) {
                    const uint4 kf = *(const uint4*)(ldsK + (32 * t + l32) * KS + st * 32 + h * 16);
                    s[t] = at_mfma16<T>(kf, qf[st], s[t]);
                }
            }
        }

        // ---- logits: scale in fp32, bias, mask; the tile's row maximum
        float mt = NEG_INF;
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
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float x = NEG_INF;
                    if (jb + u < N) {
                        x = s[t][4 * g + u] * a.scale;
                        if (has_bias) x += brow[hj] + brow[H + wj];
                    }
                    if (++wj == W) {
                        wj = 0;
                        ++hj;
                    }
                    s[t][4 * g + u] = x;
                    mt = __builtin_fmaxf(mt, x);
                }
            }
        mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = __builtin_fmaxf(m, mt);
        const float m_use = m_new == NEG_INF ? 0.f : m_new;           // nothing seen yet: exp(-inf - 0) = 0, no -inf - (-inf)
        float alpha, psum = 0.f;
        if constexpr (F32) {
            alpha = expf(m - m_use);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[0][r] = expf(s[0][r] - m_use);
                psum += s[0][r];
            }
        } else {
            const float LOG2E = 1.4426950408889634f;
            alpha = __builtin_amdgcn_exp2f((m - m_use) * LOG2E);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[t][r] = __builtin_amdgcn_exp2f((s[t][r] - m_use) * LOG2E);
                    psum += s[t][r];
                }
        }
        m = m_new;
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;

        // ---- O^T += V^T P^T: rows = channels, column = this lane's query; the k slots are the keys the lane holds
        if constexpr (F32) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 8 * (r >> 2) + 4 * h + (r & 3);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const float vf = *(const float*)(ldsV + key * VS + (cb * 32 + l32) * 4);
                    o[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, s[0][r], o[cb], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {   // a K = 16 step: registers 8 s2 .. 8 s2 + 7 = keys 16 s2 + 4 h + (0..3), + 8
                    const uint4 pf = make_uint4(at_pk<T>(s[t][8 * s2 + 0], s[t][8 * s2 + 1]), at_pk<T>(s[t][8 * s2 + 2], s[t][8 * s2 + 3]),
                                                at_pk<T>(s[t][8 * s2 + 4], s[t][8 * s2 + 5]), at_pk<T>(s[t][8 * s2 + 6], s[t][8 * s2 + 7]));
                    const unsigned char* vb = ldsV + (32 * t + 16 * s2) * VS + v_lane;
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const uint2 v0 = at_tr_read(vb + cb * 64), v1 = at_tr_read(vb + cb * 64 + 8 * VS);
                        o[cb] = at_mfma16<T>(make_uint4(v0.x, v0.y, v1.x, v1.y), pf, o[cb]);
                    }
                }
        }
    }

    if (!wave_live) return;
    lsum += __shfl_xor(lsum, 32, 64);   // the two halves hold disjoint keys of the same query; at least key 0 is valid: lsum > 0
    if (qi >= N) return;
    if constexpr (LSE) {
        if (h == 0) a.lse[(int64_t)bh * N + qi] = m + logf(lsum);   // m is finite: key 0 is valid
    }
    T* op = (T*)a.o + bb * a.os[0] + hd * a.os[1] + (int64_t)qi * a.os[2];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = cb * 32 + 8 * g + 4 * h;   // 4 consecutive channels: registers 4 g .. 4 g + 3
            if (c >= D) continue;
            const float y0 = o[cb][4 * g] / lsum, y1 = o[cb][4 * g + 1] / lsum, y2 = o[cb][4 * g + 2] / lsum, y3 = o[cb][4 * g + 3] / lsum;
            if constexpr (F32)
                *(float4*)(op + c) = make_float4(y0, y1, y2, y3);
            else
                *(uint2*)(op + c) = make_uint2(at_pk<T>(y0, y1), at_pk<T>(y2, y3));
        }
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int64_t tem_attention_ws(int B, int nH, int H, int W, int D, int has_rel_pos) {
    if (at_check_dims("tem_attention_ws", B, nH, H, W, D) != TEM_OK) return -1;
    return has_rel_pos ? (int64_t)B * nH * H * W * (H + W) * 4 : 0;
}

template <typename T, int D, int NW>
static int at_launch_fwd(const AtArgs& a, int B, bool bias, hipStream_t stream) {
    const char* who = "tem_attention_fwd";
    const size_t lds = AtLds<T, D>::KV + (bias ? (size_t)32 * NW * at_bias_stride(a.H, a.W) * 4 : 0);
    TEM_REQUIRE(lds <= AT_LDS_MAX, "%s: %zu bytes of LDS needed, %d available", who, lds, AT_LDS_MAX);
    void (*const kern)(AtArgs) = a.lse ? k_attn_fwd<T, D, NW, true> : k_attn_fwd<T, D, NW, false>;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            tem_set_error("%s: cannot reserve %zu bytes of LDS: %s", who, lds, hipGetErrorString(e));
            return TEM_ELAUNCH;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)tem_cdiv(a.N, 32 * NW), (unsigned)(B * a.nH)), dim3(64 * NW), lds, stream, a);
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}

template <typename T, int D>
static int at_run(AtArgs a, int B, const void* rel_h, const void* rel_w, float* ws, hipStream_t stream) {
    if (rel_h) {
        const int64_t total = (int64_t)B * a.nH * a.N * (a.H + a.W);
        hipLaunchKernelGGL((k_attn_relpos<T, D>), dim3(tem_grid_1d(total, 256, 256 * 16)), dim3(256), 0, stream, (const T*)a.q, a.qs[0], a.qs[1],
                           a.qs[2], (const T*)rel_h, (const T*)rel_w, a.nH, a.N, a.H, a.W, total, ws);
        TEM_CHECK_LAUNCH("tem_attention_fwd (bias pre-pass)");
        a.bias = ws;
        if (a.H + a.W > AT_NW4_MAX_HW) return at_launch_fwd<T, D, 2>(a, B, true, stream);
        return at_launch_fwd<T, D, 4>(a, B, true, stream);
    }
    a.bias = nullptr;
    return at_launch_fwd<T, D, 4>(a, B, false, stream);
}

template <typename T>
static int at_run_d(const AtArgs& a, int B, int D, const void* rel_h, const void* rel_w, float* ws, hipStream_t stream) {
    return D == 64 ? at_run<T, 64>(a, B, rel_h, rel_w, ws, stream) : at_run<T, 80>(a, B, rel_h, rel_w, ws, stream);
}

extern "C" int tem_attention_fwd(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                 const int64_t* v_strides, void* out, const int64_t* out_strides, const void* rel_h, const void* rel_w,
                                 int B, int nH, int H, int W, int D, float scale, int st, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    return tem_attention_fwd_ex(q, q_strides, k, k_strides, v, v_strides, out, out_strides, rel_h, rel_w, B, nH, H, W, D, scale, st, ws,
                                ws_bytes, nullptr, stream);
}

extern "C" int tem_attention_fwd_ex(const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                    const int64_t* v_strides, void* out, const int64_t* out_strides, const void* rel_h, const void* rel_w,
                                    int B, int nH, int H, int W, int D, float scale, int st, void* ws, int64_t ws_bytes, float* lse,
                                    tem_stream_t stream) {
    const char* who = lse ? "tem_attention_fwd_ex" : "tem_attention_fwd";
    TEM_REQUIRE(q && k && v && out && q_strides && k_strides && v_strides && out_strides, "%s: null pointer", who);
    TEM_TRY(at_check_dims(who, B, nH, H, W, D));
    TEM_REQUIRE(st == TEM_ST_F32 || st == TEM_ST_F16 || st == TEM_ST_BF16, "%s: unknown storage type %d", who, st);
    TEM_REQUIRE((rel_h != nullptr) == (rel_w != nullptr), "%s: the relative-position tables come as a pair", who);
    TEM_REQUIRE(scale == scale && scale - scale == 0.f, "%s: scale must be finite", who);
    const int vec = st == TEM_ST_F32 ? 4 : 8;   // elements of 16 bytes
    const void* ptrs[4] = {q, k, v, out};
    const int64_t* strides[4] = {q_strides, k_strides, v_strides, out_strides};
    const char* names[4] = {"q", "k", "v", "out"};
    AtArgs a;
    int64_t* dst[4] = {a.qs, a.ks, a.vs, a.os};
    for (int t = 0; t < 4; ++t) {
        TEM_REQUIRE(strides[t][3] == 1, "%s: %s must have unit stride along D (got %lld)", who, names[t], (long long)strides[t][3]);
        TEM_REQUIRE(((uintptr_t)ptrs[t] & 15u) == 0, "%s: %s must be 16-byte aligned", who, names[t]);
        for (int d = 0; d < 3; ++d) {
            TEM_REQUIRE(strides[t][d] >= 0 && strides[t][d] % vec == 0, "%s: stride %lld of %s is negative or no multiple of %d elements", who,
                        (long long)strides[t][d], names[t], vec);
            dst[t][d] = strides[t][d];
        }
    }
    TEM_REQUIRE(out_strides[2] >= D, "%s: out rows overlap (token stride %lld < D)", who, (long long)out_strides[2]);
    if (rel_h) {
        TEM_REQUIRE((((uintptr_t)rel_h | (uintptr_t)rel_w) & 15u) == 0, "%s: the tables must be 16-byte aligned", who);
        const int64_t need = tem_attention_ws(B, nH, H, W, D, 1);
        TEM_REQUIRE(ws && ((uintptr_t)ws & 15u) == 0, "%s: a 16-byte aligned workspace is needed with tables", who);
        if (ws_bytes < need) {
            tem_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)need);
            return TEM_EWS;
        }
    }
    a.q = q, a.k = k, a.v = v, a.o = out;
    a.bias = nullptr;
    a.lse = lse;
    a.nH = nH, a.N = H * W, a.H = H, a.W = W, a.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    if (st == TEM_ST_F32) return at_run_d<float>(a, B, D, rel_h, rel_w, (float*)ws, s);
    if (st == TEM_ST_F16) return at_run_d<_Float16>(a, B, D, rel_h, rel_w, (float*)ws, s);
    return at_run_d<__bf16>(a, B, D, rel_h, rel_w, (float*)ws, s);
}
