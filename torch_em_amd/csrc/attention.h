// attention.h -- what the attention kernels share (attention.hip: forward; attention_bwd.hip: gradients): vector types, the LDS
// layouts of the key-major tiles, the MFMA / packing / transposing-read helpers, the bias pre-pass and the dimension checks.
#ifndef TEM_ATTENTION_H
#define TEM_ATTENTION_H
#include "tem_common.h"
#include <type_traits>

typedef float at_fx16 __attribute__((ext_vector_type(16)));
typedef _Float16 at_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 at_h2 __attribute__((ext_vector_type(2)));
typedef __bf16 at_b8 __attribute__((ext_vector_type(8)));
typedef __bf16 at_b2 __attribute__((ext_vector_type(2)));
typedef short at_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) at_s4* at_lds_p;

#define AT_LDS_MAX (160 * 1024)   // LDS of a gfx950 compute unit
#define AT_NW4_MAX_HW 81          // with tables, 4-wave workgroups up to this H + W (K, V and 128 bias rows within 64 KB)

struct AtArgs {
    const void *q, *k, *v;
    void* o;
    int64_t qs[3], ks[3], vs[3], os[3];   // element strides of (batch, head, token); unit stride along D
    const float* bias;                    // [B][nH][N][H + W] of k_attn_relpos, or NULL
    int nH, N, H, W;
    float scale;
    float* lse;                           // [B][nH][N] log-sum-exp of the logit rows (the kernels built with the flag only)
};

template <typename T>
struct AtTile {
    static constexpr bool F32 = std::is_same<T, float>::value;
    static constexpr int NT = F32 ? 1 : 2;   // 32-key blocks of a key tile
    static constexpr int BN = 32 * NT;
};
template <typename T, int D>
struct AtLds {
    static constexpr bool F32 = AtTile<T>::F32;
    static constexpr int DP = (D + 31) / 32 * 32;                        // channels of the O^T tiles
    static constexpr int KS = F32 ? 4 * (D + 2) : 2 * D + 16;            // bytes between K rows
    static constexpr int VS = F32 ? 4 * (DP + 8) : 192;                  // bytes between V rows
    static constexpr int KV = AtTile<T>::BN * (KS + VS);
};
static inline int at_bias_stride(int H, int W) { return (H + W) | 1; }

template <typename T>
__device__ __forceinline__ at_fx16 at_mfma16(uint4 a, uint4 b, at_fx16 c) {
    if constexpr (std::is_same<T, _Float16>::value)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(at_h8, a), __builtin_bit_cast(at_h8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(at_b8, a), __builtin_bit_cast(at_b8, b), c, 0, 0, 0);
}
template <typename T>
__device__ __forceinline__ unsigned at_pk(float a, float b) {   // two values rounded to nearest even, one register
    if constexpr (std::is_same<T, _Float16>::value) {
        const at_h2 v = {(_Float16)a, (_Float16)b};
        return __builtin_bit_cast(unsigned, v);
    } else {
        const at_b2 v = {(__bf16)a, (__bf16)b};
        return __builtin_bit_cast(unsigned, v);
    }
}
__device__ __forceinline__ uint2 at_tr_read(const unsigned char* p) {
    const at_s4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((at_lds_p)(p));
    return __builtin_bit_cast(uint2, v);
}
// 4 consecutive elements as floats (p aligned to 4 elements)
template <typename T>
__device__ __forceinline__ float4 at_ld4(const T* p) {
    if constexpr (std::is_same<T, float>::value) {
        return *(const float4*)p;
    } else {
        const uint2 u = *(const uint2*)p;
        if constexpr (std::is_same<T, _Float16>::value) {
            const at_h2 a = __builtin_bit_cast(at_h2, u.x), b = __builtin_bit_cast(at_h2, u.y);
            return make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
        } else {
            return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                               __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
        }
    }
}

// ---- pre-pass: bias[b][a][i][x] = q_i . Rh[hi - x + H-1] (x < H), q_i . Rw[wi - (x - H) + W-1] (x >= H); q UNscaled; fp32
// fma chain in channel order.  One output a thread; the threads of a query read the same q row and neighbouring table rows.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_relpos(const T* __restrict__ q, int64_t qs0, int64_t qs1, int64_t qs2, const T* __restrict__ rh,
                                                     const T* __restrict__ rw, int nH, int N, int H, int W, int64_t total,
                                                     float* __restrict__ bias) {
    const int HW = H + W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % HW);
        const int64_t row = idx / HW;   // (b nH + a) N + i
        const int i = (int)(row % N);
        const int64_t bh = row / N;
        const int hi = i / W, wi = i - hi * W;
        const T* qp = q + (bh / nH) * qs0 + (bh % nH) * qs1 + (int64_t)i * qs2;
        const T* rp = x < H ? rh + (int64_t)(hi - x + H - 1) * D : rw + (int64_t)(wi - (x - H) + W - 1) * D;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
            const float4 a = at_ld4<T>(qp + c), r = at_ld4<T>(rp + c);
            acc = fmaf(a.x, r.x, acc);
            acc = fmaf(a.y, r.y, acc);
            acc = fmaf(a.z, r.z, acc);
            acc = fmaf(a.w, r.w, acc);
        }
        bias[idx] = acc;
    }
}

static int at_check_dims(const char* who, int B, int nH, int H, int W, int D) {
    TEM_REQUIRE(B > 0 && nH > 0 && H > 0 && W > 0, "%s: B, nH, H, W must be positive", who);
    TEM_REQUIRE(H <= TEM_ATTN_MAX_GRID && W <= TEM_ATTN_MAX_GRID, "%s: grid %d x %d exceeds %d a side", who, H, W, TEM_ATTN_MAX_GRID);
    TEM_REQUIRE(D == 64 || D == 80, "%s: head width %d not supported (64 or 80)", who, D);
    TEM_REQUIRE((int64_t)B * nH <= 65535, "%s: B * nH = %lld exceeds 65535", who, (long long)B * nH);
    return TEM_OK;
}
#endif  // TEM_ATTENTION_H
