// selftrain.hip -- the pseudo-labelling step of mean-teacher self-training (reference self_training/pseudo_labeling.py:39-72:
// DefaultPseudoLabeler.__call__ after the teacher's forward pass).  The reference runs a chain of element-wise passes over a
// prediction-sized tensor (sigmoid, two compares, an add, a cast); here the teacher's output streams by once: labels and
// confidence mask leave in the layout the prediction came in, so the masked Dice kernels read them in place.
//
// Pure streaming: 16-byte loads and stores in a grid-stride loop over the storage (any dense permutation is processed flat),
// a scalar loop for the tail and for bases that are not 16-byte aligned.
//
// Compare semantics (pinned by tests/golden/g17_selftrain.npz against the reference on the CPU): the compare runs on the STORED
// label -- the sigmoid is computed in fp32 and rounded once to the storage type first -- against the threshold rounded to that
// type; the caller passes both thresholds already rounded (1 - t formed in double before the rounding).
//
// Below it: the distribution alignment of FixMatch (class count and scale-and-clip pass), in the same style.
#include "tem_common.h"
#include "tem_act.h"

#define PL_MASK_NONE 0
#define PL_MASK_BOTH 1   // (l >= t) | (l <= 1 - t) as float32 0 / 1
#define PL_MASK_ONE 2    // l >= t as bool (one byte, 0 / 1)

template <typename T> __device__ __forceinline__ float pl_round(float v) { return (float)(T)v; }
template <> __device__ __forceinline__ float pl_round<float>(float v) { return v; }

template <typename T, bool SIGMOID> __device__ __forceinline__ float pl_label(float x) {
    return SIGMOID ? pl_round<T>(1.f / (1.f + expf(-x))) : x;
}
template <int MODE> __device__ __forceinline__ bool pl_keep(float l, float t_hi, float t_lo) {
    return MODE == PL_MASK_BOTH ? (l >= t_hi) | (l <= t_lo) : l >= t_hi;
}

template <typename T, int VEC> __device__ __forceinline__ void pl_load(const T* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = act_ld4(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        act_ld8(p, v);
    }
}
template <typename T, int VEC> __device__ __forceinline__ void pl_store(T* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) act_st4(p, make_float4(v[0], v[1], v[2], v[3]));
    else act_st8(p, v);
}

// One sample of S elements per blockIdx.y (the whole storage as ONE sample when no sample's mask is shared).  src >= 0: the
// mask of every sample is the mask of sample `src` (the reference's `mask_channel` slices the BATCH axis, :65-71).
// nvec: 16-byte vectors per sample on the vector path (0: everything goes through the scalar loop).
template <typename T, bool SIGMOID, int MODE>
__global__ __launch_bounds__(256) void k_pseudo_label(const T* __restrict__ x, T* __restrict__ labels, void* __restrict__ mask,
                                                      int64_t S, int64_t nvec, int src, float t_hi, float t_lo) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int n = blockIdx.y;
    const bool shared = src >= 0 && src != n;
    const T* xn = x + (int64_t)n * S;
    const T* xs = x + (int64_t)(src >= 0 ? src : n) * S;
    T* ln = SIGMOID ? labels + (int64_t)n * S : nullptr;
    float* mf = MODE == PL_MASK_BOTH ? (float*)mask + (int64_t)n * S : nullptr;
    uint8_t* mb = MODE == PL_MASK_ONE ? (uint8_t*)mask + (int64_t)n * S : nullptr;
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t q = first; q < nvec; q += step) {
        const int64_t i = q * VEC;
        float l[VEC];
        if (SIGMOID || !shared) {
            pl_load<T, VEC>(xn + i, l);
#pragma unroll
            for (int k = 0; k < VEC; ++k) l[k] = pl_label<T, SIGMOID>(l[k]);
            if constexpr (SIGMOID) pl_store<T, VEC>(ln + i, l);
        }
        if constexpr (MODE != PL_MASK_NONE) {
            if (shared) {
                pl_load<T, VEC>(xs + i, l);
#pragma unroll
                for (int k = 0; k < VEC; ++k) l[k] = pl_label<T, SIGMOID>(l[k]);
            }
            if constexpr (MODE == PL_MASK_BOTH) {
#pragma unroll
                for (int k = 0; k < VEC; k += 4)
                    act_st4(mf + i + k, make_float4(pl_keep<MODE>(l[k], t_hi, t_lo) ? 1.f : 0.f, pl_keep<MODE>(l[k + 1], t_hi, t_lo) ? 1.f : 0.f,
                                                    pl_keep<MODE>(l[k + 2], t_hi, t_lo) ? 1.f : 0.f, pl_keep<MODE>(l[k + 3], t_hi, t_lo) ? 1.f : 0.f));
            } else {
#pragma unroll
                for (int k = 0; k < VEC; k += 4) {
                    const unsigned w = (unsigned)pl_keep<MODE>(l[k], t_hi, t_lo) | ((unsigned)pl_keep<MODE>(l[k + 1], t_hi, t_lo) << 8) |
                                       ((unsigned)pl_keep<MODE>(l[k + 2], t_hi, t_lo) << 16) | ((unsigned)pl_keep<MODE>(l[k + 3], t_hi, t_lo) << 24);
                    *reinterpret_cast<unsigned*>(mb + i + k) = w;
                }
            }
        }
    }
    for (int64_t i = nvec * VEC + first; i < S; i += step) {
        if constexpr (SIGMOID) act_st1(ln + i, pl_label<T, true>(act_ld1(xn + i)));
        if constexpr (MODE != PL_MASK_NONE) {
            const bool keep = pl_keep<MODE>(pl_label<T, SIGMOID>(act_ld1(xs + i)), t_hi, t_lo);
            if constexpr (MODE == PL_MASK_BOTH) mf[i] = keep ? 1.f : 0.f;
            else mb[i] = keep ? 1 : 0;
        }
    }
}

template <typename T, bool SIGMOID, int MODE>
static void pl_launch(const void* x, void* labels, void* mask, int N, int64_t S, int src, float t_hi, float t_lo, hipStream_t stream) {
    constexpr int VEC = 16 / (int)sizeof(T);
    // vector path: every pointer on a 16-byte boundary, and every sample's base too
    const bool vec = ((uintptr_t)x % 16 == 0) && (!SIGMOID || (uintptr_t)labels % 16 == 0) && (MODE == PL_MASK_NONE || (uintptr_t)mask % 16 == 0) &&
                     (N == 1 || S % VEC == 0);
    const int64_t nvec = vec ? S / VEC : 0;
    const int64_t tail = S - nvec * VEC;
    const dim3 grid(tem_grid_1d(nvec > tail ? nvec : tail, 256, 2048), N);
    hipLaunchKernelGGL((k_pseudo_label<T, SIGMOID, MODE>), grid, dim3(256), 0, stream, (const T*)x, (T*)labels, mask, S, nvec, src, t_hi, t_lo);
}

extern "C" int tem_pseudo_label_st(const void* x, void* labels, void* mask, int N, int64_t S, int act, int mask_mode,
                                   int mask_sample, float t_hi, float t_lo, int st, tem_stream_t stream) {
    TEM_REQUIRE(x && N > 0 && N <= 65535 && S > 0, "tem_pseudo_label_st: bad arguments (N=%d)", N);
    TEM_REQUIRE(st >= TEM_ST_F32 && st <= TEM_ST_BF16, "tem_pseudo_label_st: unknown storage type %d", st);
    TEM_REQUIRE(act == TEM_ACT_NONE || act == TEM_ACT_SIGMOID, "tem_pseudo_label_st: Invalid activation: %d", act);
    TEM_REQUIRE(mask_mode >= PL_MASK_NONE && mask_mode <= PL_MASK_ONE, "tem_pseudo_label_st: unknown mask mode %d", mask_mode);
    TEM_REQUIRE((act == TEM_ACT_SIGMOID) == (labels != nullptr), "tem_pseudo_label_st: labels are written with the sigmoid only");
    TEM_REQUIRE((mask_mode != PL_MASK_NONE) == (mask != nullptr), "tem_pseudo_label_st: mask pointer and mask mode disagree");
    TEM_REQUIRE(mask_sample < N && (mask_sample < 0 || mask_mode != PL_MASK_NONE), "tem_pseudo_label_st: mask_sample %d out of range", mask_sample);
    if (act == TEM_ACT_NONE && mask_mode == PL_MASK_NONE) return TEM_OK;   // the labels are the input itself
    if (mask_sample < 0) {   // nothing shared between samples: one flat range
        S *= N;
        N = 1;
    }
    const hipStream_t s = (hipStream_t)stream;
    TEM_ST_SWITCH(st, T, {
        if (act == TEM_ACT_SIGMOID) {
            if (mask_mode == PL_MASK_NONE) pl_launch<T, true, PL_MASK_NONE>(x, labels, mask, N, S, mask_sample, t_hi, t_lo, s);
            else if (mask_mode == PL_MASK_BOTH) pl_launch<T, true, PL_MASK_BOTH>(x, labels, mask, N, S, mask_sample, t_hi, t_lo, s);
            else pl_launch<T, true, PL_MASK_ONE>(x, labels, mask, N, S, mask_sample, t_hi, t_lo, s);
        } else {
            if (mask_mode == PL_MASK_BOTH) pl_launch<T, false, PL_MASK_BOTH>(x, labels, mask, N, S, mask_sample, t_hi, t_lo, s);
            else pl_launch<T, false, PL_MASK_ONE>(x, labels, mask, N, S, mask_sample, t_hi, t_lo, s);
        }
    });
    TEM_CHECK_LAUNCH("tem_pseudo_label_st");
    return TEM_OK;
}

// ---- distribution alignment of FixMatch (reference self_training/fix_match.py:164-181: get_distribution_alignment) ----------
// The reference binarises the labels at the threshold, counts the two classes with torch.unique (a sort and a device-to-host
// synchronisation for the output size), scales each label by source_k / (count_k / n) of ITS class and clips to [0, 1].  Here:
// one integer count (k_label_count: every block writes its 64-bit partial, no atomics, no memset) and one scale-and-clip pass
// (k_distribution_align: every block sums the partials itself, so nothing crosses the host).  Compare semantics as above: on
// the stored value against the threshold rounded to the storage type; NaN is "below" for the count (l >= t is false) and takes
// the upper class's ratio in the pass (l < t is false), as in the reference -- it stays NaN either way.
#define DA_MAX_PARTS 2048   // the grid cap of the count; k_distribution_align sums at most this many partials
#define DA_MAX_N ((int64_t)1 << 40)   // per-thread and per-wave counts stay in 32 bits far beyond this

static int da_parts(int64_t n, int st) { return tem_grid_1d(tem_cdiv(n, 16 / tem_st_size(st)), 256, DA_MAX_PARTS); }

// the block's sum of one 64-bit value per thread (256 threads), in every thread: over the wave, then over the four waves
// (each kernel calls it once: sh is written once per block)
__device__ __forceinline__ unsigned long long da_block_sum(unsigned long long v, unsigned long long* sh /*[4]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // a 64-bit value travels as two 32-bit shuffles
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

template <typename T>
__global__ __launch_bounds__(256) void k_label_count(const T* __restrict__ x, int64_t n, int64_t nvec, float thr,
                                                     unsigned long long* __restrict__ partials) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned long long sh[4];
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned cnt = 0;
    for (int64_t q = first; q < nvec; q += step) {
        float l[VEC];
        pl_load<T, VEC>(x + q * VEC, l);
#pragma unroll
        for (int k = 0; k < VEC; ++k) cnt += l[k] >= thr ? 1u : 0u;
    }
    for (int64_t i = nvec * VEC + first; i < n; i += step) cnt += act_ld1(x + i) >= thr ? 1u : 0u;
    const unsigned long long total = da_block_sum(cnt, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;   // every block, zero included: the buffer is never cleared
}

template <typename T> __device__ __forceinline__ float da_one(float l, float thr, float r0, float r1) {
    const float v = l * (l < thr ? r0 : r1);
    // torch.clip lets NaN through (fminf / fmaxf would not): both compares are false for NaN
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

template <typename T>
__global__ __launch_bounds__(256) void k_distribution_align(const T* __restrict__ x, T* __restrict__ out, int64_t n, int64_t nvec,
                                                            const unsigned long long* __restrict__ partials, int parts, float thr,
                                                            float s0, float s1) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned long long sh[4];
    unsigned long long mine = 0;
    for (int i = threadIdx.x; i < parts; i += 256) mine += partials[i];
    const unsigned long long c1 = da_block_sum(mine, sh), c0 = (unsigned long long)n - c1;
    // the reference's order: counts / counts.sum() in fp32, then source / that.  An empty class is never selected -- with a
    // NaN label it can be (NaN is not < thr); the label is NaN then whatever the ratio -- so its ratio is a plain 0, not inf
    const float fn = (float)n;
    const float r0 = c0 ? s0 / ((float)c0 / fn) : 0.f, r1 = c1 ? s1 / ((float)c1 / fn) : 0.f;
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t q = first; q < nvec; q += step) {
        float l[VEC];
        pl_load<T, VEC>(x + q * VEC, l);
#pragma unroll
        for (int k = 0; k < VEC; ++k) l[k] = da_one<T>(l[k], thr, r0, r1);
        pl_store<T, VEC>(out + q * VEC, l);
    }
    for (int64_t i = nvec * VEC + first; i < n; i += step) act_st1(out + i, da_one<T>(act_ld1(x + i), thr, r0, r1));
}

extern "C" int tem_label_count_parts(int64_t n, int st) {
    if (n <= 0 || n > DA_MAX_N || st < TEM_ST_F32 || st > TEM_ST_BF16) return 0;
    return da_parts(n, st);
}

extern "C" int tem_label_count_st(const void* labels, int64_t n, float threshold, void* partials, int parts, int st,
                                  tem_stream_t stream) {
    TEM_REQUIRE(labels && partials && n > 0 && n <= DA_MAX_N, "tem_label_count_st: bad arguments (n=%lld)", (long long)n);
    TEM_REQUIRE(st >= TEM_ST_F32 && st <= TEM_ST_BF16, "tem_label_count_st: unknown storage type %d", st);
    TEM_REQUIRE(parts == da_parts(n, st), "tem_label_count_st: %d partials, tem_label_count_parts() says %d", parts, da_parts(n, st));
    TEM_REQUIRE((uintptr_t)partials % 8 == 0, "tem_label_count_st: partials must be 8-byte aligned");
    TEM_ST_SWITCH(st, T, {
        constexpr int VEC = 16 / (int)sizeof(T);
        const int64_t nvec = (uintptr_t)labels % 16 == 0 ? n / VEC : 0;
        hipLaunchKernelGGL((k_label_count<T>), dim3(parts), dim3(256), 0, (hipStream_t)stream, (const T*)labels, n, nvec, threshold,
                           (unsigned long long*)partials);
    });
    TEM_CHECK_LAUNCH("tem_label_count_st");
    return TEM_OK;
}

extern "C" int tem_distribution_align_st(const void* labels, void* out, int64_t n, float threshold, float source0, float source1,
                                         const void* partials, int parts, int st, tem_stream_t stream) {
    TEM_REQUIRE(labels && out && partials && n > 0 && n <= DA_MAX_N, "tem_distribution_align_st: bad arguments (n=%lld)", (long long)n);
    TEM_REQUIRE(st >= TEM_ST_F32 && st <= TEM_ST_BF16, "tem_distribution_align_st: unknown storage type %d", st);
    TEM_REQUIRE(parts == da_parts(n, st), "tem_distribution_align_st: %d partials, tem_label_count_parts() says %d", parts, da_parts(n, st));
    TEM_REQUIRE((uintptr_t)partials % 8 == 0, "tem_distribution_align_st: partials must be 8-byte aligned");
    TEM_REQUIRE(source0 > 0.f && source1 > 0.f && source0 <= 3.0e38f && source1 <= 3.0e38f,
                "tem_distribution_align_st: the source distribution must be finite and positive");
    const int64_t bytes = n * tem_st_size(st);
    TEM_REQUIRE((const char*)out + bytes <= (const char*)labels || (const char*)labels + bytes <= (const char*)out,
                "tem_distribution_align_st: out must not overlap the labels");
    TEM_ST_SWITCH(st, T, {
        constexpr int VEC = 16 / (int)sizeof(T);
        const int64_t nvec = ((uintptr_t)labels % 16 == 0 && (uintptr_t)out % 16 == 0) ? n / VEC : 0;
        hipLaunchKernelGGL((k_distribution_align<T>), dim3(da_parts(n, st)), dim3(256), 0, (hipStream_t)stream, (const T*)labels, (T*)out, n,
                           nvec, (const unsigned long long*)partials, parts, threshold, source0, source1);
    });
    TEM_CHECK_LAUNCH("tem_distribution_align_st");
    return TEM_OK;
}
