// rawnorm.hip -- min-max / percentile normalisation and contrast of raw data on the device (reference transform/raw.py:
// normalize :88-116, normalize_percentile :119-140, RandomPercentileNormalization :143-297, RandomContrast :305-334).
//
// Rows are N contiguous float32 rows of length L.  Three parts:
//   * row min / max: fixed grid of partials + one block per row (exact in any order => bitwise reproducible);
//   * exact row order statistics: MSB-first radix select, four passes over 8-bit digits of the order-preserving key of the
//     float bits (negatives: all bits flipped, others: sign bit flipped).  Each of the K ranks of a row carries its own key
//     prefix and residual rank (RnState); ranks that still share a prefix share one histogram (`owner`), so the usual
//     percentile quadruple (lo, lo + 1, hi, hi + 1) costs two histograms per pass, and the first pass one.  Per pass:
//     k_rn_hist counts, per workgroup in LDS, the digit of the elements that match a live prefix and adds the non-empty bins
//     to a zeroed 64-bit table with INTEGER global atomics (order-independent => bitwise reproducible; no float atomics);
//     k_rn_select scans the 256 bins per rank and advances prefix and rank.  Nothing is read back to the host;
//   * elementwise apply / contrast with per-row coefficients read from device memory, every operation one correctly
//     rounded fp32 operation in numpy's order: contraction is off for this file (pragma below and -ffp-contract=off in the
//     Makefile; hipcc's default fuses
//     a*b+c into one fma, also through __fmul_rn / __fadd_rn, which are plain operators here), and the division is IEEE.
//
// Contention (the top byte of real images is nearly constant, and quantised data puts every matching element of the late
// passes into bin 0): the option taken is WAVE AGGREGATION IN FRONT OF THE LDS ATOMIC.  A wave ballots its lanes against the
// digit of its first live lane and that lane adds the population count once; this is repeated up to RN_PEEL times on the
// lanes left over, and only what is still left does one LDS atomic per lane.  Why this one: it needs no second LDS copy of
// the histograms (per-wave private histograms of 8 ranks x 256 bins x 4 waves would be 32 KiB and halve the blocks per CU),
// no knowledge of the key range before the first pass (wider digits of key - key_min need a min pass first and still
// collapse on two-level data), it is exact for every distribution, and with diverse digits (the mantissa bytes of
// continuous data) it costs RN_PEEL ballots per element group and then runs as plain low-conflict atomics.
//
// Ranks and interpolation weights are host values: they travel in by-value kernel arguments (RN_ROWS rows per launch,
// looped over on the host) -- no device allocation, no copy, no synchronisation inside the library.
#include "tem_common.h"

// no a*b+c of this file becomes an fma, whatever builds it (the Makefile passes -ffp-contract=off as well: that also covers
// code the pragma might not reach after inlining)
#pragma clang fp contract(off)

#define RN_ROWS 16     // rows whose host values fit one by-value argument
#define RN_KMAX 8      // ranks per row and call
#define RN_PEEL 4      // wave-aggregation rounds in front of the per-lane LDS atomics
#define RN_FILL 64     // floats per tem_rawnorm_fill launch

typedef unsigned long long rn_u64;

struct RnState {       // one per (row, rank), in the workspace
    unsigned prefix;   // key bits decided so far (high bits)
    unsigned owner;    // smallest rank index of this row with the same prefix: the histogram this rank reads
    int64_t rank;      // residual rank among the elements that match the prefix
};
struct RnRanks { int64_t r[RN_ROWS][RN_KMAX]; };
struct RnWeights { float t[RN_ROWS][2]; };
struct RnFill { float v[RN_FILL]; };

__device__ __forceinline__ unsigned rn_key(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float rn_unkey(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Every element of a row once: float4 loads of the 16-byte aligned body (grid-stride over the blocks of the row), the up to
// three head and tail elements by block 0.  f(index in row, value).
template <class F>
__device__ __forceinline__ void rn_foreach(const float* __restrict__ row, int64_t L, F f) {
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > L) head = L;
    const int64_t nv = (L - head) >> 2;
    const float4* __restrict__ v = (const float4*)(row + head);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const float4 q = v[i];
        const int64_t e = head + 4 * i;
        f(e, q.x);
        f(e + 1, q.y);
        f(e + 2, q.z);
        f(e + 3, q.w);
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + 4 * nv;
        const int t = threadIdx.x;
        if (t < head) f((int64_t)t, row[t]);
        else if (t >= 64 && tail0 + (t - 64) < L) f(tail0 + (t - 64), row[tail0 + (t - 64)]);
    }
}

static inline int rn_blocks(int64_t L, int N) {   // workgroups per row
    int64_t cap = 2048 / N;
    if (cap < 8) cap = 8;
    const int64_t b = tem_cdiv(L, 1024);
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

// ---------------------------------------------------------------------------
// row min / max
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rn_minmax_partial(const float* __restrict__ x, int64_t L, float* __restrict__ part) {
    const int n = blockIdx.y;
    const float* row = x + (int64_t)n * L;
    float mn = row[0], mx = row[0];
    rn_foreach(row, L, [&](int64_t, float v) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    __shared__ float sh[2][4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = mn; sh[1][w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) {
            mn = sh[0][i] < mn ? sh[0][i] : mn;
            mx = sh[1][i] > mx ? sh[1][i] : mx;
        }
        part[((int64_t)n * gridDim.x + blockIdx.x) * 2 + 0] = mn;
        part[((int64_t)n * gridDim.x + blockIdx.x) * 2 + 1] = mx;
    }
}

__global__ __launch_bounds__(64) void k_rn_minmax_final(const float* __restrict__ part, int nblk, float* __restrict__ mn_out,
                                                        float* __restrict__ mx_out) {
    const int n = blockIdx.x;
    float mn = part[(int64_t)n * nblk * 2], mx = part[(int64_t)n * nblk * 2 + 1];
    for (int b = threadIdx.x; b < nblk; b += 64) {
        const float a = part[((int64_t)n * nblk + b) * 2], c = part[((int64_t)n * nblk + b) * 2 + 1];
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (threadIdx.x == 0) { mn_out[n] = mn; mx_out[n] = mx; }
}

extern "C" int64_t tem_rawnorm_ws(int N, int64_t L, int K) {
    if (N <= 0 || L <= 0 || K < 0 || K > RN_KMAX) return 0;
    const int64_t mm = (int64_t)N * rn_blocks(L, N) * 2 * (int64_t)sizeof(float);
    const int64_t sel = (int64_t)N * K * ((int64_t)sizeof(RnState) + 256 * (int64_t)sizeof(rn_u64));
    return mm > sel ? mm : sel;
}

#define RN_CHECK_WS(name, need)                                                                         \
    do {                                                                                                \
        if ((need) > ws_bytes) {                                                                        \
            tem_set_error(name ": workspace too small (%lld bytes needed)", (long long)(need));         \
            return TEM_EWS;                                                                             \
        }                                                                                               \
    } while (0)

extern "C" int tem_row_minmax(const float* x, int N, int64_t L, float* mn, float* mx, void* ws, int64_t ws_bytes,
                              tem_stream_t stream) {
    TEM_REQUIRE(x && mn && mx && ws && N > 0 && N <= 65535 && L > 0, "tem_row_minmax: bad arguments");
    const int nblk = rn_blocks(L, N);
    RN_CHECK_WS("tem_row_minmax", tem_rawnorm_ws(N, L, 0));
    hipLaunchKernelGGL(k_rn_minmax_partial, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, x, L, (float*)ws);
    hipLaunchKernelGGL(k_rn_minmax_final, dim3(N), dim3(64), 0, (hipStream_t)stream, (const float*)ws, nblk, mn, mx);
    TEM_CHECK_LAUNCH("tem_row_minmax");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// radix select
// ---------------------------------------------------------------------------
// One element into histogram h: the lanes of the wave that are here and `live` are counted per digit, the most frequent
// digits by one add of a population count each (see the file header).
__device__ __forceinline__ void rn_hist_add(unsigned* h, unsigned digit, bool live) {
    const int lane = threadIdx.x & 63;
    rn_u64 rest = __ballot(live);
#pragma unroll 1
    for (int it = 0; it < RN_PEEL && rest; ++it) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rest) - 1);
        const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
        const rn_u64 m = __ballot(live && digit == d0);
        if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(m));
        if (digit == d0) live = false;
        rest &= ~m;
    }
    if (live) atomicAdd(&h[digit], 1u);
}

// table: [N][K][256] counts of this pass (one table, cleared before every pass: 2 KiB of workspace per row and rank).  FIRST: no prefix yet, one histogram (rank 0's) per row.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_rn_hist(const float* __restrict__ x, int64_t L, int K, int shift,
                                                 const RnState* __restrict__ st, rn_u64* __restrict__ table) {
    __shared__ unsigned hist[RN_KMAX * 256];
    __shared__ unsigned s_pref[RN_KMAX];
    __shared__ int s_slot[RN_KMAX];
    __shared__ int s_np;
    const int n = blockIdx.y;
    const int nh = FIRST ? 1 : K;
    for (int i = threadIdx.x; i < nh * 256; i += 256) hist[i] = 0;
    if (threadIdx.x == 0) {
        int np = 0;
        if (FIRST) {
            s_pref[0] = 0;
            s_slot[0] = 0;
            np = 1;
        } else {
            for (int k = 0; k < K; ++k) {
                const RnState s = st[(int64_t)n * K + k];
                if ((int)s.owner == k) {
                    s_pref[np] = s.prefix;
                    s_slot[np] = k;
                    ++np;
                }
            }
        }
        s_np = np;
    }
    __syncthreads();
    const int np = s_np;
    const float* row = x + (int64_t)n * L;
    rn_foreach(row, L, [&](int64_t, float v) {
        const unsigned key = rn_key(v);
        const unsigned digit = (key >> shift) & 255u;
        if (FIRST) {
            rn_hist_add(hist, digit, true);
        } else {
            const unsigned hi = key >> (shift + 8);
            for (int j = 0; j < np; ++j)
                rn_hist_add(hist + s_slot[j] * 256, digit, hi == (s_pref[j] >> (shift + 8)));
        }
    });
    __syncthreads();
    for (int i = threadIdx.x; i < nh * 256; i += 256) {
        const unsigned c = hist[i];
        if (c) atomicAdd(&table[(int64_t)n * K * 256 + i], (rn_u64)c);
    }
}

// the host's ranks of up to RN_ROWS rows into the state of the first pass (st: the first of these rows)
__global__ void k_rn_init(RnRanks ranks, int rows, int K, RnState* __restrict__ st) {
    const int i = threadIdx.x / RN_KMAX, k = threadIdx.x % RN_KMAX;
    if (i < rows && k < K) {
        RnState s;
        s.prefix = 0;
        s.owner = 0;
        s.rank = ranks.r[i][k];
        st[(int64_t)i * K + k] = s;
    }
}

// One block per row: per rank, an inclusive scan of its histogram's 256 bins finds the digit that holds the rank.
// out (last pass): the key is complete, write the value.
__global__ __launch_bounds__(256) void k_rn_select(int K, int shift, const rn_u64* __restrict__ table, RnState* __restrict__ st,
                                                   float* __restrict__ out) {
    __shared__ rn_u64 sc[2][256];
    __shared__ RnState s_new[RN_KMAX];
    const int n = blockIdx.x;
    const int t = threadIdx.x;
    for (int k = 0; k < K; ++k) {
        RnState s = st[(int64_t)n * K + k];
        const rn_u64 c = table[((int64_t)n * K + s.owner) * 256 + t];
        int cur = 0;
        sc[0][t] = c;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const rn_u64 a = sc[cur][t] + (t >= o ? sc[cur][t - o] : 0ull);
            sc[cur ^ 1][t] = a;
            cur ^= 1;
            __syncthreads();
        }
        const rn_u64 incl = sc[cur][t], excl = incl - c;
        if (t == 0) s_new[k] = s;   // stays if the rank is out of range (the host checks that it is not)
        __syncthreads();
        if ((rn_u64)s.rank >= excl && (rn_u64)s.rank < incl) {
            s_new[k].prefix = s.prefix | ((unsigned)t << shift);
            s_new[k].rank = s.rank - (int64_t)excl;
        }
        __syncthreads();
    }
    if (t < K) {
        RnState s = s_new[t];
        unsigned owner = (unsigned)t;
        for (int j = t - 1; j >= 0; --j)
            if (s_new[j].prefix == s.prefix) owner = (unsigned)j;
        s.owner = owner;
        st[(int64_t)n * K + t] = s;
        if (out) out[(int64_t)n * K + t] = rn_unkey(s.prefix);
    }
}

extern "C" int tem_row_select(const float* x, int N, int64_t L, const int64_t* ranks, int K, float* out, void* ws,
                              int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(x && ranks && out && ws && N > 0 && N <= 65535 && L > 0 && K > 0 && K <= RN_KMAX,
                "tem_row_select: bad arguments (1 <= K <= %d ranks per row, N <= 65535 rows)", RN_KMAX);
    for (int64_t i = 0; i < (int64_t)N * K; ++i)
        TEM_REQUIRE(ranks[i] >= 0 && ranks[i] < L, "tem_row_select: rank %lld is outside [0, %lld)", (long long)ranks[i], (long long)L);
    RN_CHECK_WS("tem_row_select", tem_rawnorm_ws(N, L, K));
    RnState* st = (RnState*)ws;
    rn_u64* table = (rn_u64*)(st + (int64_t)N * K);
    const int64_t per_pass = (int64_t)N * K * 256;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0, per_pass * sizeof(rn_u64), s) != hipSuccess) {
        tem_set_error("tem_row_select: clearing the histogram table failed");
        return TEM_ELAUNCH;
    }
    const int nblk = rn_blocks(L, N);
    for (int row0 = 0; row0 < N; row0 += RN_ROWS) {
        const int rows = N - row0 < RN_ROWS ? N - row0 : RN_ROWS;
        RnRanks rk = {};
        for (int i = 0; i < rows; ++i)
            for (int k = 0; k < K; ++k) rk.r[i][k] = ranks[(int64_t)(row0 + i) * K + k];
        hipLaunchKernelGGL(k_rn_init, dim3(1), dim3(RN_ROWS * RN_KMAX), 0, s, rk, rows, K, st + (int64_t)row0 * K);
    }
    for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
        if (p && hipMemsetAsync(table, 0, per_pass * sizeof(rn_u64), s) != hipSuccess) {
            tem_set_error("tem_row_select: clearing the histogram table failed");
            return TEM_ELAUNCH;
        }
        if (p == 0)
            hipLaunchKernelGGL(k_rn_hist<true>, dim3(nblk, N), dim3(256), 0, s, x, L, K, shift, (const RnState*)st, table);
        else
            hipLaunchKernelGGL(k_rn_hist<false>, dim3(nblk, N), dim3(256), 0, s, x, L, K, shift, (const RnState*)st, table);
        hipLaunchKernelGGL(k_rn_select, dim3(N), dim3(256), 0, s, K, shift, (const rn_u64*)table, st, p == 3 ? out : nullptr);
    }
    TEM_CHECK_LAUNCH("tem_row_select");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// per-row coefficients: sub, div of y = (x - sub) / div
// ---------------------------------------------------------------------------
__global__ void k_rn_fill(RnFill f, int n, float* __restrict__ dst) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = f.v[threadIdx.x];
}

extern "C" int tem_rawnorm_fill(float* dst, const float* values, int64_t n, tem_stream_t stream) {
    TEM_REQUIRE(dst && values && n > 0, "tem_rawnorm_fill: bad arguments");
    for (int64_t i0 = 0; i0 < n; i0 += RN_FILL) {
        const int m = (int)(n - i0 < RN_FILL ? n - i0 : RN_FILL);
        RnFill f;
        for (int i = 0; i < RN_FILL; ++i) f.v[i] = i < m ? values[i0 + i] : 0.f;
        hipLaunchKernelGGL(k_rn_fill, dim3(1), dim3(RN_FILL), 0, (hipStream_t)stream, f, m, dst + i0);
    }
    TEM_CHECK_LAUNCH("tem_rawnorm_fill");
    return TEM_OK;
}

__global__ void k_rn_minmax_coef(const float* __restrict__ mn, const float* __restrict__ mx, int N, float eps,
                                 float* __restrict__ sub, float* __restrict__ div) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    sub[n] = mn[n];
    div[n] = __fadd_rn(__fsub_rn(mx[n], mn[n]), eps);
}

extern "C" int tem_rawnorm_minmax_coef(const float* mn, const float* mx, int N, float eps, float* sub, float* div,
                                       tem_stream_t stream) {
    TEM_REQUIRE(mn && mx && sub && div && N > 0, "tem_rawnorm_minmax_coef: bad arguments");
    hipLaunchKernelGGL(k_rn_minmax_coef, dim3((unsigned)tem_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, mn, mx, N, eps, sub, div);
    TEM_CHECK_LAUNCH("tem_rawnorm_minmax_coef");
    return TEM_OK;
}

// numpy's _lerp in float32: a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5
__device__ __forceinline__ float rn_lerp(float a, float b, float t) {
    const float d = __fsub_rn(b, a);
    return t >= 0.5f ? __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.f, t))) : __fadd_rn(a, __fmul_rn(d, t));
}

// os: [rows][4] order statistics (lower, its upper neighbour, upper, its upper neighbour) of rows row0 ...
__global__ void k_rn_percentile_coef(RnWeights w, const float* __restrict__ os, int rows, float eps, float* __restrict__ sub,
                                     float* __restrict__ div, float* __restrict__ v) {
    const int i = threadIdx.x;
    if (i >= rows) return;
    const float lo = rn_lerp(os[4 * i + 0], os[4 * i + 1], w.t[i][0]);
    const float hi = rn_lerp(os[4 * i + 2], os[4 * i + 3], w.t[i][1]);
    sub[i] = lo;
    div[i] = __fadd_rn(__fsub_rn(hi, lo), eps);
    if (v) {
        v[2 * i] = lo;
        v[2 * i + 1] = hi;
    }
}

extern "C" int tem_rawnorm_percentile_coef(const float* os, const float* t, int N, float eps, float* sub, float* div, float* v,
                                           tem_stream_t stream) {
    TEM_REQUIRE(os && t && sub && div && N > 0, "tem_rawnorm_percentile_coef: bad arguments");
    for (int row0 = 0; row0 < N; row0 += RN_ROWS) {
        const int rows = N - row0 < RN_ROWS ? N - row0 : RN_ROWS;
        RnWeights w;
        for (int i = 0; i < RN_ROWS; ++i)
            for (int j = 0; j < 2; ++j) w.t[i][j] = i < rows ? t[(int64_t)(row0 + i) * 2 + j] : 0.f;
        hipLaunchKernelGGL(k_rn_percentile_coef, dim3(1), dim3(RN_ROWS), 0, (hipStream_t)stream, w, os + (int64_t)row0 * 4, rows,
                           eps, sub + row0, div + row0, v ? v + (int64_t)row0 * 2 : nullptr);
    }
    TEM_CHECK_LAUNCH("tem_rawnorm_percentile_coef");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// elementwise: apply and contrast
// ---------------------------------------------------------------------------
__device__ __forceinline__ float rn_clip(float v, float lo, float hi) {
    v = v > lo ? v : lo;
    return v < hi ? v : hi;
}

// CONTRAST: y = m + a[n] * (x - m), else y = (x - sub[n]) / div[n]; p = sub / (unused), q = div / a
template <bool CONTRAST, bool CLIP>
__global__ __launch_bounds__(256) void k_rn_apply(const float* __restrict__ x, float* __restrict__ y, int64_t L,
                                                  const float* __restrict__ p, const float* __restrict__ q, float m, float lo,
                                                  float hi) {
    const int n = blockIdx.y;
    const float* row = x + (int64_t)n * L;
    float* out = y + (int64_t)n * L;
    const float c0 = CONTRAST ? m : p[n], c1 = q[n];
    auto f = [&](float v) {
        float r = CONTRAST ? __fadd_rn(c0, __fmul_rn(c1, __fsub_rn(v, c0))) : __fsub_rn(v, c0) / c1;
        return CLIP ? rn_clip(r, lo, hi) : r;
    };
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > L) head = L;
    const int64_t nv = (L - head) >> 2;
    const float4* __restrict__ v = (const float4*)(row + head);
    const bool vec_out = (((uintptr_t)(out + head)) & 15u) == 0;   // wave-uniform: y may sit at another offset mod 16 than x
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const float4 a = v[i];
        const float4 r = make_float4(f(a.x), f(a.y), f(a.z), f(a.w));
        float* o = out + head + 4 * i;
        if (vec_out) {
            *(float4*)o = r;
        } else {
            o[0] = r.x;
            o[1] = r.y;
            o[2] = r.z;
            o[3] = r.w;
        }
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + 4 * nv;
        const int t = threadIdx.x;
        if (t < head) out[t] = f(row[t]);
        else if (t >= 64 && tail0 + (t - 64) < L) out[tail0 + (t - 64)] = f(row[tail0 + (t - 64)]);
    }
}

template <bool CONTRAST>
static int rn_launch_apply(const char* name, const float* x, float* y, int N, int64_t L, const float* p, const float* q, float m,
                           int clip, float lo, float hi, tem_stream_t stream) {
    const dim3 grid(rn_blocks(L, N), N);
    if (clip)
        hipLaunchKernelGGL((k_rn_apply<CONTRAST, true>), grid, dim3(256), 0, (hipStream_t)stream, x, y, L, p, q, m, lo, hi);
    else
        hipLaunchKernelGGL((k_rn_apply<CONTRAST, false>), grid, dim3(256), 0, (hipStream_t)stream, x, y, L, p, q, m, lo, hi);
    TEM_CHECK_LAUNCH(name);
    return TEM_OK;
}

extern "C" int tem_rawnorm_apply(const float* x, float* y, int N, int64_t L, const float* sub, const float* div, int clip,
                                 float lo, float hi, tem_stream_t stream) {
    TEM_REQUIRE(x && y && sub && div && N > 0 && N <= 65535 && L > 0, "tem_rawnorm_apply: bad arguments");
    return rn_launch_apply<false>("tem_rawnorm_apply", x, y, N, L, sub, div, 0.f, clip, lo, hi, stream);
}

extern "C" int tem_rawnorm_contrast(const float* x, float* y, int N, int64_t L, const float* alpha, float mean, int clip,
                                    float lo, float hi, tem_stream_t stream) {
    TEM_REQUIRE(x && y && alpha && N > 0 && N <= 65535 && L > 0, "tem_rawnorm_contrast: bad arguments");
    return rn_launch_apply<true>("tem_rawnorm_contrast", x, y, N, L, alpha, alpha, mean, clip, lo, hi, stream);
}
