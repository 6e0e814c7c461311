// defect.hip -- the EM defect augmentation on the device (reference transform/defect.py: EMDefectAugmentation :41-245).
//
// All kernels work on S contiguous float32 slices of H x W (L = H * W elements).  Two small device tables written by the
// host describe a call, so the number of launches does not depend on what the plan says:
//   plan[S][4]  (int32): code (DF_*), plane (artifact / alpha plane of a paste), bits of the contrast scale, 0
//   rec[D][8]   (int32), one record per deformed slice: slice, mode (0 undirected, 1 compress with one line interval per
//               row, 2 compress with one per column), offset of the interval table in `tables`, stream row of the first
//               noise field (the second: + 1), bits of the positive side's flow along columns and along rows, bits of cval, 0
//   tables      (int32): per compress slice H (mode 1) or W (mode 2) entries lo | hi << 16: the pixels of the line in that
//               row (column) are lo..hi
// Nothing is read back, allocated or synchronised, and there are no atomics: every result is bitwise reproducible.
//
// Streaming pass (k_df_apply): rows walked as k_rn_apply of rawnorm.hip walks them (float4 body, up to three scalar head and
// tail elements, the output's alignment checked apart from the input's).  Deformed slices are skipped: the warp writes them.
// Mean (k_df_mean): one workgroup per low-contrast slice, float64 accumulation in a fixed order.
//
// Separable filter (k_df_sep), one kernel for the smoothed flow planes and for the cubic B-spline prefilter: a workgroup
// stages its tile with the halo in LDS, runs the pass along W into a second LDS buffer and the pass along H from there to
// global memory (the structure of k_ra_blur2d of rawaug.hip).  For the flow the staged values are generated, not loaded:
// noise(cy, cx) * strength at the CLAMPED index (edge repeat), noise = 2u - 1 with u = (w0 >> 8) * 2^-24 of the package's
// Philox stream, so the noise never exists in HBM.  For the prefilter they are the slice's pixels at the MIRRORED index
// (whole-sample mirror, period 2(n - 1)), and the weights are the two-sided impulse response sqrt(3) z^|k| of the recursion
// (z = sqrt(3) - 2) cut after 16 taps a side (|z|^17 < 2e-10).  One output per lane in both passes: consecutive lanes read
// consecutive dwords of LDS (conflict-free within each 32-lane half) and store consecutive dwords.
//
// Warp (k_df_warp): one lane per output pixel of a deformed slice.  Coordinates, B-spline weights and the 4 x 4 sum are
// float64 (the coordinate column + flow is then exact, so the range test agrees with a float64 reference fed the same flow);
// the sum is rounded to float32 once.  Compress: side and the zeroed band (L1 distance <= 10 to a line pixel) come from the
// interval table, the small noise from the stream, and the flow is rounded as numpy rounds it:
// fl32(double(side * f) + noise * (strength / 8)).
//
// Floating point: contraction is OFF for this file (pragma below and -ffp-contract=off in the Makefile), so the low-contrast
// chain and the alpha blend are numpy's float32 expressions bit for bit.  The filter asks for its fused multiply-adds
// explicitly (__builtin_fmaf).
#include "tem_common.h"

#pragma clang fp contract(off)

enum { DF_KEEP = 0, DF_DROP = 1, DF_LOW = 2, DF_PASTE = 3, DF_DEFORM = 4 };

#define DF_M0 0xD2511F53u
#define DF_M1 0xCD9E8D57u
#define DF_W0 0x9E3779B9u
#define DF_W1 0xBB67AE85u

// w0 of Philox4x32-10 with key = seed, counter = (i lo, i hi, row, 0): the stream of rawaug.hip
__device__ __forceinline__ unsigned df_word0(uint64_t seed, unsigned row, uint64_t i) {
    unsigned c0 = (unsigned)i, c1 = (unsigned)(i >> 32), c2 = row, c3 = 0u;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(DF_M0, c0), l0 = DF_M0 * c0;
        const unsigned h1 = __umulhi(DF_M1, c2), l1 = DF_M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += DF_W0;
        k1 += DF_W1;
    }
    return c0;
}

// 2u - 1, u = (w >> 8) * 2^-24: a multiple of 2^-23 in [-1, 1), exact in float32
__device__ __forceinline__ float df_noise(unsigned w) { return 2.f * ((float)(w >> 8) * 0x1p-24f) - 1.f; }

// ---------------------------------------------------------------------------
// per-slice mean of the low-contrast slices
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_df_mean(const float* __restrict__ x, int64_t L, const int* __restrict__ plan,
                                                 float* __restrict__ mean) {
    const int n = blockIdx.x;
    if (plan[4 * n] != DF_LOW) {   // uniform over the workgroup
        if (threadIdx.x == 0) mean[n] = 0.f;
        return;
    }
    const float* row = x + (int64_t)n * L;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < L; i += 256) acc += (double)row[i];
    acc = tem_wave_sum_d(acc);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) mean[n] = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)L);
}

extern "C" int tem_defect_mean(const float* x, int S, int64_t L, const int32_t* plan, float* mean, tem_stream_t stream) {
    TEM_REQUIRE(x && plan && mean && S > 0 && L > 0, "tem_defect_mean: bad arguments");
    hipLaunchKernelGGL(k_df_mean, dim3(S), dim3(256), 0, (hipStream_t)stream, x, L, plan, mean);
    TEM_CHECK_LAUNCH("tem_defect_mean");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// streaming pass: keep, drop, low contrast, paste
// ---------------------------------------------------------------------------
static inline int df_blocks(int64_t L, int N) {   // workgroups per row: the launch shape of rawnorm.hip
    int64_t cap = 2048 / N;
    if (cap < 8) cap = 8;
    const int64_t b = tem_cdiv(L, 1024);
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

__device__ __forceinline__ float4 df_ld4(const float* p, bool vec) {
    return vec ? *(const float4*)p : make_float4(p[0], p[1], p[2], p[3]);
}

__global__ __launch_bounds__(256) void k_df_apply(const float* __restrict__ x, float* __restrict__ y, int64_t L,
                                                  const int* __restrict__ plan, const float* __restrict__ mean,
                                                  const float* __restrict__ art, const float* __restrict__ alpha) {
    const int n = blockIdx.y;
    const int code = plan[4 * n];   // uniform over the workgroup
    if (code == DF_DEFORM) return;  // the warp writes this slice
    const float* row = x + (int64_t)n * L;
    float* out = y + (int64_t)n * L;
    const bool paste = code == DF_PASTE;
    const float s = __int_as_float(plan[4 * n + 2]);
    const float m = code == DF_LOW ? mean[n] : 0.f;
    const float* ar = paste ? art + (int64_t)plan[4 * n + 1] * L : row;
    const float* al = paste ? alpha + (int64_t)plan[4 * n + 1] * L : row;
    auto f = [&](float v, float a, float w) {
        if (code == DF_DROP) return 0.f;
        if (code == DF_LOW) return (v - m) * s + m;          // raw -= mean; raw *= scale; raw += mean
        if (code == DF_PASTE) return v * (1.f - w) + a * w;  // raw * (1 - alpha) + artifact * alpha
        return v;
    };
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > L) head = L;
    const int64_t nv = (L - head) >> 2;
    const float4* __restrict__ v = (const float4*)(row + head);
    const bool vec_out = (((uintptr_t)(out + head)) & 15u) == 0;   // y, art and alpha may sit at other offsets mod 16 than x
    const bool vec_ar = (((uintptr_t)(ar + head)) & 15u) == 0, vec_al = (((uintptr_t)(al + head)) & 15u) == 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const float4 a = v[i];
        const int64_t e = head + 4 * i;
        float4 b = a, c = a;
        if (paste) {
            b = df_ld4(ar + e, vec_ar);
            c = df_ld4(al + e, vec_al);
        }
        const float4 r = make_float4(f(a.x, b.x, c.x), f(a.y, b.y, c.y), f(a.z, b.z, c.z), f(a.w, b.w, c.w));
        float* o = out + e;
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
        int64_t e = -1;
        if (t < head) e = t;
        else if (t >= 64 && tail0 + (t - 64) < L) e = tail0 + (t - 64);
        if (e >= 0) out[e] = f(row[e], ar[e], al[e]);
    }
}

extern "C" int tem_defect_apply(const float* x, float* y, int S, int64_t L, const int32_t* plan, const float* mean,
                                const float* art, const float* alpha, tem_stream_t stream) {
    TEM_REQUIRE(x && y && x != y && plan && mean && S > 0 && S <= 65535 && L > 0, "tem_defect_apply: bad arguments (x and y must differ)");
    hipLaunchKernelGGL(k_df_apply, dim3(df_blocks(L, S), S), dim3(256), 0, (hipStream_t)stream, x, y, L, plan, mean, art, alpha);
    TEM_CHECK_LAUNCH("tem_defect_apply");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// separable filter: smoothed noise planes (edge repeat) and spline coefficients (mirror)
// ---------------------------------------------------------------------------
#define DF_TH 32
#define DF_TW 64
#define DF_KMAX 33

__device__ __forceinline__ int df_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ int df_mirror(int i, int n) {   // whole-sample mirror, reflected as often as it takes; n >= 2
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// grid (tiles in x, tiles in y, planes); plane z: NOISE -> field z & 1 of record z >> 1, else the slice of record z;
// out + z * H * W receives it.  LDS: in[TH + 2 r][TW + 2 r], then (16-byte aligned) mid[TH + 2 r][TW]
template <bool NOISE>
__global__ __launch_bounds__(256) void k_df_sep(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                const int* __restrict__ rec, const float* __restrict__ w, int k, uint64_t seed,
                                                float strength) {
    extern __shared__ float4 df_lds4[];
    float* lds = (float*)df_lds4;
    const int* rc = rec + 8 * (NOISE ? (int)(blockIdx.z >> 1) : (int)blockIdx.z);
    if (NOISE && rc[1] != 0) return;   // a compress slice has no smoothed planes (uniform over the workgroup, before any barrier)
    const int r = k >> 1;
    const int IH = DF_TH + 2 * r, IW = DF_TW + 2 * r;
    float* in = lds;
    float* mid = lds + ((IH * IW + 3) & ~3);
    const int x0 = blockIdx.x * DF_TW, y0 = blockIdx.y * DF_TH;
    const int t = threadIdx.x;
    const unsigned srow = (unsigned)rc[3] + (blockIdx.z & 1u);
    const float* src = NOISE ? nullptr : x + (int64_t)rc[0] * H * W;
    float* dst = out + (int64_t)blockIdx.z * H * W;
    for (int e = t; e < IH * IW; e += 256) {
        const int yy = e / IW, xx = e - yy * IW;
        const int gy = y0 - r + yy, gx = x0 - r + xx;
        if (NOISE) in[e] = df_noise(df_word0(seed, srow, (uint64_t)((int64_t)df_clamp(gy, H) * W + df_clamp(gx, W)))) * strength;
        else in[e] = src[(int64_t)df_mirror(gy, H) * W + df_mirror(gx, W)];
    }
    __syncthreads();
    for (int e = t; e < IH * DF_TW; e += 256) {
        const int yy = e / DF_TW, xx = e % DF_TW;
        const float* p = in + yy * IW + xx;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc = __builtin_fmaf(w[j], p[j], acc);
        mid[e] = acc;
    }
    __syncthreads();
    for (int e = t; e < DF_TH * DF_TW; e += 256) {
        const int oy = e / DF_TW, ox = e % DF_TW;
        const int gy = y0 + oy, gx = x0 + ox;
        if (gy >= H || gx >= W) continue;
        const float* p = mid + oy * DF_TW + ox;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc = __builtin_fmaf(w[j], p[j * DF_TW], acc);
        dst[(int64_t)gy * W + gx] = acc;
    }
}

template <bool NOISE>
static int df_launch_sep(const char* name, const float* x, float* out, int planes, int H, int W, const int32_t* rec, const float* w,
                         int k, uint64_t seed, float strength, tem_stream_t stream) {
    const int r = k / 2;
    const int IH = DF_TH + 2 * r, IW = DF_TW + 2 * r;
    const size_t lds = ((size_t)((IH * IW + 3) & ~3) + (size_t)IH * DF_TW) * sizeof(float);
    const dim3 grid((unsigned)tem_cdiv(W, DF_TW), (unsigned)tem_cdiv(H, DF_TH), (unsigned)planes);
    TEM_REQUIRE(grid.y <= 65535 && planes <= 65535, "%s: at most %d rows per slice and 65535 planes", name, 65535 * DF_TH);
    hipLaunchKernelGGL(k_df_sep<NOISE>, grid, dim3(256), lds, (hipStream_t)stream, x, out, H, W, rec, w, k, seed, strength);
    TEM_CHECK_LAUNCH(name);
    return TEM_OK;
}

#define DF_GEOM_OK(D, H, W) ((D) > 0 && (H) >= 4 && (W) >= 4 && (int64_t)(H) * (W) < 0x7fffffffll)

extern "C" int tem_defect_flow(float* flow, int D, int H, int W, const int32_t* rec, uint64_t seed, float strength, const float* w,
                               int k, tem_stream_t stream) {
    TEM_REQUIRE(flow && rec && w && DF_GEOM_OK(D, H, W) && D <= 32767, "tem_defect_flow: bad arguments (slices of at least 4 x 4)");
    TEM_REQUIRE(k >= 1 && k <= DF_KMAX && (k & 1), "tem_defect_flow: the tap count must be odd and within 1..%d (got %d)", DF_KMAX, k);
    return df_launch_sep<true>("tem_defect_flow", nullptr, flow, 2 * D, H, W, rec, w, k, seed, strength, stream);
}

extern "C" int tem_defect_prefilter(const float* x, float* coef, int D, int H, int W, const int32_t* rec, const float* w, int k,
                                    tem_stream_t stream) {
    TEM_REQUIRE(x && coef && rec && w && DF_GEOM_OK(D, H, W), "tem_defect_prefilter: bad arguments (slices of at least 4 x 4)");
    TEM_REQUIRE(k >= 1 && k <= DF_KMAX && (k & 1), "tem_defect_prefilter: the tap count must be odd and within 1..%d (got %d)", DF_KMAX, k);
    return df_launch_sep<false>("tem_defect_prefilter", x, coef, D, H, W, rec, w, k, 0, 0.f, stream);
}

// ---------------------------------------------------------------------------
// cubic warp
// ---------------------------------------------------------------------------
// scipy's weights of the cubic B-spline at offset t in [0, 1) from the second of the four coefficients
__device__ __forceinline__ void df_weights(double t, double* w) {
    const double z = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}

// grid (pixels / 256, D)
__global__ __launch_bounds__(256) void k_df_warp(const float* __restrict__ coef, const float* __restrict__ flow, float* __restrict__ y,
                                                 int H, int W, const int* __restrict__ rec, const int* __restrict__ tables, uint64_t seed,
                                                 double nscale) {
    const int d = blockIdx.y;
    const int* rc = rec + 8 * d;
    const int HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int r = p / W, c = p - r * W;
    const int mode = rc[1];
    float* out = y + (int64_t)rc[0] * HW;
    const float* cf = coef + (int64_t)d * HW;
    double cy, cx;
    if (mode == 0) {
        const float* fl = flow + (int64_t)d * 2 * HW;
        cx = (double)c + (double)fl[p];
        cy = (double)r + (double)fl[HW + p];
    } else {
        const int* tab = tables + rc[2];
        const bool rows = mode == 1;
        const int nt = rows ? H : W, a = rows ? r : c, b = rows ? c : r;
        bool band = false;
        for (int da = -10; da <= 10; ++da) {
            const int aa = a + da;
            if (aa < 0 || aa >= nt) continue;
            const int e = tab[aa], lo = e & 0xffff, hi = (e >> 16) & 0xffff;
            const int dist = b < lo ? lo - b : (b > hi ? b - hi : 0);
            band = band || dist <= 10 - (da < 0 ? -da : da);
        }
        if (band) {
            out[p] = 0.f;
            return;
        }
        const int e = tab[a], lo = e & 0xffff, hi = (e >> 16) & 0xffff;
        float sgn = b < lo ? -1.f : (b > hi ? 1.f : 0.f);   // rows: left of the line is the negative side
        if (!rows) sgn = -sgn;                             // columns: above the line is the positive side
        const double nx = (double)df_noise(df_word0(seed, (unsigned)rc[3], (uint64_t)p));
        const double ny = (double)df_noise(df_word0(seed, (unsigned)rc[3] + 1u, (uint64_t)p));
        const float fx = (float)((double)(__int_as_float(rc[4]) * sgn) + nx * nscale);
        const float fy = (float)((double)(__int_as_float(rc[5]) * sgn) + ny * nscale);
        cx = (double)c + (double)fx;
        cy = (double)r + (double)fy;
    }
    float v = __int_as_float(rc[6]);
    if (cy >= 0.0 && cy <= (double)(H - 1) && cx >= 0.0 && cx <= (double)(W - 1)) {
        const double fy0 = floor(cy), fx0 = floor(cx);
        double wy[4], wx[4];
        df_weights(cy - fy0, wy);
        df_weights(cx - fx0, wx);
        const int iy = (int)fy0 - 1, ix = (int)fx0 - 1;
        int xs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xs[i] = df_mirror(ix + i, W);
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* line = cf + (int64_t)df_mirror(iy + j, H) * W;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) s += wx[i] * (double)line[xs[i]];
            acc += wy[j] * s;
        }
        v = (float)acc;
    }
    out[p] = v;
}

extern "C" int tem_defect_warp(const float* coef, const float* flow, float* y, int D, int H, int W, const int32_t* rec,
                               const int32_t* tables, uint64_t seed, double noise_scale, tem_stream_t stream) {
    TEM_REQUIRE(coef && flow && y && rec && tables && DF_GEOM_OK(D, H, W) && D <= 65535 && H <= 65535 && W <= 65535,
                "tem_defect_warp: bad arguments (slices of at least 4 x 4)");
    hipLaunchKernelGGL(k_df_warp, dim3((unsigned)tem_cdiv((int64_t)H * W, 256), D), dim3(256), 0, (hipStream_t)stream, coef, flow, y, H, W,
                       rec, tables, seed, noise_scale);
    TEM_CHECK_LAUNCH("tem_defect_warp");
    return TEM_OK;
}
