// rawaug.hip -- the noise and blur raw augmentations on the device (reference transform/raw.py: AdditiveGaussianNoise
// :337-363, AdditivePoissonNoise :366-391, PoissonNoise :394-425, GaussianBlur :428-454).
//
// Noise: rows are N contiguous float32 rows of length L, walked as k_rn_apply of rawnorm.hip walks them (float4 body, up to
// three scalar head and tail elements, the output's alignment checked apart from the input's, one grid row per data row).
// The random stream is Philox4x32-10 keyed by the call's 64-bit seed with the counter (i lo, i hi, row, round): the sample
// of element i of row `row` is a pure function of (seed, row, i) -- it does not depend on the grid, on the alignment of a
// pointer, on the head / body / tail split or on how many rows a launch carries ("The stream of the raw noise
// transforms", is the specification; torch_em_amd/transform/_philox.py is the same text in numpy).  Both sampler loops are
// bounded (80 search steps, 64 rejection rounds).  Per-row scalars are read from device arrays, the seed is a by-value
// argument; nothing is read back, allocated or synchronised, and there are no atomics.
//
// Floating point: contraction is OFF for this file (pragma below and -ffp-contract=off in the Makefile), so y = x + std * z,
// x + k / lam and k / mult + offset are a rounded multiply or IEEE division and a rounded add, and lam = (x - offset) * mult
// is what numpy computes in float32.  logf, expf, sqrtf, cospif and lgammaf are the accurate library functions: no
// __logf / __cosf, no fast-math flag.  The blur asks for its fused multiply-adds explicitly (__builtin_fmaf).
//
// Blur: one kernel, separable inside the workgroup.  A workgroup stages the input tile with its halo (reflect border, no
// edge repeat) in LDS, runs the row pass into a second LDS buffer and the column pass from there to global memory, so every
// input element is fetched once per tile plus the halo overlap.  The staged rows start at x0 - k/2, which is 16-byte aligned
// only by accident, so staging uses dword loads, consecutive lanes on consecutive addresses.  Row pass: one output per lane,
// consecutive lanes read consecutive dwords (ds_read_b32: conflict-free within each 32-lane half).  Column pass: one float4
// of four neighbouring outputs per lane and tap (ds_read_b128); the row-pass buffer is TW floats wide without padding: with
// TW = 64 (32) a 16-lane group of that instruction -- lanes {0-3, 12-15, 20-27} and so on -- touches two (four) buffer rows
// at 16 distinct 16-byte slots of the 256-byte bank row, which is conflict-free; a padded stride would break that.  The
// output tile starts at a multiple of TW, so stores are float4 wherever the plane's row is 16-byte aligned.
#include "tem_common.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------
// the stream
// ---------------------------------------------------------------------------
#define RA_M0 0xD2511F53u
#define RA_M1 0xCD9E8D57u
#define RA_W0 0x9E3779B9u
#define RA_W1 0xBB67AE85u
#define RA_INV_STEPS 80
#define RA_PTRS_ROUNDS 64

struct RaWords { unsigned w0, w1, w2, w3; };

__device__ __forceinline__ RaWords ra_philox(uint64_t seed, unsigned row, uint64_t i, unsigned round) {
    unsigned c0 = (unsigned)i, c1 = (unsigned)(i >> 32), c2 = row, c3 = round;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(RA_M0, c0), l0 = RA_M0 * c0;
        const unsigned h1 = __umulhi(RA_M1, c2), l1 = RA_M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += RA_W0;
        k1 += RA_W1;
    }
    RaWords w = {c0, c1, c2, c3};
    return w;
}

__device__ __forceinline__ float ra_u_oc(unsigned w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }   // (0, 1]
__device__ __forceinline__ float ra_u_co(unsigned w) { return (float)(w >> 8) * 0x1p-24f; }          // [0, 1)

__device__ __forceinline__ float ra_normal(uint64_t seed, unsigned row, uint64_t i) {
    const RaWords w = ra_philox(seed, row, i, 0u);
    return sqrtf(-2.f * logf(ra_u_oc(w.w0))) * cospif(2.f * ra_u_co(w.w1));
}

// lam < 0, NaN or >= 2^24: undefined (the loops still end)
__device__ float ra_poisson(float lam, uint64_t seed, unsigned row, uint64_t i) {
    if (lam == 0.f) return 0.f;
    if (lam < 10.f) {
        const float u = ra_u_co(ra_philox(seed, row, i, 0u).w0);
        float p = expf(-lam), s = p;
        int k = 0;
        while (u >= s && k < RA_INV_STEPS) {
            ++k;
            p = p * lam / (float)k;
            s += p;
        }
        return (float)k;
    }
    const float slam = sqrtf(lam), loglam = logf(lam);
    const float b = 0.931f + 2.53f * slam;
    const float a = -0.059f + 0.02483f * b;
    const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f);
    const float vr = 0.9277f - 3.6224f / (b - 2.f);
    for (unsigned r = 0; r < RA_PTRS_ROUNDS; ++r) {
        const RaWords w = ra_philox(seed, row, i, r);
        const float U = ra_u_co(w.w0) - 0.5f, V = ra_u_oc(w.w1);
        const float us = 0.5f - fabsf(U);
        const float k = floorf((2.f * a / us + b) * U + lam + 0.43f);
        if (us >= 0.07f && V <= vr) return k;
        if (k < 0.f || (us < 0.013f && V > us)) continue;
        if (logf(V) + logf(inv_alpha) - logf(a / (us * us) + b) <= -lam + k * loglam - lgammaf(k + 1.f)) return k;
    }
    return rintf(lam);
}

__global__ __launch_bounds__(256) void k_ra_words(unsigned* __restrict__ out, uint64_t seed, unsigned row, uint64_t i0,
                                                  unsigned round, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const RaWords w = ra_philox(seed, row, i0 + (uint64_t)t, round);
        out[4 * t + 0] = w.w0;
        out[4 * t + 1] = w.w1;
        out[4 * t + 2] = w.w2;
        out[4 * t + 3] = w.w3;
    }
}

extern "C" int tem_rawaug_philox_words(uint32_t* out, uint64_t seed, uint32_t row, uint64_t i0, uint32_t round, int64_t n,
                                       tem_stream_t stream) {
    TEM_REQUIRE(out && n > 0, "tem_rawaug_philox_words: bad arguments");
    hipLaunchKernelGGL(k_ra_words, dim3(tem_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, out, seed, row, i0, round, n);
    TEM_CHECK_LAUNCH("tem_rawaug_philox_words");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// elementwise noise
// ---------------------------------------------------------------------------
enum { RA_GAUSS = 0, RA_POISSON_ADD = 1, RA_POISSON_SCALED = 2 };

static inline int ra_blocks(int64_t L, int N) {   // workgroups per row: the launch shape of rawnorm.hip
    int64_t cap = 2048 / N;
    if (cap < 8) cap = 8;
    const int64_t b = tem_cdiv(L, 1024);
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

__device__ __forceinline__ float ra_clip(float v, float lo, float hi) {
    v = v > lo ? v : lo;
    return v < hi ? v : hi;
}

// GAUSS: y = x + p[n] * z;  POISSON_ADD: y = x + k / p[n], k ~ Poisson(p[n]);
// POISSON_SCALED: y = k / q[n] + p[n], k ~ Poisson((x - p[n]) * q[n]);  row0: the stream's row of the first data row
template <int OP, bool CLIP>
__global__ __launch_bounds__(256) void k_ra_noise(const float* __restrict__ x, float* __restrict__ y, int64_t L,
                                                  const float* __restrict__ p, const float* __restrict__ q, uint64_t seed,
                                                  unsigned row0, float lo, float hi) {
    const int n = blockIdx.y;
    const unsigned srow = row0 + (unsigned)n;
    const float* row = x + (int64_t)n * L;
    float* out = y + (int64_t)n * L;
    const float c0 = p[n], c1 = OP == RA_POISSON_SCALED ? q[n] : 0.f;
    auto f = [&](int64_t i, float v) {
        float r;
        if (OP == RA_GAUSS) r = c0 == 0.f ? v : v + c0 * ra_normal(seed, srow, (uint64_t)i);
        else if (OP == RA_POISSON_ADD) r = v + ra_poisson(c0, seed, srow, (uint64_t)i) / c0;
        else r = ra_poisson((v - c0) * c1, seed, srow, (uint64_t)i) / c1 + c0;
        return CLIP ? ra_clip(r, lo, hi) : r;
    };
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > L) head = L;
    const int64_t nv = (L - head) >> 2;
    const float4* __restrict__ v = (const float4*)(row + head);
    const bool vec_out = (((uintptr_t)(out + head)) & 15u) == 0;   // wave-uniform: y may sit at another offset mod 16 than x
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const float4 a = v[i];
        const int64_t e = head + 4 * i;
        const float4 r = make_float4(f(e, a.x), f(e + 1, a.y), f(e + 2, a.z), f(e + 3, a.w));
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
        if (t < head) out[t] = f((int64_t)t, row[t]);
        else if (t >= 64 && tail0 + (t - 64) < L) out[tail0 + (t - 64)] = f(tail0 + (t - 64), row[tail0 + (t - 64)]);
    }
}

template <int OP>
static int ra_launch_noise(const char* name, const float* x, float* y, int N, int64_t L, const float* p, const float* q,
                           uint64_t seed, uint32_t row0, int clip, float lo, float hi, tem_stream_t stream) {
    const dim3 grid(ra_blocks(L, N), N);
    if (clip)
        hipLaunchKernelGGL((k_ra_noise<OP, true>), grid, dim3(256), 0, (hipStream_t)stream, x, y, L, p, q, seed, row0, lo, hi);
    else
        hipLaunchKernelGGL((k_ra_noise<OP, false>), grid, dim3(256), 0, (hipStream_t)stream, x, y, L, p, q, seed, row0, lo, hi);
    TEM_CHECK_LAUNCH(name);
    return TEM_OK;
}

#define RA_ROWS_OK(N, L, row0) ((N) > 0 && (N) <= 65535 && (L) > 0 && (uint64_t)(row0) + (uint64_t)(N) <= 0x100000000ull)

extern "C" int tem_rawaug_gauss_noise(const float* x, float* y, int N, int64_t L, const float* std, uint64_t seed, uint32_t row0,
                                      int clip, float lo, float hi, tem_stream_t stream) {
    TEM_REQUIRE(x && y && std && RA_ROWS_OK(N, L, row0), "tem_rawaug_gauss_noise: bad arguments");
    return ra_launch_noise<RA_GAUSS>("tem_rawaug_gauss_noise", x, y, N, L, std, std, seed, row0, clip, lo, hi, stream);
}

extern "C" int tem_rawaug_poisson_add(const float* x, float* y, int N, int64_t L, const float* lam, uint64_t seed, uint32_t row0,
                                      int clip, float lo, float hi, tem_stream_t stream) {
    TEM_REQUIRE(x && y && lam && RA_ROWS_OK(N, L, row0), "tem_rawaug_poisson_add: bad arguments");
    return ra_launch_noise<RA_POISSON_ADD>("tem_rawaug_poisson_add", x, y, N, L, lam, lam, seed, row0, clip, lo, hi, stream);
}

extern "C" int tem_rawaug_poisson_scaled(const float* x, float* y, int N, int64_t L, const float* offset, const float* mult,
                                         uint64_t seed, uint32_t row0, int clip, float lo, float hi, tem_stream_t stream) {
    TEM_REQUIRE(x && y && offset && mult && RA_ROWS_OK(N, L, row0), "tem_rawaug_poisson_scaled: bad arguments");
    return ra_launch_noise<RA_POISSON_SCALED>("tem_rawaug_poisson_scaled", x, y, N, L, offset, mult, seed, row0, clip, lo, hi,
                                              stream);
}

// ---------------------------------------------------------------------------
// separable blur of the last two axes
// ---------------------------------------------------------------------------
#define RA_KMAX 63
#define RA_TH 32

__device__ __forceinline__ int ra_reflect(int i, int n) {   // -j -> j, n-1+j -> n-1-j; beyond the halo (never summed): clamped
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// grid (tiles in x, tiles in y, planes); LDS: in[(TH + 2 ry)][TW + 2 rx], then (16-byte aligned) mid[(TH + 2 ry)][TW]
template <int TW>
__global__ __launch_bounds__(256) void k_ra_blur2d(const float* __restrict__ x, float* __restrict__ y, int64_t P, int H, int W,
                                                   const float* __restrict__ wy, const float* __restrict__ wx, int ky, int kx) {
    extern __shared__ float4 ra_lds4[];
    float* lds = (float*)ra_lds4;
    const int ry = ky >> 1, rx = kx >> 1;
    const int IH = RA_TH + 2 * ry, IW = TW + 2 * rx;
    float* in = lds;
    float* mid = lds + ((IH * IW + 3) & ~3);
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * RA_TH;
    const int t = threadIdx.x;
    for (int64_t pl = blockIdx.z; pl < P; pl += gridDim.z) {
        const float* src = x + pl * (int64_t)H * W;
        float* dst = y + pl * (int64_t)H * W;
        for (int e = t; e < IH * IW; e += 256) {
            const int yy = e / IW, xx = e - yy * IW;
            in[e] = src[(int64_t)ra_reflect(y0 - ry + yy, H) * W + ra_reflect(x0 - rx + xx, W)];
        }
        __syncthreads();
        for (int e = t; e < IH * TW; e += 256) {
            const int yy = e / TW, xx = e % TW;
            const float* r = in + yy * IW + xx;
            float acc = 0.f;
            for (int j = 0; j < kx; ++j) acc = __builtin_fmaf(wx[j], r[j], acc);
            mid[e] = acc;
        }
        __syncthreads();
        for (int e = t; e < RA_TH * (TW / 4); e += 256) {
            const int oy = e / (TW / 4), ox = 4 * (e % (TW / 4));
            const int gy = y0 + oy, gx = x0 + ox;
            if (gy >= H || gx >= W) continue;
            const float4* m = (const float4*)(mid + oy * TW + ox);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < ky; ++j) {
                const float4 v = m[j * (TW / 4)];
                const float w = wy[j];
                acc.x = __builtin_fmaf(w, v.x, acc.x);
                acc.y = __builtin_fmaf(w, v.y, acc.y);
                acc.z = __builtin_fmaf(w, v.z, acc.z);
                acc.w = __builtin_fmaf(w, v.w, acc.w);
            }
            float* o = dst + (int64_t)gy * W + gx;
            if (gx + 3 < W && (((uintptr_t)o) & 15u) == 0) {
                *(float4*)o = acc;
            } else {
                o[0] = acc.x;
                if (gx + 1 < W) o[1] = acc.y;
                if (gx + 2 < W) o[2] = acc.z;
                if (gx + 3 < W) o[3] = acc.w;
            }
        }
        __syncthreads();   // the next plane overwrites both buffers
    }
}

extern "C" int tem_rawaug_blur2d(const float* x, float* y, int64_t P, int H, int W, const float* wy, const float* wx, int ky,
                                 int kx, tem_stream_t stream) {
    TEM_REQUIRE(x && y && wy && wx && x != y && P > 0 && H > 0 && W > 0, "tem_rawaug_blur2d: bad arguments (x and y must differ)");
    TEM_REQUIRE(ky >= 1 && ky <= RA_KMAX && (ky & 1) && kx >= 1 && kx <= RA_KMAX && (kx & 1),
                "tem_rawaug_blur2d: tap counts must be odd and within 1..%d (got %d, %d)", RA_KMAX, ky, kx);
    TEM_REQUIRE(ky / 2 < H && kx / 2 < W,
                "tem_rawaug_blur2d: the reflect border needs k/2 < size on each axis (taps %d x %d on a %d x %d plane)", ky, kx, H, W);
    const int ry = ky / 2, rx = kx / 2;
    const bool wide = rx <= 15 && ry <= 15;   // 64-wide tiles while both buffers stay under 40 KiB of LDS
    const int TW = wide ? 64 : 32;
    const int IH = RA_TH + 2 * ry, IW = TW + 2 * rx;
    const size_t lds = ((size_t)((IH * IW + 3) & ~3) + (size_t)IH * TW) * sizeof(float);
    const dim3 grid((unsigned)tem_cdiv(W, TW), (unsigned)tem_cdiv(H, RA_TH), (unsigned)(P < 65535 ? P : 65535));
    TEM_REQUIRE(grid.y <= 65535, "tem_rawaug_blur2d: at most %d rows per plane", 65535 * RA_TH);
    if (wide)
        hipLaunchKernelGGL(k_ra_blur2d<64>, grid, dim3(256), lds, (hipStream_t)stream, x, y, P, H, W, wy, wx, ky, kx);
    else
        hipLaunchKernelGGL(k_ra_blur2d<32>, grid, dim3(256), lds, (hipStream_t)stream, x, y, P, H, W, wy, wx, ky, kx);
    TEM_CHECK_LAUNCH("tem_rawaug_blur2d");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// the third pass of a separable blur: taps along z, streaming along the H*W plane
// ---------------------------------------------------------------------------
// grid-stride over groups of VEC consecutive elements of a plane (VEC = 4: planes of a multiple of 4 elements at 16-byte
// aligned bases); one accumulation chain per output, taps in ascending order
template <int VEC>
__global__ __launch_bounds__(256) void k_ra_blur_z(const float* __restrict__ x, float* __restrict__ y, int64_t P, int D, int64_t HW,
                                                   const float* __restrict__ wz, int kz) {
    const int rz = kz >> 1;
    const int64_t per = HW / VEC, total = P * D * per;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = (e % per) * VEC, pz = e / per;
        const int z = (int)(pz % D);
        const float* src = x + (pz - z) * HW + i;
        float acc[VEC];
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[c] = 0.f;
        for (int j = 0; j < kz; ++j) {
            const float* s = src + (int64_t)ra_reflect(z - rz + j, D) * HW;
            const float w = wz[j];
            if (VEC == 4) {
                const float4 v = *(const float4*)s;
                acc[0] = __builtin_fmaf(w, v.x, acc[0]);
                acc[1] = __builtin_fmaf(w, v.y, acc[1]);
                acc[2] = __builtin_fmaf(w, v.z, acc[2]);
                acc[3] = __builtin_fmaf(w, v.w, acc[3]);
            } else {
                acc[0] = __builtin_fmaf(w, s[0], acc[0]);
            }
        }
        float* o = y + pz * HW + i;
        if (VEC == 4)
            *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            o[0] = acc[0];
    }
}

extern "C" int tem_rawaug_blur_z(const float* x, float* y, int64_t P, int D, int64_t HW, const float* wz, int kz,
                                 tem_stream_t stream) {
    TEM_REQUIRE(x && y && wz && x != y && P > 0 && D > 0 && HW > 0, "tem_rawaug_blur_z: bad arguments (x and y must differ)");
    TEM_REQUIRE(kz >= 1 && kz <= RA_KMAX && (kz & 1), "tem_rawaug_blur_z: the tap count must be odd and within 1..%d (got %d)",
                RA_KMAX, kz);
    TEM_REQUIRE(kz / 2 < D, "tem_rawaug_blur_z: the reflect border needs k/2 < size (%d taps on %d planes)", kz, D);
    const bool vec = HW % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0;
    const int64_t groups = P * D * (vec ? HW / 4 : HW);
    if (vec)
        hipLaunchKernelGGL(k_ra_blur_z<4>, dim3(tem_grid_1d(groups, 256)), dim3(256), 0, (hipStream_t)stream, x, y, P, D, HW, wz, kz);
    else
        hipLaunchKernelGGL(k_ra_blur_z<1>, dim3(tem_grid_1d(groups, 256)), dim3(256), 0, (hipStream_t)stream, x, y, P, D, HW, wz, kz);
    TEM_CHECK_LAUNCH("tem_rawaug_blur_z");
    return TEM_OK;
}
