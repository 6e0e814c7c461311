// filters.hip -- the Gaussian 2-jet feature bank of Shallow2Deep inference (DESIGN.md "Shallow2Deep front end").
//
// At one scale every filter of the bank is a pointwise function of the 2-jet J_o = gaussian_filter(x, sigma, order = o,
// mode = "mirror", truncate = 4), |o| <= 2: smoothing J_0, the Laplacian sum_a J_2a, the gradient magnitude, the Hessian's
// eigenvalues and -- through a second chain at outer_sigma over the products of the gradient -- the structure tensor's.  The
// jet is computed ONCE per scale and never stored:
//   x pass   1 volume -> 3 (orders 0, 1, 2 along x from one staged line)
//   y pass   3 -> 6     (x0: y0 y1 y2, x1: y0 y1, x2: y0)                       the 6 jets of a 2-D sample
//   z pass   6 -> 10    (streamed along the plane, as tem_rawaug_blur_z does)   the 10 jets of a volume
// and the LAST pass (y in 2-D, z in 3-D) ends in an epilogue that turns the jets in registers into the requested channels of
// the caller's bank [N][F][D][H][W] and, when a structure tensor is asked for, into the gradient products in the workspace.
// The second chain smooths the 3 (2-D) or 6 (3-D) products with order 0 only and ends in the eigenvalue epilogue.
//   k_flt_xy    x and y fused over one 32 x 32 output tile: the tile with its halo in LDS (odd pitch), the x pass into a second
//               LDS array [orders][rows][32], the y pass from there into registers (4 outputs a thread).  Taken while both
//               arrays fit 64 KiB: radii up to 27 at equal ry, rx (every default scale; sigma 5 has radius 20).
//   k_flt_line  the x pass alone (one row segment of 256 outputs in LDS), for the radii beyond that, followed by
//   k_flt_axis  a pass along a strided axis: thread = (column, 8 consecutive outputs), it walks the 8 + 2r inputs once, loads
//               coalesced over the contiguous axis; the y pass after k_flt_line and the z pass of every volume.
// Borders: the whole-sample mirror extension (period 2(n - 1)) folded by index arithmetic where a value is staged or loaded,
// so a radius beyond the axis is correct.  Weights: float32 [axis z, y, x][order][TEM_FILTERS_MAX_TAPS], made on the host in
// float64, in correlation order; a tap index is wave-uniform, so the weights arrive through the constant cache.
// Eigenvalues are computed in float64 registers (2 x 2: mean +- root; 3 x 3: the trigonometric form on the deviator, whose
// loss of half the digits where eigenvalues meet then costs 2^-26 of the matrix norm, below a float32 unit), then sorted, so
// they are finite and descending on every degenerate matrix.  Every store is a plain vector store.
#include "tem_common.h"

#define FLT_TAPS TEM_FILTERS_MAX_TAPS
#define FLT_R TEM_FILTERS_MAX_RADIUS
#define FLT_T 32               // outputs of k_flt_xy a side
#define FLT_SEG 8              // outputs of k_flt_axis a thread
#define FLT_LINE 256           // outputs of k_flt_line a block
#define FLT_LDS_FLOATS 16384   // 64 KiB

struct FltGeom {
    int N, D, H, W;
};
// where the epilogue writes: channel indices of the bank (-1: not asked for); hess and st are the first of ndim channels
struct FltOut {
    float* bank;
    int64_t sample_stride;   // F * D * H * W
    int smooth, log, ggm, hess, st;
    float* prod;             // [N][3 or 6][V] gradient products (NULL: not asked for)
};

__device__ __forceinline__ int flt_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    i += i < 0 ? p : 0;
    return i < n ? i : p - i;
}

__device__ __forceinline__ void flt_sort3(double& a, double& b, double& c) {   // descending
    double t;
    if (a < b) t = a, a = b, b = t;
    if (b < c) t = b, b = c, c = t;
    if (a < b) t = a, a = b, b = t;
}

// the eigenvalues of [[a, b], [b, c]], descending
__device__ __forceinline__ void flt_eig2(float a, float b, float c, float* e) {
    const double m = 0.5 * ((double)a + (double)c), d = 0.5 * ((double)a - (double)c);
    const double r = __builtin_sqrt(d * d + (double)b * (double)b);
    e[0] = (float)(m + r);
    e[1] = (float)(m - r);
}

// the eigenvalues of the symmetric [[zz, zy, zx], [zy, yy, yx], [zx, yx, xx]], descending
__device__ __forceinline__ void flt_eig3(float zz, float zy, float zx, float yy, float yx, float xx, float* e) {
    const double a00 = zz, a01 = zy, a02 = zx, a11 = yy, a12 = yx, a22 = xx;
    const double q = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (a01 * a01 + a02 * a02 + a12 * a12);
    double e0 = q, e1 = q, e2 = q;
    if (p2 > 0.0) {
        const double p = __builtin_sqrt(p2 / 6.0);
        const double det = b00 * (b11 * b22 - a12 * a12) - a01 * (a01 * b22 - a12 * a02) + a02 * (a01 * a12 - b11 * a02);
        double r = det / (2.0 * p * p * p);
        r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        r = r == r ? r : 0.0;   // p^3 underflowed: the deviator is below float32's reach
        const double phi = acos(r) / 3.0;
        e0 = q + 2.0 * p * cos(phi);
        e2 = q + 2.0 * p * cos(phi + 2.0943951023931954923);
        e1 = 3.0 * q - e0 - e2;
        flt_sort3(e0, e1, e2);
    }
    e[0] = (float)e0, e[1] = (float)e1, e[2] = (float)e2;
}

// the jets of one voxel -> the channels asked for.  ND == 2: J = [00, y, yy, x, yx, xx]; ND == 3: J = [000, z, zz, y, zy, yy,
// x, zx, yx, xx].  at: n * sample_stride + voxel; pat: n * NP * V + voxel (NP = 3 or 6 products)
template <int ND>
__device__ __forceinline__ void flt_emit_jet(const float* J, const FltOut& o, int64_t at, int64_t pat, int64_t V) {
    float gz = 0.f, gy, gx, hzz = 0.f, hzy = 0.f, hzx = 0.f, hyy, hyx, hxx;
    if (ND == 2) gy = J[1], gx = J[3], hyy = J[2], hyx = J[4], hxx = J[5];
    else gz = J[1], gy = J[3], gx = J[6], hzz = J[2], hzy = J[4], hyy = J[5], hzx = J[7], hyx = J[8], hxx = J[9];
    if (o.smooth >= 0) o.bank[at + o.smooth * V] = J[0];
    if (o.log >= 0) o.bank[at + o.log * V] = ND == 2 ? hyy + hxx : (hzz + hyy) + hxx;
    if (o.ggm >= 0) o.bank[at + o.ggm * V] = __builtin_sqrtf(ND == 2 ? gy * gy + gx * gx : gz * gz + gy * gy + gx * gx);
    if (o.hess >= 0) {
        float e[3];
        if (ND == 2) flt_eig2(hyy, hyx, hxx, e);
        else flt_eig3(hzz, hzy, hzx, hyy, hyx, hxx, e);
#pragma unroll
        for (int k = 0; k < ND; ++k) o.bank[at + (o.hess + k) * V] = e[k];
    }
    if (o.prod) {
        float* p = o.prod + pat;
        if (ND == 2) p[0] = gy * gy, p[V] = gy * gx, p[2 * V] = gx * gx;
        else p[0] = gz * gz, p[V] = gz * gy, p[2 * V] = gz * gx, p[3 * V] = gy * gy, p[4 * V] = gy * gx, p[5 * V] = gx * gx;
    }
}

// the smoothed products of one voxel (ND == 2: yy, yx, xx; ND == 3: zz, zy, zx, yy, yx, xx) -> the tensor's eigenvalues
template <int ND>
__device__ __forceinline__ void flt_emit_tensor(const float* T, const FltOut& o, int64_t at, int64_t V) {
    float e[3];
    if (ND == 2) flt_eig2(T[0], T[1], T[2], e);
    else flt_eig3(T[0], T[1], T[2], T[3], T[4], T[5], e);
#pragma unroll
    for (int k = 0; k < ND; ++k) o.bank[at + (o.st + k) * V] = e[k];
}

// ---------------------------------------------------------------------------------------------------------------
// x and y fused.  JET: src [N][1][V] -> the 6 xy jets; else src [N][nin][V] -> nin volumes smoothed in x and y.
// last (a 2-D sample): the epilogue instead of the store to dst [N][6 or nin][V].  grid (tiles, planes), LDS dynamic.
// ---------------------------------------------------------------------------------------------------------------
template <bool JET>
__global__ __launch_bounds__(256) void k_flt_xy(const float* __restrict__ src, int nin, float* __restrict__ dst, const float* __restrict__ w,
                                                FltGeom g, int ry, int rx, FltOut o, int last) {
    extern __shared__ float flt_lds[];
    constexpr int NO = JET ? 3 : 1, CMAX = JET ? 1 : 6;
    const int Ry = FLT_T + 2 * ry, Rx = FLT_T + 2 * rx, pitch = Rx | 1;
    float* tile = flt_lds;
    float* xo = flt_lds + Ry * pitch;   // [NO][Ry][FLT_T]
    const float* wy = w + 3 * FLT_TAPS;
    const float* wx = w + 6 * FLT_TAPS;
    const int ntx = (g.W + FLT_T - 1) / FLT_T;
    const int x0 = (blockIdx.x % ntx) * FLT_T, y0 = (blockIdx.x / ntx) * FLT_T;
    const int64_t HW = (int64_t)g.H * g.W, V = HW * g.D;
    const int tid = threadIdx.x, col = tid & 31, rg = tid >> 5;
    const int K = JET ? 6 : nin;
    for (int plane = blockIdx.y; plane < g.N * g.D; plane += gridDim.y) {
        const int n = plane / g.D, z = plane - n * g.D;
        float jet[4][6];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 6; ++j) jet[q][j] = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < nin) {
                const float* sp = src + ((int64_t)(n * nin + c) * g.D + z) * HW;
                __syncthreads();   // the arrays are free again
                for (int e = tid; e < Ry * Rx; e += 256) {
                    const int ty = e / Rx, tx = e - ty * Rx;
                    tile[ty * pitch + tx] = sp[(int64_t)flt_mirror(y0 - ry + ty, g.H) * g.W + flt_mirror(x0 - rx + tx, g.W)];
                }
                __syncthreads();
                // x: item = (row, column g8 and the three columns 8, 16, 24 further on)
                for (int e = tid; e < Ry * 8; e += 256) {
                    const int row = e >> 3, g8 = e & 7;
                    const float* t = tile + row * pitch + g8;
                    float a[NO][4];
#pragma unroll
                    for (int k = 0; k < NO; ++k)
#pragma unroll
                        for (int q = 0; q < 4; ++q) a[k][q] = 0.f;
                    for (int tap = 0; tap <= 2 * rx; ++tap) {
                        float wk[NO];
#pragma unroll
                        for (int k = 0; k < NO; ++k) wk[k] = wx[k * FLT_TAPS + tap];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float v = t[tap + 8 * q];
#pragma unroll
                            for (int k = 0; k < NO; ++k) a[k][q] = __builtin_fmaf(wk[k], v, a[k][q]);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NO; ++k)
#pragma unroll
                        for (int q = 0; q < 4; ++q) xo[(k * Ry + row) * FLT_T + g8 + 8 * q] = a[k][q];
                }
                __syncthreads();
                // y: thread = (column, rows rg, rg + 8, rg + 16, rg + 24)
                for (int tap = 0; tap <= 2 * ry; ++tap) {
                    const float w0 = wy[tap];
                    if (JET) {
                        const float w1 = wy[FLT_TAPS + tap], w2 = wy[2 * FLT_TAPS + tap];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int r = rg + 8 * q + tap;
                            const float v0 = xo[r * FLT_T + col], v1 = xo[(Ry + r) * FLT_T + col], v2 = xo[(2 * Ry + r) * FLT_T + col];
                            jet[q][0] = __builtin_fmaf(w0, v0, jet[q][0]);
                            jet[q][1] = __builtin_fmaf(w1, v0, jet[q][1]);
                            jet[q][2] = __builtin_fmaf(w2, v0, jet[q][2]);
                            jet[q][3] = __builtin_fmaf(w0, v1, jet[q][3]);
                            jet[q][4] = __builtin_fmaf(w1, v1, jet[q][4]);
                            jet[q][5] = __builtin_fmaf(w0, v2, jet[q][5]);
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) jet[q][c] = __builtin_fmaf(w0, xo[(rg + 8 * q + tap) * FLT_T + col], jet[q][c]);
                    }
                }
            }
        }
        const int x = x0 + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = y0 + rg + 8 * q;
            if (x < g.W && y < g.H) {
                const int64_t v = (int64_t)z * HW + (int64_t)y * g.W + x;
                if (last) {
                    if (JET) flt_emit_jet<2>(jet[q], o, n * o.sample_stride + v, (int64_t)n * 3 * V + v, V);
                    else flt_emit_tensor<2>(jet[q], o, n * o.sample_stride + v, V);
                } else {
#pragma unroll
                    for (int j = 0; j < 6; ++j)
                        if (j < K) dst[((int64_t)n * K + j) * V + v] = jet[q][j];
                }
            }
        }
    }
}

// the x pass of the jet alone (the tensor's chain has one order an axis and always fits k_flt_xy): src [N][1][V] -> dst
// [N][3][V].  grid (segments, rows)
__global__ __launch_bounds__(FLT_LINE) void k_flt_line(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ w,
                                                       FltGeom g, int rx) {
    __shared__ float line[FLT_LINE + 2 * FLT_R];
    constexpr int NO = 3;
    const float* wx = w + 6 * FLT_TAPS;
    const int x0 = blockIdx.x * FLT_LINE, tid = threadIdx.x;
    const int64_t rows = (int64_t)g.N * g.D * g.H, per = (int64_t)g.D * g.H, V = per * g.W;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const float* sp = src + row * g.W;
        __syncthreads();
        for (int e = tid; e < FLT_LINE + 2 * rx; e += FLT_LINE) line[e] = sp[flt_mirror(x0 - rx + e, g.W)];
        __syncthreads();
        float a[NO];
#pragma unroll
        for (int k = 0; k < NO; ++k) a[k] = 0.f;
        for (int tap = 0; tap <= 2 * rx; ++tap) {
            const float v = line[tid + tap];
#pragma unroll
            for (int k = 0; k < NO; ++k) a[k] = __builtin_fmaf(wx[k * FLT_TAPS + tap], v, a[k]);
        }
        if (x0 + tid < g.W) {
            const int64_t n = row / per, rem = row - n * per;
#pragma unroll
            for (int k = 0; k < NO; ++k) dst[(n * 3 + k) * V + rem * g.W + x0 + tid] = a[k];
        }
    }
}

// A pass along a strided axis of length L (element stride `inner`; `slabs` blocks of L * inner elements a volume: the y pass
// has slabs = D, inner = W, the z pass slabs = 1, inner = H * W).  KIND 0: the y pass of the jet, 3 volumes -> 6; KIND 1: its
// z pass, 6 -> 10; KIND 2: order 0 of nin <= 6 volumes.  last: the epilogue (ND = 2 after a y pass, 3 after a z pass) instead of
// the store to dst.  item = (n, slab, segment of FLT_SEG outputs, position in the slab's line), the position fastest.
template <int KIND> struct FltKind;
template <> struct FltKind<0> { static constexpr int NIN = 3, NOUT = 6; static constexpr int no(int c) { return 3 - c; } };
template <> struct FltKind<1> { static constexpr int NIN = 6, NOUT = 10; static constexpr int no(int c) { return c == 0 ? 3 : (c == 1 || c == 3 ? 2 : 1); } };
template <> struct FltKind<2> { static constexpr int NIN = 6, NOUT = 6; static constexpr int no(int) { return 1; } };

template <int KIND>
__global__ __launch_bounds__(256) void k_flt_axis(const float* __restrict__ src, int nin, float* __restrict__ dst, const float* __restrict__ wa,
                                                  int r, int N, int slabs, int L, int64_t inner, FltOut o, int last) {
    using Kd = FltKind<KIND>;
    constexpr int NIN = Kd::NIN, NOUT = Kd::NOUT;
    const int nseg = (L + FLT_SEG - 1) / FLT_SEG;
    const int64_t V = (int64_t)slabs * L * inner;
    const int64_t items = (int64_t)N * slabs * nseg * inner;
    const int nout = KIND == 2 ? nin : NOUT;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t p = it % inner, rest = it / inner;
        const int seg = (int)(rest % nseg);
        const int64_t ns = rest / nseg;
        const int64_t n = ns / slabs, slab = ns - n * slabs;
        const int64_t off = slab * L * inner + p;   // of the line's first element in its volume
        const float* sp = src + n * nin * V + off;
        const int l0 = seg * FLT_SEG;
        float acc[FLT_SEG][NOUT];
#pragma unroll
        for (int k = 0; k < FLT_SEG; ++k)
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[k][j] = 0.f;
        for (int i = 0; i < FLT_SEG + 2 * r; ++i) {
            const int64_t at = (int64_t)flt_mirror(l0 - r + i, L) * inner;
            float v[NIN];
#pragma unroll
            for (int c = 0; c < NIN; ++c) v[c] = c < nin ? sp[c * V + at] : 0.f;
#pragma unroll
            for (int k = 0; k < FLT_SEG; ++k) {
                const int tap = i - k;
                if (tap >= 0 && tap <= 2 * r) {
                    const float wk[3] = {wa[tap], KIND == 2 ? 0.f : wa[FLT_TAPS + tap], KIND == 2 ? 0.f : wa[2 * FLT_TAPS + tap]};
                    int j = 0;
#pragma unroll
                    for (int c = 0; c < NIN; ++c)
#pragma unroll
                        for (int oo = 0; oo < Kd::no(c); ++oo, ++j) acc[k][j] = __builtin_fmaf(wk[oo], v[c], acc[k][j]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FLT_SEG; ++k) {
            if (l0 + k < L) {
                const int64_t vox = off + (int64_t)(l0 + k) * inner;
                if (!last) {
#pragma unroll
                    for (int j = 0; j < NOUT; ++j)
                        if (j < nout) dst[(n * nout + j) * V + vox] = acc[k][j];
                } else if constexpr (KIND == 0) {
                    flt_emit_jet<2>(acc[k], o, n * o.sample_stride + vox, n * 3 * V + vox, V);
                } else if constexpr (KIND == 1) {
                    flt_emit_jet<3>(acc[k], o, n * o.sample_stride + vox, n * 6 * V + vox, V);
                } else if (nin == 3) {
                    flt_emit_tensor<2>(acc[k], o, n * o.sample_stride + vox, V);
                } else {
                    flt_emit_tensor<3>(acc[k], o, n * o.sample_stride + vox, V);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
static int64_t flt_xy_floats(int ry, int rx, bool jet) {
    const int64_t Ry = FLT_T + 2 * ry, Rx = FLT_T + 2 * rx;
    return Ry * (Rx | 1) + (jet ? 3 : 1) * Ry * FLT_T;
}

extern "C" int tem_filters_fused(int ry, int rx, int jet) {
    if (ry < 0 || rx < 0 || ry > FLT_R || rx > FLT_R) return -1;
    return flt_xy_floats(ry, rx, jet != 0) <= FLT_LDS_FLOATS ? 1 : 0;
}

extern "C" int64_t tem_filters_ws(int N, int D, int H, int W) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)3 * (D > 1 ? 6 : 3) * N * D * H * W * (int64_t)sizeof(float);
}

// one chain: src (1 volume a sample for the jet, nin for the tensor) through x, y and, in a volume, z into the epilogue;
// A, B: scratch of 6 (2-D: 3) volumes a sample each
template <bool JET>
static void flt_chain(const float* src, int nin, const float* w, const int* r, float* A, float* B, const FltGeom& g, const FltOut& o,
                      hipStream_t st) {
    const bool vol = g.D > 1;
    const int rz = r[0], ry = r[1], rx = r[2];
    const int64_t HW = (int64_t)g.H * g.W;
    const int64_t planes = (int64_t)g.N * g.D;
    if (flt_xy_floats(ry, rx, JET) <= FLT_LDS_FLOATS) {
        const dim3 grid((unsigned)(tem_cdiv(g.W, FLT_T) * tem_cdiv(g.H, FLT_T)), (unsigned)(planes > 65535 ? 65535 : planes));
        hipLaunchKernelGGL(k_flt_xy<JET>, grid, dim3(256), (size_t)flt_xy_floats(ry, rx, JET) * sizeof(float), st, src, nin, A, w, g, ry, rx, o,
                           vol ? 0 : 1);
    } else if constexpr (JET) {   // flt_xy_floats(FLT_R, FLT_R, false) fits: the tensor's chain never comes here
        const int64_t rows = planes * g.H;
        hipLaunchKernelGGL(k_flt_line, dim3((unsigned)tem_cdiv(g.W, FLT_LINE), (unsigned)(rows > 65535 ? 65535 : rows)), dim3(FLT_LINE), 0, st,
                           src, B, w, g, rx);
        const int64_t items = planes * tem_cdiv(g.H, FLT_SEG) * g.W;
        hipLaunchKernelGGL(k_flt_axis<0>, dim3(tem_grid_1d(items, 256, 256 * 16)), dim3(256), 0, st, (const float*)B, 3, A, w + 3 * FLT_TAPS, ry,
                           g.N, g.D, g.H, (int64_t)g.W, o, vol ? 0 : 1);
    }
    static_assert((FLT_T + 2 * FLT_R) * ((FLT_T + 2 * FLT_R) | 1) + (FLT_T + 2 * FLT_R) * FLT_T <= FLT_LDS_FLOATS, "the tensor's tile fits LDS");
    if (vol) {
        const int64_t items = (int64_t)g.N * tem_cdiv(g.D, FLT_SEG) * HW;
        hipLaunchKernelGGL(k_flt_axis<JET ? 1 : 2>, dim3(tem_grid_1d(items, 256, 256 * 16)), dim3(256), 0, st, (const float*)A, JET ? 6 : nin,
                           (float*)nullptr, w, rz, g.N, 1, g.D, HW, o, 1);
    }
}

static int flt_radii(const char* who, const int* r, int D) {
    TEM_REQUIRE(r, "%s: null pointer", who);
    for (int a = 0; a < 3; ++a)
        TEM_REQUIRE(r[a] >= 0 && r[a] <= FLT_R, "%s: radius %d outside 0..%d (sigma too large: the radius is int(4 sigma + 0.5))", who, r[a], FLT_R);
    TEM_REQUIRE(D > 1 || r[0] == 0, "%s: a 2-D sample (D == 1) takes no z radius", who);
    return TEM_OK;
}

extern "C" int tem_filters_scale(const float* x, int N, int D, int H, int W, const float* weights, const int* radii,
                                 const float* outer_weights, const int* outer_radii, float* bank, int F, int ch_smooth, int ch_log,
                                 int ch_ggm, int ch_hess, int ch_st, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    const char* who = "tem_filters_scale";
    TEM_REQUIRE(x && weights && bank && ws, "%s: null pointer", who);
    TEM_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && F > 0, "%s: bad shape", who);
    TEM_REQUIRE((int64_t)D * H * W < INT32_MAX && (int64_t)N * D * H < INT32_MAX, "%s: D*H*W and N*D*H must stay below 2^31 - 1", who);
    TEM_REQUIRE(D == 1 || (H > 1 && W > 1), "%s: H and W of a volume must exceed 1 (a 2-D sample has D == 1)", who);
    TEM_TRY(flt_radii(who, radii, D));
    const int nd = D > 1 ? 3 : 2;
    const int chs[5] = {ch_smooth, ch_log, ch_ggm, ch_hess, ch_st};
    for (int k = 0; k < 5; ++k)
        TEM_REQUIRE(chs[k] == -1 || (chs[k] >= 0 && chs[k] + (k >= 3 ? nd : 1) <= F), "%s: channel %d leaves the bank of %d", who, chs[k], F);
    if (ch_st >= 0) {
        TEM_REQUIRE(outer_weights, "%s: the structure tensor needs the outer weights", who);
        TEM_TRY(flt_radii(who, outer_radii, D));
    }
    if (ws_bytes < tem_filters_ws(N, D, H, W)) {
        tem_set_error("%s: workspace too small (%lld bytes, %lld needed)", who, (long long)ws_bytes, (long long)tem_filters_ws(N, D, H, W));
        return TEM_EWS;
    }
    const int K = D > 1 ? 6 : 3;
    const int64_t NV = (int64_t)N * D * H * W;
    float* A = (float*)ws;
    float* B = A + K * NV;
    float* P = B + K * NV;
    FltGeom g{N, D, H, W};
    FltOut o{bank, (int64_t)F * D * H * W, ch_smooth, ch_log, ch_ggm, ch_hess, -1, ch_st >= 0 ? P : nullptr};
    hipStream_t st = (hipStream_t)stream;
    if (ch_smooth >= 0 || ch_log >= 0 || ch_ggm >= 0 || ch_hess >= 0 || ch_st >= 0) flt_chain<true>(x, 1, weights, radii, A, B, g, o, st);
    if (ch_st >= 0) {
        FltOut t{bank, o.sample_stride, -1, -1, -1, -1, ch_st, nullptr};
        flt_chain<false>(P, K, outer_weights, outer_radii, A, B, g, t, st);
    }
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}
