// peaks.hip -- peak_local_max on the device: a box maximum filter with the peak test folded into its last pass, the greedy
// minimum-spacing pass as parallel rounds over a dense state volume, a raster-order compaction of the kept peaks and the
// scatter of their ranks into a marker volume.  Everything compared is an integer or a float tested for equality: the result
// does not depend on the execution order.
//
// The contract (DESIGN.md "Peak maxima"): image_max = the maximum over the box of half-width d clamped to the sample; a voxel
// is a candidate when image == image_max, the sample is not constant, image > threshold (threshold_abs or the sample's
// minimum, raised to threshold_rel * maximum) and it is at least `border` away from both ends of every axis longer than 1.
// Candidates are taken by height descending, equal heights in raster order; one is kept unless an earlier kept one lies at
// dz^2 + dy^2 + dx^2 < d^2.  Two candidates that close are in each other's box, so they have EQUAL height: the pass only
// arbitrates inside plateaus, by raster order -- the lexicographically first maximal independent set of the conflict graph.
//
// The filter.  Every 1-D running maximum is pk_line16<B>: a thread produces 16 consecutive outputs of one line from the
// 16 + 2d inputs they cover, in blocks of B (the largest power of two <= 2d + 1, at most 16): a suffix maximum up to the
// block's last element, a prefix maximum behind it, one max of the two per output (van Herk / Gil-Werman with the block in
// registers).  2d + B reads per B outputs, whatever d; read-only on its input, so no barrier sits inside a pass.
//   k_pk_zmax  (D > 1 only) streams along planes: thread = (column, 16 planes), loads clamped in z, coalesced over the plane.
//   k_pk_xy    one 64 x 64 output tile with its halo of d (clamped to the plane: the "nearest" border) in LDS, odd pitch.
//              x: thread = (row, 16 columns), results held in registers over one barrier and written back in place; y:
//              thread = (column, 16 rows), each result goes straight into the peak test against the image: image_max is never
//              written.  It writes the state byte of every voxel and adds the tile's candidates to one counter.
// The spacing rounds (k_pk_round).  State: 0 none, 1 undecided, 2 kept, 3 rejected.  An undecided candidate is kept once
// every conflicting candidate of a lower linear index is rejected, rejected once one of them is kept; nothing else is ever
// written, so a state that is read is either undecided or final and any interleaving of reads and writes gives the
// sequential answer.  A workgroup owns a box of voxels, lists its undecided candidates in LDS and sweeps the list until a
// sweep decides nothing: a plateau inside one box costs one launch.  A wave takes a candidate; its lanes are the x offsets
// of the half ball (|dx| <= d - 1 <= 30), it walks the (dz, dy) rows: neighbours are a window read of the state volume.
// A launch returns at once when the one before it left nothing undecided; the host reads the head back once per batch.
#include <limits.h>

#include "tem_common.h"

#define PK_NONE 0
#define PK_OPEN 1
#define PK_KEPT 2
#define PK_REJ 3
#define PK_TILE 64             // outputs of k_pk_xy a side
#define PK_SEG 16              // outputs of pk_line16
#define PK_CHUNK 1024          // voxels of a compaction chunk: 256 threads x 4
#define PK_LIST 4096           // voxels of a box of k_pk_round
// the head of the workspace, in ints: [0] working rounds, [1] the last batch left candidates undecided, [2] candidates,
// [3] unused, [4 .. 4 + N) kept peaks per sample (valid once [1] is 0), then pending[0 .. TEM_PEAKS_MAX_BATCH], then the
// order-preserving keys of the per-sample minimum and maximum
#define PK_H_WORK 0
#define PK_H_ALIVE 1
#define PK_H_CAND 2
#define PK_H_KEPT 4
#define PK_H_PENDING(N) (PK_H_KEPT + (N))
#define PK_H_MM(N) (PK_H_PENDING(N) + TEM_PEAKS_MAX_BATCH + 1)
#define PK_H_INTS(N) (PK_H_MM(N) + 2 * (N))

struct PkTest {
    int has_abs, has_rel;
    float thr_abs, thr_rel;
    int bz, by, bx;   // the excluded border per axis (0 on an axis of size 1)
};

__device__ __forceinline__ int pk_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pk_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int pk_ldb(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pk_stb(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned pk_key(float f) {
    const unsigned b = __builtin_bit_cast(unsigned, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pk_unkey(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int pk_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// out[k] = max(ld(k) .. ld(k + w2)), k < 16; B <= w2 + 1 so that every window of a block holds the block's last element
template <int B, class L>
__device__ __forceinline__ void pk_line16(L ld, int w2, float (&out)[PK_SEG]) {
#pragma unroll
    for (int sb = 0; sb < PK_SEG; sb += B) {
        float suf[B];
        suf[B - 1] = ld(sb + B - 1);
#pragma unroll
        for (int k = B - 2; k >= 0; --k) suf[k] = __builtin_fmaxf(ld(sb + k), suf[k + 1]);
        float run = -__builtin_huge_valf();
        for (int q = sb + B; q <= sb + w2; ++q) run = __builtin_fmaxf(run, ld(q));
        out[sb] = __builtin_fmaxf(suf[0], run);
#pragma unroll
        for (int k = 1; k < B; ++k) {
            run = __builtin_fmaxf(run, ld(sb + k + w2));
            out[sb + k] = __builtin_fmaxf(suf[k], run);
        }
    }
}

__global__ __launch_bounds__(256) void k_pk_init(int* head, int N) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < PK_H_INTS(N); i += gridDim.x * 256) {
        const int m = i - PK_H_MM(N);
        head[i] = (m >= 0 && (m & 1) == 0) ? -1 : 0;   // minimum keys start at 0xffffffff, everything else at 0
    }
}

// grid (blocks, N): the sample's minimum and maximum as integer atomics on order-preserving keys (exact, any order); four
// independent loads a trip, one pair of atomics a block, spared when a plain read shows that it cannot change the word
__global__ __launch_bounds__(256) void k_pk_minmax(const float* __restrict__ img, int* head, int64_t V, int N) {
    const int n = blockIdx.y;
    const float* x = img + (int64_t)n * V;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    const int64_t span = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += 4 * span) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u * span < V ? x[i + u * span] : x[i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            mn = __builtin_fminf(mn, v[u]);
            mx = __builtin_fmaxf(mx, v[u]);
        }
    }
    mn = tem_wave_reduce(mn, [](float a, float b) { return __builtin_fminf(a, b); });
    mx = tem_wave_reduce(mx, [](float a, float b) { return __builtin_fmaxf(a, b); });
    __shared__ float part[2][4];
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = mn, part[1][threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = __builtin_fminf(__builtin_fminf(part[0][0], part[0][1]), __builtin_fminf(part[0][2], part[0][3]));
        mx = __builtin_fmaxf(__builtin_fmaxf(part[1][0], part[1][1]), __builtin_fmaxf(part[1][2], part[1][3]));
        unsigned* mm = (unsigned*)(head + PK_H_MM(N)) + 2 * n;
        if (pk_key(mn) < (unsigned)pk_ld((const int*)mm)) atomicMin(mm, pk_key(mn));
        if (pk_key(mx) > (unsigned)pk_ld((const int*)mm + 1)) atomicMax(mm + 1, pk_key(mx));
    }
}

// out[n][z][p] = max of img[n][z - d .. z + d][p], z clamped; item = (n, 16 planes, p), p fastest
template <int B>
__global__ __launch_bounds__(256) void k_pk_zmax(const float* __restrict__ img, float* __restrict__ out, int N, int D, int64_t HW, int d) {
    const int nseg = (D + PK_SEG - 1) / PK_SEG;
    const int64_t items = (int64_t)N * nseg * HW;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t p = it % HW, ns = it / HW;
        const int seg = (int)(ns % nseg);
        const int64_t base = (ns / nseg) * D * HW + p;
        const int z0 = seg * PK_SEG;
        float r[PK_SEG];
        pk_line16<B>([&](int i) { return img[base + (int64_t)pk_clamp(z0 + i - d, D - 1) * HW]; }, 2 * d, r);
#pragma unroll
        for (int k = 0; k < PK_SEG; ++k)
            if (z0 + k < D) out[base + (int64_t)(z0 + k) * HW] = r[k];
    }
}

// src: what the x and y maxima are taken of (the image, or its z maximum); img: what the result is compared with
template <int B>
__global__ __launch_bounds__(256) void k_pk_xy(const float* __restrict__ src, const float* __restrict__ img, uint8_t* __restrict__ state,
                                               int* head, int N, int D, int H, int W, int d, PkTest t) {
    extern __shared__ float pk_tile[];
    const int R = PK_TILE + 2 * d, pitch = R | 1;
    const int ntx = (W + PK_TILE - 1) / PK_TILE;
    const int x0 = (blockIdx.x % ntx) * PK_TILE, y0 = (blockIdx.x / ntx) * PK_TILE;
    const int64_t HW = (int64_t)H * W;
    const int tid = threadIdx.x;
    int found = 0;
    for (int plane = blockIdx.y; plane < N * D; plane += gridDim.y) {
        const int n = plane / D, z = plane - n * D;
        const float* sp = src + (int64_t)plane * HW;
        for (int e = tid; e < R * R; e += 256) {
            const int ty = e / R, tx = e - ty * R;
            pk_tile[ty * pitch + tx] = sp[(int64_t)pk_clamp(y0 - d + ty, H - 1) * W + pk_clamp(x0 - d + tx, W - 1)];
        }
        __syncthreads();
        // x: R rows x 4 segments, at most 504 items: two trips, the results kept in registers over the barrier
        float rx[2][PK_SEG];
#pragma unroll
        for (int trip = 0; trip < 2; ++trip) {
            const int item = tid + trip * 256;
            if (item < R * 4) {
                const int seg = item / R, row = item - seg * R;
                const float* a = pk_tile + row * pitch + seg * PK_SEG;
                pk_line16<B>([&](int i) { return a[i]; }, 2 * d, rx[trip]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int trip = 0; trip < 2; ++trip) {
            const int item = tid + trip * 256;
            if (item < R * 4) {
                const int seg = item / R, row = item - seg * R;
                float* a = pk_tile + row * pitch + seg * PK_SEG;
#pragma unroll
                for (int k = 0; k < PK_SEG; ++k) a[k] = rx[trip][k];
            }
        }
        __syncthreads();
        // y: 64 columns x 4 segments, one item a thread; the peak test on the result
        const int col = tid & 63, seg = tid >> 6;
        float ry[PK_SEG];
        const float* a = pk_tile + seg * PK_SEG * pitch + col;
        pk_line16<B>([&](int i) { return a[i * pitch]; }, 2 * d, ry);
        const unsigned* mm = (const unsigned*)(head + PK_H_MM(N)) + 2 * n;
        const float mn = pk_unkey(mm[0]), mx = pk_unkey(mm[1]);
        float thr = t.has_abs ? t.thr_abs : mn;
        if (t.has_rel) thr = __builtin_fmaxf(thr, t.thr_rel * mx);
        const int x = x0 + col;
        const bool in_z = z >= t.bz && z < D - t.bz, in_x = x >= t.bx && x < W - t.bx;
#pragma unroll
        for (int k = 0; k < PK_SEG; ++k) {
            const int y = y0 + seg * PK_SEG + k;
            if (x < W && y < H) {
                const int64_t g = (int64_t)plane * HW + (int64_t)y * W + x;
                const float v = img[g];
                const bool cand = v == ry[k] && mn != mx && v > thr && in_z && in_x && y >= t.by && y < H - t.by;
                state[g] = cand ? PK_OPEN : PK_NONE;
                found += cand ? 1 : 0;
            }
        }
        __syncthreads();   // the tile is reloaded for the next plane
    }
    found = tem_wave_sum(found);
    if ((tid & 63) == 0 && found) atomicAdd(&head[PK_H_CAND], found);
}

__global__ void k_pk_batch_begin(int* head, int N, int first) {
    int* pending = head + PK_H_PENDING(N);
    const int carry = first ? 1 : head[PK_H_ALIVE];
    for (int i = 0; i <= TEM_PEAKS_MAX_BATCH; ++i) pending[i] = i == 0 ? carry : 0;
}
__global__ void k_pk_batch_end(int* head, int N, int rounds) {
    const int* pending = head + PK_H_PENDING(N);
    int n = 0;
    for (int i = 0; i < rounds; ++i) n += pending[i];
    head[PK_H_WORK] += n;
    head[PK_H_ALIVE] = pending[rounds];
}

struct PkBoxes {
    int D, H, W, d;
    int bz, by, bx;      // the box of a workgroup, bz * by * bx <= PK_LIST
    int nz, ny, nx;      // boxes per sample and axis
};

__global__ __launch_bounds__(256) void k_pk_round(uint8_t* state, int* head, int round, PkBoxes g, int N) {
    int* pending = head + PK_H_PENDING(N);
    if (pending[round] == 0) return;
    __shared__ int list[PK_LIST];
    __shared__ int n_list;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = g.H * g.W, r = g.d - 1, dd = g.d * g.d;
    const int64_t V = (int64_t)g.D * HW;
    const int per = g.nz * g.ny * g.nx;
    bool left = false;
    for (int64_t box = blockIdx.x; box < (int64_t)N * per; box += gridDim.x) {
        const int n = (int)(box / per), b = (int)(box - (int64_t)n * per);
        const int z0 = (b / (g.nx * g.ny)) * g.bz, y0 = ((b / g.nx) % g.ny) * g.by, x0 = (b % g.nx) * g.bx;
        uint8_t* S = state + (int64_t)n * V;
        if (tid == 0) n_list = 0;
        __syncthreads();
        for (int e = tid; e < g.bz * g.by * g.bx; e += 256) {
            const int x = x0 + e % g.bx, y = y0 + (e / g.bx) % g.by, z = z0 + e / (g.bx * g.by);
            if (x < g.W && y < g.H && z < g.D) {
                const int v = z * HW + y * g.W + x;
                if (S[v] == PK_OPEN) list[atomicAdd(&n_list, 1)] = v;   // the order of the list decides nothing
            }
        }
        __syncthreads();
        const int cnt = n_list;
        // every sweep but the last decides a candidate: at most cnt + 1 sweeps
        for (int sweep = 0; sweep <= cnt; ++sweep) {
            bool changed = false;
            for (int i = wave; i < cnt; i += 4) {
                const int v = list[i];
                if (v < 0) continue;
                const int z = v / HW, y = (v - z * HW) / g.W, x = v - z * HW - y * g.W;
                const int dx = lane - r;
                const bool lane_in = lane <= 2 * r && x + dx >= 0 && x + dx < g.W;
                bool kept = false, und = false;
                // the rows (dz, dy) of the half ball, eight independent loads a trip
                for (int dz = -(z < r ? z : r); dz <= 0 && !kept; ++dz) {
                    const int room = dd - 1 - dz * dz;   // dy^2 + dx^2 <= room, and room >= 2d - 2 >= 0
                    int ry = (int)__builtin_sqrtf((float)room);
                    ry -= ry * ry > room ? 1 : 0;
                    ry += (ry + 1) * (ry + 1) <= room ? 1 : 0;
                    const int dy_lo = -(y < ry ? y : ry), dy_hi = dz < 0 ? (g.H - 1 - y < ry ? g.H - 1 - y : ry) : 0;
                    for (int dy0 = dy_lo; dy0 <= dy_hi; dy0 += 8) {
                        int s[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int dy = dy0 + u;
                            const bool ok = dy <= dy_hi && lane_in && dx * dx <= room - dy * dy && (dz < 0 || dy < 0 || dx < 0);
                            s[u] = ok ? pk_ldb(S + v + dz * HW + dy * g.W + dx) : PK_NONE;
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            kept = kept || s[u] == PK_KEPT;
                            und = und || s[u] == PK_OPEN;
                        }
                    }
                    kept = __any(kept);
                }
                kept = __any(kept);
                und = __any(und);
                if (kept || !und) {
                    if (lane == 0) {
                        pk_stb(S + v, kept ? PK_REJ : PK_KEPT);
                        list[i] = -1;
                    }
                    changed = true;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (int i = tid; i < cnt; i += 256) left = left || list[i] >= 0;
        __syncthreads();   // the list is rebuilt for the next box
    }
    if (__syncthreads_or(left) && tid == 0 && pk_ld(&pending[round + 1]) == 0) pk_st(&pending[round + 1], 1);
}

// grid (chunks, N): the kept peaks of every chunk of PK_CHUNK voxels and of every sample, once nothing is undecided
__global__ __launch_bounds__(256) void k_pk_count(const uint8_t* __restrict__ state, int* __restrict__ counts, int* head, int64_t V, int N) {
    if (head[PK_H_ALIVE] != 0) return;
    const int n = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * PK_CHUNK + threadIdx.x * 4;
    const uint8_t* S = state + (int64_t)n * V;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v0 + k < V) c += S[v0 + k] == PK_KEPT ? 1 : 0;
    __shared__ int part[4];
    const int total = tem_block_reduce<4>(c, part, tem_op_sum());
    if (threadIdx.x == 0) {
        counts[(int64_t)n * gridDim.x + blockIdx.x] = total;
        if (total) atomicAdd(&head[PK_H_KEPT + n], total);
    }
}

// grid (chunks, N): the kept peaks of a chunk in raster order, from its exclusive prefix over the flat list of chunks
__global__ __launch_bounds__(256) void k_pk_compact(const uint8_t* __restrict__ state, const float* __restrict__ img,
                                                    const int64_t* __restrict__ base, int* __restrict__ idx, float* __restrict__ height,
                                                    int* __restrict__ sample, int64_t V) {
    const int n = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * PK_CHUNK + threadIdx.x * 4;
    const uint8_t* S = state + (int64_t)n * V;
    bool k4[4];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        k4[k] = v0 + k < V && S[v0 + k] == PK_KEPT;
        c += k4[k] ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;   // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __shared__ int part[4];
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int64_t pos = base[(int64_t)n * gridDim.x + blockIdx.x] + inc - c;
    for (int w = 0; w < wave; ++w) pos += part[w];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k4[k]) {
            idx[pos] = (int)(v0 + k);
            height[pos] = img[(int64_t)n * V + v0 + k];
            sample[pos] = n;
            ++pos;
        }
}

__global__ __launch_bounds__(256) void k_pk_zero(int* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = 0;
}
// peak i of the flat, ordered list is number i - start[its sample] + 1; the first `limit` of a sample are written (0: all)
__global__ __launch_bounds__(256) void k_pk_seeds(const int* __restrict__ idx, const int* __restrict__ sample, const int64_t* __restrict__ start,
                                                  int64_t T, int limit, int* __restrict__ out, int64_t V) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
        const int n = sample[i];
        const int64_t rank = i - start[n];
        if (limit <= 0 || rank < limit) out[(int64_t)n * V + idx[i]] = (int)rank + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
static bool pk_shape_ok(int N, int D, int H, int W) {
    if (N <= 0 || N > 65535 || D <= 0 || H <= 0 || W <= 0) return false;
    return (int64_t)D * H * W < INT_MAX;
}
static int64_t pk_head_bytes(int N) { return tem_align_up((int64_t)PK_H_INTS(N) * sizeof(int), 16); }

extern "C" int64_t tem_peaks_chunks(int64_t V) { return V <= 0 || V >= INT_MAX ? -1 : tem_cdiv(V, PK_CHUNK); }

extern "C" int64_t tem_peaks_ws(int N, int D, int H, int W) {
    if (!pk_shape_ok(N, D, H, W)) return -1;
    const int64_t NV = (int64_t)N * D * H * W;
    return pk_head_bytes(N) + tem_align_up(NV, 16) + (D > 1 ? NV * 4 : 0);
}

static int pk_args(const char* who, int N, int D, int H, int W, int d, const void* ws, int64_t ws_bytes) {
    TEM_REQUIRE(ws, "%s: null pointer", who);
    TEM_REQUIRE(pk_shape_ok(N, D, H, W), "%s: bad shape (N within 1..65535, D, H, W positive, D*H*W below 2^31 - 1)", who);
    TEM_REQUIRE(d >= 1 && d <= TEM_PEAKS_MAX_DISTANCE, "%s: min_distance %d outside 1..%d", who, d, TEM_PEAKS_MAX_DISTANCE);
    TEM_REQUIRE(((uintptr_t)ws & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);
    if (ws_bytes < tem_peaks_ws(N, D, H, W)) {
        tem_set_error("%s: workspace too small (%lld bytes, %lld needed)", who, (long long)ws_bytes, (long long)tem_peaks_ws(N, D, H, W));
        return TEM_EWS;
    }
    return TEM_OK;
}

template <int B>
static void pk_filter(const float* image, float* zmax, uint8_t* state, int* head, int N, int D, int H, int W, int d, const PkTest& t,
                      hipStream_t st) {
    const int64_t HW = (int64_t)H * W;
    const float* src = image;
    if (D > 1) {
        const int64_t items = (int64_t)N * tem_cdiv(D, PK_SEG) * HW;
        hipLaunchKernelGGL(k_pk_zmax<B>, dim3(tem_grid_1d(items, 256)), dim3(256), 0, st, image, zmax, N, D, HW, d);
        src = zmax;
    }
    const int R = PK_TILE + 2 * d;
    const size_t lds = (size_t)R * (R | 1) * sizeof(float);   // at most 126 * 127 * 4 = 64008 bytes
    const int64_t planes = (int64_t)N * D;
    const dim3 grid((unsigned)(tem_cdiv(W, PK_TILE) * tem_cdiv(H, PK_TILE)), (unsigned)(planes > 65535 ? 65535 : planes));
    hipLaunchKernelGGL(k_pk_xy<B>, grid, dim3(256), lds, st, src, image, state, head, N, D, H, W, d, t);
}

extern "C" int tem_peaks_candidates(const float* image, int N, int D, int H, int W, int min_distance, int has_abs, float threshold_abs,
                                    int has_rel, float threshold_rel, int border, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    const int d = min_distance;
    TEM_TRY(pk_args("tem_peaks_candidates", N, D, H, W, d, ws, ws_bytes));
    TEM_REQUIRE(image, "tem_peaks_candidates: null pointer");
    TEM_REQUIRE(border >= 0, "tem_peaks_candidates: border %d is negative", border);
    TEM_REQUIRE(tem_cdiv(W, PK_TILE) * tem_cdiv(H, PK_TILE) < INT_MAX, "tem_peaks_candidates: too many tiles a plane");
    const int64_t V = (int64_t)D * H * W, NV = V * N;
    int* head = (int*)ws;
    uint8_t* state = (uint8_t*)ws + pk_head_bytes(N);
    float* zmax = (float*)(state + tem_align_up(NV, 16));
    PkTest t;
    t.has_abs = has_abs != 0, t.has_rel = has_rel != 0, t.thr_abs = threshold_abs, t.thr_rel = threshold_rel;
    t.bz = D > 1 ? border : 0, t.by = H > 1 ? border : 0, t.bx = W > 1 ? border : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pk_init, dim3(tem_grid_1d(PK_H_INTS(N), 256)), dim3(256), 0, st, head, N);
    hipLaunchKernelGGL(k_pk_minmax, dim3(tem_grid_1d(V, 256 * 4, N > 8 ? 256 : 2048), N), dim3(256), 0, st, image, head, V, N);
    const int w = 2 * d + 1;
    if (w >= 16) pk_filter<16>(image, zmax, state, head, N, D, H, W, d, t, st);
    else if (w >= 8) pk_filter<8>(image, zmax, state, head, N, D, H, W, d, t, st);
    else if (w >= 4) pk_filter<4>(image, zmax, state, head, N, D, H, W, d, t, st);
    else pk_filter<2>(image, zmax, state, head, N, D, H, W, d, t, st);
    TEM_CHECK_LAUNCH("tem_peaks_candidates");
    return TEM_OK;
}

extern "C" int tem_peaks_rounds(int N, int D, int H, int W, int min_distance, void* ws, int64_t ws_bytes, int* counts, int first,
                                int rounds, tem_stream_t stream) {
    TEM_TRY(pk_args("tem_peaks_rounds", N, D, H, W, min_distance, ws, ws_bytes));
    TEM_REQUIRE(counts, "tem_peaks_rounds: null pointer");
    TEM_REQUIRE(rounds >= 1 && rounds <= TEM_PEAKS_MAX_BATCH, "tem_peaks_rounds: 1..%d rounds a call (got %d)", TEM_PEAKS_MAX_BATCH, rounds);
    const int64_t V = (int64_t)D * H * W;
    int* head = (int*)ws;
    uint8_t* state = (uint8_t*)ws + pk_head_bytes(N);
    PkBoxes g;
    g.D = D, g.H = H, g.W = W, g.d = min_distance;
    g.bz = D > 1 ? 4 : 1, g.by = D > 1 ? 16 : 64, g.bx = 64;
    g.nz = (int)tem_cdiv(D, g.bz), g.ny = (int)tem_cdiv(H, g.by), g.nx = (int)tem_cdiv(W, g.bx);
    const int64_t boxes = (int64_t)N * g.nz * g.ny * g.nx;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pk_batch_begin, dim3(1), dim3(1), 0, st, head, N, first ? 1 : 0);
    for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(k_pk_round, dim3(tem_grid_1d(boxes, 1)), dim3(256), 0, st, state, head, r, g, N);
    hipLaunchKernelGGL(k_pk_batch_end, dim3(1), dim3(1), 0, st, head, N, rounds);
    hipLaunchKernelGGL(k_pk_count, dim3((unsigned)tem_cdiv(V, PK_CHUNK), N), dim3(256), 0, st, state, counts, head, V, N);
    TEM_CHECK_LAUNCH("tem_peaks_rounds");
    return TEM_OK;
}

extern "C" int tem_peaks_compact(const float* image, const int64_t* base, int* idx, float* height, int* sample, int N, int D, int H, int W,
                                 void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_TRY(pk_args("tem_peaks_compact", N, D, H, W, 1, ws, ws_bytes));
    TEM_REQUIRE(image && base && idx && height && sample, "tem_peaks_compact: null pointer");
    const int64_t V = (int64_t)D * H * W;
    const uint8_t* state = (const uint8_t*)ws + pk_head_bytes(N);
    hipLaunchKernelGGL(k_pk_compact, dim3((unsigned)tem_cdiv(V, PK_CHUNK), N), dim3(256), 0, (hipStream_t)stream, state, image, base, idx,
                       height, sample, V);
    TEM_CHECK_LAUNCH("tem_peaks_compact");
    return TEM_OK;
}

extern "C" int tem_peaks_seeds(const int* idx, const int* sample, const int64_t* start, int64_t T, int limit, int* out, int N, int64_t V,
                               tem_stream_t stream) {
    TEM_REQUIRE(out && N > 0 && V > 0 && V < INT_MAX && T >= 0 && T <= (int64_t)N * V, "tem_peaks_seeds: bad arguments");
    TEM_REQUIRE(T == 0 || (idx && sample && start), "tem_peaks_seeds: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pk_zero, dim3(tem_grid_1d((int64_t)N * V, 256)), dim3(256), 0, st, out, (int64_t)N * V);
    if (T > 0) hipLaunchKernelGGL(k_pk_seeds, dim3(tem_grid_1d(T, 256)), dim3(256), 0, st, idx, sample, start, T, limit, out, V);
    TEM_CHECK_LAUNCH("tem_peaks_seeds");
    return TEM_OK;
}
