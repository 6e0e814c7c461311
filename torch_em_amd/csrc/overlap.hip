// overlap.hip -- the contingency table of two label batches and the instance-segmentation scores that are functions of it
// (DESIGN.md "Instance segmentation scores").  Integer results are exact; every floating-point sum is reduced in a fixed
// order (per thread in index order, a butterfly per wave, the four waves of a block in order, the blocks of a sample by one
// block in the same way), so a record is bit-identical from run to run.  Nothing is read back by the host and no loop waits.
//
// Inputs: per sample the sorted keys a * (V + 1) + b (int64 [N][V]; a, b: dense ids 0..V of the two volumes, sorted by the
// caller) and the flat inclusive prefix sum of the run-end flags.  The table:
//   pa, pb, n_ab  int32 [N][V]      the distinct pairs in ascending (a, b) order and their voxel counts, valid below npairs[n]
//   npairs        int32 [N]
//   n_a, n_b      int32 [N][V + 1]  the marginals, indexed by id
// Run lengths are differences of run-end positions; the marginals are integer atomic adds of the pair counts (far fewer than
// voxels), reduced per wave first: the pairs are sorted by a, so neighbouring lanes share it.
//
// Workspace (tem_overlap_ws bytes): part [N][OV_BLOCKS][OV_SLOTS] 8-byte partials, match_a, match_b int32 [N][V + 1] (matched
// pairs per object), end int32 [N][V] (the run-end positions).
#include <limits.h>

#include "tem_common.h"

#define OV_BLOCKS 256     // blocks per sample of the two score passes at most: the partials one block reduces
#define OV_SLOTS 13
#define OV_WAVE_IDS 4     // distinct ids a wave reduces before its lanes fall back to one atomic each

typedef unsigned long long ov_u64;

enum { OV_SUM_AB = 0, OV_S_AB, OV_MATCHED, OV_SUM_A, OV_SUM_B, OV_S_A, OV_S_B, OV_BD_A, OV_BD_B, OV_N_A, OV_N_B, OV_DUP_A, OV_DUP_B };

static int ov_blocks(int64_t items) { return (int)(tem_cdiv(items, 256) < OV_BLOCKS ? tem_cdiv(items, 256) : OV_BLOCKS); }

__device__ __forceinline__ int ov_lane() { return threadIdx.x & 63; }

__device__ __forceinline__ ov_u64 ov_wave_sum(ov_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (ov_u64)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ ov_u64 ov_wave_max(ov_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const ov_u64 w = (ov_u64)__shfl_xor((long long)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// the sum of v over the 256 threads of the block, in every thread; the order is fixed: butterfly per wave, then wave 0..3
__device__ __forceinline__ ov_u64 ov_block_sum(ov_u64 v, ov_u64* sh) {
    v = ov_wave_sum(v);
    __syncthreads();
    if (ov_lane() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ double ov_block_sum(double v, double* sh) {
    v = tem_wave_sum_d(v);
    __syncthreads();
    if (ov_lane() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// cnt[slot] += val for every lane with slot >= 0 (all 64 lanes call): lanes that share a slot send one atomic
__device__ __forceinline__ void ov_wave_add(int* cnt, long long slot, int val) {
    ov_u64 pending = __ballot(slot >= 0);
    for (int it = 0; it < OV_WAVE_IDS && pending; ++it) {
        const int leader = __ffsll((long long)pending) - 1;
        const long long s = __shfl(slot, leader, 64);
        const bool mine = slot == s;
        const int sum = (int)ov_wave_sum(mine ? (ov_u64)val : 0ull);
        if (ov_lane() == leader) atomicAdd(&cnt[s], sum);
        pending &= ~__ballot(mine);
        if (mine) slot = -1;
    }
    if (slot >= 0) atomicAdd(&cnt[slot], val);
}

// best[slot] = max(best[slot], val) on the bit patterns of non-negative doubles (they order as unsigned integers)
__device__ __forceinline__ void ov_wave_best(ov_u64* best, long long slot, ov_u64 val) {
    ov_u64 pending = __ballot(slot >= 0);
    for (int it = 0; it < OV_WAVE_IDS && pending; ++it) {
        const int leader = __ffsll((long long)pending) - 1;
        const long long s = __shfl(slot, leader, 64);
        const bool mine = slot == s;
        const ov_u64 m = ov_wave_max(mine ? val : 0ull);
        if (ov_lane() == leader) atomicMax(&best[s], m);
        pending &= ~__ballot(mine);
        if (mine) slot = -1;
    }
    if (slot >= 0) atomicMax(&best[slot], val);
}

__device__ __forceinline__ int ov_prev_total(const int* __restrict__ rank, int64_t n, int64_t V) { return n > 0 ? rank[n * V - 1] : 0; }

// flag[g] = 1 where a run of equal keys ends
__global__ __launch_bounds__(256) void k_ov_flag(const int64_t* __restrict__ sorted, int* __restrict__ flag, int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256)
        flag[g] = (g % V == V - 1 || sorted[g + 1] != sorted[g]) ? 1 : 0;
}

// rank: the flat inclusive prefix sum of flag.  A run end takes row rank - 1 of its sample's table; an id outside 0..V (not
// produced by dense ids) is clamped, so no table is indexed outside.
__global__ __launch_bounds__(256) void k_ov_compact(const int64_t* __restrict__ sorted, const int* __restrict__ rank,
                                                    int* __restrict__ pa, int* __restrict__ pb, int* __restrict__ end,
                                                    int* __restrict__ npairs, int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t n = g / V, v = g - n * V;
        const int64_t key = sorted[g];
        if (!(v == V - 1 || sorted[g + 1] != key)) continue;
        const int64_t row = (int64_t)rank[g] - ov_prev_total(rank, n, V) - 1;
        if (v == V - 1) npairs[n] = (row >= 0 && row < V) ? (int)row + 1 : 0;
        if (row < 0 || row >= V) continue;
        int64_t a = key / (V + 1), b = key - a * (V + 1);
        a = a < 0 ? 0 : (a > V ? V : a);
        b = b < 0 ? 0 : (b > V ? V : b);
        pa[n * V + row] = (int)a;
        pb[n * V + row] = (int)b;
        end[n * V + row] = (int)v;
    }
}

// grid (blocks, N): n_ab = the distance of a run end from the one before; both marginals += n_ab
__global__ __launch_bounds__(256) void k_ov_counts(const int* __restrict__ pa, const int* __restrict__ pb, const int* __restrict__ end,
                                                   const int* __restrict__ npairs, int* __restrict__ n_ab, int* n_a, int* n_b,
                                                   int64_t V) {
    const int64_t n = blockIdx.y;
    int np = npairs[n];
    np = np < 0 ? 0 : (np > V ? (int)V : np);
    pa += n * V, pb += n * V, end += n * V, n_ab += n * V;
    n_a += n * (V + 1), n_b += n * (V + 1);
    // every lane of a wave makes the same number of trips: the wave reductions need all 64
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < np; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        long long a = -1, b = -1;
        int c = 0;
        if (i < np) {
            c = end[i] - (i > 0 ? end[i - 1] : -1);
            n_ab[i] = c;
            a = pa[i], b = pb[i];
            a = a > V ? -1 : a, b = b > V ? -1 : b;   // rows a consistent rank fills never hold such ids
        }
        ov_wave_add(n_a, a, c);
        ov_wave_add(n_b, b, c);
    }
}

__device__ __forceinline__ double ov_nlog2n(int c) { return c > 1 ? (double)c * log2((double)c) : 0.0; }

// grid (blocks, N), over the pairs: sum n_ab^2, sum n_ab log2 n_ab, the matched pairs (and how many each object has), the
// best Dice of every object in both directions
__global__ __launch_bounds__(256) void k_ov_pairs(const int* __restrict__ pa, const int* __restrict__ pb, const int* __restrict__ n_ab,
                                                  const int* __restrict__ npairs, const int* __restrict__ n_a,
                                                  const int* __restrict__ n_b, double threshold, ov_u64* best_a, ov_u64* best_b,
                                                  int* match_a, int* match_b, ov_u64* __restrict__ part, int64_t V) {
    __shared__ ov_u64 sh[4];
    const int64_t n = blockIdx.y;
    int np = npairs[n];
    np = np < 0 ? 0 : (np > V ? (int)V : np);
    pa += n * V, pb += n * V, n_ab += n * V;
    const int64_t off = n * (V + 1);
    ov_u64 sum = 0, matched = 0;
    double s = 0.0;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < np; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        long long a = -1, b = -1;
        ov_u64 dice = 0;
        if (i < np) {
            const int c = n_ab[i];
            sum += (ov_u64)c * (ov_u64)c;
            s += ov_nlog2n(c);
            const int ia = pa[i], ib = pb[i];
            if (ia > 0 && ib > 0 && ia <= V && ib <= V) {
                const int64_t na = n_a[off + ia], nb = n_b[off + ib];
                if ((double)c >= threshold * (double)(na + nb - c)) {
                    ++matched;
                    atomicAdd(&match_a[off + ia], 1);
                    atomicAdd(&match_b[off + ib], 1);
                }
                a = ia, b = ib;
                dice = (ov_u64)__double_as_longlong(2.0 * (double)c / (double)(na + nb));
            }
        }
        ov_wave_best(best_a + off, a, dice);
        ov_wave_best(best_b + off, b, dice);
    }
    ov_u64* p = part + (n * OV_BLOCKS + blockIdx.x) * OV_SLOTS;
    const ov_u64 t_sum = ov_block_sum(sum, sh), t_matched = ov_block_sum(matched, sh);
    const double t_s = ov_block_sum(s, (double*)sh);
    if (threadIdx.x == 0) {
        p[OV_SUM_AB] = t_sum;
        p[OV_MATCHED] = t_matched;
        p[OV_S_AB] = (ov_u64)__double_as_longlong(t_s);
    }
}

// grid (blocks, N), over the ids 0..V: the sums of both marginals, the objects of both sides, the sums of their best Dice, the
// objects with two matched pairs
__global__ __launch_bounds__(256) void k_ov_objects(const int* __restrict__ n_a, const int* __restrict__ n_b,
                                                    const ov_u64* __restrict__ best_a, const ov_u64* __restrict__ best_b,
                                                    const int* __restrict__ match_a, const int* __restrict__ match_b,
                                                    ov_u64* __restrict__ part, int64_t V) {
    __shared__ ov_u64 sh[4];
    const int64_t n = blockIdx.y, off = n * (V + 1);
    ov_u64 sq[2] = {0, 0}, cnt[2] = {0, 0}, dup[2] = {0, 0};
    double s[2] = {0.0, 0.0}, bd[2] = {0.0, 0.0};
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id <= V; id += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = (k ? n_b : n_a)[off + id];
            sq[k] += (ov_u64)c * (ov_u64)c;
            s[k] += ov_nlog2n(c);
            if (id > 0 && c > 0) {
                ++cnt[k];
                bd[k] += __longlong_as_double((long long)(k ? best_b : best_a)[off + id]);
                if ((k ? match_b : match_a)[off + id] >= 2) ++dup[k];
            }
        }
    }
    ov_u64* p = part + (n * OV_BLOCKS + blockIdx.x) * OV_SLOTS;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const ov_u64 t_sq = ov_block_sum(sq[k], sh), t_cnt = ov_block_sum(cnt[k], sh), t_dup = ov_block_sum(dup[k], sh);
        const double t_s = ov_block_sum(s[k], (double*)sh), t_bd = ov_block_sum(bd[k], (double*)sh);
        if (threadIdx.x == 0) {
            p[OV_SUM_A + k] = t_sq;
            p[OV_N_A + k] = t_cnt;
            p[OV_DUP_A + k] = t_dup;
            p[OV_S_A + k] = (ov_u64)__double_as_longlong(t_s);
            p[OV_BD_A + k] = (ov_u64)__double_as_longlong(t_bd);
        }
    }
}

// one block per sample: the partials of block t in thread t, reduced in the same fixed order
__global__ __launch_bounds__(256) void k_ov_record(const ov_u64* __restrict__ part, const int* __restrict__ npairs,
                                                   TemOverlapRecord* __restrict__ rec, int nblk_pairs, int nblk_objects, int64_t V) {
    __shared__ ov_u64 sh[4];
    const int64_t n = blockIdx.x;
    const ov_u64* p = part + (n * OV_BLOCKS + threadIdx.x) * OV_SLOTS;
    ov_u64 iv[OV_SLOTS];
#pragma unroll
    for (int k = 0; k < OV_SLOTS; ++k) {
        const bool have = (int)threadIdx.x < (k <= OV_MATCHED ? nblk_pairs : nblk_objects);
        const bool real = k == OV_S_AB || k == OV_S_A || k == OV_S_B || k == OV_BD_A || k == OV_BD_B;
        const ov_u64 x = have ? p[k] : 0ull;   // the bits of 0.0 are 0
        iv[k] = real ? (ov_u64)__double_as_longlong(ov_block_sum(__longlong_as_double((long long)x), (double*)sh))
                     : ov_block_sum(x, sh);
    }
    if (threadIdx.x != 0) return;
    TemOverlapRecord r;
    r.sum_ab = iv[OV_SUM_AB], r.sum_a = iv[OV_SUM_A], r.sum_b = iv[OV_SUM_B];
    r.s_ab = __longlong_as_double((long long)iv[OV_S_AB]);
    r.s_a = __longlong_as_double((long long)iv[OV_S_A]);
    r.s_b = __longlong_as_double((long long)iv[OV_S_B]);
    r.n_pred = (int)iv[OV_N_A], r.n_true = (int)iv[OV_N_B];
    r.tp = (int)((long long)iv[OV_MATCHED] - (long long)iv[OV_DUP_A] - (long long)iv[OV_DUP_B]);
    r.npairs = npairs[n];
    r.dice_pred = r.n_pred > 0 ? __longlong_as_double((long long)iv[OV_BD_A]) / (double)r.n_pred : 0.0;
    r.dice_true = r.n_true > 0 ? __longlong_as_double((long long)iv[OV_BD_B]) / (double)r.n_true : 0.0;
    rec[n] = r;
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
static bool ov_shape_ok(int N, int64_t V) { return N > 0 && N <= 65535 && V > 0 && V < INT_MAX && (int64_t)N * V < INT_MAX; }

struct OvWs {
    ov_u64* part;
    int *match_a, *match_b, *end;
    int64_t match_bytes;
};
static OvWs ov_carve(void* ws, int N, int64_t V) {
    OvWs w;
    w.part = (ov_u64*)ws;
    w.match_a = (int*)(w.part + (int64_t)N * OV_BLOCKS * OV_SLOTS);
    w.match_b = w.match_a + (int64_t)N * (V + 1);
    w.end = w.match_b + (int64_t)N * (V + 1);
    w.match_bytes = (int64_t)N * (V + 1) * 2 * sizeof(int);
    return w;
}

extern "C" int64_t tem_overlap_ws(int N, int64_t V) {
    if (!ov_shape_ok(N, V)) return -1;
    return tem_align_up((int64_t)N * OV_BLOCKS * OV_SLOTS * 8 + (int64_t)N * (V + 1) * 8 + (int64_t)N * V * 4, 16);
}

static int ov_ws_ok(const char* who, int N, int64_t V, const void* ws, int64_t ws_bytes) {
    TEM_REQUIRE(ov_shape_ok(N, V), "%s: bad shape (N in 1..65535, V positive, N * V below 2^31 - 1)", who);
    TEM_REQUIRE(ws && ((uintptr_t)ws & 15u) == 0, "%s: the workspace must be non-null and 16-byte aligned", who);
    if (ws_bytes < tem_overlap_ws(N, V)) {
        tem_set_error("%s: workspace too small (%lld bytes, %lld needed)", who, (long long)ws_bytes, (long long)tem_overlap_ws(N, V));
        return TEM_EWS;
    }
    return TEM_OK;
}

extern "C" int tem_overlap_flag(const int64_t* sorted, int* flag, int N, int64_t V, tem_stream_t stream) {
    TEM_REQUIRE(sorted && flag, "tem_overlap_flag: null pointer");
    TEM_REQUIRE(ov_shape_ok(N, V), "tem_overlap_flag: bad shape (N in 1..65535, V positive, N * V below 2^31 - 1)");
    hipLaunchKernelGGL(k_ov_flag, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, (hipStream_t)stream, sorted, flag, V, N * V);
    TEM_CHECK_LAUNCH("tem_overlap_flag");
    return TEM_OK;
}

extern "C" int tem_overlap_table(const int64_t* sorted, const int* rank, int* pa, int* pb, int* n_ab, int* npairs, int* n_a,
                                 int* n_b, int N, int64_t V, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(sorted && rank && pa && pb && n_ab && npairs && n_a && n_b, "tem_overlap_table: null pointer");
    TEM_TRY(ov_ws_ok("tem_overlap_table", N, V, ws, ws_bytes));
    const OvWs w = ov_carve(ws, N, V);
    hipStream_t st = (hipStream_t)stream;
    const size_t mbytes = (size_t)N * (V + 1) * sizeof(int);
    if (hipMemsetAsync(n_a, 0, mbytes, st) != hipSuccess || hipMemsetAsync(n_b, 0, mbytes, st) != hipSuccess) {
        tem_set_error("tem_overlap_table: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    hipLaunchKernelGGL(k_ov_compact, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, st, sorted, rank, pa, pb, w.end, npairs, V, N * V);
    hipLaunchKernelGGL(k_ov_counts, dim3(ov_blocks(V), N), dim3(256), 0, st, pa, pb, w.end, npairs, n_ab, n_a, n_b, V);
    TEM_CHECK_LAUNCH("tem_overlap_table");
    return TEM_OK;
}

extern "C" int tem_overlap_scores(const int* pa, const int* pb, const int* n_ab, const int* npairs, const int* n_a, const int* n_b,
                                  double threshold, TemOverlapRecord* rec, double* best_a, double* best_b, int N, int64_t V,
                                  void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(pa && pb && n_ab && npairs && n_a && n_b && rec && best_a && best_b, "tem_overlap_scores: null pointer");
    TEM_REQUIRE(threshold >= 0.5 && threshold <= 1.0,
                "tem_overlap_scores: threshold %g: a threshold below 0.5 needs an assignment solver and is not provided (0.5 <= "
                "threshold <= 1)", threshold);
    TEM_REQUIRE((((uintptr_t)rec | (uintptr_t)best_a | (uintptr_t)best_b) & 7u) == 0, "tem_overlap_scores: rec, best_a, best_b must be 8-byte aligned");
    TEM_TRY(ov_ws_ok("tem_overlap_scores", N, V, ws, ws_bytes));
    const OvWs w = ov_carve(ws, N, V);
    hipStream_t st = (hipStream_t)stream;
    const size_t bbytes = (size_t)N * (V + 1) * sizeof(double);
    if (hipMemsetAsync(w.match_a, 0, (size_t)w.match_bytes, st) != hipSuccess || hipMemsetAsync(best_a, 0, bbytes, st) != hipSuccess ||
        hipMemsetAsync(best_b, 0, bbytes, st) != hipSuccess) {
        tem_set_error("tem_overlap_scores: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    const int nbp = ov_blocks(V), nbo = ov_blocks(V + 1);
    hipLaunchKernelGGL(k_ov_pairs, dim3(nbp, N), dim3(256), 0, st, pa, pb, n_ab, npairs, n_a, n_b, threshold, (ov_u64*)best_a,
                       (ov_u64*)best_b, w.match_a, w.match_b, w.part, V);
    hipLaunchKernelGGL(k_ov_objects, dim3(nbo, N), dim3(256), 0, st, n_a, n_b, (const ov_u64*)best_a, (const ov_u64*)best_b,
                       w.match_a, w.match_b, w.part, V);
    hipLaunchKernelGGL(k_ov_record, dim3(N), dim3(256), 0, st, w.part, npairs, rec, nbp, nbo, V);
    TEM_CHECK_LAUNCH("tem_overlap_scores");
    return TEM_OK;
}
