// watershed.hip -- seeded watershed on the device: the minimum spanning forest rooted in the markers (the watershed cut of
// Cousty et al.), computed by Boruvka rounds.  Integer compares only; the result does not depend on the execution order.
//
// The contract (DESIGN.md "Seeded watershed"): per sample the voxels are ranked by (height, linear index) -- rank / order,
// int32 [N][V], supplied by the caller (a stable sort) -- the nodes are the voxels inside the mask, the edges join masked face
// neighbours, and an edge's weight is the pair (higher rank, lower rank).  All weights differ, so the forest is unique.
//
// State per voxel (workspace of tem_watershed_ws bytes, 20 per voxel, and WS_FLAGS ints):
//   comp  int32   the root of the voxel's component, sample-local (flat at the start of every round); -1 outside the mask
//   lab   int32   the marker value, read at roots only; a marked root never hooks, so it never changes
//   best  uint64  at roots: the lightest edge that leaves the component this round, as hi << 32 | lo << 1 | dir (dir: the
//                 end inside the component is the higher one -- the lowest bit, so it never decides between two edges)
//   nxt   int32   the parent forest of the round between hook and commit
// One round = pick (atomicMin of the edge keys into best[root]; marked components pick nothing), hook (every unmarked
// root with a pick points at the root of the edge's far end, read from the untouched comp; of two roots that picked the
// same edge the larger one stays), WS_PASSES(V) flatten passes (a chase of at most WS_CHASE steps each: a pass divides every
// depth by WS_CHASE, so WS_CHASE ^ passes >= V flattens any forest on V nodes), commit (comp = nxt, best reset).
// Every round reads `did[round]`, written by its pick, and returns at once when nothing was picked; nothing is read back
// by the host, and no loop -- on the host or in a kernel -- waits for a condition.
#include <limits.h>

#include "tem_common.h"

#define WS_NONE 0xffffffffffffffffull
#define WS_CHASE 256          // steps of one chase
#define WS_CHASE_LOG2 8
#define WS_MAX_ROUNDS 33      // ceil(log2(V)) + 1 for V < 2^31
#define WS_MAX_PASSES 4       // ceil(31 / WS_CHASE_LOG2)
#define WS_FLAGS (WS_MAX_ROUNDS * (1 + WS_MAX_PASSES))   // did[round], then deep[round][pass]
#define WS_WAVE_ROOTS 4       // distinct roots a wave reduces before its lanes fall back to one atomic each

typedef unsigned long long ws_u64;

static int ws_log2_ceil(int64_t V) {
    int l = 0;
    while (((int64_t)1 << l) < V) ++l;
    return l;
}
static int ws_rounds(int64_t V) { return ws_log2_ceil(V) + 1; }
static int ws_passes(int64_t V) {
    const int p = (ws_log2_ceil(V) + WS_CHASE_LOG2 - 1) / WS_CHASE_LOG2;
    return p < 1 ? 1 : p;
}

__device__ __forceinline__ int ws_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ws_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a batch index g -> the voxel's index inside its sample (below 2^31) and the sample's first batch index
__device__ __forceinline__ int ws_local(int64_t g, int64_t V, int64_t& base) {
    base = (g / V) * V;
    return (int)(g - base);
}

__device__ __forceinline__ ws_u64 ws_wave_min(ws_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const ws_u64 w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// markers: int32 or int64 (marker64); a negative marker and a marker outside the mask count as none
__global__ __launch_bounds__(256) void k_ws_init(const void* __restrict__ markers, int marker64, const uint8_t* __restrict__ mask,
                                                 int* __restrict__ comp, int* __restrict__ lab, ws_u64* __restrict__ best,
                                                 int* __restrict__ flags, int64_t V, int64_t NV) {
    if (blockIdx.x == 0 && threadIdx.x < WS_FLAGS) flags[threadIdx.x] = 0;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const bool in = mask == nullptr || mask[g] != 0;
        int64_t m = marker64 ? ((const int64_t*)markers)[g] : (int64_t)((const int*)markers)[g];
        m = (m < 0 || m > INT_MAX) ? 0 : m;
        int64_t base;
        comp[g] = in ? ws_local(g, V, base) : -1;
        lab[g] = in ? (int)m : 0;
        best[g] = WS_NONE;
    }
}

// the key of the edge from a voxel of rank rv in component r to the voxel u, if u is a masked voxel of another component
__device__ __forceinline__ ws_u64 ws_edge(ws_u64 m, int rv, int r, const int* __restrict__ comp, const int* __restrict__ rank,
                                          int64_t u) {
    const int cu = comp[u];
    if (cu < 0 || cu == r) return m;
    const int ru = rank[u];
    const bool dir = rv > ru;
    const ws_u64 k = ((ws_u64)(unsigned)(dir ? rv : ru) << 32) | ((ws_u64)(unsigned)(dir ? ru : rv) << 1) | (dir ? 1u : 0u);
    return k < m ? k : m;
}

__global__ __launch_bounds__(256) void k_ws_pick(const int* __restrict__ rank, const int* __restrict__ comp,
                                                 const int* __restrict__ lab, ws_u64* best, int* flags, int round, int D,
                                                 int H, int W, int64_t NV) {
    if (round > 0 && flags[round - 1] == 0) return;
    const int HW = H * W;   // D * H * W < 2^31
    const int64_t V = (int64_t)HW * D;
    const int64_t span = (int64_t)gridDim.x * 256;
    bool any = false;
    // every lane of a wave makes the same number of trips: the wave reduction below needs all 64
    for (int64_t g0 = (int64_t)blockIdx.x * 256; g0 < NV; g0 += span) {
        const int64_t g = g0 + threadIdx.x;
        ws_u64 m = WS_NONE;
        int r = -1;
        int64_t base = 0;
        if (g < NV) {
            r = comp[g];
            const unsigned v = (unsigned)ws_local(g, V, base);
            if (r >= 0 && lab[base + r] == 0) {
                const int x = (int)(v % (unsigned)W), y = (int)((v / (unsigned)W) % (unsigned)H), z = (int)(v / (unsigned)HW);
                const int rv = rank[g];
                if (x > 0) m = ws_edge(m, rv, r, comp, rank, g - 1);
                if (x + 1 < W) m = ws_edge(m, rv, r, comp, rank, g + 1);
                if (y > 0) m = ws_edge(m, rv, r, comp, rank, g - W);
                if (y + 1 < H) m = ws_edge(m, rv, r, comp, rank, g + W);
                if (z > 0) m = ws_edge(m, rv, r, comp, rank, g - HW);
                if (z + 1 < D) m = ws_edge(m, rv, r, comp, rank, g + HW);
            }
        }
        bool active = m != WS_NONE;
        any = any || active;
        ws_u64* slot = best + base + (r < 0 ? 0 : r);
        // an older (larger) value may be read here: then the atomic below is merely not spared
        if (active && m >= __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) active = false;
        // lanes that share a root: one atomic for all of them (components are spatially coherent)
        for (int it = 0; it < WS_WAVE_ROOTS; ++it) {
            const ws_u64 ballot = __ballot(active);
            if (ballot == 0) break;
            const int leader = __ffsll((long long)ballot) - 1;
            const int64_t lslot = __shfl((long long)(base + r), leader, 64);
            const bool mine = active && base + r == lslot;
            const ws_u64 mm = ws_wave_min(mine ? m : WS_NONE);
            if ((threadIdx.x & 63) == leader) atomicMin(slot, mm);
            if (mine) active = false;
        }
        if (active) atomicMin(slot, m);
    }
    // one word for the whole grid: stores to one address queue up behind each other, so a block stores only while it reads 0
    if (__syncthreads_or(any) && threadIdx.x == 0 && ws_ld(&flags[round]) == 0) ws_st(&flags[round], 1);
}

__global__ __launch_bounds__(256) void k_ws_hook(const int* __restrict__ order, const int* __restrict__ comp,
                                                 const int* __restrict__ lab, const ws_u64* __restrict__ best,
                                                 int* __restrict__ nxt, const int* __restrict__ flags, int round, int64_t V,
                                                 int64_t NV) {
    if (flags[round] == 0) return;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        int p = comp[g];
        if (p < 0) {
            nxt[g] = -1;   // the flatten passes read every entry
            continue;
        }
        int64_t base;
        const int v = ws_local(g, V, base);
        const ws_u64 k = (p == v && lab[g] == 0) ? best[g] : WS_NONE;
        if (k != WS_NONE) {
            const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)(k & 0xffffffffu) >> 1;
            const unsigned far_rank = (k & 1) ? lo : hi;
            if ((int64_t)far_rank < V) {
                const int far = order[base + far_rank];
                const int ro = ((unsigned)far < (uint64_t)V) ? comp[base + far] : -1;
                // two unmarked roots that picked the same edge would point at each other: the larger one stays a root
                if (ro >= 0 && !(lab[base + ro] == 0 && best[base + ro] == (k ^ 1) && v > ro)) p = ro;
            }
        }
        nxt[g] = p;
    }
}

// every voxel moves up to WS_CHASE steps towards its root; a value read while other lanes write is an ancestor as well
__global__ __launch_bounds__(256) void k_ws_flatten(int* nxt, int* flags, int round, int pass, int64_t V, int64_t NV) {
    if (flags[round] == 0) return;
    int* deep = flags + WS_MAX_ROUNDS + round * WS_MAX_PASSES;
    if (pass > 0 && deep[pass - 1] == 0) return;
    bool open = false;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        int x = ws_ld(&nxt[g]);
        if (x < 0) continue;
        int64_t base;
        ws_local(g, V, base);
        int* row = nxt + base;
        bool flat = false;
        for (int s = 0; s < WS_CHASE; ++s) {
            const int y = ws_ld(&row[x]);
            if (y == x || y < 0) {
                flat = true;
                break;
            }
            x = y;
        }
        open = open || !flat;
        ws_st(&nxt[g], x);
    }
    if (__syncthreads_or(open) && threadIdx.x == 0 && ws_ld(&deep[pass]) == 0) ws_st(&deep[pass], 1);
}

__global__ __launch_bounds__(256) void k_ws_commit(int* __restrict__ comp, const int* __restrict__ nxt, ws_u64* __restrict__ best,
                                                   const int* __restrict__ flags, int round, int64_t V, int64_t NV) {
    if (flags[round] == 0) return;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int old = comp[g];
        if (old < 0) continue;
        int64_t base;
        if (old == ws_local(g, V, base) && best[g] != WS_NONE) best[g] = WS_NONE;
        comp[g] = nxt[g];
    }
}

__global__ __launch_bounds__(256) void k_ws_write(const int* __restrict__ comp, const int* __restrict__ lab, int* __restrict__ out,
                                                  const int* __restrict__ flags, int* __restrict__ rounds_out, int rounds,
                                                  int64_t V, int64_t NV) {
    if (rounds_out && blockIdx.x == 0 && threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < rounds; ++i) n += flags[i];
        *rounds_out = n;
    }
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int r = comp[g];
        int64_t base;
        ws_local(g, V, base);
        out[g] = r < 0 ? 0 : lab[base + r];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
static bool ws_shape_ok(int N, int D, int H, int W) {
    return N > 0 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < INT_MAX;
}

extern "C" int tem_watershed_rounds(int64_t V) { return V > 0 && V < INT_MAX ? ws_rounds(V) : -1; }

extern "C" int64_t tem_watershed_ws(int N, int64_t V) {
    if (N <= 0 || V <= 0 || V >= INT_MAX) return -1;
    return (int64_t)N * V * 20 + tem_align_up(WS_FLAGS * sizeof(int), 16);
}

extern "C" int tem_watershed(const int* rank, const int* order, const void* markers, int marker_bytes, const uint8_t* mask,
                             int* out, int* rounds_out, int N, int D, int H, int W, void* ws, int64_t ws_bytes,
                             tem_stream_t stream) {
    TEM_REQUIRE(rank && order && markers && out && ws, "tem_watershed: null pointer");
    TEM_REQUIRE(ws_shape_ok(N, D, H, W), "tem_watershed: bad shape (N, D, H, W positive, D*H*W below 2^31 - 1)");
    TEM_REQUIRE(marker_bytes == 4 || marker_bytes == 8, "tem_watershed: markers are int32 or int64 (marker_bytes 4 or 8, got %d)",
                marker_bytes);
    TEM_REQUIRE(((uintptr_t)ws & 15u) == 0, "tem_watershed: the workspace must be 16-byte aligned");
    const int64_t V = (int64_t)D * H * W, NV = V * N;
    if (ws_bytes < tem_watershed_ws(N, V)) {
        tem_set_error("tem_watershed: workspace too small (%lld bytes, %lld needed)", (long long)ws_bytes,
                      (long long)tem_watershed_ws(N, V));
        return TEM_EWS;
    }
    int* flags = (int*)ws;
    ws_u64* best = (ws_u64*)((char*)ws + tem_align_up(WS_FLAGS * sizeof(int), 16));
    int* comp = (int*)(best + NV);
    int* lab = comp + NV;
    int* nxt = lab + NV;
    const int grid = tem_grid_1d(NV, 256);
    const int rounds = ws_rounds(V), passes = ws_passes(V);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ws_init, dim3(grid), dim3(256), 0, st, markers, marker_bytes == 8 ? 1 : 0, mask, comp, lab, best, flags, V,
                       NV);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_ws_pick, dim3(grid), dim3(256), 0, st, rank, comp, lab, best, flags, r, D, H, W, NV);
        hipLaunchKernelGGL(k_ws_hook, dim3(grid), dim3(256), 0, st, order, comp, lab, best, nxt, flags, r, V, NV);
        for (int p = 0; p < passes; ++p)
            hipLaunchKernelGGL(k_ws_flatten, dim3(grid), dim3(256), 0, st, nxt, flags, r, p, V, NV);
        hipLaunchKernelGGL(k_ws_commit, dim3(grid), dim3(256), 0, st, comp, nxt, best, flags, r, V, NV);
    }
    hipLaunchKernelGGL(k_ws_write, dim3(grid), dim3(256), 0, st, comp, lab, out, flags, rounds_out, rounds, V, NV);
    TEM_CHECK_LAUNCH("tem_watershed");
    return TEM_OK;
}
