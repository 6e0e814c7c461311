// mws.hip -- the mutex watershed on the device: Kruskal with mutex constraints over the affinity graph of a volume,
// computed by rounds that commit, in parallel, exactly the edges whose sequential decision is already certain.  Integer
// compares only; the result does not depend on the execution order.
//
// The contract (DESIGN.md "Mutex watershed"): edge (c, v) joins voxel v and u = v + offsets[c] when u is inside the sample,
// both ends are inside the mask and edge_valid[c][v] is set; its id is c * V + v.  Its priority is p = 1 - aff for the
// n_attractive leading channels and p = aff for the others (float32, -0.0 tied with 0.0); edges are taken by p descending,
// ties by the lower id -- as one 64-bit key: the order-preserving uint32 of p << 32 | 0xffffffff - id, the larger key first.
// Keys are pairwise distinct, never 0, and decode to their edge.
//
// State (workspace of tem_mws_ws bytes): per voxel comp (the flat root, sample-local, -1 outside the mask), nxt (the parent
// forest of a round), best (uint64 at roots: the largest key of an open edge that touches the cluster; 0: none), has (a
// byte at roots: the cluster has a mutex), veto (a byte at roots: R3 is off this round); per edge one byte: open, mutex or dead.  The mutex set: an open-addressing hash
// set of uint64 root pairs, rebuilt every round from the edges in state mutex, at most half full.
// One round = mutex (every mutex edge inserts the pair of its ends' roots and flags both), pick (an open edge whose ends or are mutually exclusive dies for good; any other atomicMaxes its key into best of both roots), hook (at
// share a root or are mutually exclusive dies for good; any other atomicMaxes its key into best of both roots), veto (every
// mutex edge (X, Y) asks for both ends: is the cluster X's best edge leads to mutually exclusive with Y?  if not, X is
// vetoed), hook (at every root A with best = e = (A, B): R1 e repulsive -> e becomes a mutex edge; R2 e attractive and B's
// best too -> the larger root hooks to the smaller, e dies; R3 e attractive and A not vetoed -- A has no mutex, or every
// mutex partner of A is one of B as well -> A hooks to B), MWS_PASSES(V) flatten passes as in watershed.hip, commit
// (comp = nxt; best, has, veto and the set are reset).  DESIGN.md has the argument why every
// one of these decisions is the sequential one.
// The number of rounds depends on the data: tem_mws_run enqueues a batch of rounds, every round reads the flag the previous
// one's pick wrote and returns at once when nothing was picked, and the caller reads two ints back per batch.  No loop -- on
// the host or in a kernel -- waits for a condition: the probe loops are bounded by the table size.
#include <limits.h>

#include "tem_common.h"

#define MWS_EMPTY 0xffffffffffffffffull
#define MWS_OPEN 1
#define MWS_MUTEX 2
#define MWS_DEAD 0
#define MWS_CHASE 256          // steps of one chase
#define MWS_CHASE_LOG2 8
#define MWS_MAX_PASSES 4       // ceil(31 / MWS_CHASE_LOG2)
#define MWS_WAVE_ROOTS 4       // distinct roots a wave reduces before its lanes fall back to one atomic each
// the head of the workspace, in ints: [0..1] valid edges (uint64), [2..3] valid repulsive edges (uint64), [4] working
// rounds so far, [5] the last round of the last batch did work, [6] unused, [7] did[0] = the carry into the batch, then
// did[1 + i] of round i, then deep[i][pass]
#define MWS_H_WORK 4
#define MWS_H_ALIVE 5
#define MWS_H_DID 7
#define MWS_H_DEEP (MWS_H_DID + 1 + TEM_MWS_MAX_BATCH)
#define MWS_H_INTS (MWS_H_DEEP + TEM_MWS_MAX_BATCH * MWS_MAX_PASSES)

typedef unsigned long long mws_u64;

struct MwsGeom {
    int D, H, W, C, n_attr;
    int off[TEM_MWS_MAX_CHANNELS][3];   // (dz, dy, dx)
};

static int mws_log2_ceil(int64_t V) {
    int l = 0;
    while (((int64_t)1 << l) < V) ++l;
    return l;
}
static int mws_passes(int64_t V) {
    const int p = (mws_log2_ceil(V) + MWS_CHASE_LOG2 - 1) / MWS_CHASE_LOG2;
    return p < 1 ? 1 : p;
}

__device__ __forceinline__ int mws_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mws_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the far end of edge (c, v): its sample-local index, or -1 outside the sample
__device__ __forceinline__ int mws_far(const MwsGeom& g, int c, unsigned v) {
    const int HW = g.H * g.W;
    const int x = (int)(v % (unsigned)g.W) + g.off[c][2], y = (int)((v / (unsigned)g.W) % (unsigned)g.H) + g.off[c][1],
              z = (int)(v / (unsigned)HW) + g.off[c][0];
    if (x < 0 || x >= g.W || y < 0 || y >= g.H || z < 0 || z >= g.D) return -1;
    return z * HW + y * g.W + x;
}

// a batch edge index E = (n * C + c) * V + v -> channel, voxel and the sample's first voxel index in the batch
__device__ __forceinline__ void mws_edge(int64_t E, int C, int64_t V, int& c, unsigned& v, int64_t& base) {
    const int64_t nc = E / V;
    v = (unsigned)(E - nc * V);
    c = (int)(nc % C);
    base = (nc / C) * V;
}

__device__ __forceinline__ mws_u64 mws_key(float aff, bool attractive, unsigned id) {
    float p = attractive ? 1.0f - aff : aff;
    if (p == 0.0f) p = 0.0f;   // -0.0 ties with 0.0
    const unsigned b = __builtin_bit_cast(unsigned, p);
    const unsigned o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((mws_u64)o << 32) | (mws_u64)(0xffffffffu - id);
}

// two sample-local roots -> the set's key: (batch index of the smaller << 31) | the larger; N * V < 2^33 - 1 keeps it off MWS_EMPTY
__device__ __forceinline__ mws_u64 mws_pair(int64_t base, int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return ((mws_u64)(base + lo) << 31) | (mws_u64)(unsigned)hi;
}
__device__ __forceinline__ uint64_t mws_hash(mws_u64 k) {   // the finaliser of splitmix64
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

__device__ __forceinline__ mws_u64 mws_wave_max(mws_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const mws_u64 w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ mws_u64 mws_wave_sum(mws_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_mws_init_voxels(const uint8_t* __restrict__ mask, int* __restrict__ comp, mws_u64* __restrict__ best,
                                                         uint8_t* __restrict__ has, uint8_t* __restrict__ veto, int* __restrict__ head,
                                                         int64_t V, int64_t NV) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < MWS_H_INTS; i += 256) head[i] = 0;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const bool in = mask == nullptr || mask[g] != 0;
        comp[g] = in ? (int)(g % V) : -1;
        best[g] = 0;
        has[g] = 0;
        veto[g] = 0;
    }
}

// after k_mws_init_voxels (it zeroes the counters): the state of every edge, and the counts of the existing ones
__global__ __launch_bounds__(256) void k_mws_init_edges(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ edge_valid,
                                                        uint8_t* __restrict__ state, int* head, MwsGeom geo, int64_t V, int64_t NE) {
    mws_u64 n_all = 0, n_rep = 0;
    for (int64_t E = (int64_t)blockIdx.x * 256 + threadIdx.x; E < NE; E += (int64_t)gridDim.x * 256) {
        int c;
        unsigned v;
        int64_t base;
        mws_edge(E, geo.C, V, c, v, base);
        const int u = mws_far(geo, c, v);
        bool ok = u >= 0 && (edge_valid == nullptr || edge_valid[E] != 0);
        if (ok && mask != nullptr) ok = mask[base + v] != 0 && mask[base + u] != 0;
        state[E] = ok ? MWS_OPEN : MWS_DEAD;
        n_all += ok ? 1 : 0;
        n_rep += (ok && c >= geo.n_attr) ? 1 : 0;
    }
    n_all = mws_wave_sum(n_all);
    n_rep = mws_wave_sum(n_rep);
    if ((threadIdx.x & 63) == 0) {
        if (n_all) atomicAdd((mws_u64*)head, n_all);
        if (n_rep) atomicAdd((mws_u64*)head + 1, n_rep);
    }
}

__global__ __launch_bounds__(256) void k_mws_clear(mws_u64* __restrict__ table, int64_t slots) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) table[i] = MWS_EMPTY;
}

// one block: the carry into the batch and clean flags.  first: the call's first batch, whose first round always runs.
__global__ __launch_bounds__(256) void k_mws_batch_begin(int* head, int first) {
    const int carry = first ? 1 : head[MWS_H_ALIVE];
    __syncthreads();
    for (int i = MWS_H_DID + threadIdx.x; i < MWS_H_INTS; i += 256) head[i] = (i == MWS_H_DID) ? carry : 0;
}

// one block, one thread: the working rounds so far and whether the batch's last round was one of them
__global__ void k_mws_batch_end(int* head, int rounds) {
    int n = 0;
    for (int i = 1; i <= rounds; ++i) n += head[MWS_H_DID + i];
    head[MWS_H_WORK] += n;
    head[MWS_H_ALIVE] = head[MWS_H_DID + rounds];
}

__global__ __launch_bounds__(256) void k_mws_mutex(const uint8_t* __restrict__ state, const int* __restrict__ comp, uint8_t* has,
                                                   mws_u64* table, int64_t slots, const int* __restrict__ did, int round, MwsGeom geo,
                                                   int64_t V, int64_t NE) {
    if (did[round] == 0) return;
    const uint64_t hmask = (uint64_t)slots - 1;
    for (int64_t E = (int64_t)blockIdx.x * 256 + threadIdx.x; E < NE; E += (int64_t)gridDim.x * 256) {
        if (state[E] != MWS_MUTEX) continue;
        int c;
        unsigned v;
        int64_t base;
        mws_edge(E, geo.C, V, c, v, base);
        const int u = mws_far(geo, c, v);
        if (u < 0) continue;   // cannot happen: a mutex edge exists
        const int A = comp[base + v], B = comp[base + u];
        if (A < 0 || B < 0 || A == B) continue;   // cannot happen: mutually exclusive clusters never merge
        has[base + A] = 1;
        has[base + B] = 1;
        const mws_u64 k = mws_pair(base, A, B);
        uint64_t h = mws_hash(k) & hmask;
        for (int64_t i = 0; i < slots; ++i) {   // the set is at most half full: an empty slot comes long before the bound
            mws_u64 cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == MWS_EMPTY) cur = atomicCAS(&table[h], MWS_EMPTY, k);
            if (cur == MWS_EMPTY || cur == k) break;
            h = (h + 1) & hmask;
        }
    }
}

__device__ __forceinline__ bool mws_in_set(const mws_u64* __restrict__ table, int64_t slots, mws_u64 k) {
    const uint64_t hmask = (uint64_t)slots - 1;
    uint64_t h = mws_hash(k) & hmask;
    for (int64_t i = 0; i < slots; ++i) {
        const mws_u64 cur = table[h];
        if (cur == k) return true;
        if (cur == MWS_EMPTY) return false;
        h = (h + 1) & hmask;
    }
    return false;
}

// all 64 lanes of a wave: atomicMax(best[slot], key) of the active lanes, lanes that share a slot reduced to one atomic
__device__ __forceinline__ void mws_offer(mws_u64* best, int64_t slot, mws_u64 key, bool active) {
    mws_u64* p = best + (active ? slot : 0);
    // an older (smaller) value may be read here: then the atomic below is merely not spared
    if (active && key <= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) active = false;
    for (int it = 0; it < MWS_WAVE_ROOTS; ++it) {
        const mws_u64 ballot = __ballot(active);
        if (ballot == 0) break;
        const int leader = __ffsll((long long)ballot) - 1;
        const int64_t lslot = __shfl((long long)slot, leader, 64);
        const bool mine = active && slot == lslot;
        const mws_u64 mm = mws_wave_max(mine ? key : 0);
        if ((threadIdx.x & 63) == leader) atomicMax(p, mm);
        if (mine) active = false;
    }
    if (active) atomicMax(p, key);
}

__global__ __launch_bounds__(256) void k_mws_pick(const float* __restrict__ aff, uint8_t* __restrict__ state, const int* __restrict__ comp,
                                                  const uint8_t* __restrict__ has, const mws_u64* __restrict__ table, int64_t slots,
                                                  mws_u64* best, int* did, int round, MwsGeom geo, int64_t V, int64_t NE) {
    if (did[round] == 0) return;
    const int64_t span = (int64_t)gridDim.x * 256;
    bool any = false;
    // every lane of a wave makes the same number of trips: the wave reduction needs all 64
    for (int64_t E0 = (int64_t)blockIdx.x * 256; E0 < NE; E0 += span) {
        const int64_t E = E0 + threadIdx.x;
        mws_u64 key = 0;
        int64_t sa = 0, sb = 0;
        if (E < NE && state[E] == MWS_OPEN) {
            int c;
            unsigned v;
            int64_t base;
            mws_edge(E, geo.C, V, c, v, base);
            const int u = mws_far(geo, c, v);
            const int A = comp[base + v], B = u < 0 ? -1 : comp[base + u];
            // A, B >= 0: an open edge exists, so both of its ends are inside the sample and the mask
            if (A < 0 || B < 0 || A == B || (has[base + A] && has[base + B] && mws_in_set(table, slots, mws_pair(base, A, B)))) {
                state[E] = MWS_DEAD;
            } else {
                key = mws_key(aff[E], c < geo.n_attr, (unsigned)c * (unsigned)V + v);
                sa = base + A;
                sb = base + B;
            }
        }
        const bool active = key != 0;
        any = any || active;
        mws_offer(best, sa, key, active);
        mws_offer(best, sb, key, active);
    }
    // one word for the whole grid: stores to one address queue up behind each other, so a block stores only while it reads 0
    if (__syncthreads_or(any) && threadIdx.x == 0 && mws_ld(&did[round + 1]) == 0) mws_st(&did[round + 1], 1);
}

// the edge a root's best key names: its channel and voxel, and the root b of the end that is not in cluster a (row = comp of
// the sample); false when the key names no edge of a -- which cannot happen for a key a pick of this round wrote
__device__ __forceinline__ bool mws_decode(mws_u64 k, const MwsGeom& geo, int64_t V, const int* __restrict__ row, int a, int& c,
                                           unsigned& v, int& b) {
    const unsigned id = 0xffffffffu - (unsigned)(k & 0xffffffffu);
    c = (int)(id / (unsigned)V);
    v = id % (unsigned)V;
    const int u = c < geo.C ? mws_far(geo, c, v) : -1;
    if (u < 0) return false;
    const int x = row[v], y = row[u];
    b = x == a ? y : x;
    return b >= 0 && b != a && (x == a || y == a);
}

// R3 lets a root A hook along its best edge e = (A, B) before e's turn.  That is the sequential decision when no mutex
// partner C of A can be in B's cluster by then -- certain when B and C are mutually exclusive already.  Every mutex edge
// (X, Y) checks this for X with partner Y and for Y with partner X; a root that fails once is vetoed for the round.
__global__ __launch_bounds__(256) void k_mws_veto(const uint8_t* __restrict__ state, const int* __restrict__ comp,
                                                  const mws_u64* __restrict__ best, const mws_u64* __restrict__ table, int64_t slots,
                                                  uint8_t* veto, const int* __restrict__ did, int round, MwsGeom geo, int64_t V,
                                                  int64_t NE) {
    if (did[round + 1] == 0) return;
    for (int64_t E = (int64_t)blockIdx.x * 256 + threadIdx.x; E < NE; E += (int64_t)gridDim.x * 256) {
        if (state[E] != MWS_MUTEX) continue;
        int c;
        unsigned v;
        int64_t base;
        mws_edge(E, geo.C, V, c, v, base);
        const int u = mws_far(geo, c, v);
        if (u < 0) continue;   // cannot happen: a mutex edge exists
        const int* row = comp + base;
        const int X = row[v], Y = row[u];
        if (X < 0 || Y < 0 || X == Y) continue;   // cannot happen
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int a = side ? Y : X, partner = side ? X : Y;
            const mws_u64 k = best[base + a];
            if (k == 0 || veto[base + a]) continue;
            int c2, b;
            unsigned v2;
            if (!mws_decode(k, geo, V, row, a, c2, v2, b) || c2 >= geo.n_attr) continue;
            if (b == partner || !mws_in_set(table, slots, mws_pair(base, b, partner))) veto[base + a] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_mws_hook(const int* __restrict__ comp, const mws_u64* __restrict__ best,
                                                  const uint8_t* __restrict__ veto, uint8_t* state, int* __restrict__ nxt,
                                                  const int* __restrict__ did, int round, MwsGeom geo, int64_t V, int64_t NV) {
    if (did[round + 1] == 0) return;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        int p = comp[g];
        if (p < 0) {
            nxt[g] = -1;   // the flatten passes read every entry
            continue;
        }
        const int64_t n = g / V, base = n * V;
        const int a = (int)(g - base);
        const mws_u64 k = p == a ? best[g] : 0;
        int c, b;
        unsigned v;
        if (k != 0 && mws_decode(k, geo, V, comp + base, a, c, v, b)) {
            const int64_t E = (n * geo.C + c) * V + v;
            if (c >= geo.n_attr) {
                state[E] = MWS_MUTEX;                          // R1
            } else if (best[base + b] == k) {
                state[E] = MWS_DEAD;                           // R2: the larger root hooks to the smaller
                if (a > b) p = b;
            } else if (!veto[g]) {
                p = b;                                         // R3
            }
        }
        nxt[g] = p;
    }
}

// every voxel moves up to MWS_CHASE steps towards its root; a value read while other lanes write is an ancestor as well
__global__ __launch_bounds__(256) void k_mws_flatten(int* nxt, int* head, int round, int pass, int64_t V, int64_t NV) {
    if (head[MWS_H_DID + round + 1] == 0) return;
    int* deep = head + MWS_H_DEEP + round * MWS_MAX_PASSES;
    if (pass > 0 && deep[pass - 1] == 0) return;
    bool open = false;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        int x = mws_ld(&nxt[g]);
        if (x < 0) continue;
        int* row = nxt + (g / V) * V;
        bool flat = false;
        for (int s = 0; s < MWS_CHASE; ++s) {
            const int y = mws_ld(&row[x]);
            if (y == x || y < 0) {
                flat = true;
                break;
            }
            x = y;
        }
        open = open || !flat;
        mws_st(&nxt[g], x);
    }
    if (__syncthreads_or(open) && threadIdx.x == 0 && mws_ld(&deep[pass]) == 0) mws_st(&deep[pass], 1);
}

// comp = nxt; best, has and veto reset at the old roots, the set emptied for the next round
__global__ __launch_bounds__(256) void k_mws_commit(int* __restrict__ comp, const int* __restrict__ nxt, mws_u64* __restrict__ best,
                                                    uint8_t* __restrict__ has, uint8_t* __restrict__ veto,
                                                    mws_u64* __restrict__ table, int64_t slots,
                                                    const int* __restrict__ did, int round, int64_t V, int64_t NV) {
    if (did[round + 1] == 0) return;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int old = comp[g];
        if (old < 0) continue;
        if (old == (int)(g % V)) {
            if (best[g] != 0) best[g] = 0;
            if (has[g]) has[g] = 0;
            if (veto[g]) veto[g] = 0;
        }
        comp[g] = nxt[g];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256)
        if (table[i] != MWS_EMPTY) table[i] = MWS_EMPTY;
}

// the labels: first[root] = the smallest voxel of the cluster (in nxt), out = first + 1 inside the mask, 0 outside
__global__ __launch_bounds__(256) void k_mws_first_init(int* __restrict__ nxt, int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) nxt[g] = (int)(g % V);
}
__global__ __launch_bounds__(256) void k_mws_first_min(const int* __restrict__ comp, int* nxt, int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int r = comp[g];
        const int v = (int)(g % V);
        if (r >= 0 && v < r) atomicMin(&nxt[g - v + r], v);
    }
}
__global__ __launch_bounds__(256) void k_mws_write(const int* __restrict__ comp, const int* __restrict__ nxt, int* __restrict__ out,
                                                   int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int r = comp[g];
        out[g] = r < 0 ? 0 : nxt[g - g % V + r] + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
struct MwsWs {
    int* head;
    mws_u64* best;
    int *comp, *nxt;
    uint8_t *has, *veto, *state;
};

static bool mws_shape_ok(int N, int C, int D, int H, int W) {
    if (N <= 0 || C <= 0 || C > TEM_MWS_MAX_CHANNELS || D <= 0 || H <= 0 || W <= 0) return false;
    const int64_t V = (int64_t)D * H * W;
    return V < INT_MAX && (int64_t)C * V < 0xffffffffll && (int64_t)N * V < (((int64_t)1 << 33) - 1);
}

static int64_t mws_head_bytes() { return tem_align_up(MWS_H_INTS * sizeof(int), 16); }

extern "C" int64_t tem_mws_ws(int N, int C, int D, int H, int W) {
    if (!mws_shape_ok(N, C, D, H, W)) return -1;
    const int64_t NV = (int64_t)N * D * H * W;
    return mws_head_bytes() + NV * 16 + 2 * tem_align_up(NV, 16) + tem_align_up(NV * C, 16);
}

extern "C" int64_t tem_mws_table_slots(int64_t n_repulsive) {
    if (n_repulsive < 0 || n_repulsive > ((int64_t)1 << 40)) return -1;
    int64_t s = 64;
    while (s < 2 * n_repulsive) s <<= 1;
    return s;
}

static MwsWs mws_carve(void* ws, int64_t NV) {
    MwsWs w;
    w.head = (int*)ws;
    w.best = (mws_u64*)((char*)ws + mws_head_bytes());
    w.comp = (int*)(w.best + NV);
    w.nxt = w.comp + NV;
    w.has = (uint8_t*)(w.nxt + NV);
    w.veto = w.has + tem_align_up(NV, 16);
    w.state = w.veto + tem_align_up(NV, 16);
    return w;
}

static int mws_geom(MwsGeom& g, const char* who, const int* offsets, int n_attractive, int N, int C, int D, int H, int W, const void* ws,
                    int64_t ws_bytes) {
    TEM_REQUIRE(offsets && ws, "%s: null pointer", who);
    TEM_REQUIRE(mws_shape_ok(N, C, D, H, W),
                "%s: bad shape (N, C, D, H, W positive, C at most %d, D*H*W below 2^31 - 1, C*D*H*W below 2^32 - 1, N*D*H*W below 2^33 - 1)",
                who, TEM_MWS_MAX_CHANNELS);
    TEM_REQUIRE(n_attractive >= 0 && n_attractive <= C, "%s: n_attractive %d outside 0..%d", who, n_attractive, C);
    TEM_REQUIRE(((uintptr_t)ws & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);
    if (ws_bytes < tem_mws_ws(N, C, D, H, W)) {
        tem_set_error("%s: workspace too small (%lld bytes, %lld needed)", who, (long long)ws_bytes, (long long)tem_mws_ws(N, C, D, H, W));
        return TEM_EWS;
    }
    g.D = D, g.H = H, g.W = W, g.C = C, g.n_attr = n_attractive;
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < 3; ++k) {
            const int o = offsets[c * 3 + k];
            TEM_REQUIRE(o > -(1 << 30) && o < (1 << 30), "%s: offset %d of channel %d is out of range", who, o, c);
            g.off[c][k] = o;
        }
    return TEM_OK;
}

extern "C" int tem_mws_init(const uint8_t* mask, const uint8_t* edge_valid, const int* offsets, int n_attractive, int N, int C, int D,
                            int H, int W, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    MwsGeom geo;
    TEM_TRY(mws_geom(geo, "tem_mws_init", offsets, n_attractive, N, C, D, H, W, ws, ws_bytes));
    const int64_t V = (int64_t)D * H * W, NV = V * N, NE = NV * C;
    const MwsWs w = mws_carve(ws, NV);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mws_init_voxels, dim3(tem_grid_1d(NV, 256)), dim3(256), 0, st, mask, w.comp, w.best, w.has, w.veto, w.head, V, NV);
    hipLaunchKernelGGL(k_mws_init_edges, dim3(tem_grid_1d(NE, 256)), dim3(256), 0, st, mask, edge_valid, w.state, w.head, geo, V, NE);
    TEM_CHECK_LAUNCH("tem_mws_init");
    return TEM_OK;
}

extern "C" int tem_mws_run(const float* aff, const int* offsets, int n_attractive, int N, int C, int D, int H, int W, void* ws,
                           int64_t ws_bytes, uint64_t* table, int64_t slots, int first, int rounds, tem_stream_t stream) {
    MwsGeom geo;
    TEM_TRY(mws_geom(geo, "tem_mws_run", offsets, n_attractive, N, C, D, H, W, ws, ws_bytes));
    TEM_REQUIRE(aff && table, "tem_mws_run: null pointer");
    TEM_REQUIRE(slots >= 64 && (slots & (slots - 1)) == 0, "tem_mws_run: the table has a power of two of slots, at least 64 (got %lld)",
                (long long)slots);
    TEM_REQUIRE(rounds >= 1 && rounds <= TEM_MWS_MAX_BATCH, "tem_mws_run: 1..%d rounds a call (got %d)", TEM_MWS_MAX_BATCH, rounds);
    const int64_t V = (int64_t)D * H * W, NV = V * N, NE = NV * C;
    const MwsWs w = mws_carve(ws, NV);
    int* did = w.head + MWS_H_DID;
    mws_u64* tab = (mws_u64*)table;
    const int gv = tem_grid_1d(NV, 256), ge = tem_grid_1d(NE, 256);
    const int passes = mws_passes(V);
    hipStream_t st = (hipStream_t)stream;
    if (first) hipLaunchKernelGGL(k_mws_clear, dim3(tem_grid_1d(slots, 256)), dim3(256), 0, st, tab, slots);
    hipLaunchKernelGGL(k_mws_batch_begin, dim3(1), dim3(256), 0, st, w.head, first ? 1 : 0);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_mws_mutex, dim3(ge), dim3(256), 0, st, w.state, w.comp, w.has, tab, slots, did, r, geo, V, NE);
        hipLaunchKernelGGL(k_mws_pick, dim3(ge), dim3(256), 0, st, aff, w.state, w.comp, w.has, tab, slots, w.best, did, r, geo, V, NE);
        hipLaunchKernelGGL(k_mws_veto, dim3(ge), dim3(256), 0, st, w.state, w.comp, w.best, tab, slots, w.veto, did, r, geo, V, NE);
        hipLaunchKernelGGL(k_mws_hook, dim3(gv), dim3(256), 0, st, w.comp, w.best, w.veto, w.state, w.nxt, did, r, geo, V, NV);
        for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(k_mws_flatten, dim3(gv), dim3(256), 0, st, w.nxt, w.head, r, p, V, NV);
        hipLaunchKernelGGL(k_mws_commit, dim3(gv), dim3(256), 0, st, w.comp, w.nxt, w.best, w.has, w.veto, tab, slots, did, r, V, NV);
    }
    hipLaunchKernelGGL(k_mws_batch_end, dim3(1), dim3(1), 0, st, w.head, rounds);
    TEM_CHECK_LAUNCH("tem_mws_run");
    return TEM_OK;
}

extern "C" int tem_mws_labels(int* out, int N, int C, int D, int H, int W, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(out && ws, "tem_mws_labels: null pointer");
    TEM_REQUIRE(mws_shape_ok(N, C, D, H, W), "tem_mws_labels: bad shape");
    TEM_REQUIRE(((uintptr_t)ws & 15u) == 0, "tem_mws_labels: the workspace must be 16-byte aligned");
    TEM_REQUIRE(ws_bytes >= tem_mws_ws(N, C, D, H, W), "tem_mws_labels: workspace too small");
    const int64_t V = (int64_t)D * H * W, NV = V * N;
    const MwsWs w = mws_carve(ws, NV);
    const int gv = tem_grid_1d(NV, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mws_first_init, dim3(gv), dim3(256), 0, st, w.nxt, V, NV);
    hipLaunchKernelGGL(k_mws_first_min, dim3(gv), dim3(256), 0, st, w.comp, w.nxt, V, NV);
    hipLaunchKernelGGL(k_mws_write, dim3(gv), dim3(256), 0, st, w.comp, w.nxt, out, V, NV);
    TEM_CHECK_LAUNCH("tem_mws_labels");
    return TEM_OK;
}
