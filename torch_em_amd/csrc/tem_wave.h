// tem_wave.h -- the wave and block reductions of the kernels (included by tem_common.h).  A 64-lane butterfly, the keyed
// wave aggregate in front of an atomic, and the fixed-order block reduction are spelled here and nowhere else.
// Every helper is called by all 64 lanes of a wave (tem_block_reduce: by every thread of the block), converged.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>

__device__ __forceinline__ int tem_lane() { return threadIdx.x & 63; }

struct tem_op_sum {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct tem_op_min {   // the earlier operand stays on a tie, and when a compare with NaN is false
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct tem_op_max {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? b : a; }
};

// op over the 64 lanes, in every lane: lane i combines with lane i ^ 32, then ^ 16, ... ^ 1 (op(own, partner's)).
// T: int, unsigned, float, double, long long, unsigned long long; a 64-bit value is one __shfl_xor.
template <class T, class Op> __device__ __forceinline__ T tem_wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <class T> __device__ __forceinline__ T tem_wave_sum(T v) { return tem_wave_reduce(v, tem_op_sum()); }
template <class T> __device__ __forceinline__ T tem_wave_min(T v) { return tem_wave_reduce(v, tem_op_min()); }
template <class T> __device__ __forceinline__ T tem_wave_max(T v) { return tem_wave_reduce(v, tem_op_max()); }
__device__ __forceinline__ double tem_wave_sum_d(double v) { return tem_wave_sum(v); }

// The keyed aggregate: the active lanes are grouped by slot, and per_slot(s, mine, leader) runs once per distinct slot with
// the whole wave converged inside it -- s: the slot (wave-uniform), mine: this lane holds it, leader: the lane that sends
// the group's one atomic.  Slots are taken in the order of their first lane.  ROUNDS = 0: until no lane is pending, false
// is returned.  ROUNDS > 0: at most that many slots; true is returned in a lane that is still pending, which the caller
// then serves alone.  An inactive lane's slot is never looked at.
template <int ROUNDS, class F> __device__ __forceinline__ bool tem_wave_by_slot(long long slot, bool active, F&& per_slot) {
    unsigned long long pending = __ballot(active);
    for (int it = 0; (ROUNDS == 0 || it < ROUNDS) && pending; ++it) {
        const int leader = __ffsll((long long)pending) - 1;
        const long long s = __shfl(slot, leader, 64);
        const bool mine = active && slot == s;
        per_slot(s, mine, leader);
        pending &= ~__ballot(mine);
        if (mine) active = false;
    }
    return ROUNDS > 0 && active;
}

// dst[slot] (+=, max=, min=) val for every active lane: lanes that share a slot send one atomic.  Integer types only:
// the result does not depend on the grouping.
template <int ROUNDS, class T> __device__ __forceinline__ void tem_wave_atomic_add(T* dst, long long slot, bool active, T val) {
    if (tem_wave_by_slot<ROUNDS>(slot, active, [&](long long s, bool mine, int leader) {
            const T r = tem_wave_sum(mine ? val : T(0));
            if (tem_lane() == leader) atomicAdd(&dst[s], r);
        }))
        atomicAdd(&dst[slot], val);
}
template <int ROUNDS, class T> __device__ __forceinline__ void tem_wave_atomic_max(T* dst, long long slot, bool active, T val) {
    if (tem_wave_by_slot<ROUNDS>(slot, active, [&](long long s, bool mine, int leader) {
            const T r = tem_wave_max(mine ? val : std::numeric_limits<T>::lowest());
            if (tem_lane() == leader) atomicMax(&dst[s], r);
        }))
        atomicMax(&dst[slot], val);
}
template <int ROUNDS, class T> __device__ __forceinline__ void tem_wave_atomic_min(T* dst, long long slot, bool active, T val) {
    if (tem_wave_by_slot<ROUNDS>(slot, active, [&](long long s, bool mine, int leader) {
            const T r = tem_wave_min(mine ? val : std::numeric_limits<T>::max());
            if (tem_lane() == leader) atomicMin(&dst[s], r);
        }))
        atomicMin(&dst[slot], val);
}

// op over the NW * 64 threads of the block, in every thread, in a fixed order: the butterfly of each wave, then
// op(...op(op(sh[0], sh[1]), sh[2])..., sh[NW - 1]).  sh: NW words of LDS.  One barrier between the write of sh and its
// reads; LEAD_BARRIER adds one in front of the write, for a block that calls again while another wave may still read sh.
template <int NW, bool LEAD_BARRIER = false, class T, class Op>
__device__ __forceinline__ T tem_block_reduce(T v, T* sh, Op op) {
    v = tem_wave_reduce(v, op);
    if (LEAD_BARRIER) __syncthreads();
    if (tem_lane() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = op(r, sh[w]);
    return r;
}
