// patch.hip -- patch supply from volumes that live on the device (data/device_dataset.py; reference
// data/segmentation_dataset.py: _sample_bounding_box / _get_sample, data/sampler.py): judge candidate boxes, gather the
// accepted ones into the batch.
//
// Two device tables written by the host describe a call (include/tem_hip.h):
//   vols[V][6]  (int64): base pointer, dtype code (TEM_PT_*), C, D, H, W of a contiguous volume [C][D][H][W]
//   boxes[M][8] (int32): volume, z0, y0, x0, dz, dy, dx, 0 -- dz, dy, dx already clipped to the volume
// The kernels index with what the tables hold and check nothing: the HOST validates every box against its descriptor before
// a launch (ops.PatchVolumes.boxes).  All offsets are 64-bit (a 2048^3 volume is addressable); counts are int32 (a box holds
// fewer than 2^31 voxels).  Every accumulation is an integer add, so every result is bitwise reproducible.
//
// k_pt_count: one streaming pass over the boxes of a label volume.  A row of a box (dx elements along x) is contiguous; its
//   start is aligned to the element only (x0 and W are arbitrary), so the row is cut into the 16-byte ALIGNED chunks it
//   touches: a chunk that lies inside the row is one 16-byte load, the (at most two) chunks that straddle the row's ends are
//   read element by element -- nothing outside the row is loaded.  Work items are (row, chunk) pairs, consecutive lanes take
//   consecutive chunks (1 KiB per wave instruction).  Counts: lane -> wave (shuffles) -> workgroup (LDS) -> one atomicAdd per
//   workgroup and output word.
// k_pt_hist: histogram of DENSE int32 ids (0..n_ids-1) per box.  The box is walked in row-major voxel order, 64 consecutive
//   voxels per wave step.  Labels are spatially coherent, so a wave first finds its runs of equal ids (ballot on "differs from
//   the previous lane"; a run may continue over a row end) and only each run's first lane adds, the run length.  Where n_ids
//   fits the workgroup's LDS table (PT_LDS_IDS) the adds are LDS atomics and the table's non-zero entries are flushed to
//   global memory once; above that the run leaders add to global memory directly.
// k_pt_reduce_*: per box, the number of ids with enough voxels that are not masked out, or the counts of listed ids.
// k_pt_gather: boxes -> dense [B][C][pd][ph][pw] with dtype conversion and zeros where the box is smaller than the patch.
#include <limits.h>

#include "tem_common.h"

#define PT_LDS_IDS 8192   // ids of the LDS histogram: 32 KiB of the workgroup's 160 KiB

struct PtVol {
    const void* ptr;
    int64_t dtype, C, D, H, W;
};
static_assert(sizeof(PtVol) == 48, "vols is int64[V][6]");

struct PtBox {
    int vol, z0, y0, x0, dz, dy, dx, zero;
};

// one workgroup's (c0, c1) -> out[0], out[1]: all 256 threads call
__device__ __forceinline__ void pt_commit2(int c0, int c1, int* out) {
    __shared__ int part[4][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o, 64);
        c1 += __shfl_xor(c1, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = c0;
        part[threadIdx.x >> 6][1] = c1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s0 = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        const int s1 = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (s0) atomicAdd(out, s0);
        if (s1) atomicAdd(out + 1, s1);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pt_count(const PtVol* __restrict__ vols, const PtBox* __restrict__ boxes, int64_t value,
                                                  int* __restrict__ out) {
    constexpr int E = 16 / (int)sizeof(T);   // elements of one aligned chunk
    const int m = blockIdx.y;
    const PtBox b = boxes[m];
    const PtVol v = vols[b.vol];
    const T* base = (const T*)v.ptr;
    const int64_t H = v.H, W = v.W;
    const T first = base[((int64_t)b.z0 * H + b.y0) * W + b.x0];
    // a value the element type cannot hold equals no voxel
    const bool holds = (int64_t)(T)value == value;
    const T val = (T)value;
    const int nchunk = (b.dx + E - 1) / E + 1;   // >= the aligned chunks a row of dx elements can touch at any alignment
    const int64_t items = (int64_t)b.dz * b.dy * nchunk;
    int c0 = 0, c1 = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / nchunk;
        const int k = (int)(i - r * nchunk);
        const int z = (int)(r / b.dy), y = (int)(r - (int64_t)z * b.dy);
        const T* row = base + ((int64_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        const int head = (int)(((uintptr_t)row & 15) / sizeof(T));   // elements between the aligned address below and the row
        const int lo = k * E - head, hi = lo + E;                      // this chunk's elements, relative to the row
        if (lo >= 0 && hi <= b.dx) {
            union {
                uint4 q;
                T e[E];
            } u;
            u.q = *reinterpret_cast<const uint4*>(row + lo);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                c0 += (!holds || u.e[j] != val) ? 1 : 0;
                c1 += (u.e[j] != first) ? 1 : 0;
            }
        } else {
            const int a = lo < 0 ? 0 : lo, e = hi > b.dx ? b.dx : hi;
            for (int j = a; j < e; ++j) {
                const T t = row[j];
                c0 += (!holds || t != val) ? 1 : 0;
                c1 += (t != first) ? 1 : 0;
            }
        }
    }
    pt_commit2(c0, c1, out + 2 * m);
}

// one wave step of the histogram: `id` of this lane's voxel (-1: none); run leaders add their run's length to table[id]
__device__ __forceinline__ void pt_hist_step(int id, int lane, int n_ids, int* table) {
    const int prev = __shfl_up(id, 1, 64);
    const bool lead = lane == 0 || id != prev;
    const unsigned long long leaders = __ballot(lead);
    if (lead && (unsigned)id < (unsigned)n_ids) {   // also drops the run of voxel-less lanes
        const unsigned long long above = lane == 63 ? 0ull : leaders >> (lane + 1);
        const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
        atomicAdd(table + id, len);
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_pt_hist(const PtVol* __restrict__ vols, const PtBox* __restrict__ boxes, int n_ids,
                                                 int* __restrict__ hist) {
    __shared__ int tab[LDS ? PT_LDS_IDS : 1];
    const int m = blockIdx.y;
    const PtBox b = boxes[m];
    const PtVol v = vols[b.vol];
    const int* base = (const int*)v.ptr;
    const int64_t H = v.H, W = v.W;
    int* dst = hist + (int64_t)m * n_ids;
    if (LDS) {
        for (int i = threadIdx.x; i < n_ids; i += 256) tab[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int plane = b.dy * b.dx;
    const int64_t nvox = (int64_t)b.dz * plane;
    // every lane of a wave runs the same number of steps: the ballot needs them all
    for (int64_t w0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); w0 < nvox; w0 += (int64_t)gridDim.x * 256) {
        const int64_t i = w0 + lane;
        int id = -1;
        if (i < nvox) {
            const int z = (int)(i / plane);
            const int rem = (int)(i - (int64_t)z * plane);
            const int y = rem / b.dx, x = rem - y * b.dx;
            id = base[((int64_t)(b.z0 + z) * H + (b.y0 + y)) * W + (b.x0 + x)];
        }
        pt_hist_step(id, lane, n_ids, LDS ? tab : dst);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_ids; i += 256) {
            const int c = tab[i];
            if (c) atomicAdd(dst + i, c);
        }
    }
}

// out[m] = number of ids with hist[m][id] >= min_size (>= 1) and excluded[id] == 0; one workgroup per box, no atomics
__global__ __launch_bounds__(256) void k_pt_reduce_instances(const int* __restrict__ hist, int n_ids, const int* __restrict__ excluded,
                                                             int min_size, int* __restrict__ out) {
    __shared__ int part[4];
    const int m = blockIdx.x;
    const int* h = hist + (int64_t)m * n_ids;
    int c = 0;
    for (int i = threadIdx.x; i < n_ids; i += 256) c += (h[i] >= min_size && excluded[i] == 0) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[m] = part[0] + part[1] + part[2] + part[3];
}

// out[m][k] = hist[m][ids[k]] (0 for ids[k] < 0: a label the volumes do not hold)
__global__ __launch_bounds__(256) void k_pt_reduce_listed(const int* __restrict__ hist, int M, int n_ids, const int* __restrict__ ids,
                                                          int K, int* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * K) return;
    const int m = i / K, id = ids[i - m * K];
    out[i] = (unsigned)id < (unsigned)n_ids ? hist[(int64_t)m * n_ids + id] : 0;
}

template <typename TI>
__device__ __forceinline__ void pt_store(void* out, int out_dtype, int64_t o, TI t) {
    if (out_dtype == TEM_PT_F32) ((float*)out)[o] = (float)t;
    else if (out_dtype == TEM_PT_I32) ((int*)out)[o] = (int)t;
    else ((int64_t*)out)[o] = (int64_t)t;
}

// one output element per lane: plane blockIdx.y = b * C + c of the batch, elements of the plane along x first
template <typename TI>
__global__ __launch_bounds__(256) void k_pt_gather(const PtVol* __restrict__ vols, const PtBox* __restrict__ boxes, int C, int pd, int ph,
                                                   int pw, void* __restrict__ out, int out_dtype) {
    const int bi = blockIdx.y / C, c = blockIdx.y - bi * C;
    const PtBox b = boxes[bi];
    const PtVol v = vols[b.vol];
    const TI* base = (const TI*)v.ptr + (int64_t)c * v.D * v.H * v.W;
    const int64_t H = v.H, W = v.W;
    const int n = pd * ph * pw;
    const int64_t o0 = (int64_t)blockIdx.y * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int x = i % pw, t = i / pw;
        const int y = t % ph, z = t / ph;
        TI val = (TI)0;
        if (z < b.dz && y < b.dy && x < b.dx) val = base[((int64_t)(b.z0 + z) * H + (b.y0 + y)) * W + (b.x0 + x)];
        pt_store<TI>(out, out_dtype, o0 + i, val);
    }
}

static int pt_box_grid(int64_t max_vox, int per_thread) {
    int64_t g = tem_cdiv(max_vox, (int64_t)256 * per_thread);
    return (int)(g < 1 ? 1 : g > 128 ? 128 : g);
}

extern "C" int tem_patch_count(const void* vols, const int32_t* boxes, int M, int dtype, int64_t max_vox, int64_t value,
                               int32_t* out, tem_stream_t stream) {
    TEM_REQUIRE(vols && boxes && out, "tem_patch_count: null pointer");
    TEM_REQUIRE(M > 0 && M <= 65535 && max_vox > 0 && max_vox < INT_MAX, "tem_patch_count: 1..65535 boxes of 1..2^31-1 voxels");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)M * 2 * sizeof(int), st) != hipSuccess) {
        tem_set_error("tem_patch_count: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    const dim3 grid(pt_box_grid(max_vox, 16), M), block(256);
    const PtVol* pv = (const PtVol*)vols;
    const PtBox* pb = (const PtBox*)boxes;
    switch (dtype) {
        case TEM_PT_U8: hipLaunchKernelGGL(k_pt_count<uint8_t>, grid, block, 0, st, pv, pb, value, out); break;
        case TEM_PT_U16: hipLaunchKernelGGL(k_pt_count<uint16_t>, grid, block, 0, st, pv, pb, value, out); break;
        case TEM_PT_I32: hipLaunchKernelGGL(k_pt_count<int32_t>, grid, block, 0, st, pv, pb, value, out); break;
        case TEM_PT_I64: hipLaunchKernelGGL(k_pt_count<int64_t>, grid, block, 0, st, pv, pb, value, out); break;
        default: TEM_REQUIRE(false, "tem_patch_count: labels are uint8, uint16, int32 or int64 (got dtype code %d)", dtype);
    }
    TEM_CHECK_LAUNCH("tem_patch_count");
    return TEM_OK;
}

extern "C" int tem_patch_hist_path(int n_ids) { return n_ids < 1 ? -1 : n_ids <= PT_LDS_IDS ? 0 : 1; }

extern "C" int tem_patch_hist(const void* vols, const int32_t* boxes, int M, int64_t max_vox, int n_ids, int32_t* hist,
                              tem_stream_t stream) {
    TEM_REQUIRE(vols && boxes && hist, "tem_patch_hist: null pointer");
    TEM_REQUIRE(M > 0 && M <= 65535 && max_vox > 0 && max_vox < INT_MAX && n_ids > 0,
                "tem_patch_hist: 1..65535 boxes of 1..2^31-1 voxels, n_ids >= 1");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)M * n_ids * sizeof(int), st) != hipSuccess) {
        tem_set_error("tem_patch_hist: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    // few workgroups per box with long walks: each flushes its table (or its runs) once, so the global adds per id and box
    // are bounded by the grid's x extent
    const dim3 grid(pt_box_grid(max_vox, 128), M), block(256);
    if (tem_patch_hist_path(n_ids) == 0)
        hipLaunchKernelGGL(k_pt_hist<true>, grid, block, 0, st, (const PtVol*)vols, (const PtBox*)boxes, n_ids, hist);
    else
        hipLaunchKernelGGL(k_pt_hist<false>, grid, block, 0, st, (const PtVol*)vols, (const PtBox*)boxes, n_ids, hist);
    TEM_CHECK_LAUNCH("tem_patch_hist");
    return TEM_OK;
}

extern "C" int tem_patch_hist_reduce(const int32_t* hist, int M, int n_ids, int mode, const int32_t* sel, int K, int min_size,
                                     int32_t* out, tem_stream_t stream) {
    TEM_REQUIRE(hist && sel && out, "tem_patch_hist_reduce: null pointer");
    TEM_REQUIRE(M > 0 && M <= 65535 && n_ids > 0 && (mode == 0 || (mode == 1 && K > 0 && (int64_t)M * K < INT_MAX)),
                "tem_patch_hist_reduce: mode 0 (instances) or 1 (K >= 1 listed ids), 1..65535 boxes");
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0)
        hipLaunchKernelGGL(k_pt_reduce_instances, dim3(M), dim3(256), 0, st, hist, n_ids, sel, min_size < 1 ? 1 : min_size, out);
    else
        hipLaunchKernelGGL(k_pt_reduce_listed, dim3((unsigned)tem_cdiv((int64_t)M * K, 256)), dim3(256), 0, st, hist, M, n_ids, sel, K, out);
    TEM_CHECK_LAUNCH("tem_patch_hist_reduce");
    return TEM_OK;
}

extern "C" int tem_patch_gather(const void* vols, const int32_t* boxes, int B, int C, int in_dtype, int pd, int ph, int pw,
                                void* out, int out_dtype, tem_stream_t stream) {
    TEM_REQUIRE(vols && boxes && out, "tem_patch_gather: null pointer");
    TEM_REQUIRE(B > 0 && C > 0 && (int64_t)B * C <= 65535 && pd > 0 && ph > 0 && pw > 0 && (int64_t)pd * ph * pw < INT_MAX,
                "tem_patch_gather: B * C in 1..65535 planes of 1..2^31-1 voxels");
    TEM_REQUIRE(out_dtype == TEM_PT_F32 || out_dtype == TEM_PT_I32 || out_dtype == TEM_PT_I64,
                "tem_patch_gather: the batch is float32, int32 or int64 (got dtype code %d)", out_dtype);
    TEM_REQUIRE(in_dtype != TEM_PT_F32 || out_dtype == TEM_PT_F32, "tem_patch_gather: float32 volumes gather to float32 only");
    hipStream_t st = (hipStream_t)stream;
    const int n = pd * ph * pw;
    const dim3 grid((unsigned)tem_grid_1d(n, 256, 1024), (unsigned)(B * C)), block(256);
    const PtVol* pv = (const PtVol*)vols;
    const PtBox* pb = (const PtBox*)boxes;
    switch (in_dtype) {
        case TEM_PT_U8: hipLaunchKernelGGL(k_pt_gather<uint8_t>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        case TEM_PT_U16: hipLaunchKernelGGL(k_pt_gather<uint16_t>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        case TEM_PT_I16: hipLaunchKernelGGL(k_pt_gather<int16_t>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        case TEM_PT_I32: hipLaunchKernelGGL(k_pt_gather<int32_t>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        case TEM_PT_I64: hipLaunchKernelGGL(k_pt_gather<int64_t>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        case TEM_PT_F32: hipLaunchKernelGGL(k_pt_gather<float>, grid, block, 0, st, pv, pb, C, pd, ph, pw, out, out_dtype); break;
        default: TEM_REQUIRE(false, "tem_patch_gather: unknown volume dtype code %d", in_dtype);
    }
    TEM_CHECK_LAUNCH("tem_patch_gather");
    return TEM_OK;
}
