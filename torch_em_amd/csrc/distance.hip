// distance.hip -- distance-based instance segmentation on device:
//   * PerObjectDistanceTransform targets (reference transform/label.py:454-633), batched [N][D][H][W] (2-D: D == 1);
//   * the vector EDT and the DistanceTransform targets (reference transform/label.py:356-451; tem_vector_edt,
//     tem_distance_targets, further down);
//   * the DistanceLoss / DiceBasedDistanceLoss sums and gradient (reference loss/distance_based.py).
//
// Transform passes (tem_pod_*; the Python side adds torch.sort / torch.cumsum for the id compaction):
//   labels   apply_label: union-find over equal nonzero face neighbours, every link toward the smaller linear index
//            (atomicMin), so a root is its component's first voxel in raster order and a root flag + prefix sum numbers
//            components in first-occurrence order.  The prefix sums run once over the whole batch (torch's flat scan;
//            a per-sample row scan measured 4.7 ms at 2 x 128^3) and each sample subtracts its predecessor's total.
//            apply_label=False: ascending original id -> 1..n (sorted values).
//            min_size: per-id voxel counts, small ids dropped, survivors renumbered in order.
//   targets  (tem_pod_targets) inner boundaries + per-object count / coordinate sums / bounding-box minimum, one exact
//            squared EDT of the boundary mask over the whole sample, per-object arg-max of the boundary distance,
//            centers, per-object per-channel max |value|, and the normalised output.
//
// Why one EDT over the whole sample equals the reference's EDT inside each object's bounding-box crop, on every voxel
// of the object (the only voxels the reference keeps): take a voxel x of object L and any voxel y outside L's box.  y
// lies beyond some face of the box, along axis a, at least (k + 1) sample steps s_a from x, where k is the number of
// steps from x to that face (the face is not the volume border, since y exists).  Walk from x toward that face: the
// last L voxel before a non-L voxel, or before the face, has a face neighbour of another label (no L voxel lies
// outside the box), so it is an inner-boundary voxel inside the box, at most k * s_a from x.  The nearest boundary
// voxel inside the box is therefore strictly closer than anything outside it, and both transforms agree.
#include <math.h>

#include "tem_common.h"

#define POD_MAX_LINE 4096
#define POD_BLOCKS 2048

// ---------------------------------------------------------------------------------------------------------------
// wave helpers: a wave walks its distinct object slots one at a time (objects are spatially coherent, so most waves
// see one or two), reducing the lanes of one slot before a single atomic.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ int uf_find(int* par, int x) {
    int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// Playne & Hawick union: hook the larger root under the smaller; atomicMin returns what was there, retry on a race
__device__ void uf_union(int* par, int a, int b) {
    bool done;
    do {
        a = uf_find(par, a);
        b = uf_find(par, b);
        if (a < b) {
            int old = atomicMin(&par[b], a);
            done = old == b;
            b = old;
        } else if (b < a) {
            int old = atomicMin(&par[a], b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

// ---- labels: connected components --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_init(int* __restrict__ par, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) par[g] = (int)g;
}

__global__ __launch_bounds__(256) void k_cc_link(const int64_t* __restrict__ lab, int* par, int N, int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W, NV = V * N;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t c = lab[g];
        if (c == 0) continue;
        const int64_t v = g % V;
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((int64_t)W * H));
        if (x + 1 < W && lab[g + 1] == c) uf_union(par, (int)g, (int)(g + 1));
        if (y + 1 < H && lab[g + W] == c) uf_union(par, (int)g, (int)(g + W));
        if (z + 1 < D && lab[g + (int64_t)W * H] == c) uf_union(par, (int)g, (int)(g + (int64_t)W * H));
    }
}

// path compression + root flag (a root is its component's first voxel in raster order)
__global__ __launch_bounds__(256) void k_cc_flag(const int64_t* __restrict__ lab, int* par, int* __restrict__ flag,
                                                 int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int r = uf_find(par, (int)g);
        par[g] = r;
        flag[g] = (lab[g] != 0 && r == (int)g) ? 1 : 0;
    }
}

// inclusive prefix sum over the whole batch (one flat scan), minus its value at the end of the previous sample:
// the sample-local count
__device__ __forceinline__ int sample_rank(const int* __restrict__ rank, int64_t i, int64_t n, int64_t len) {
    return rank[i] - (n > 0 ? rank[n * len - 1] : 0);
}

// rank: prefix sum of the root flags, so a root's sample-local rank is its component's id
__global__ __launch_bounds__(256) void k_cc_assign(const int64_t* __restrict__ lab, const int* __restrict__ par,
                                                   const int* __restrict__ rank, int* __restrict__ ids, int64_t V,
                                                   int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256)
        ids[g] = lab[g] != 0 ? sample_rank(rank, par[g], g / V, V) : 0;
}

// ---- labels: relabel_sequential (sorted values of each sample; first of each distinct nonzero value flagged) --------
__global__ __launch_bounds__(256) void k_seq_flag(const int64_t* __restrict__ sorted, int* __restrict__ flag, int64_t V,
                                                  int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t s = sorted[g];
        flag[g] = (s != 0 && (g % V == 0 || sorted[g - 1] != s)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_seq_assign(const int64_t* __restrict__ sorted, const int64_t* __restrict__ order,
                                                    const int* __restrict__ rank, int* __restrict__ ids, int64_t V,
                                                    int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t n = g / V;
        ids[n * V + order[g]] = sorted[g] != 0 ? sample_rank(rank, g, n, V) : 0;
    }
}

// ---- labels: min_size ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_size_count(const int* __restrict__ ids, int* __restrict__ cnt, int64_t V,
                                                    int64_t NV) {
    for (int64_t base = (int64_t)blockIdx.x * 256; base < NV; base += (int64_t)gridDim.x * 256) {
        const int64_t g = base + threadIdx.x;
        const int id = g < NV ? ids[g] : 0;
        const long long slot = id > 0 ? (g / V) * (V + 1) + id : -1;
        unsigned long long pending = __ballot(slot >= 0);
        while (pending) {
            const long long s = __shfl(slot, __ffsll((long long)pending) - 1, 64);
            const unsigned long long mine = __ballot(slot == s);
            if (lane_id() == __ffsll((long long)pending) - 1) atomicAdd(&cnt[s], (int)__popcll(mine));
            pending &= ~mine;
        }
    }
}

__global__ __launch_bounds__(256) void k_size_keep(const int* __restrict__ cnt, int* __restrict__ keep, int64_t V,
                                                   int64_t NS, int min_size) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (int64_t)gridDim.x * 256)
        keep[s] = (s % (V + 1) != 0 && cnt[s] >= min_size) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_size_apply(int* __restrict__ ids, const int* __restrict__ keep,
                                                    const int* __restrict__ newid, int64_t V, int64_t NV) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int id = ids[g];
        if (id == 0) continue;
        const int64_t n = g / V, s = n * (V + 1) + id;
        ids[g] = keep[s] ? sample_rank(newid, s, n, V + 1) : 0;
    }
}

// ---- targets ------------------------------------------------------------------------------------------------------
struct PodObj {             // per-object slots, [N][V + 1] each (slot 0 of a sample unused): sized from the voxel count
    int* cnt;               // voxels
    long long* csum;        // [3] coordinate sums (z, y, x)
    int* cmin;              // [3] bounding-box minimum (z, y, x)
    unsigned long long* key;   // (bits of the max squared boundary distance << 32) | ~(first linear index with it)
    int* center;            // linear index of the chosen center
    unsigned long long* chmax; // [nch] bits of max |value| (double) per distance channel
};

struct PodGeo {
    int N, D, H, W, ndim, flags, nch;
    int64_t V;
    float s[3];   // sampling (z, y, x)
};

enum { POD_DIST = 1, POD_BOUNDARY = 2, POD_DIRECTED = 4, POD_FOREGROUND = 8, POD_INSTANCES = 16 };

// inner boundary (find_boundaries mode="inner": foreground with a face neighbour of another label, inside the volume)
// -> f = 0 on the boundary, +inf elsewhere; the per-object count, coordinate sums and box minimum ride along
__global__ __launch_bounds__(256) void k_pod_init(const int* __restrict__ ids, float* __restrict__ f, PodObj ob, PodGeo G) {
    const int64_t V = G.V, NV = V * G.N, HW = (int64_t)G.H * G.W;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < NV; base += (int64_t)gridDim.x * 256) {
        const int64_t g = base + threadIdx.x;
        int id = 0, x = 0, y = 0, z = 0;
        long long slot = -1;
        if (g < NV) {
            const int64_t v = g % V;
            x = (int)(v % G.W);
            y = (int)((v / G.W) % G.H);
            z = (int)(v / HW);
            id = ids[g];
            bool b = false;
            if (id != 0) {
                if (x > 0) b |= ids[g - 1] != id;
                if (x < G.W - 1) b |= ids[g + 1] != id;
                if (y > 0) b |= ids[g - G.W] != id;
                if (y < G.H - 1) b |= ids[g + G.W] != id;
                if (z > 0) b |= ids[g - HW] != id;
                if (z < G.D - 1) b |= ids[g + HW] != id;
                slot = (g / V) * (V + 1) + id;
            }
            f[g] = b ? 0.f : __builtin_inff();
        }
        unsigned long long pending = __ballot(slot >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const long long s = __shfl(slot, leader, 64);
            const bool mine = slot == s;
            const unsigned long long m = __ballot(mine);
            const long long sz = wave_sum_i64(mine ? z : 0), sy = wave_sum_i64(mine ? y : 0),
                            sx = wave_sum_i64(mine ? x : 0);
            const int mz = wave_min_i32(mine ? z : INT_MAX), my = wave_min_i32(mine ? y : INT_MAX),
                      mx = wave_min_i32(mine ? x : INT_MAX);
            if (lane_id() == leader) {
                atomicAdd(&ob.cnt[s], (int)__popcll(m));
                atomicAdd((unsigned long long*)&ob.csum[3 * s + 0], (unsigned long long)sz);
                atomicAdd((unsigned long long*)&ob.csum[3 * s + 1], (unsigned long long)sy);
                atomicAdd((unsigned long long*)&ob.csum[3 * s + 2], (unsigned long long)sx);
                atomicMin(&ob.cmin[3 * s + 0], mz);
                atomicMin(&ob.cmin[3 * s + 1], my);
                atomicMin(&ob.cmin[3 * s + 2], mx);
            }
            pending &= ~m;
        }
    }
}

// One pass of the separable exact squared EDT along one axis: d(i) = min_j f(j) + ((i - j) s)^2, the lower envelope
// of the parabolas rooted at the line's samples, by brute force over the line held in LDS (every lane reads the same
// f(j): an LDS broadcast).  Exact in fp32 while the squared distances are exactly representable (integer offsets
// times the sampling values the tests use: 1, 2, 2.5).  One workgroup per line.  O(L^2) per line instead of the O(L)
// Felzenszwalb / Meijster envelope: ~0.2 ms per pass at 2 x 128^3 (profiles/distance_kernels.txt); lines up to 4096.
__global__ __launch_bounds__(256) void k_pod_edt(float* __restrict__ f, PodGeo G, int axis) {
    __shared__ float line[POD_MAX_LINE];
    const int64_t HW = (int64_t)G.H * G.W;
    int L;
    int64_t stride, nl;
    if (axis == 2) {
        L = G.W;
        stride = 1;
        nl = (int64_t)G.N * G.D * G.H;
    } else if (axis == 1) {
        L = G.H;
        stride = G.W;
        nl = (int64_t)G.N * G.D * G.W;
    } else {
        L = G.D;
        stride = HW;
        nl = (int64_t)G.N * HW;
    }
    const float s = G.s[axis];
    for (int64_t l = blockIdx.x; l < nl; l += gridDim.x) {
        int64_t base;
        if (axis == 2) base = l * G.W;
        else if (axis == 1) base = (l / G.W) * HW + l % G.W;    // (n, z) plane, column x
        else base = (l / HW) * G.V + l % HW;                      // sample n, (y, x)
        __syncthreads();   // the previous line's readers are done with the LDS
        for (int i = threadIdx.x; i < L; i += 256) line[i] = f[base + i * stride];
        __syncthreads();
        for (int i = threadIdx.x; i < L; i += 256) {
            float d = line[i];
            for (int j = 0; j < L; ++j) {
                const float t = (float)(i - j) * s;
                d = fminf(d, line[j] + t * t);
            }
            f[base + i * stride] = d;
        }
    }
}

// arg-max of the squared boundary distance per object, ties to the smallest linear index (np.argmax's first voxel in
// C order inside the crop): one 64-bit atomicMax of (distance bits, inverted index)
__global__ __launch_bounds__(256) void k_pod_argmax(const int* __restrict__ ids, const float* __restrict__ f, PodObj ob,
                                                    PodGeo G) {
    const int64_t V = G.V, NV = V * G.N;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < NV; base += (int64_t)gridDim.x * 256) {
        const int64_t g = base + threadIdx.x;
        long long slot = -1;
        unsigned long long key = 0;
        if (g < NV) {
            const int id = ids[g];
            if (id != 0) {
                slot = (g / V) * (V + 1) + id;
                key = ((unsigned long long)__float_as_uint(f[g]) << 32) | (0xffffffffu - (unsigned)(g % V));
            }
        }
        unsigned long long pending = __ballot(slot >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const long long s = __shfl(slot, leader, 64);
            const bool mine = slot == s;
            const unsigned long long k = wave_max_u64(mine ? key : 0ull);
            if (lane_id() == leader) atomicMax(&ob.key[s], k);
            pending &= ~__ballot(mine);
        }
    }
}

// center: np.round(centroid) (round half to even, in double); where that voxel is not in the object, the arg-max of the
// boundary distance -- and when that maximum is 0 (every voxel of the object is boundary), np.argmax over the crop's
// zeros returns the crop's first voxel: the box minimum, which the reference then uses as the center
__global__ __launch_bounds__(256) void k_pod_center(const int* __restrict__ ids, PodObj ob, PodGeo G) {
    const int64_t V = G.V, NS = (V + 1) * G.N;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (int64_t)gridDim.x * 256) {
        const int c = ob.cnt[s];
        if (c == 0) continue;
        const int64_t n = s / (V + 1);
        const int id = (int)(s % (V + 1));
        const int cz = (int)rint((double)ob.csum[3 * s + 0] / c), cy = (int)rint((double)ob.csum[3 * s + 1] / c),
                  cx = (int)rint((double)ob.csum[3 * s + 2] / c);
        int64_t lin = ((int64_t)cz * G.H + cy) * G.W + cx;
        if (ids[n * V + lin] != id) {
            const unsigned long long k = ob.key[s];
            if (__uint_as_float((unsigned)(k >> 32)) == 0.f)
                lin = ((int64_t)ob.cmin[3 * s] * G.H + ob.cmin[3 * s + 1]) * G.W + ob.cmin[3 * s + 2];
            else
                lin = 0xffffffffu - (unsigned)(k & 0xffffffffu);
        }
        ob.center[s] = (int)lin;
    }
}

// boundary distance from a squared EDT value: no boundary voxel in the whole sample (one object fills it) -> 0
__device__ __forceinline__ double pod_bdist(float d2) { return isinf(d2) ? 0.0 : sqrt((double)d2); }

// the unnormalised distance channels of voxel v (linear index in its sample) of the object in slot s, in output order:
// [distance?] [directed x ndim?] [boundary?]; returns the channel count
__device__ __forceinline__ int pod_values(const PodObj& ob, const PodGeo& G, int64_t s, int64_t v, float d2, double* val) {
    const int64_t HW = (int64_t)G.H * G.W;
    const int x = (int)(v % G.W), y = (int)((v / G.W) % G.H), z = (int)(v / HW);
    const int64_t c = ob.center[s];
    const int ccx = (int)(c % G.W), ccy = (int)((c / G.W) % G.H), ccz = (int)(c / HW);
    const double dz = (double)(ccz - z) * G.s[0], dy = (double)(ccy - y) * G.s[1], dx = (double)(ccx - x) * G.s[2];
    int k = 0;
    if (G.flags & POD_DIST) val[k++] = sqrt(dz * dz + dy * dy + dx * dx);
    if (G.flags & POD_DIRECTED) {
        if (G.ndim == 3) val[k++] = dz;
        val[k++] = dy;
        val[k++] = dx;
    }
    if (G.flags & POD_BOUNDARY) val[k++] = pod_bdist(__uint_as_float((unsigned)(ob.key[s] >> 32))) - pod_bdist(d2);
    return k;
}

__global__ __launch_bounds__(256) void k_pod_chmax(const int* __restrict__ ids, const float* __restrict__ f, PodObj ob,
                                                   PodGeo G) {
    const int64_t V = G.V, NV = V * G.N;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < NV; base += (int64_t)gridDim.x * 256) {
        const int64_t g = base + threadIdx.x;
        long long slot = -1;
        double val[5] = {0, 0, 0, 0, 0};
        if (g < NV) {
            const int id = ids[g];
            if (id != 0) {
                slot = (g / V) * (V + 1) + id;
                pod_values(ob, G, slot, g % V, f[g], val);
            }
        }
        unsigned long long pending = __ballot(slot >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const long long s = __shfl(slot, leader, 64);
            const bool mine = slot == s;
            for (int c = 0; c < G.nch; ++c) {   // |value| >= 0: its double bits order as unsigned integers
                const unsigned long long m = wave_max_u64(mine ? (unsigned long long)__double_as_longlong(fabs(val[c])) : 0ull);
                if (lane_id() == leader) atomicMax(&ob.chmax[(int64_t)G.nch * s + c], m);
            }
            pending &= ~__ballot(mine);
        }
    }
}

// out [N][C][V]: [ids?] [foreground?] then the distance channels, value / (max + 1e-7) on objects, fill on background
__global__ __launch_bounds__(256) void k_pod_write(const int* __restrict__ ids, const float* __restrict__ f, PodObj ob,
                                                   PodGeo G, float fill, float* __restrict__ out) {
    const int64_t V = G.V, NV = V * G.N;
    const int nc = G.nch + ((G.flags & POD_INSTANCES) ? 1 : 0) + ((G.flags & POD_FOREGROUND) ? 1 : 0);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t n = g / V, v = g % V;
        float* o = out + n * nc * V + v;
        const int id = ids[g];
        int c = 0;
        if (G.flags & POD_INSTANCES) o[V * c++] = (float)id;
        if (G.flags & POD_FOREGROUND) o[V * c++] = id != 0 ? 1.f : 0.f;
        if (id == 0) {
            for (int k = 0; k < G.nch; ++k) o[V * (c + k)] = fill;
            continue;
        }
        const int64_t s = n * (V + 1) + id;
        double val[5];
        pod_values(ob, G, s, v, f[g], val);
        for (int k = 0; k < G.nch; ++k)
            o[V * (c + k)] = (float)(val[k] / (__longlong_as_double((long long)ob.chmax[(int64_t)G.nch * s + k]) + 1e-7));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
static bool pod_shape_ok(int N, int D, int H, int W) {
    return N > 0 && D > 0 && H > 0 && W > 0 && (int64_t)N * D * H * W < INT_MAX;
}

extern "C" int tem_pod_cc_roots(const int64_t* labels, int* parent, int* flag, int N, int D, int H, int W,
                                tem_stream_t stream) {
    TEM_REQUIRE(labels && parent && flag, "tem_pod_cc_roots: null pointer");
    TEM_REQUIRE(pod_shape_ok(N, D, H, W), "tem_pod_cc_roots: bad shape (N*D*H*W must be positive and below 2^31)");
    const int64_t NV = (int64_t)N * D * H * W;
    const int grid = tem_grid_1d(NV, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cc_init, dim3(grid), dim3(256), 0, st, parent, NV);
    hipLaunchKernelGGL(k_cc_link, dim3(grid), dim3(256), 0, st, labels, parent, N, D, H, W);
    hipLaunchKernelGGL(k_cc_flag, dim3(grid), dim3(256), 0, st, labels, parent, flag, NV);
    TEM_CHECK_LAUNCH("tem_pod_cc_roots");
    return TEM_OK;
}

extern "C" int tem_pod_cc_assign(const int64_t* labels, const int* parent, const int* rank, int* ids, int N, int64_t V,
                                 tem_stream_t stream) {
    TEM_REQUIRE(labels && parent && rank && ids && N > 0 && V > 0 && N * V < INT_MAX, "tem_pod_cc_assign: bad arguments");
    hipLaunchKernelGGL(k_cc_assign, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, (hipStream_t)stream, labels, parent, rank,
                       ids, V, N * V);
    TEM_CHECK_LAUNCH("tem_pod_cc_assign");
    return TEM_OK;
}

extern "C" int tem_pod_seq_flag(const int64_t* sorted, int* flag, int N, int64_t V, tem_stream_t stream) {
    TEM_REQUIRE(sorted && flag && N > 0 && V > 0 && N * V < INT_MAX, "tem_pod_seq_flag: bad arguments");
    hipLaunchKernelGGL(k_seq_flag, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, (hipStream_t)stream, sorted, flag, V,
                       N * V);
    TEM_CHECK_LAUNCH("tem_pod_seq_flag");
    return TEM_OK;
}

extern "C" int tem_pod_seq_assign(const int64_t* sorted, const int64_t* order, const int* rank, int* ids, int N,
                                  int64_t V, tem_stream_t stream) {
    TEM_REQUIRE(sorted && order && rank && ids && N > 0 && V > 0 && N * V < INT_MAX, "tem_pod_seq_assign: bad arguments");
    hipLaunchKernelGGL(k_seq_assign, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, (hipStream_t)stream, sorted, order,
                       rank, ids, V, N * V);
    TEM_CHECK_LAUNCH("tem_pod_seq_assign");
    return TEM_OK;
}

extern "C" int tem_pod_size_keep(const int* ids, int* cnt, int* keep, int N, int64_t V, int min_size,
                                 tem_stream_t stream) {
    TEM_REQUIRE(ids && cnt && keep && N > 0 && V > 0 && N * V < INT_MAX, "tem_pod_size_keep: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int64_t NS = N * (V + 1);
    if (hipMemsetAsync(cnt, 0, NS * sizeof(int), st) != hipSuccess) {
        tem_set_error("tem_pod_size_keep: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    hipLaunchKernelGGL(k_size_count, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, st, ids, cnt, V, N * V);
    hipLaunchKernelGGL(k_size_keep, dim3(tem_grid_1d(NS, 256)), dim3(256), 0, st, cnt, keep, V, NS, min_size);
    TEM_CHECK_LAUNCH("tem_pod_size_keep");
    return TEM_OK;
}

extern "C" int tem_pod_size_apply(int* ids, const int* keep, const int* newid, int N, int64_t V, tem_stream_t stream) {
    TEM_REQUIRE(ids && keep && newid && N > 0 && V > 0 && N * V < INT_MAX, "tem_pod_size_apply: bad arguments");
    hipLaunchKernelGGL(k_size_apply, dim3(tem_grid_1d(N * V, 256)), dim3(256), 0, (hipStream_t)stream, ids, keep, newid,
                       V, N * V);
    TEM_CHECK_LAUNCH("tem_pod_size_apply");
    return TEM_OK;
}

static int pod_nch(int ndim, int flags) {
    return ((flags & POD_DIST) ? 1 : 0) + ((flags & POD_DIRECTED) ? ndim : 0) + ((flags & POD_BOUNDARY) ? 1 : 0);
}

// workspace layout (8-byte aligned pieces): f[NV] float, then per-object slots [N][V+1]: cnt, csum[3], cmin[3], key,
// center, chmax[nch]
extern "C" int64_t tem_pod_ws(int N, int64_t V, int ndim, int flags) {
    const int64_t NV = N * V, NS = N * (V + 1);
    return tem_align_up(NV * 4, 8) + tem_align_up(NS * 4, 8) + NS * 24 + tem_align_up(NS * 12, 8) + NS * 8 +
           tem_align_up(NS * 4, 8) + NS * 8 * pod_nch(ndim, flags);
}

extern "C" int tem_pod_targets(const int* ids, float* out, int N, int D, int H, int W, int ndim, const float* sampling,
                               int flags, float fill, void* ws, int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(ids && out && sampling && ws, "tem_pod_targets: null pointer");
    TEM_REQUIRE(pod_shape_ok(N, D, H, W) && (ndim == 3 || (ndim == 2 && D == 1)), "tem_pod_targets: bad shape");
    TEM_REQUIRE(D <= POD_MAX_LINE && H <= POD_MAX_LINE && W <= POD_MAX_LINE,
                "tem_pod_targets: spatial extents up to %d supported", POD_MAX_LINE);
    TEM_REQUIRE((flags & ~31) == 0 && (flags & (POD_DIST | POD_BOUNDARY | POD_DIRECTED)),
                "tem_pod_targets: at least one distance kind required");
    PodGeo G;
    G.N = N, G.D = D, G.H = H, G.W = W, G.ndim = ndim, G.flags = flags, G.nch = pod_nch(ndim, flags);
    G.V = (int64_t)D * H * W;
    for (int a = 0; a < 3; ++a) G.s[a] = sampling[a];
    const int64_t NV = G.V * N, NS = (G.V + 1) * N;
    if (ws_bytes < tem_pod_ws(N, G.V, ndim, flags)) {
        tem_set_error("tem_pod_targets: workspace too small");
        return TEM_EWS;
    }
    char* p = (char*)ws;
    float* f = (float*)p;
    p += tem_align_up(NV * 4, 8);
    char* zero_begin = p;
    PodObj ob;
    ob.cnt = (int*)p;
    p += tem_align_up(NS * 4, 8);
    ob.csum = (long long*)p;
    p += NS * 24;
    ob.key = (unsigned long long*)p;
    p += NS * 8;
    ob.chmax = (unsigned long long*)p;
    p += NS * 8 * G.nch;
    char* zero_end = p;
    ob.cmin = (int*)p;
    p += tem_align_up(NS * 12, 8);
    ob.center = (int*)p;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(zero_begin, 0, zero_end - zero_begin, st) != hipSuccess ||
        hipMemsetAsync(ob.cmin, 0x7f, NS * 12, st) != hipSuccess) {   // 0x7f7f7f7f: above every coordinate
        tem_set_error("tem_pod_targets: hipMemsetAsync failed");
        return TEM_ELAUNCH;
    }
    const int grid = tem_grid_1d(NV, 256);
    hipLaunchKernelGGL(k_pod_init, dim3(grid), dim3(256), 0, st, ids, f, ob, G);
    hipLaunchKernelGGL(k_pod_edt, dim3(POD_BLOCKS), dim3(256), 0, st, f, G, 2);
    hipLaunchKernelGGL(k_pod_edt, dim3(POD_BLOCKS), dim3(256), 0, st, f, G, 1);
    if (D > 1) hipLaunchKernelGGL(k_pod_edt, dim3(POD_BLOCKS), dim3(256), 0, st, f, G, 0);
    hipLaunchKernelGGL(k_pod_argmax, dim3(grid), dim3(256), 0, st, ids, f, ob, G);
    hipLaunchKernelGGL(k_pod_center, dim3(tem_grid_1d(NS, 256)), dim3(256), 0, st, ids, ob, G);
    hipLaunchKernelGGL(k_pod_chmax, dim3(grid), dim3(256), 0, st, ids, f, ob, G);
    hipLaunchKernelGGL(k_pod_write, dim3(grid), dim3(256), 0, st, ids, f, ob, G, fill, out);
    TEM_CHECK_LAUNCH("tem_pod_targets");
    return TEM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Vector (feature-transform) EDT and the DistanceTransform targets (reference transform/label.py:356-451).
//
// tem_vector_edt: T = voxels equal to foreground_id; per voxel x the integer offset v(x) = t - x to a nearest t in T and
// |v|^2, all in int32: exact by construction.  The same separable lower envelope as k_pod_edt, one pass per axis (x, y,
// then z), a workgroup per line, the line staged in LDS; each pass carries the offsets found by the passes before it
// along with the value.  After the x pass d2(i) = vx(i)^2 with vx the offset to the nearest target of the row; a later
// pass along axis a picks j minimising d2(j) + (i - j)^2, sets v_a(i) = j - i and copies the earlier components from j,
// so v(i) always points at a target voxel at squared distance d2(i), and the minimum over j is the minimum over T.
// Tie rule: candidates j are scanned in ascending index along the axis being processed and replace the best so far
// only when strictly smaller (`<`): among equally near candidates the smallest j wins, in every pass.  No atomics.
// A line (or sample) without any target keeps d2 = VDT_NONE and offset 0; empty[n] = (d2 of the sample's first voxel
// == VDT_NONE), read after the last pass: a sample has a target iff every voxel found one.
// Brute force over the line like k_pod_edt: O(L^2) per line, priced in profiles/label_targets_bench.txt.
// ---------------------------------------------------------------------------------------------------------------
#define VDT_NONE TEM_VDT_NONE   // 0x3fffffff: above every squared distance (3 * 4095^2), and VDT_NONE + 4095^2 still fits an int

// vec [N][3][V] (z, y, x), d2 [N][V].  axis 2 reads the labels; axes 1 and 0 update vec / d2 in place (a line is read
// into LDS whole before any of it is written, and lines are disjoint).
__global__ __launch_bounds__(256) void k_vdt_pass(const int64_t* __restrict__ lab, int64_t fg, int* __restrict__ vec,
                                                  int* __restrict__ d2, int N, int D, int H, int W, int axis) {
    __shared__ int lf[POD_MAX_LINE];   // value
    __shared__ int la[POD_MAX_LINE];   // carried x offset (axes 1, 0)
    __shared__ int lb[POD_MAX_LINE];   // carried y offset (axis 0)
    const int64_t HW = (int64_t)H * W, V = HW * D;
    int L;
    int64_t stride, nl;
    if (axis == 2) {
        L = W;
        stride = 1;
        nl = (int64_t)N * D * H;
    } else if (axis == 1) {
        L = H;
        stride = W;
        nl = (int64_t)N * D * W;
    } else {
        L = D;
        stride = HW;
        nl = (int64_t)N * HW;
    }
    for (int64_t l = blockIdx.x; l < nl; l += gridDim.x) {
        int64_t n, off;   // sample and offset of the line's first voxel inside it
        if (axis == 2) {
            n = l / ((int64_t)D * H);
            off = (l % ((int64_t)D * H)) * W;
        } else if (axis == 1) {
            n = l / ((int64_t)D * W);
            const int64_t r = l % ((int64_t)D * W);
            off = (r / W) * HW + r % W;
        } else {
            n = l / HW;
            off = l % HW;
        }
        int* vz = vec + n * 3 * V + off;
        int* vy = vz + V;
        int* vx = vy + V;
        int* dd = d2 + n * V + off;
        __syncthreads();   // the previous line's readers are done with the LDS
        for (int i = threadIdx.x; i < L; i += 256) {
            if (axis == 2) {
                lf[i] = lab[n * V + off + i] == fg ? 0 : VDT_NONE;
            } else {
                lf[i] = dd[i * stride];
                la[i] = vx[i * stride];
                if (axis == 0) lb[i] = vy[i * stride];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < L; i += 256) {
            int best = VDT_NONE, bj = -1;
            for (int j = 0; j < L; ++j) {
                const int t = i - j, c = lf[j] + t * t;
                if (c < best) {
                    best = c;
                    bj = j;
                }
            }
            dd[i * stride] = best;
            if (axis == 2) {
                vz[i] = 0;
                vy[i] = 0;
                vx[i] = bj < 0 ? 0 : bj - i;
            } else if (axis == 1) {
                vy[i * stride] = bj < 0 ? 0 : bj - i;
                vx[i * stride] = bj < 0 ? 0 : la[bj];
            } else {
                vz[i * stride] = bj < 0 ? 0 : bj - i;
                vy[i * stride] = bj < 0 ? 0 : lb[bj];
                vx[i * stride] = bj < 0 ? 0 : la[bj];
            }
        }
    }
}

__global__ void k_vdt_empty(const int* __restrict__ d2, int* __restrict__ empty, int N, int64_t V) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) empty[n] = d2[n * V] == VDT_NONE ? 1 : 0;
}

static bool vdt_shape_ok(const char* who, int N, int D, int H, int W) {
    if (!pod_shape_ok(N, D, H, W)) {
        tem_set_error("%s: bad shape (N*D*H*W must be positive and below 2^31)", who);
        return false;
    }
    if (D > POD_MAX_LINE || H > POD_MAX_LINE || W > POD_MAX_LINE) {
        tem_set_error("%s: spatial extents up to %d supported", who, POD_MAX_LINE);
        return false;
    }
    return true;
}

extern "C" int tem_vector_edt(const int64_t* labels, int64_t foreground_id, int* vec, int* d2, int* empty, int N, int D,
                              int H, int W, tem_stream_t stream) {
    TEM_REQUIRE(labels && vec && d2 && empty, "tem_vector_edt: null pointer");
    if (!vdt_shape_ok("tem_vector_edt", N, D, H, W)) return TEM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vdt_pass, dim3(POD_BLOCKS), dim3(256), 0, st, labels, foreground_id, vec, d2, N, D, H, W, 2);
    hipLaunchKernelGGL(k_vdt_pass, dim3(POD_BLOCKS), dim3(256), 0, st, labels, foreground_id, vec, d2, N, D, H, W, 1);
    if (D > 1) hipLaunchKernelGGL(k_vdt_pass, dim3(POD_BLOCKS), dim3(256), 0, st, labels, foreground_id, vec, d2, N, D, H, W, 0);
    hipLaunchKernelGGL(k_vdt_empty, dim3((unsigned)tem_cdiv(N, 64)), dim3(64), 0, st, d2, empty, N, (int64_t)D * H * W);
    TEM_CHECK_LAUNCH("tem_vector_edt");
    return TEM_OK;
}

// ---- DistanceTransform finishing pass -------------------------------------------------------------------------------
// The maxima the normalisation needs, as integers (the offsets and d2 are integers; clipping and the division by a
// positive constant are monotone, so max and clip / divide commute): per sample max d2, and per group max |v_c| and
// max v_c.  A group is what the reference's `max(axis=(1, 2), keepdims=True)` on [ndim, *spatial] leaves: 2-D labels
// one per channel; 3-D labels one per (channel, x column) -- the axes (1, 2) are z and y there, a quirk of the
// reference that is mirrored, not repaired.  Slots per sample: [0] max d2, [1 + c * W + x] max |v_c|,
// [1 + (3 + c) * W + x] max v_c (2-D labels use x = 0 only).  Integer atomicMax: order-independent.
enum { DT_DIST = 1, DT_DIRECTED = 2, DT_NORMALIZE = 4, DT_INVERT = 8, DT_CLIP = 16 };

__device__ __forceinline__ int64_t dt_slots(int W) { return 1 + 6 * (int64_t)W; }

__global__ __launch_bounds__(256) void k_dt_init(int* __restrict__ mx, int N, int W) {
    const int64_t S = dt_slots(W), NS = S * N;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NS; g += (int64_t)gridDim.x * 256)
        mx[g] = g % S <= 3 * (int64_t)W ? 0 : INT_MIN;
}

// grid (column chunks of 256, row chunks, N): a thread owns one x column and walks rows (z, y) of its chunk
__global__ __launch_bounds__(256) void k_dt_max(const int* __restrict__ vec, const int* __restrict__ d2,
                                                int* __restrict__ mx, int D, int H, int W, int ndim) {
    const int64_t rows = (int64_t)D * H, V = rows * W;
    const int n = blockIdx.z, x = blockIdx.x * 256 + threadIdx.x;
    int md = 0, ma[3] = {0, 0, 0}, ms[3] = {INT_MIN, INT_MIN, INT_MIN};
    if (x < W) {
        const int* v = vec + (int64_t)n * 3 * V;
        const int* d = d2 + (int64_t)n * V;
        for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
            const int64_t g = r * W + x;
            md = max(md, d[g]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int q = v[c * V + g];
                ma[c] = max(ma[c], abs(q));
                ms[c] = max(ms[c], q);
            }
        }
    }
    int* m = mx + n * dt_slots(W);
    if (ndim == 3 && x < W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMax(&m[1 + c * (int64_t)W + x], ma[c]);
            atomicMax(&m[1 + (3 + c) * (int64_t)W + x], ms[c]);
        }
    }
    // whole-sample maxima: wave reduction, one atomic per wave (all lanes take part; idle lanes hold the identities)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        md = max(md, __shfl_xor(md, o, 64));
        if (ndim == 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ma[c] = max(ma[c], __shfl_xor(ma[c], o, 64));
                ms[c] = max(ms[c], __shfl_xor(ms[c], o, 64));
            }
        }
    }
    if (lane_id() == 0) {
        atomicMax(&m[0], md);
        if (ndim == 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMax(&m[1 + c * (int64_t)W], ma[c]);
                atomicMax(&m[1 + (3 + c) * (int64_t)W], ms[c]);
            }
        }
    }
}

// out [N][C][V], channels [distances?][directed x ndim?], following _compute_distances / _compute_directed_distances
// step by step in double, rounded once to float32.  An empty sample (no target voxel) takes the reference's fill vector
// (`fill` in every component) through the same steps.
__global__ __launch_bounds__(256) void k_dt_write(const int* __restrict__ vec, const int* __restrict__ d2,
                                                  const int* __restrict__ empty, const int* __restrict__ mx,
                                                  float* __restrict__ out, int N, int D, int H, int W, int ndim, int flags,
                                                  double maxd, double fill) {
    const int64_t V = (int64_t)D * H * W, NV = V * N;
    const int nc = ((flags & DT_DIST) ? 1 : 0) + ((flags & DT_DIRECTED) ? ndim : 0);
    const double eps = 1e-7;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t n = g / V, v = g % V;
        const int x = ndim == 3 ? (int)(v % W) : 0;
        const bool e = empty[n] != 0;
        const int* m = mx + n * dt_slots(W);
        float* o = out + n * nc * V + v;
        int k = 0;
        if (flags & DT_DIST) {
            const double dfill = sqrt(fill * fill * ndim);   // |(fill, ..., fill)|
            double d = e ? dfill : sqrt((double)d2[g]), top = e ? dfill : sqrt((double)m[0]);
            if (flags & DT_CLIP) {
                d = fmin(fmax(d, 0.0), maxd);
                top = fmin(fmax(top, 0.0), maxd);
            }
            if (flags & DT_NORMALIZE) {
                const double den = top + eps;
                d /= den;
                top /= den;
            }
            if (flags & DT_INVERT) d = top - d;
            o[V * k++] = (float)d;
        }
        if (flags & DT_DIRECTED) {
            for (int c = 3 - ndim; c < 3; ++c) {
                double q = e ? fill : (double)vec[(n * 3 + c) * V + v];
                double ma = e ? fill : (double)m[1 + c * (int64_t)W + x];
                double ms = e ? fill : (double)m[1 + (3 + c) * (int64_t)W + x];
                if (flags & DT_CLIP) {
                    q = fmin(fmax(q, -maxd), maxd);
                    ma = fmin(ma, fabs(maxd));   // max |clip(v)| = clip(max |v|) for the symmetric interval
                    ms = fmin(fmax(ms, -maxd), maxd);
                }
                if (flags & DT_NORMALIZE) {
                    const double den = ma + eps;
                    q /= den;
                    ms /= den;
                }
                if (flags & DT_INVERT) q = ms - q;
                o[V * k++] = (float)q;
            }
        }
    }
}

extern "C" int64_t tem_distance_targets_ws(int N, int W) { return (int64_t)N * (1 + 6 * (int64_t)W) * sizeof(int); }

extern "C" int tem_distance_targets(const int* vec, const int* d2, const int* empty, float* out, int N, int D, int H, int W,
                                    int ndim, int flags, double max_distance, void* ws, int64_t ws_bytes,
                                    tem_stream_t stream) {
    TEM_REQUIRE(vec && d2 && empty && out && ws, "tem_distance_targets: null pointer");
    if (!vdt_shape_ok("tem_distance_targets", N, D, H, W)) return TEM_EINVAL;
    TEM_REQUIRE(ndim == 3 || (ndim == 2 && D == 1), "tem_distance_targets: bad shape (2-D labels need D == 1)");
    TEM_REQUIRE((flags & ~31) == 0 && (flags & (DT_DIST | DT_DIRECTED)),
                "tem_distance_targets: at least one of distances and directed distances required");
    TEM_REQUIRE(N <= 65535, "tem_distance_targets: at most 65535 samples per call");
    if (ws_bytes < tem_distance_targets_ws(N, W)) {
        tem_set_error("tem_distance_targets: workspace too small");
        return TEM_EWS;
    }
    // reference :413-417: 0 if invert else sqrt(|shape|^2 / 2)
    const double sumsq = (ndim == 3 ? (double)D * D : 0.0) + (double)H * H + (double)W * W;
    const double fill = (flags & DT_INVERT) ? 0.0 : sqrt(sumsq / 2);
    hipStream_t st = (hipStream_t)stream;
    int* mx = (int*)ws;
    const int64_t rows = (int64_t)D * H, NV = rows * W * N;
    const int gx = (int)tem_cdiv(W, 256);
    int64_t gy = tem_cdiv(2048, (int64_t)gx * N);
    if (gy > rows) gy = rows;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(k_dt_init, dim3(tem_grid_1d((int64_t)N * (1 + 6 * (int64_t)W), 256)), dim3(256), 0, st, mx, N, W);
    hipLaunchKernelGGL(k_dt_max, dim3(gx, (unsigned)gy, N), dim3(256), 0, st, vec, d2, mx, D, H, W, ndim);
    hipLaunchKernelGGL(k_dt_write, dim3(tem_grid_1d(NV, 256)), dim3(256), 0, st, vec, d2, empty, mx, out, N, D, H, W, ndim,
                       flags, max_distance, fill);
    TEM_CHECK_LAUNCH("tem_distance_targets");
    return TEM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// DistanceLoss / DiceBasedDistanceLoss on [N][3][V] prediction p and target t (strides sn, sc, sv each).
// m = t[:, 0] when masking distances in the background, else 1; channel 0 unmasked.  Per channel k, with
// pm = p_k * m_k, tm = t_k * m_k: sums[4k + 0..3] = (sum pm*tm, sum pm^2, sum tm^2, sum (pm - tm)^2).
// Dice term 1 - 2 A / max(P + T, eps) (loss/dice.py:65-67); MSE term E / (N * V).  d loss / d p_k = m_k (ca_k tm + cb_k pm).
// Per-block double partials in a fixed grid, summed in block order: bitwise reproducible.
// ---------------------------------------------------------------------------------------------------------------
#define DL_BLOCKS 1024
#define DL_NS 12

extern "C" int64_t tem_dist_loss_ws(void) { return (int64_t)DL_BLOCKS * DL_NS * sizeof(double); }

__global__ __launch_bounds__(256) void k_dl_partial(const float* __restrict__ p, int64_t p_sn, int64_t p_sc, int64_t p_sv,
                                                    const float* __restrict__ t, int64_t t_sn, int64_t t_sc, int64_t t_sv,
                                                    int N, int64_t V, int mask_bg, double* __restrict__ part) {
    __shared__ double sh[4][DL_NS];
    double acc[DL_NS];
#pragma unroll
    for (int k = 0; k < DL_NS; ++k) acc[k] = 0.0;
    const int64_t NV = (int64_t)N * V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)DL_BLOCKS * 256) {
        const int64_t n = g / V, v = g % V;
        const float* pp = p + n * p_sn + v * p_sv;
        const float* tt = t + n * t_sn + v * t_sv;
        const float t0 = tt[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m = (k > 0 && mask_bg) ? t0 : 1.f;
            const double pm = (double)(pp[k * p_sc] * m), tm = (double)(tt[k * t_sc] * m);
            acc[4 * k + 0] += pm * tm;
            acc[4 * k + 1] += pm * pm;
            acc[4 * k + 2] += tm * tm;
            acc[4 * k + 3] += (pm - tm) * (pm - tm);
        }
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < DL_NS; ++k) {
        const double s = tem_wave_sum_d(acc[k]);
        if (lane_id() == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < DL_NS)
        part[(int64_t)blockIdx.x * DL_NS + threadIdx.x] =
            ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// sums in block order; loss and the gradient coefficients coef[0..2] = ca, coef[3..5] = cb
__global__ void k_dl_finalize(const double* __restrict__ part, int64_t count, int mse, double eps_fg, double eps_dist,
                              double* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ double s[DL_NS];
    if (threadIdx.x < DL_NS) {
        double a = 0.0;
        for (int b = 0; b < DL_BLOCKS; ++b) a += part[(int64_t)b * DL_NS + threadIdx.x];
        s[threadIdx.x] = a;
        sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double A = s[4 * k], den = s[4 * k + 1] + s[4 * k + 2], E = s[4 * k + 3];
        if (k > 0 && mse) {
            total += E / (double)count;
            coef[k] = (float)(-2.0 / (double)count);
            coef[3 + k] = (float)(2.0 / (double)count);
        } else {
            const double eps = k == 0 ? eps_fg : eps_dist;
            const double cd = den < eps ? eps : den;
            total += 1.0 - 2.0 * A / cd;
            coef[k] = (float)(-2.0 / cd);
            coef[3 + k] = (float)(den >= eps ? 4.0 * A / (cd * cd) : 0.0);
        }
    }
    loss[0] = (float)total;
}

__global__ __launch_bounds__(256) void k_dl_grad(const float* __restrict__ p, int64_t p_sn, int64_t p_sc, int64_t p_sv,
                                                 const float* __restrict__ t, int64_t t_sn, int64_t t_sc, int64_t t_sv,
                                                 const float* __restrict__ coef, const float* __restrict__ gout,
                                                 float* __restrict__ gp, int N, int64_t V, int mask_bg) {
    const float go = gout[0];
    float ca[3], cb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ca[k] = coef[k] * go;
        cb[k] = coef[3 + k] * go;
    }
    const int64_t NV = (int64_t)N * V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < NV; g += (int64_t)gridDim.x * 256) {
        const int64_t n = g / V, v = g % V;
        const int64_t po = n * p_sn + v * p_sv;
        const float* tt = t + n * t_sn + v * t_sv;
        const float t0 = tt[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m = (k > 0 && mask_bg) ? t0 : 1.f;
            const float pm = p[po + k * p_sc] * m, tm = tt[k * t_sc] * m;
            gp[po + k * p_sc] = m * (ca[k] * tm + cb[k] * pm);
        }
    }
}

extern "C" int tem_dist_loss_fwd(const float* p, int64_t p_sn, int64_t p_sc, int64_t p_sv, const float* t, int64_t t_sn,
                                 int64_t t_sc, int64_t t_sv, int N, int64_t V, int mask_bg, int mse, double eps_fg,
                                 double eps_dist, double* sums, float* loss, float* coef, void* ws, int64_t ws_bytes,
                                 tem_stream_t stream) {
    TEM_REQUIRE(p && t && sums && loss && coef && ws, "tem_dist_loss_fwd: null pointer");
    TEM_REQUIRE(N > 0 && V > 0, "tem_dist_loss_fwd: bad shape");
    if (ws_bytes < tem_dist_loss_ws()) {
        tem_set_error("tem_dist_loss_fwd: workspace too small");
        return TEM_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dl_partial, dim3(DL_BLOCKS), dim3(256), 0, st, p, p_sn, p_sc, p_sv, t, t_sn, t_sc, t_sv, N, V,
                       mask_bg, (double*)ws);
    hipLaunchKernelGGL(k_dl_finalize, dim3(1), dim3(64), 0, st, (const double*)ws, (int64_t)N * V, mse, eps_fg, eps_dist,
                       sums, loss, coef);
    TEM_CHECK_LAUNCH("tem_dist_loss_fwd");
    return TEM_OK;
}

extern "C" int tem_dist_loss_grad(const float* p, int64_t p_sn, int64_t p_sc, int64_t p_sv, const float* t, int64_t t_sn,
                                  int64_t t_sc, int64_t t_sv, const float* coef, const float* gout, float* gp, int N,
                                  int64_t V, int mask_bg, tem_stream_t stream) {
    TEM_REQUIRE(p && t && coef && gout && gp, "tem_dist_loss_grad: null pointer");
    TEM_REQUIRE(N > 0 && V > 0, "tem_dist_loss_grad: bad shape");
    hipLaunchKernelGGL(k_dl_grad, dim3(tem_grid_1d((int64_t)N * V, 256)), dim3(256), 0, (hipStream_t)stream, p, p_sn,
                       p_sc, p_sv, t, t_sn, t_sc, t_sv, coef, gout, gp, N, V, mask_bg);
    TEM_CHECK_LAUNCH("tem_dist_loss_grad");
    return TEM_OK;
}
