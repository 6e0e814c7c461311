// embmws.hip -- the two ends of an embedding mutex watershed (DESIGN.md "Embedding mutex watershed"): embeddings to edge
// weights for every offset, with the strided repulsive-edge mask (tem_emb_edges), and the background merge of the
// segmentation by mean embedding (tem_emb_bg_stats).  The mutex watershed itself is mws.hip.
//
// tem_emb_edges.  For voxel v and u = v + o_c inside the sample: d = sqrt(sum_e (x_e(v) - x_e(u))^2) (l1: sum_e |.|),
// s = (max(2 delta - d, 0) / (2 delta))^2, aff = 1 - s; aff = 0 where u is outside.  Every difference, product, sum and the
// final 1 - s is one float32 operation, the sum runs over the channels in ascending order from 0, sqrt and the division are
// the correctly rounded ones: a numpy float32 expression gives the same bits.  No a*b+c here may become an fma (the pragma
// below and -ffp-contract=off in the Makefile).
//
// One work-group (256 threads) owns EE_TH consecutive rows x EE_TW columns of one plane; a thread owns four consecutive
// voxels of a row.  The embedding tile with a halo of EE_HALO rows and columns is staged in LDS in chunks of EE_EC channels:
// an in-plane offset within the halo (dz = 0, |dy|, |dx| <= EE_HALO) reads its far ends there.  Every other offset (9, 27,
// any dz) reads them from global memory: a shift keeps the four voxels contiguous, so that is one 16-byte load where all
// four ends are inside the row.  Offsets are taken EE_G at a time: 4 x EE_G running sums in registers whatever C is.  The
// same thread writes edge_valid, four bytes as one word.  The kernel is memory-bound; the byte floor is (E + 5 C / 4) V 4.
//
// tem_emb_bg_stats.  ids 1..n (0: ignored and kept) -> keep[N][V + 1]: 0 for the segments that merge into the background.
// Counts by wave-aggregated integer atomics; bg = the largest count, ties to the lowest id, as one 64-bit atomicMax key;
// per channel the per-segment sums in 64-bit fixed point (2^-28; integer adds commute, so the atomics give one answer from
// run to run), folded channel by channel, in ascending order, into the float64 squared distance of the segment's mean to the
// background's; keep = !(p > 0.5) with p = (max(2 delta - dist, 0) / (2 delta))^2 in float64.  The two sum buffers
// alternate: folding channel e clears the buffer channel e + 1 adds into.
#include <limits.h>

#include "tem_common.h"

#pragma clang fp contract(off)

#define EE_TW 128              // tile columns: 32 threads x 4 voxels
#define EE_TH 8                // tile rows
#define EE_HALO 4              // rows / columns of halo in LDS
#define EE_EC 4                // embedding channels a stage
#define EE_G 8                 // offsets a pass
#define EE_LW (EE_TW + 2 * EE_HALO)
#define EE_LH (EE_TH + 2 * EE_HALO)
#define EE_FIX 268435456.0     // 2^28

typedef unsigned long long ee_u64;

struct EeGeom {
    int N, E, D, H, W, C, n_attr;
    int sz, sy, sx;
    int off[TEM_MWS_MAX_CHANNELS][3];   // (dz, dy, dx)
};

struct __attribute__((packed, aligned(4))) EeF4 { float v[4]; };   // 16 bytes at any 4-byte boundary

// one block = one tile of one plane; grid = N * D * tiles_y * tiles_x
template <bool L1>
__global__ __launch_bounds__(256) void k_emb_edges(const float* __restrict__ emb, float* __restrict__ aff, uint8_t* __restrict__ valid,
                                                   EeGeom g, float two_delta, int vec_ok) {
    __shared__ __attribute__((aligned(16))) float sm[EE_EC][EE_LH][EE_LW];
    const int tx_n = (g.W + EE_TW - 1) / EE_TW, ty_n = (g.H + EE_TH - 1) / EE_TH;
    int b = blockIdx.x;
    const int tx = b % tx_n;
    b /= tx_n;
    const int ty = b % ty_n;
    b /= ty_n;
    const int z = b % g.D, n = b / g.D;
    const int64_t HW = (int64_t)g.H * g.W, V = HW * g.D;
    const int lx = (threadIdx.x & 31) * 4, ly = threadIdx.x >> 5;
    const int x0 = tx * EE_TW, y0 = ty * EE_TH;
    const int x = x0 + lx, y = y0 + ly;
    const bool row_in = y < g.H;
    const float* src = emb + (int64_t)n * g.E * V;           // the sample's embedding
    const int64_t at = (int64_t)z * HW + (int64_t)y * g.W + x;   // the thread's first voxel in the sample (when inside)

    for (int c0 = 0; c0 < g.C; c0 += EE_G) {
        const int ng = g.C - c0 < EE_G ? g.C - c0 : EE_G;
        // bit 4 j + i: voxel i of the thread is inside and its far end along offset c0 + j is inside the sample
        unsigned ok = 0;
#pragma unroll
        for (int j = 0; j < EE_G; ++j) {
            if (j >= ng) break;
            const int zz = z + g.off[c0 + j][0], yy = y + g.off[c0 + j][1];
            const bool r = row_in && zz >= 0 && zz < g.D && yy >= 0 && yy < g.H;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xx = x + i + g.off[c0 + j][2];
                if (r && x + i < g.W && xx >= 0 && xx < g.W) ok |= 1u << (4 * j + i);
            }
        }
        float acc[EE_G][4];
#pragma unroll
        for (int j = 0; j < EE_G; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = 0.0f;

        for (int e0 = 0; e0 < g.E; e0 += EE_EC) {
            const int ec = g.E - e0 < EE_EC ? g.E - e0 : EE_EC;
            __syncthreads();   // the previous stage has been read
            // stage ec channels of rows y0 - HALO .. y0 + TH + HALO - 1, columns x0 - HALO .. x0 + TW + HALO - 1; 0 outside the plane
            for (int t = threadIdx.x; t < ec * EE_LH * (EE_LW / 4); t += 256) {
                const int q = t % (EE_LW / 4), r = (t / (EE_LW / 4)) % EE_LH, e = t / ((EE_LW / 4) * EE_LH);
                const int gy = y0 - EE_HALO + r, gx = x0 - EE_HALO + 4 * q;
                float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gy >= 0 && gy < g.H) {
                    const float* p = src + (int64_t)(e0 + e) * V + (int64_t)z * HW + (int64_t)gy * g.W + gx;
                    if (vec_ok) {   // W % 4 == 0 and gx % 4 == 0: the four columns are inside together or not at all
                        if (gx >= 0 && gx < g.W) val = *(const float4*)p;
                    } else {
                        if (gx >= 0 && gx < g.W) val.x = p[0];
                        if (gx + 1 >= 0 && gx + 1 < g.W) val.y = p[1];
                        if (gx + 2 >= 0 && gx + 2 < g.W) val.z = p[2];
                        if (gx + 3 >= 0 && gx + 3 < g.W) val.w = p[3];
                    }
                }
                *(float4*)&sm[e][r][4 * q] = val;
            }
            __syncthreads();
            for (int e = 0; e < ec; ++e) {
                const float4 own4 = *(const float4*)&sm[e][ly + EE_HALO][lx + EE_HALO];
                const float own[4] = {own4.x, own4.y, own4.z, own4.w};
                const float* plane = src + (int64_t)(e0 + e) * V;
#pragma unroll
                for (int j = 0; j < EE_G; ++j) {
                    if (j >= ng) break;
                    const int dz = g.off[c0 + j][0], dy = g.off[c0 + j][1], dx = g.off[c0 + j][2];
                    const unsigned m = (ok >> (4 * j)) & 15u;
                    float far[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (dz == 0 && dy >= -EE_HALO && dy <= EE_HALO && dx >= -EE_HALO && dx <= EE_HALO) {
                        const float* row = &sm[e][ly + EE_HALO + dy][lx + EE_HALO + dx];
#pragma unroll
                        for (int i = 0; i < 4; ++i) far[i] = row[i];
                    } else if (m == 15u) {
                        const EeF4 f = *(const EeF4*)(plane + at + (int64_t)dz * HW + (int64_t)dy * g.W + dx);
#pragma unroll
                        for (int i = 0; i < 4; ++i) far[i] = f.v[i];
                    } else if (m != 0u) {
                        const float* p = plane + at + (int64_t)dz * HW + (int64_t)dy * g.W + dx;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (m & (1u << i)) far[i] = p[i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float df = own[i] - far[i];
                        const float term = L1 ? __builtin_fabsf(df) : df * df;
                        acc[j][i] = acc[j][i] + term;
                    }
                }
            }
        }

        if (!row_in || x >= g.W) continue;   // no barrier below depends on this thread: the loop's barriers come first for all
#pragma unroll
        for (int j = 0; j < EE_G; ++j) {
            if (j >= ng) break;
            const int c = c0 + j;
            const unsigned m = (ok >> (4 * j)) & 15u;
            float a[4];
            uint8_t ev[4];
            const bool rep_row = c < g.n_attr || (z % g.sz == 0 && y % g.sy == 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = L1 ? acc[j][i] : __builtin_sqrtf(acc[j][i]);
                const float h = __builtin_fmaxf(two_delta - d, 0.0f);
                const float r = h / two_delta;
                const float s = r * r;
                a[i] = (m & (1u << i)) ? 1.0f - s : 0.0f;
                ev[i] = (c < g.n_attr || (rep_row && (x + i) % g.sx == 0)) ? 1 : 0;
            }
            const int64_t o = ((int64_t)n * g.C + c) * V + at;
            if (vec_ok) {   // x % 4 == 0, W % 4 == 0: four voxels inside, 16-byte aligned
                *(float4*)(aff + o) = make_float4(a[0], a[1], a[2], a[3]);
                *(uint32_t*)(valid + o) = (uint32_t)ev[0] | ((uint32_t)ev[1] << 8) | ((uint32_t)ev[2] << 16) | ((uint32_t)ev[3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < g.W) {
                        aff[o + i] = a[i];
                        valid[o + i] = ev[i];
                    }
            }
        }
    }
}

// ---- background merge -------------------------------------------------------------------------------------------------------
struct EeBg {
    ee_u64* key;       // [N]: (count << 32) | (0xffffffff - id) of the background segment
    int* cnt;          // [N][V + 1]
    long long* sum[2]; // [N][V + 1] each: fixed-point sums of one channel
    double* dist2;     // [N][V + 1]
};

__global__ __launch_bounds__(256) void k_embg_zero(ee_u64* __restrict__ p, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

// cnt[slot of the voxel's id] += 1 (E_SUM: sum[slot] += the fixed-point value).  The lanes of a wave's first segment add
// once (a wave inside one segment: one atomic), the others one each; every lane of a wave makes the same number of trips.
template <bool E_SUM>
__global__ __launch_bounds__(256) void k_embg_add(const int* __restrict__ ids, const float* __restrict__ emb, int e, int E,
                                                  int* __restrict__ cnt, long long* __restrict__ sum, int64_t V, int64_t NV) {
    for (int64_t base = (int64_t)blockIdx.x * 256; base < NV; base += (int64_t)gridDim.x * 256) {
        const int64_t gi = base + threadIdx.x;
        const int id = gi < NV ? ids[gi] : 0;
        const int64_t n = gi < NV ? gi / V : 0;
        const int64_t slot = id > 0 && id <= V ? n * (V + 1) + id : -1;
        long long val = 1;
        if (E_SUM) val = slot >= 0 ? __double2ll_rn((double)emb[(n * E + e) * V + (gi - n * V)] * EE_FIX) : 0;
        if (E_SUM) tem_wave_atomic_add<1>((ee_u64*)sum, slot, slot >= 0, (ee_u64)val);
        else tem_wave_atomic_add<1>(cnt, slot, slot >= 0, 1);
    }
}

__global__ __launch_bounds__(256) void k_embg_argmax(const int* __restrict__ cnt, ee_u64* key, int64_t V, int64_t NS) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (int64_t)gridDim.x * 256) {
        const int64_t n = s / (V + 1), id = s - n * (V + 1);
        const int c = cnt[s];
        if (id == 0 || c <= 0) continue;
        const ee_u64 k = ((ee_u64)(unsigned)c << 32) | (ee_u64)(0xffffffffu - (unsigned)id);
        if (k > __hip_atomic_load(&key[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&key[n], k);
    }
}

// dist2[k] += (mean_k - mean_bg)^2 for the channel whose sums are in `cur`; `nxt` (the buffer of the next channel) is cleared
__global__ __launch_bounds__(256) void k_embg_fold(const int* __restrict__ cnt, const long long* __restrict__ cur,
                                                   long long* __restrict__ nxt, const ee_u64* __restrict__ key,
                                                   double* __restrict__ dist2, int64_t V, int64_t NS) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (int64_t)gridDim.x * 256) {
        nxt[s] = 0;
        const int64_t n = s / (V + 1);
        const int c = cnt[s];
        const ee_u64 k = key[n];
        if (c <= 0 || k == 0) continue;
        const int64_t bg = n * (V + 1) + (int64_t)(0xffffffffu - (unsigned)(k & 0xffffffffu));
        const double m = ((double)cur[s] * (1.0 / EE_FIX)) / (double)c;
        const double mb = ((double)cur[bg] * (1.0 / EE_FIX)) / (double)(unsigned)(k >> 32);
        const double df = m - mb;
        dist2[s] = dist2[s] + df * df;
    }
}

__global__ __launch_bounds__(256) void k_embg_keep(const int* __restrict__ cnt, const double* __restrict__ dist2,
                                                   int* __restrict__ keep, double two_delta, int64_t V, int64_t NS) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (int64_t)gridDim.x * 256) {
        int kp = 0;
        if (s % (V + 1) != 0 && cnt[s] > 0) {
            const double r = fmax(two_delta - sqrt(dist2[s]), 0.0) / two_delta;
            kp = (r * r > 0.5) ? 0 : 1;
        }
        keep[s] = kp;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tem_emb_edges(const float* emb, const int* offsets, int n_attractive, const int* strides, float delta, int distance_type,
                             int N, int E, int C, int D, int H, int W, float* aff, uint8_t* edge_valid, tem_stream_t stream) {
    TEM_REQUIRE(emb && offsets && strides && aff && edge_valid, "tem_emb_edges: null pointer");
    TEM_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && E >= 1 && E <= TEM_EMB_MAX_DIM && C >= 1 && C <= TEM_MWS_MAX_CHANNELS,
                "tem_emb_edges: bad shape (N, D, H, W positive, E within 1..%d, C within 1..%d)", TEM_EMB_MAX_DIM, TEM_MWS_MAX_CHANNELS);
    const int64_t V = (int64_t)D * H * W;
    TEM_REQUIRE(V < INT_MAX, "tem_emb_edges: D*H*W must be below 2^31 - 1");
    TEM_REQUIRE(n_attractive >= 0 && n_attractive <= C, "tem_emb_edges: n_attractive %d outside 0..%d", n_attractive, C);
    TEM_REQUIRE(delta > 0.0f && delta < 1e18f, "tem_emb_edges: delta must be positive and finite");
    TEM_REQUIRE(distance_type == TEM_EMB_L2 || distance_type == TEM_EMB_L1, "tem_emb_edges: distance_type is TEM_EMB_L2 or TEM_EMB_L1");
    TEM_REQUIRE(strides[0] >= 1 && strides[1] >= 1 && strides[2] >= 1, "tem_emb_edges: strides must be >= 1");
    TEM_REQUIRE((((uintptr_t)emb | (uintptr_t)aff) & 3u) == 0, "tem_emb_edges: float pointers must be 4-byte aligned");
    EeGeom g;
    g.N = N, g.E = E, g.D = D, g.H = H, g.W = W, g.C = C, g.n_attr = n_attractive;
    g.sz = strides[0], g.sy = strides[1], g.sx = strides[2];
    for (int c = 0; c < TEM_MWS_MAX_CHANNELS; ++c)
        for (int k = 0; k < 3; ++k) {
            const int o = c < C ? offsets[c * 3 + k] : 0;
            TEM_REQUIRE(o > -(1 << 30) && o < (1 << 30), "tem_emb_edges: offset %d of channel %d is out of range", o, c);
            g.off[c][k] = o;
        }
    const int64_t blocks = (int64_t)N * D * tem_cdiv(H, EE_TH) * tem_cdiv(W, EE_TW);
    TEM_REQUIRE(blocks < INT_MAX, "tem_emb_edges: too many tiles");
    // 16-byte loads and stores of four voxels of a row: rows start on a 16-byte boundary in all three tensors
    const int vec_ok = (W % 4 == 0 && (((uintptr_t)emb | (uintptr_t)aff) & 15u) == 0 && ((uintptr_t)edge_valid & 3u) == 0) ? 1 : 0;
    const float two_delta = 2.0f * delta;
    hipStream_t st = (hipStream_t)stream;
    if (distance_type == TEM_EMB_L1)
        hipLaunchKernelGGL(k_emb_edges<true>, dim3((unsigned)blocks), dim3(256), 0, st, emb, aff, edge_valid, g, two_delta, vec_ok);
    else
        hipLaunchKernelGGL(k_emb_edges<false>, dim3((unsigned)blocks), dim3(256), 0, st, emb, aff, edge_valid, g, two_delta, vec_ok);
    TEM_CHECK_LAUNCH("tem_emb_edges");
    return TEM_OK;
}

static bool embg_shape_ok(int N, int E, int64_t V) {
    return N > 0 && E >= 1 && E <= TEM_EMB_MAX_DIM && V > 0 && V < INT_MAX - 1 && (int64_t)N * (V + 1) < INT_MAX;
}

static int64_t embg_head_bytes(int N) { return tem_align_up((int64_t)N * 8, 16); }

extern "C" int64_t tem_emb_bg_ws(int N, int64_t V) {
    if (!embg_shape_ok(N, 1, V)) return -1;
    const int64_t NS = (int64_t)N * (V + 1);
    return embg_head_bytes(N) + 3 * NS * 8 + tem_align_up(NS * 4, 16);
}

extern "C" int tem_emb_bg_stats(const int* ids, const float* emb, int N, int E, int64_t V, double delta, int* keep, void* ws,
                                int64_t ws_bytes, tem_stream_t stream) {
    TEM_REQUIRE(ids && emb && keep && ws, "tem_emb_bg_stats: null pointer");
    TEM_REQUIRE(embg_shape_ok(N, E, V), "tem_emb_bg_stats: bad shape (N, V positive, E within 1..%d, N*(V+1) below 2^31 - 1)",
                TEM_EMB_MAX_DIM);
    TEM_REQUIRE(delta > 0.0 && delta < 1e18, "tem_emb_bg_stats: delta must be positive and finite");
    TEM_REQUIRE(((uintptr_t)ws & 15u) == 0, "tem_emb_bg_stats: the workspace must be 16-byte aligned");
    if (ws_bytes < tem_emb_bg_ws(N, V)) {
        tem_set_error("tem_emb_bg_stats: workspace too small (%lld bytes, %lld needed)", (long long)ws_bytes, (long long)tem_emb_bg_ws(N, V));
        return TEM_EWS;
    }
    const int64_t NS = (int64_t)N * (V + 1), NV = (int64_t)N * V;
    EeBg w;
    w.key = (ee_u64*)ws;
    w.sum[0] = (long long*)((char*)ws + embg_head_bytes(N));
    w.sum[1] = w.sum[0] + NS;
    w.dist2 = (double*)(w.sum[1] + NS);
    w.cnt = (int*)(w.dist2 + NS);
    const int gv = tem_grid_1d(NV, 256), gs = tem_grid_1d(NS, 256);
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = tem_emb_bg_ws(N, V) / 8;
    hipLaunchKernelGGL(k_embg_zero, dim3(tem_grid_1d(words, 256)), dim3(256), 0, st, (ee_u64*)ws, words);
    hipLaunchKernelGGL(k_embg_add<false>, dim3(gv), dim3(256), 0, st, ids, emb, 0, E, w.cnt, w.sum[0], V, NV);
    hipLaunchKernelGGL(k_embg_argmax, dim3(gs), dim3(256), 0, st, w.cnt, w.key, V, NS);
    for (int e = 0; e < E; ++e) {
        hipLaunchKernelGGL(k_embg_add<true>, dim3(gv), dim3(256), 0, st, ids, emb, e, E, w.cnt, w.sum[e & 1], V, NV);
        hipLaunchKernelGGL(k_embg_fold, dim3(gs), dim3(256), 0, st, w.cnt, w.sum[e & 1], w.sum[(e + 1) & 1], w.key, w.dist2, V, NS);
    }
    hipLaunchKernelGGL(k_embg_keep, dim3(gs), dim3(256), 0, st, w.cnt, w.dist2, keep, 2.0 * delta, V, NS);
    TEM_CHECK_LAUNCH("tem_emb_bg_stats");
    return TEM_OK;
}
