// forest.hip -- predict_proba of a packed random forest over a feature-planar bank (DESIGN.md "Shallow2Deep front end").
//
// The forest (ops.pack_forest): nodes int32 [nodes][4] = (feature or -1 for a leaf, the bits of the float32 threshold, left
// child, right child; a leaf keeps its row of the leaf table in the third word), leaves float64 [rows][C] -- the normalised
// class fractions --, roots int32 [T].  A decision is `feature <= threshold` in float32: the stored threshold is the largest
// float32 that is <= sklearn's float64 threshold, so it is sklearn's decision for every float32 feature.  Non-finite
// features are outside the contract.
//
// One voxel a lane.  A block stages the F features of its 256 voxels ONCE into LDS as [F][256], read coalesced from the planar
// bank [N][F][V]; a lane reads back only its own column, so no barrier is needed, and the divergent per-node gathers of the
// walk hit LDS.  Node records are one 16-byte load each and stay in L2 (a forest is a few MB at most).  Per class the leaf rows
// are summed in float64 registers in tree order, divided by the tree count and rounded once to float32: predict_proba's own
// arithmetic.  The selected classes alone are stored: out [N][n_sel][V].
#include "tem_common.h"

#define FR_BLOCK 256

struct FrSel {
    int n;
    int cls[TEM_FOREST_MAX_CLASSES];
};

__global__ __launch_bounds__(FR_BLOCK) void k_forest(const float* __restrict__ bank, const int4* __restrict__ nodes, const double* __restrict__ leaves,
                                                     const int* __restrict__ roots, int T, int F, int C, int64_t V, FrSel sel,
                                                     float* __restrict__ out) {
    extern __shared__ float fr_feat[];   // [F][FR_BLOCK]
    const int tid = threadIdx.x, n = blockIdx.y;
    const int64_t v = (int64_t)blockIdx.x * FR_BLOCK + tid;
    if (v >= V) return;   // no barrier below
    const float* b = bank + (int64_t)n * F * V + v;
    for (int f = 0; f < F; ++f) fr_feat[f * FR_BLOCK + tid] = b[(int64_t)f * V];
    double sum[TEM_FOREST_MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < TEM_FOREST_MAX_CLASSES; ++c) sum[c] = 0.0;
    for (int t = 0; t < T; ++t) {
        int4 nd = nodes[roots[t]];
        while (nd.x >= 0) nd = nodes[fr_feat[nd.x * FR_BLOCK + tid] <= __builtin_bit_cast(float, nd.y) ? nd.z : nd.w];
        const double* row = leaves + (int64_t)nd.z * C;
#pragma unroll
        for (int c = 0; c < TEM_FOREST_MAX_CLASSES; ++c)
            if (c < C) sum[c] += row[c];
    }
    for (int j = 0; j < sel.n; ++j) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < TEM_FOREST_MAX_CLASSES; ++c) s = sel.cls[j] == c ? sum[c] : s;
        out[((int64_t)n * sel.n + j) * V + v] = (float)(s / (double)T);
    }
}

// the walk of k_forest can only leave the tables if they are inconsistent: checked once, on the host, where they are made
// (ops.pack_forest); here the sizes and the selection
extern "C" int tem_forest_predict(const float* bank, int N, int F, int64_t V, const int* nodes, const double* leaves, const int* roots,
                                  int T, int C, const int* sel, int n_sel, float* out, tem_stream_t stream) {
    const char* who = "tem_forest_predict";
    TEM_REQUIRE(bank && nodes && leaves && roots && sel && out, "%s: null pointer", who);
    TEM_REQUIRE(N > 0 && N <= 65535 && V > 0 && T > 0, "%s: bad sizes (N within 1..65535, V and the tree count positive)", who);
    TEM_REQUIRE(F >= 1 && F <= TEM_FOREST_MAX_FEATURES, "%s: %d features outside 1..%d", who, F, TEM_FOREST_MAX_FEATURES);
    TEM_REQUIRE(C >= 1 && C <= TEM_FOREST_MAX_CLASSES, "%s: %d classes outside 1..%d", who, C, TEM_FOREST_MAX_CLASSES);
    TEM_REQUIRE(n_sel >= 1 && n_sel <= TEM_FOREST_MAX_CLASSES, "%s: %d output channels outside 1..%d", who, n_sel, TEM_FOREST_MAX_CLASSES);
    TEM_REQUIRE(tem_cdiv(V, FR_BLOCK) < INT32_MAX, "%s: too many voxels a sample", who);
    TEM_REQUIRE(((uintptr_t)nodes & 15u) == 0, "%s: the node table must be 16-byte aligned", who);
    FrSel s;
    s.n = n_sel;
    for (int j = 0; j < TEM_FOREST_MAX_CLASSES; ++j) {
        s.cls[j] = j < n_sel ? sel[j] : 0;
        TEM_REQUIRE(s.cls[j] >= 0 && s.cls[j] < C, "%s: output channel %d outside the %d classes", who, s.cls[j], C);
    }
    hipLaunchKernelGGL(k_forest, dim3((unsigned)tem_cdiv(V, FR_BLOCK), N), dim3(FR_BLOCK), (size_t)F * FR_BLOCK * sizeof(float),
                       (hipStream_t)stream, bank, (const int4*)nodes, leaves, roots, T, F, C, V, s, out);
    TEM_CHECK_LAUNCH(who);
    return TEM_OK;
}
