// conv.hip -- convolution entry points (reference nn.Conv3d/nn.Conv2d inside ConvBlock,
// Upsampler.conv and out_conv: model/unet.py:417-438,453,638, and their autograd backward),
// weight (un)packing, and the VALU kernels used where the MFMA path does not apply:
// Cin==1 first layer (HBM-bound, 13 flop/B), the 32->Cout<=16 output projection
// (HBM-bound, 0.9 flop/B) and the small test networks.
#include <stdarg.h>
#include "tem_common.h"
#include "conv_internal.h"
#include "conv_arith.h"
#include "tem_act.h"

// `use_mfma` of the conv entry points carries the storage types of the call in its high bits (tem_hip.h: TEM_MFMA_STX / _STY):
// every entry point splits it ONCE, into the arithmetic mode (left in use_mfma) and the call descriptor that goes down to the
// launchers and dispatch queries (conv_internal.h: TemConvCall); the entry point adds what else its arguments carry
static TemConvCall conv_call(int& use_mfma) {
    const TemConvCall c = {(use_mfma >> 8) & 15, (use_mfma >> 12) & 15};
    use_mfma &= 0xff;
    return c;
}

// ---------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------
extern "C" int64_t tem_conv_packed_size(int Cout, int Cin, int kd, int kh, int kw) {
    // floats; the bf16x6 layout stores 3 bf16 planes = 1.5 floats per weight
    return ((int64_t)Cout * Cin * kd * kh * kw * 3 + 1) / 2;
}

__global__ __launch_bounds__(256) void k_pack_weights(const float* __restrict__ w, float* __restrict__ dst, int Cout,
                                                      int Cin, int KD, int KH, int KW, int transpose, int layout) {
    const int ntaps = KD * KH * KW;
    const int64_t total = (int64_t)Cout * Cin * ntaps;
    // logical operator: CoutL x CinL
    const int CoutL = transpose ? Cin : Cout, CinL = transpose ? Cout : Cin;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        // enumerate logical (tap, ci, co), co fastest
        int co = (int)(i % CoutL);
        int64_t r = i / CoutL;
        int ci = (int)(r % CinL);
        int tap = (int)(r / CinL);
        int tz = tap / (KH * KW), ty = (tap / KW) % KH, tx = tap % KW;
        float val;
        if (!transpose) {
            val = w[(((int64_t)co * Cin + ci) * KD + tz) * KH * KW + ty * KW + tx];
        } else {
            // Wl[co][ci][tap] = w[ci][co][flip(tap)]  (source is [Cout=CinL][Cin=CoutL])
            val = w[(((int64_t)ci * Cin + co) * KD + (KD - 1 - tz)) * KH * KW + (KH - 1 - ty) * KW + (KW - 1 - tx)];
        }
        int64_t o;
        if (layout == TEM_WL_GENERIC) {
            o = ((int64_t)tap * CinL + ci) * CoutL + co;
        } else {
            int nt = co >> 5, col = co & 31, c8 = ci >> 3, kh = (ci >> 2) & 1, j = ci & 3;
            o = (((((int64_t)nt * ntaps + tap) * (CinL >> 3) + c8) * 2 + kh) * 32 + col) * 4 + j;
        }
        dst[o] = val;
    }
}

extern "C" int tem_conv_pack_weights(const float* w, float* dst, int Cout, int Cin, int kd, int kh, int kw,
                                     int transpose, int layout, tem_stream_t stream) {
    TEM_REQUIRE(w && dst && Cout > 0 && Cin > 0, "tem_conv_pack_weights: bad arguments");
    TEM_REQUIRE((kd == 1 || kd == 3) && (kh == 1 || kh == 3) && (kw == 1 || kw == 3),
                "tem_conv_pack_weights: kernel size (%d,%d,%d) not supported (1 or 3 per axis)", kd, kh, kw);
    if (tem_layout_is_split(layout)) {
        int rc = tem_pack_weights_bf16x3(w, dst, Cout, Cin, kd, kh, kw, transpose, tem_arith(layout).planes, tem_arith(layout).pack,
                                         (hipStream_t)stream);
        if (rc != TEM_OK) return rc;
        TEM_CHECK_LAUNCH("tem_conv_pack_weights(bf16x3)");
        return TEM_OK;
    }
    if (layout == TEM_WL_MFMA) {
        int CoutL = transpose ? Cin : Cout, CinL = transpose ? Cout : Cin;
        TEM_REQUIRE(CinL % 16 == 0 && CoutL % 32 == 0, "tem_conv_pack_weights: MFMA layout needs Cin%%16==0, Cout%%32==0");
    } else {
        TEM_REQUIRE(layout == TEM_WL_GENERIC, "tem_conv_pack_weights: unknown layout %d", layout);
    }
    int64_t total = (int64_t)Cout * Cin * kd * kh * kw;
    hipLaunchKernelGGL(k_pack_weights, dim3(tem_grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, w, dst, Cout,
                       Cin, kd, kh, kw, transpose, layout);
    TEM_CHECK_LAUNCH("tem_conv_pack_weights");
    return TEM_OK;
}

__global__ __launch_bounds__(256) void k_unpack_wgrad(const float* __restrict__ src, float* __restrict__ dw, int Cout,
                                                      int Cin, int ntaps) {
    const int64_t total = (int64_t)Cout * Cin * ntaps;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        // i enumerates the destination [co][ci][tap]
        int tap = (int)(i % ntaps);
        int64_t r = i / ntaps;
        int ci = (int)(r % Cin);
        int co = (int)(r / Cin);
        dw[i] = src[((int64_t)tap * Cin + ci) * Cout + co];
    }
}

extern "C" int tem_conv_unpack_wgrad(const float* src, float* dw, int Cout, int Cin, int kd, int kh, int kw,
                                     tem_stream_t stream) {
    TEM_REQUIRE(src && dw && Cout > 0 && Cin > 0, "tem_conv_unpack_wgrad: bad arguments");
    int64_t total = (int64_t)Cout * Cin * kd * kh * kw;
    hipLaunchKernelGGL(k_unpack_wgrad, dim3(tem_grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dw, Cout,
                       Cin, kd * kh * kw);
    TEM_CHECK_LAUNCH("tem_conv_unpack_wgrad");
    return TEM_OK;
}

// ---------------------------------------------------------------------------
// generic VALU forward: thread <-> (voxel, co), co fastest.  Lanes that share a
// voxel broadcast the x reads; weight reads and the output store are coalesced.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == TEM_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == TEM_ACT_SIGMOID) return 1.f / (1.f + __expf(-v));
    return v;
}

template <int KD, int KH, int KW, typename TX, typename TY>
__global__ __launch_bounds__(256) void k_conv_fwd_generic(const TX* __restrict__ x, int64_t x_ld,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ w,
                                                          const float* __restrict__ bias, TY* __restrict__ y,
                                                          int64_t y_ld, const TY* __restrict__ ref, int64_t ref_ld,
                                                          int N, int D, int H, int W, int Cin, int Cout, int act) {
    constexpr int PZ = KD / 2, PY = KH / 2, PX = KW / 2;
    const int64_t NV = (int64_t)N * D * H * W;
    const int64_t items = NV * Cout;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t v = i / Cout;
    int co = (int)(i % Cout);
    const int64_t dv = stride / Cout;
    const int dco = (int)(stride % Cout);
    for (; i < items; i += stride, v += dv, co += dco) {
        if (co >= Cout) {
            co -= Cout;
            ++v;
        }
        float acc = bias ? bias[co] : 0.f;
        if constexpr (KD * KH * KW == 1) {
            const int n1 = scale ? (int)(v / ((int64_t)D * H * W)) : 0;
            const TX* xp = x + v * x_ld;
            for (int ci = 0; ci < Cin; ++ci) {
                float xv = act_ld1(xp + ci);
                if (scale) xv = fmaf(xv, scale[(int64_t)n1 * Cin + ci], shift[(int64_t)n1 * Cin + ci]);
                acc = fmaf(xv, w[(int64_t)ci * Cout + co], acc);
            }
            acc = apply_act(acc, act);
            if (ref && !(act_ld1(ref + v * ref_ld + co) > 0.f)) acc = 0.f;
            act_st1(y + v * y_ld + co, acc);
            continue;
        }
        int xx = (int)(v % W);
        int64_t r = v / W;
        int yy = (int)(r % H);
        r /= H;
        int zz = (int)(r % D);
        int n = (int)(r / D);
        const float* sc = scale ? scale + (int64_t)n * Cin : nullptr;
        const float* sf = shift ? shift + (int64_t)n * Cin : nullptr;
#pragma unroll
        for (int tz = 0; tz < KD; ++tz) {
            int z2 = zz + tz - PZ;
            if (z2 < 0 || z2 >= D) continue;
#pragma unroll
            for (int ty = 0; ty < KH; ++ty) {
                int y2 = yy + ty - PY;
                if (y2 < 0 || y2 >= H) continue;
#pragma unroll
                for (int tx = 0; tx < KW; ++tx) {
                    int x2 = xx + tx - PX;
                    if (x2 < 0 || x2 >= W) continue;
                    const int tap = (tz * KH + ty) * KW + tx;
                    const TX* xp = x + ((((int64_t)n * D + z2) * H + y2) * W + x2) * x_ld;
                    const float* wp = w + (int64_t)tap * Cin * Cout + co;
                    for (int ci = 0; ci < Cin; ++ci) {
                        float xv = act_ld1(xp + ci);
                        if (sc) xv = fmaf(xv, sc[ci], sf[ci]);
                        acc = fmaf(xv, wp[(int64_t)ci * Cout], acc);
                    }
                }
            }
        }
        acc = apply_act(acc, act);
        if (ref && !(act_ld1(ref + v * ref_ld + co) > 0.f)) acc = 0.f;
        act_st1(y + v * y_ld + co, acc);
    }
}

// 1x1x1 projection to a few channels (out_conv 32->2/12): thread <-> voxel, reads its
// whole channel row with 16-byte loads, keeps Cout accumulators; weights via L1.
template <int COUT, typename TX, typename TY>
__global__ __launch_bounds__(256) void k_conv1x1_smallcout(const TX* __restrict__ x, int64_t x_ld,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ w /*[ci][co]*/,
                                                           const float* __restrict__ bias, TY* __restrict__ y,
                                                           int64_t y_ld, const TY* __restrict__ ref, int64_t ref_ld,
                                                           int64_t V, int64_t NV, int Cin, int act) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < NV; v += (int64_t)gridDim.x * 256) {
        const int n = (int)(v / V);
        float acc[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = bias ? bias[co] : 0.f;
        const TX* xp = x + v * x_ld;
        for (int ci = 0; ci < Cin; ci += 4) {
            float4 t = act_ld4(xp + ci);
            float xv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (scale) xv[j] = fmaf(xv[j], scale[(int64_t)n * Cin + ci + j], shift[(int64_t)n * Cin + ci + j]);
#pragma unroll
                for (int co = 0; co < COUT; ++co) acc[co] = fmaf(xv[j], w[(ci + j) * COUT + co], acc[co]);
            }
        }
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            float a = apply_act(acc[co], act);
            if (ref && !(act_ld1(ref + v * ref_ld + co) > 0.f)) a = 0.f;
            act_st1(y + v * y_ld + co, a);
        }
    }
}

template <int KD, int KH, int KW>
static void launch_fwd_generic(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w,
                               const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, int N, int D,
                               int H, int W, int Cin, int Cout, int act, hipStream_t s) {
    int64_t items = (int64_t)N * D * H * W * Cout;
    TEM_ST2_SWITCH(c.stx, c.sty, TX, TY, (void)0,
                   hipLaunchKernelGGL((k_conv_fwd_generic<KD, KH, KW, TX, TY>), dim3(tem_grid_1d(items, 256, 256 * 16)), dim3(256), 0, s,
                                      (const TX*)x, x_ld, scale, shift, w, bias, (TY*)y, y_ld, (const TY*)ref, ref_ld, N, D, H, W, Cin,
                                      Cout, act));
}

static void launch_fwd_smallcout(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w,
                                 const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, int64_t V, int64_t NV,
                                 int Cin, int Cout, int act, hipStream_t s) {
    dim3 grid(tem_grid_1d(NV, 256, 256 * 16));
#define SC(CO)                                                                                                   \
    case CO:                                                                                                     \
        TEM_ST2_SWITCH(c.stx, c.sty, TX, TY, (void)0,                                            \
                       hipLaunchKernelGGL((k_conv1x1_smallcout<CO, TX, TY>), grid, dim3(256), 0, s, (const TX*)x, x_ld, scale, shift, \
                                          w, bias, (TY*)y, y_ld, (const TY*)ref, ref_ld, V, NV, Cin, act)); \
        break;
    switch (Cout) {
        SC(1) SC(2) SC(3) SC(4) SC(8) SC(12) SC(16)
    }
#undef SC
}

#define DISPATCH_K(KD, KH, KW, CALL)                                  \
    do {                                                              \
        int key__ = ((KD) == 3) * 4 + ((KH) == 3) * 2 + ((KW) == 3);  \
        switch (key__) {                                              \
            case 0: { CALL(1, 1, 1); } break;                         \
            case 1: { CALL(1, 1, 3); } break;                         \
            case 2: { CALL(1, 3, 1); } break;                         \
            case 3: { CALL(1, 3, 3); } break;                         \
            case 4: { CALL(3, 1, 1); } break;                         \
            case 5: { CALL(3, 1, 3); } break;                         \
            case 6: { CALL(3, 3, 1); } break;                         \
            default: { CALL(3, 3, 3); } break;                        \
        }                                                             \
    } while (0)

// ---------------------------------------------------------------------------
// The forward / data-gradient dispatch (DESIGN.md "Forward dispatch: one plan"): fwd_plan() decides ONCE which kernel a call
// takes, with which geometry, and which statistics rows it writes.  conv3d_fwd_impl executes the plan; the dispatch queries
// (tem_conv3d_fwd_kernel[_ld], tem_conv3d_fwd_stat_blocks[_ld]) and the argument checks of the _stats / _gscaled / _refnorm
// calls print it for synthetic facts.  Order of preference: z-reuse, ping-pong, z-reuse split-K, 1x1 stream, patch; exact fp32
// has no ping-pong and no stream instantiation (conv_arith.h), the VALU mode has the kernels of this file and conv_small.hip.
// ---------------------------------------------------------------------------
enum FwdKernel { FK_VALU, FK_ZR, FK_ZR_SPLITK, FK_PP, FK_STREAM1X1, FK_PATCH, FK_PATCH_FP32, FK_REFUSED };
static_assert(FK_ZR == TEM_MFMA_ZR && FK_ZR_SPLITK == TEM_MFMA_ZR_SPLITK && FK_PP == TEM_MFMA_PP && FK_STREAM1X1 == TEM_MFMA_STREAM &&
                  FK_PATCH == TEM_MFMA_PATCH && FK_PATCH_FP32 == TEM_MFMA_PATCH_FP32,
              "tem_conv3d_fwd_mfma_path() returns the plan's kernel");

// what the decision depends on besides the call, the shape and the mode
struct FwdFacts {
    int64_t x_ld, y_ld, ref_ld;   // ref_ld 0: no ref
    // operand groups on 16-byte boundaries (an absent operand counts as aligned)
    bool xw16;      // x, packed weights, scale and shift
    bool yref16;    // y and ref
    bool yref_v4;   // y and ref on boundaries of 4 ELEMENTS (16-bit tensors: 8 bytes; the 1x1 stream and the cin1 kernel ask no more)
    bool bias16;
    bool scale;     // a pre-norm is applied to x
    bool sigmoid;
    bool stat;      // statistics rows are requested
    int64_t ws_bytes;
};

struct FwdPlan {
    FwdKernel kernel;
    int ks;                  // FK_ZR_SPLITK / FK_PATCH / FK_PATCH_FP32: slices of the input channels (1: no split-K)
    ZrGeom zr;               // FK_ZR, FK_ZR_SPLITK
    PpGeom pp;               // FK_PP
    TemPatchTiling patch;    // FK_PATCH, FK_PATCH_FP32
    // rows [N][stat_blocks][Cout][2] the launch writes when it is asked for statistics, 0: none (such a request is refused).
    // FK_STREAM1X1 answers for the patch kernel, which takes the launch when statistics are requested.
    int64_t stat_blocks;
    char error[320];         // FK_REFUSED: the message of the TEM_EINVAL the launch returns
    // tem_conv3d_fwd_kernel(): 3 z-reuse, 4 its split-K launch, 1 / 2 ping-pong with that many column tiles per team, 0 the rest
    int family() const { return kernel == FK_ZR ? 3 : kernel == FK_ZR_SPLITK ? 4 : kernel == FK_PP ? pp.CT : 0; }
};

static void plan_refuse(FwdPlan& p, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void plan_refuse(FwdPlan& p, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.error, sizeof(p.error), fmt, ap);
    va_end(ap);
    p.kernel = FK_REFUSED;
    p.stat_blocks = 0;
}

static const char kSplitXLayout[] =
    "tem_conv3d_fwd(split-bf16): x / packed weights must be 16-byte aligned with ld%%4==0 (16-bit storage: ld%%8==0)";

// split-K factor of the z-reuse kernel for a shape neither team kernel takes directly (0: none)
static int fwd_zr_splitk_ks(const TemConvCall& c, const ZrGeom& zr, const PpGeom& pp, const TemConvShape& sh, int mode) {
    return pp.variant ? 0 : tem_zr_splitk_ks(c, zr, sh, mode);
}

static FwdPlan fwd_plan(const TemConvCall& c, const TemConvShape& sh, int mode, const FwdFacts& f) {
    FwdPlan p = {};
    p.kernel = FK_VALU;
    p.ks = 1;
    const bool ref = f.ref_ld != 0;
    const bool ld4 = f.y_ld % 4 == 0 && f.ref_ld % 4 == 0;   // y / ref rows of whole 4-element vectors
    if (mode == TEM_ARITH_VALU) {   // VALU kernels: only the small-Cin first-layer kernel (conv_small.hip) provides statistics
        if (ld4 && f.yref_v4 && f.bias16 && !ref && sh.Cout % 4 == 0)
            p.stat_blocks = tem_conv_fwd_cin1_stat_blocks(sh.D, sh.H, sh.W, sh.Cin, sh.Cout, sh.kd, sh.kh, sh.kw);
        return p;
    }
    const bool split = tem_arith_split_fwd(mode);   // (any other MFMA mode runs the exact-fp32 kernels)
    const char* const who = split ? "split-bf16" : "mfma";
    if (sh.Cin % 16 || sh.Cout % 32) {
        plan_refuse(p, "tem_conv3d_fwd(%s): needs Cin%%16==0 and Cout%%32==0 (got %d,%d)", who, sh.Cin, sh.Cout);
        return p;
    }
    if (split && f.x_ld % (c.stx ? 8 : 4)) {
        plan_refuse(p, kSplitXLayout);
        return p;
    }
    const int64_t part_bytes = sh.NV() * sh.Cout * 4;   // one split-K slice of partial sums
    // a team kernel (or the split-K launch) is meant for the shape but declines the layout: the patch kernel runs it, without
    // statistics -- their rows would have another shape than the caller's buffer
    bool no_rows = false;
    // exact fp32 stays on the patch kernel when it cannot load x / weights / scale as 16-byte vectors (the split modes raise)
    if (split || (mode == TEM_ARITH_FP32 && f.x_ld % 4 == 0 && f.xw16)) {
        int64_t max_ld = f.x_ld > f.y_ld ? f.x_ld : f.y_ld;
        if (f.ref_ld > max_ld) max_ld = f.ref_ld;
        const bool plane = tem_plane32_ok(sh, max_ld);
        // the team kernels' 16-byte epilogue; statistics of a masked output are never asked for
        const bool epi = ld4 && f.yref16 && !f.sigmoid && !(f.stat && ref);
        p.zr = tem_zr_geometry(c, sh, mode);
        p.pp = tem_pp_geometry(c, sh, mode);
        if (p.zr.ok && plane) {
            if (epi && f.bias16) {
                p.kernel = FK_ZR;
                p.stat_blocks = ref ? 0 : (int64_t)p.zr.nZ * p.zr.nY * p.zr.nX * 4;
                return p;
            }
            if (f.stat) {
                plan_refuse(p, "tem_conv3d_fwd_stats / _ex: statistics were sized for the z-reuse kernel but this launch "
                               "cannot take it (y / ref / bias need 16-byte alignment and ld %% 4 == 0, no ref, no sigmoid)");
                return p;
            }
            no_rows = true;
        }
        if (p.pp.variant && plane) {   // (reads bias with scalar loads)
            if (epi) {
                p.kernel = FK_PP;
                p.stat_blocks = ref || no_rows ? 0 : (int64_t)p.pp.nZ * p.pp.nY * p.pp.nX * p.pp.WM;
                return p;
            }
            if (f.stat) {
                plan_refuse(p, "tem_conv3d_fwd_stats: statistics were sized for the ping-pong kernel but this launch cannot take it "
                               "(y / ref need 16-byte alignment and ld %% 4 == 0, no ref, no sigmoid)");
                return p;
            }
            no_rows = true;
        }
        const int ks = fwd_zr_splitk_ks(c, p.zr, p.pp, sh, mode);
        if (ks) {
            const int64_t skb = tem_splitk_stat_blocks(sh.V(), sh.Cout);   // rows of the summing epilogue (0: it has none for this Cout)
            // 32-bit offsets over x and the Cout-wide workspace; the epilogue handles ref, sigmoid and bias vectors
            if (!(f.stat && !skb) && tem_plane32_ok(sh, f.x_ld > sh.Cout ? f.x_ld : sh.Cout) && ld4 && f.yref16 && f.bias16 &&
                f.ws_bytes >= ks * part_bytes) {
                p.kernel = FK_ZR_SPLITK;
                p.ks = ks;
                p.stat_blocks = skb;
                return p;
            }
            if (f.stat && skb) {
                plan_refuse(p, "tem_conv3d_fwd_stats: the split-K launch that writes the statistics needs its workspace "
                               "(tem_conv3d_fwd_ws) and 16-byte aligned y / ref / bias");
                return p;
            }
            no_rows = true;
        }
    }
    const int key = sh.key();
    if (key != 7 && key != 3 && key != 0) {
        plan_refuse(p, "tem_conv3d_fwd(%s): kernel (%d,%d,%d) has no MFMA instantiation", who, sh.kd, sh.kh, sh.kw);
        return p;
    }
    // patch kernels: split-K where the grid asks for it and the launch has the workspace and a 16-byte epilogue
    p.patch = tem_fwd_patch_tiling(sh);
    p.ks = p.patch.ks;
    if (p.ks > 1 && !(ld4 && f.yref16 && f.bias16 && f.ws_bytes >= p.ks * part_bytes)) p.ks = 1;
    if (!split) {
        p.kernel = FK_PATCH_FP32;
        if (f.stat)
            plan_refuse(p, "tem_conv3d_fwd_stats: the exact-fp32 patch kernel writes no statistics (tem_conv3d_fwd_stat_blocks() == 0)");
        return p;
    }
    p.stat_blocks = no_rows || p.patch.ks > 1 ? 0 : p.patch.per;
    if (f.stat && !p.stat_blocks) {
        plan_refuse(p, p.patch.ks > 1 ? "tem_conv3d_fwd_stats: this shape runs split-K (tem_conv3d_fwd_stat_blocks() == 0)"
                                      : "tem_conv3d_fwd_stats: this launch cannot write statistics (tem_conv3d_fwd_stat_blocks_ld() == 0)");
        return p;
    }
    // 1x1x1 as a streaming GEMM: no pre-norm, statistics or sigmoid; enough 32-voxel tiles to hide the k-loop's load latency
    const bool stream = key == 0 && tem_option(TEM_OPT_CONV1X1_STREAM) && tem_stream1x1_takes(mode) && !f.scale && !f.stat &&
                        !f.sigmoid && sh.NV() >= 16384 && ld4 && f.yref_v4 && f.bias16;
    p.kernel = stream ? FK_STREAM1X1 : FK_PATCH;
    return p;
}

// The VALU family (fwd_plan: FK_VALU) has eight kernels.  fwd_valu_select() names the ONE a launch takes, with the template
// arguments of its instantiation, from the launch's real pointers, leading dimensions, storage pair, shape and operands;
// conv3d_fwd_impl switches on the answer and tem_conv3d_fwd_valu_path() reports it.  Order of preference: first layer (small Cin,
// 3x3x3 / 1x3x3), its data gradient (Cout 1), then for 1x1x1 the projection, the expansion and the one-thread-per-voxel
// projection; the generic kernel takes everything.  Only the first-layer kernels write statistics rows.
struct ValuSel {
    int path;               // TemValuPath
    int cout, nj, cin, kd;  // the instantiation: COUT / NJ / CIN / KD template arguments, 0 where the path has none
};

static bool smallcout_takes(int Cin, int Cout) {
    return Cin % 4 == 0 && (Cout == 1 || Cout == 2 || Cout == 3 || Cout == 4 || Cout == 8 || Cout == 12 || Cout == 16);
}

static ValuSel fwd_valu_select(const TemConvCall& c, const TemConvShape& sh, const void* x, int64_t x_ld, bool scale, const void* w,
                               const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, bool stat) {
    auto al = [](const void* ptr, uintptr_t a) { return (uintptr_t)ptr % a == 0; };   // (an absent operand counts as aligned)
    const int Cin = sh.Cin, Cout = sh.Cout;
    const bool x16 = x_ld % 4 == 0 && al(x, 16);   // x in 16-byte rows
    const bool one = sh.key() == 0;
    const int first = tem_conv_fwd_cin1_takes(sh);
    if (first && !ref && y_ld % 4 == 0 && al(y, tem_st_align4(c.sty)) && al(bias, 16)) {
        if (stat && !tem_conv_fwd_cin1_stat_blocks(sh.D, sh.H, sh.W, Cin, Cout, sh.kd, sh.kh, sh.kw)) return {TEM_VP_REFUSED, 0, 0, 0, 0};
        if (first == 2) return {TEM_VP_C1ROWS, 0, 0, 0, sh.kd};
        return {TEM_VP_CIN1, 0, 0, Cin, sh.kd};
    }
    if (stat) return {TEM_VP_REFUSED, 0, 0, 0, 0};
    if (tem_conv_fwd_cout1_takes(sh) && !scale && !ref && x16) return {TEM_VP_COUT1, 0, 0, 0, sh.kd};
    if (one && !scale) {
        const int nj = tem_conv1x1_proj_nj(Cin, Cout);
        if (nj >= 0 && !ref && x16) return {nj ? TEM_VP_PROJ_R : TEM_VP_PROJ, Cout, nj, 0, 0};
        if (tem_conv1x1_expand_takes(Cin, Cout) && y_ld % 4 == 0 && al(y, 16) && al(w, 16) && al(bias, 16) &&
            (!ref || (ref_ld % 4 == 0 && al(ref, 16))))
            return {TEM_VP_EXPAND, 0, 0, 0, 0};
    }
    if (one && smallcout_takes(Cin, Cout) && x16) return {TEM_VP_SMALLCOUT, Cout, 0, 0, 0};
    return {TEM_VP_GENERIC, 0, 0, 0, sh.kd * 100 + sh.kh * 10 + sh.kw};   // <KD, KH, KW> as decimal digits
}

static int64_t fwd_ws(const TemConvCall& c, const TemConvShape& sh, int mode) {
    if (!mode || sh.Cin % 16 || sh.Cout % 32) return 0;
    const TemPatchTiling t = tem_fwd_patch_tiling(sh);
    int ks = t.ks > 1 ? t.ks : 0;
    if (tem_arith_mfma_fwd(mode)) {   // the z-reuse kernel's split-K launch may want more slices than the patch kernel's
        const int zk = fwd_zr_splitk_ks(c, tem_zr_geometry(c, sh, mode), tem_pp_geometry(c, sh, mode), sh, mode);
        if (zk > ks) ks = zk;
    }
    return ks * sh.NV() * sh.Cout * 4;
}

extern "C" int64_t tem_conv3d_fwd_ws(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                                     int use_mfma) {
    const TemConvCall c = conv_call(use_mfma);
    return fwd_ws(c, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma);
}

// the argument checks of every forward / data-gradient launch, shared by conv3d_fwd_impl and the dispatch query of an actual
// launch (tem_conv3d_fwd_valu_path): a failed check leaves its message for tem_last_error()
static int fwd_args_check(const TemConvCall& c, const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                          const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, const TemConvShape& sh, int act, int use_mfma) {
    const int N = sh.N, D = sh.D, H = sh.H, W = sh.W, Cin = sh.Cin, Cout = sh.Cout, kd = sh.kd, kh = sh.kh, kw = sh.kw;
    TEM_REQUIRE(x && w_packed && y, "tem_conv3d_fwd: null pointer");
    TEM_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && x_ld >= (c.x_cs ? 32 : Cin) &&
                    y_ld >= (c.y_cs ? 32 : Cout),
                "tem_conv3d_fwd: bad shape");
    TEM_REQUIRE((kd == 1 || kd == 3) && (kh == 1 || kh == 3) && (kw == 1 || kw == 3),
                "tem_conv3d_fwd: kernel size (%d,%d,%d) not supported (1 or 3 per axis)", kd, kh, kw);
    TEM_REQUIRE((scale == nullptr) == (shift == nullptr), "tem_conv3d_fwd: scale and shift must both be given");
    TEM_REQUIRE(act >= 0 && act <= 2, "tem_conv3d_fwd: Invalid activation: %d", act);
    TEM_REQUIRE(!ref || ref_ld >= Cout, "tem_conv3d_fwd: bad ref_ld");
    const int stx = c.stx, sty = c.sty;
    TEM_REQUIRE(stx >= 0 && stx <= 2 && sty >= 0 && sty <= 2 && (stx == 0 || sty == 0 || stx == sty),
                "tem_conv3d_fwd: unsupported storage types (x %d, y %d)", stx, sty);
    TEM_REQUIRE(!(stx || sty) || use_mfma != TEM_ARITH_FP32, "tem_conv3d_fwd: the exact-fp32 MFMA kernels take fp32 tensors only");
    TEM_REQUIRE(!(c.x_cs || c.y_cs) || tem_arith_one_term(use_mfma), "tem_conv3d_fwd_ex: chunk strides need use_mfma 5 / 7");
    auto al16 = [](const void* ptr) { return (uintptr_t)ptr % 16 == 0; };
    if (tem_arith_split_fwd(use_mfma)) {   // every split-precision kernel loads x / weights / scale as 16-byte vectors
        TEM_REQUIRE(stx == sty, "tem_conv3d_fwd(split-bf16): x and y must have the same storage type");
        TEM_REQUIRE(tem_storage_ok(use_mfma, stx),
                    "tem_conv3d_fwd(split-bf16): 16-bit storage goes with the one-term mode of the same type (fp16: use_mfma 5, "
                    "bf16: use_mfma 7), got storage %d with use_mfma %d", stx, use_mfma);
        TEM_REQUIRE(al16(x) && al16(w_packed), kSplitXLayout);
        TEM_REQUIRE(al16(scale) && al16(shift), "tem_conv3d_fwd(split-bf16): scale/shift must be 16-byte aligned");
    }
    return TEM_OK;
}

// The plan of a launch with exactly these arguments, after every check that stands between the arguments and the launch: the
// argument checks, the plan's own refusals, and what only the z-reuse kernel honours.  Shared by conv3d_fwd_impl and the
// dispatch query of an actual launch (tem_conv3d_fwd_mfma_path).  ws_bytes: 0 without a workspace
static int fwd_launch_plan(const TemConvCall& c, const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                           const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, int64_t ws_bytes,
                           const TemConvShape& sh, int act, int use_mfma, bool stat, FwdPlan& p) {
    TEM_TRY(fwd_args_check(c, x, x_ld, scale, shift, w_packed, y, y_ld, ref, ref_ld, sh, act, use_mfma));
    auto al16 = [](const void* ptr) { return (uintptr_t)ptr % 16 == 0; };
    const uintptr_t v4 = tem_st_align4(c.sty);
    const FwdFacts facts = {x_ld, y_ld, ref ? ref_ld : 0,
                            al16(x) && al16(w_packed) && al16(scale) && al16(shift), al16(y) && al16(ref),
                            (uintptr_t)y % v4 == 0 && (uintptr_t)ref % v4 == 0, al16(bias),
                            scale != nullptr, act == TEM_ACT_SIGMOID, stat, ws_bytes};
    p = fwd_plan(c, sh, use_mfma, facts);
    if (p.kernel == FK_REFUSED) {
        tem_set_error("%s", p.error);
        return TEM_EINVAL;
    }
    // what only the z-reuse kernel honours
    TEM_REQUIRE(!(c.x_cs || c.y_cs) || (p.kernel == FK_ZR && c.stx && !ref && !(c.x_cs && sh.Cin % 32) && c.x_cs % 8 == 0 && c.y_cs % 8 == 0),
                "tem_conv3d_fwd_ex: chunk strides (x_cs / y_cs) need 16-bit tensors on the z-reuse kernel (tem_conv3d_fwd_kernel() "
                "== 3), no ref, strides %% 8 == 0");
    TEM_REQUIRE(!c.in_amax || p.kernel == FK_ZR, "tem_conv3d_fwd_gscaled: the launch did not take the z-reuse kernel (alignment of y / ref?)");
    TEM_REQUIRE(!c.ref_coef || p.kernel == FK_ZR, "tem_conv3d_fwd_refnorm: the launch did not take the z-reuse kernel (alignment of y / ref?)");
    TEM_REQUIRE(!c.ref_coef || (ref && !stat && al16(c.ref_coef)), "tem_conv3d_fwd_refnorm: needs ref, no statistics, 16-byte aligned coefficients");
    TEM_REQUIRE(!c.in_amax || (use_mfma == TEM_ARITH_F16X3 && !bias && !scale && !stat),
                "tem_conv3d_fwd_gscaled: fp16 two-term layout, no bias / norm / statistics");
    return TEM_OK;
}

static int conv3d_fwd_impl(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift,
                           const float* w_packed, const float* bias, float* y, int64_t y_ld, const float* ref,
                           int64_t ref_ld, void* ws, int64_t ws_bytes, const TemConvShape& sh, int act, int use_mfma, float* stat,
                           tem_stream_t stream) {
    const int N = sh.N, D = sh.D, H = sh.H, W = sh.W, Cin = sh.Cin, Cout = sh.Cout, kd = sh.kd, kh = sh.kh, kw = sh.kw;
    FwdPlan p;
    TEM_TRY(fwd_launch_plan(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws ? ws_bytes : 0, sh, act, use_mfma,
                            stat != nullptr, p));
    hipStream_t s = (hipStream_t)stream;

    if (p.kernel != FK_VALU) {
        static const char* const what[] = {"", "tem_conv3d_fwd(z-reuse)", "tem_conv3d_fwd(z-reuse split-K)", "tem_conv3d_fwd(ping-pong)",
                                           "tem_conv3d_fwd(1x1 stream)", "tem_conv3d_fwd(bf16x3)", "tem_conv3d_fwd(mfma)"};
        if (p.kernel == FK_ZR)
            tem_conv_fwd_zr(c, p.zr, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, act, use_mfma, stat, s);
        else if (p.kernel == FK_ZR_SPLITK)
            tem_conv_fwd_zr_splitk(c, p.zr, p.ks, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, sh, act, use_mfma, stat, s);
        else if (p.kernel == FK_PP)
            tem_conv_fwd_pp(p.pp, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, act, use_mfma, stat, s);
        else if (p.kernel == FK_STREAM1X1)
            tem_conv1x1_stream(c, x, x_ld, w_packed, bias, y, y_ld, ref, ref_ld, sh, act, use_mfma, s);
        else if (p.kernel == FK_PATCH)
            tem_conv_fwd_bf16x3(c, p.patch, p.ks, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, sh, act, use_mfma, stat, s);
        else
            TEM_TRY(tem_conv_fwd_mfma(p.patch, p.ks, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, sh, act, s));
        TEM_CHECK_LAUNCH(what[p.kernel]);
        return TEM_OK;
    }
    // VALU kernels: the one fwd_valu_select names
    const int64_t NV = sh.NV();
    const ValuSel v = fwd_valu_select(c, sh, x, x_ld, scale != nullptr, w_packed, bias, y, y_ld, ref, ref_ld, stat != nullptr);
    switch (v.path) {
        case TEM_VP_C1ROWS:
        case TEM_VP_CIN1:
            tem_conv_fwd_cin1(c, v.path == TEM_VP_C1ROWS, x, x_ld, scale, shift, w_packed, bias, y, y_ld, N, D, H, W, Cin, Cout, kd, kh, kw,
                              act, stat, s);
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(cin1)");
            return TEM_OK;
        case TEM_VP_COUT1:
            tem_conv_fwd_cout1(c, x, x_ld, w_packed, bias, y, y_ld, N, D, H, W, Cin, kd, kh, kw, act, s);
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(cout1)");
            return TEM_OK;
        case TEM_VP_PROJ_R:
        case TEM_VP_PROJ:
            tem_conv1x1_proj(c, v.nj, x, x_ld, w_packed, bias, y, y_ld, NV, Cin, Cout, act, s);
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(proj)");
            return TEM_OK;
        case TEM_VP_EXPAND:
            tem_conv1x1_expand(c, x, x_ld, w_packed, bias, y, y_ld, ref, ref_ld, NV, Cin, Cout, act, s);
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(expand)");
            return TEM_OK;
        case TEM_VP_SMALLCOUT:
            launch_fwd_smallcout(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, (int64_t)D * H * W, NV, Cin, Cout, act, s);
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(1x1)");
            return TEM_OK;
        case TEM_VP_GENERIC: {
#define CALL(A, B, C) \
    launch_fwd_generic<A, B, C>(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, N, D, H, W, Cin, Cout, act, s)
            DISPATCH_K(kd, kh, kw, CALL);
#undef CALL
            TEM_CHECK_LAUNCH("tem_conv3d_fwd(generic)");
            return TEM_OK;
        }
        default:
            TEM_REQUIRE(false, "tem_conv3d_fwd_stats: this launch cannot write statistics (tem_conv3d_fwd_stat_blocks() == 0)");
    }
    return TEM_EINVAL;
}

extern "C" int tem_conv3d_fwd(const float* x, int64_t x_ld, const float* scale, const float* shift,
                              const float* w_packed, const float* bias, float* y, int64_t y_ld, const float* ref,
                              int64_t ref_ld, void* ws, int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout,
                              int kd, int kh, int kw, int act, int use_mfma, tem_stream_t stream) {
    const TemConvCall c = conv_call(use_mfma);
    return conv3d_fwd_impl(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, ws_bytes,
                           TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, act, use_mfma, nullptr, stream);
}

// The plan of a launch of this shape and layout as the queries see it.  ref_ld 0: no ref.  misaligned: a pointer of the launch
// (x, y, ref, bias, scale, shift, packed weights) is off a 16-byte boundary -- every operand group then counts as misaligned.
// Assumes the tem_conv3d_fwd_ws() workspace, no pre-norm, no sigmoid.
static FwdPlan fwd_query(const TemConvCall& c, const TemConvShape& sh, int mode, int64_t x_ld, int64_t y_ld, int64_t ref_ld,
                         int misaligned) {
    const bool al = !misaligned;
    const FwdFacts f = {x_ld, y_ld, ref_ld, al, al, al, al, false, false, false, fwd_ws(c, sh, mode)};
    return fwd_plan(c, sh, mode, f);
}

static int fwd_misaligned(const void* x, const void* scale, const void* shift, const void* w, const void* bias, const void* y,
                          const void* ref) {
    return (int)(((uintptr_t)x | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y |
                  (uintptr_t)ref) % 16 != 0);
}

extern "C" int64_t tem_conv3d_fwd_stat_blocks_ld(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                                                 int use_mfma, int64_t x_ld, int64_t y_ld, int64_t ref_ld, int misaligned) {
    const TemConvCall c = conv_call(use_mfma);
    return fwd_query(c, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma, x_ld, y_ld, ref_ld, misaligned).stat_blocks;
}

extern "C" int tem_conv3d_fwd_kernel_ld(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma,
                                        int64_t x_ld, int64_t y_ld, int64_t ref_ld, int misaligned) {
    const TemConvCall c = conv_call(use_mfma);
    return fwd_query(c, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma, x_ld, y_ld, ref_ld, misaligned).family();
}

// the shape-only queries: dense, aligned x and y, no ref
extern "C" int64_t tem_conv3d_fwd_stat_blocks(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                                              int use_mfma) {
    return tem_conv3d_fwd_stat_blocks_ld(N, D, H, W, Cin, Cout, kd, kh, kw, use_mfma, Cin, Cout, 0, 0);
}

extern "C" int tem_conv3d_fwd_kernel(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma) {
    return tem_conv3d_fwd_kernel_ld(N, D, H, W, Cin, Cout, kd, kh, kw, use_mfma, Cin, Cout, 0, 0);
}

// The kernel of the VALU family a tem_conv3d_fwd / _stats / _ex launch with exactly these arguments takes (tem_hip.h; launches
// nothing): the argument checks of conv3d_fwd_impl, the plan, the selector.  inst (optional): int[4] = COUT, NJ, CIN, KD
extern "C" int tem_conv3d_fwd_valu_path(const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                                        const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, int N, int D,
                                        int H, int W, int Cin, int Cout, int kd, int kh, int kw, int act, int use_mfma, int has_stat,
                                        int* inst) {
    if (inst) inst[0] = inst[1] = inst[2] = inst[3] = 0;
    const TemConvCall c = conv_call(use_mfma);
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    if (use_mfma != TEM_ARITH_VALU || fwd_args_check(c, x, x_ld, scale, shift, w_packed, y, y_ld, ref, ref_ld, sh, act, use_mfma) != TEM_OK)
        return TEM_VP_REFUSED;
    if (has_stat && !fwd_query(c, sh, use_mfma, x_ld, y_ld, ref ? ref_ld : 0, fwd_misaligned(x, scale, shift, w_packed, bias, y, ref))
                         .stat_blocks)
        return TEM_VP_REFUSED;   // (fwd_stats_check)
    const ValuSel v = fwd_valu_select(c, sh, x, x_ld, scale != nullptr, w_packed, bias, y, y_ld, ref, ref_ld, has_stat != 0);
    if (inst && v.path != TEM_VP_REFUSED) {
        inst[0] = v.cout;
        inst[1] = v.nj;
        inst[2] = v.cin;
        inst[3] = v.kd;
    }
    return v.path;
}

// the argument checks of tem_conv3d_fwd_stats (also a tem_conv3d_fwd_ex with stat_part)
static int fwd_stats_check(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift,
                           const float* w_packed, const float* bias, const float* y, int64_t y_ld, const float* ref, int64_t ref_ld,
                           const TemConvShape& sh, int use_mfma, const float* stat_part, int64_t stat_blocks) {
    TEM_REQUIRE(stat_part, "tem_conv3d_fwd_stats: null statistics buffer");
    const int64_t nblk = fwd_query(c, sh, use_mfma, x_ld, y_ld, ref ? ref_ld : 0,
                                   fwd_misaligned(x, scale, shift, w_packed, bias, y, ref)).stat_blocks;
    TEM_REQUIRE(stat_blocks > 0 && stat_blocks == nblk,
                "tem_conv3d_fwd_stats: stat_blocks must be tem_conv3d_fwd_stat_blocks_ld() of this launch's layout (and > 0): "
                "got %lld, the launch writes %lld", (long long)stat_blocks, (long long)nblk);
    return TEM_OK;
}

extern "C" int tem_conv3d_fwd_stats(const float* x, int64_t x_ld, const float* scale, const float* shift,
                                    const float* w_packed, const float* bias, float* y, int64_t y_ld, const float* ref,
                                    int64_t ref_ld, void* ws, int64_t ws_bytes, int N, int D, int H, int W, int Cin,
                                    int Cout, int kd, int kh, int kw, int act, int use_mfma, float* stat_part,
                                    int64_t stat_blocks, tem_stream_t stream) {
    const TemConvCall c = conv_call(use_mfma);
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TEM_TRY(fwd_stats_check(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, use_mfma, stat_part, stat_blocks));
    return conv3d_fwd_impl(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, ws_bytes, sh, act, use_mfma, stat_part,
                           stream);
}

// ---------------------------------------------------------------------------
// generic VALU weight gradient.  thread <-> (pair=(ci,co) of a <=256-pair block, row r);
// all taps accumulate in registers so g is read once.  Two-stage deterministic:
// partial[chunk][tap][ci][co] -> fp64 merge.
// ---------------------------------------------------------------------------
template <int KD, int KH, int KW, typename TX, typename TG>
__global__ __launch_bounds__(256) void k_conv_wgrad_generic(const TX* __restrict__ x, int64_t x_ld,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift,
                                                            const TG* __restrict__ g, int64_t g_ld, int N, int D,
                                                            int H, int W, int Cin, int Cout, int npairs_blk, int rows,
                                                            int64_t vper, float* __restrict__ part) {
    constexpr int NT = KD * KH * KW;
    constexpr int PZ = KD / 2, PY = KH / 2, PX = KW / 2;
    extern __shared__ float sh[];  // [NT][rows][npairs_blk]
    const int64_t NV = (int64_t)N * D * H * W;
    const int chunk = blockIdx.x, pb = blockIdx.y;
    const int pl = threadIdx.x % npairs_blk, r = threadIdx.x / npairs_blk;
    const int pair = pb * npairs_blk + pl;
    const bool active = pair < Cin * Cout && r < rows;
    const int ci = active ? pair / Cout : 0, co = active ? pair % Cout : 0;
    float acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.f;
    int64_t v0 = (int64_t)chunk * vper, v1 = v0 + vper;
    if (v1 > NV) v1 = NV;
    if (active) {
        for (int64_t v = v0 + r; v < v1; v += rows) {
            int xx = (int)(v % W);
            int64_t q = v / W;
            int yy = (int)(q % H);
            q /= H;
            int zz = (int)(q % D);
            int n = (int)(q / D);
            const float gv = act_ld1(g + v * g_ld + co);
            float sc = 1.f, sf = 0.f;
            if (scale) {
                sc = scale[(int64_t)n * Cin + ci];
                sf = shift[(int64_t)n * Cin + ci];
            }
#pragma unroll
            for (int tz = 0; tz < KD; ++tz) {
                int z2 = zz + tz - PZ;
#pragma unroll
                for (int ty = 0; ty < KH; ++ty) {
                    int y2 = yy + ty - PY;
#pragma unroll
                    for (int tx = 0; tx < KW; ++tx) {
                        int x2 = xx + tx - PX;
                        if (z2 < 0 || z2 >= D || y2 < 0 || y2 >= H || x2 < 0 || x2 >= W) continue;
                        float xv = act_ld1(x + ((((int64_t)n * D + z2) * H + y2) * W + x2) * x_ld + ci);
                        xv = fmaf(xv, sc, sf);
                        acc[(tz * KH + ty) * KW + tx] = fmaf(xv, gv, acc[(tz * KH + ty) * KW + tx]);
                    }
                }
            }
        }
    }
    if (r < rows) {
#pragma unroll
        for (int t = 0; t < NT; ++t) sh[((int64_t)t * rows + r) * npairs_blk + pl] = acc[t];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NT * npairs_blk; idx += 256) {
        int t = idx / npairs_blk, p = idx % npairs_blk;
        int gp = pb * npairs_blk + p;
        if (gp >= Cin * Cout) continue;
        float s = 0.f;
        for (int rr = 0; rr < rows; ++rr) s += sh[((int64_t)t * rows + rr) * npairs_blk + p];
        // partial[chunk][tap][ci][co]; pair index == ci*Cout+co
        part[((int64_t)chunk * NT + t) * Cin * Cout + gp] = s;
    }
}

// column sums: db[co] = sum_v g[v][co]
template <typename TG>
__global__ __launch_bounds__(256) void k_colsum_partial(const TG* __restrict__ g, int64_t g_ld, int64_t NV, int C,
                                                        int rows, int64_t vper, float* __restrict__ part) {
    extern __shared__ float sh[];  // [rows][Cb]
    const int Cb = C < 256 ? C : 256;
    const int cl = threadIdx.x % Cb, r = threadIdx.x / Cb;
    int64_t v0 = (int64_t)blockIdx.x * vper, v1 = v0 + vper;
    if (v1 > NV) v1 = NV;
    for (int c0 = 0; c0 < C; c0 += Cb) {
        int c = c0 + cl;
        float s = 0.f;
        if (c < C && r < rows)
            for (int64_t v = v0 + r; v < v1; v += rows) s += act_ld1(g + v * g_ld + c);
        if (r < rows) sh[r * Cb + cl] = s;
        __syncthreads();
        if (r == 0 && c < C) {
            float a = 0.f;
            for (int rr = 0; rr < rows; ++rr) a += sh[rr * Cb + cl];
            part[(int64_t)blockIdx.x * C + c] = a;
        }
        __syncthreads();
    }
}

struct WgradGenericPlan {
    int npairs_blk, rows, npb, nchunks;
    int64_t vper;
    int64_t part_floats;   // wgrad partials
    int db_chunks;
    int64_t db_floats;
};

static WgradGenericPlan wgrad_generic_plan(int64_t NV, int Cin, int Cout, int ntaps) {
    WgradGenericPlan p;
    int pairs = Cin * Cout;
    p.npairs_blk = pairs < 256 ? pairs : 256;
    p.rows = 256 / p.npairs_blk;
    if (p.rows < 1) p.rows = 1;
    p.npb = (int)tem_cdiv(pairs, p.npairs_blk);
    int64_t nch = tem_cdiv(NV, (int64_t)p.rows * 64);
    int64_t cap = (64ll << 20) / ((int64_t)ntaps * pairs * 4);
    if (cap < 1) cap = 1;
    if (nch > cap) nch = cap;
    if (nch > 2048) nch = 2048;
    if (nch < 1) nch = 1;
    p.nchunks = (int)nch;
    p.vper = tem_cdiv(NV, nch);
    p.part_floats = (int64_t)p.nchunks * ntaps * pairs;
    int64_t dbc = tem_cdiv(NV, 2048);
    if (dbc > 512) dbc = 512;
    if (dbc < 1) dbc = 1;
    p.db_chunks = (int)dbc;
    p.db_floats = (int64_t)p.db_chunks * Cout;
    return p;
}

template <int KD, int KH, int KW>
static void launch_wgrad_generic(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                                 int64_t g_ld, int N, int D, int H, int W, int Cin, int Cout,
                                 const WgradGenericPlan& p, float* part, hipStream_t s) {
    constexpr int NT = KD * KH * KW;
    size_t lds = (size_t)NT * p.rows * p.npairs_blk * sizeof(float);
    TEM_ST2_SWITCH(c.stx, c.sty, TX, TG, (void)0,
                   hipLaunchKernelGGL((k_conv_wgrad_generic<KD, KH, KW, TX, TG>), dim3(p.nchunks, p.npb), dim3(256), lds, s, (const TX*)x,
                                      x_ld, scale, shift, (const TG*)g, g_ld, N, D, H, W, Cin, Cout, p.npairs_blk, p.rows, p.vper, part));
}

// ---------------------------------------------------------------------------
// The weight-gradient dispatch (DESIGN.md "Weight-gradient dispatch: one plan"): wgrad_plan() decides ONCE which kernel a call
// takes, with which geometry and workspace regions, and which by-products that kernel delivers.  conv3d_wgrad_impl executes the
// plan; the queries (tem_conv3d_wgrad_ws, _sums_ok, _gmax_ok, _gscaled_ok, _cs_ok, _gnorm_ok) print it for synthetic facts.
// Split modes: z-sliding, else the split-precision patch kernel.  Every other MFMA mode runs exact fp32: the transposing
// z-sliding kernel where the layout allows its 16-byte loads, else the fp32 patch kernel.  VALU: first layer, projection, generic.
// ---------------------------------------------------------------------------
enum WgradKernel { WK_GENERIC, WK_CIN1, WK_PROJ, WK_ZS, WK_PATCH, WK_PATCH_FP32, WK_REFUSED };

// what the decision depends on besides the call, the shape and the mode
struct WgradFacts {
    int64_t x_ld, g_ld, gnx_ld;
    // operand groups on 16-byte boundaries (an absent operand counts as aligned)
    bool x16, g16;
    bool ss16;   // scale and shift
    bool gn16;   // gnx and gcoef
    bool scale, db, norm_sums, w, gcoef, sd_layout;   // which optional operands the call carries (w: the weights the sums read)
    int64_t ws_bytes;
};

struct WgradPlan {
    WgradKernel kernel;
    int rc;                  // WK_REFUSED: TEM_EINVAL or TEM_EWS
    TemWgradKind kind;       // the arithmetic of the MFMA families
    ZsPlan zs;               // WK_ZS (k_conv_wgrad_zs<zs.nco> / _zt if zs.teams / _tr if zs.tr)
    WbPlan wb;               // WK_PATCH
    WgradFp32Plan fp32;      // WK_PATCH_FP32
    WgradGenericPlan gen;    // WK_GENERIC; its bias partials lie at the start of the workspace in every plan
    int64_t ws_bytes;        // the workspace the launch needs (also of a plan refused for its layout)
    int64_t part, dbpart, extra;   // regions of the planned kernel, in floats from the start of the workspace: partial slabs, bias
                                   // partials, WK_ZS: what the sums merge needs behind them
    // what the planned kernel delivers when a call asks for it (a call that asks for more is refused)
    bool sums;    // the norm-backward sums
    bool gmax;    // max |g| (g_amax_out)
    bool f16x2;   // the fp16 2x1 arithmetic from a prescale (g_amax_in)
    bool cs;      // this call's chunk stride of x
    char error[320];         // WK_REFUSED: the message of the error the launch returns
};

static WgradPlan& wgrad_refuse(WgradPlan& p, int rc, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static WgradPlan& wgrad_refuse(WgradPlan& p, int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.error, sizeof(p.error), fmt, ap);
    va_end(ap);
    p.kernel = WK_REFUSED;
    p.rc = rc;
    return p;
}

static WgradPlan wgrad_plan(const TemConvCall& c, const TemConvShape& sh, int mode, const WgradFacts& f) {
    WgradPlan p = {};
    const int Cin = sh.Cin, Cout = sh.Cout, ntaps = sh.kd * sh.kh * sh.kw, st = c.stx;
    const bool split = tem_arith_split_wgrad(mode);   // (any other MFMA mode runs exact fp32)
    p.kind = split ? tem_arith(mode).wgrad : mode != TEM_ARITH_VALU ? TEM_WG_FP32 : TEM_WG_NONE;
    // the MFMA geometries divide by Cin / 32: an MFMA mode on other channel counts is sized as the VALU family and refused below
    const bool chan32 = Cin % 32 == 0 && Cout % 32 == 0;
    p.kernel = WK_GENERIC;
    p.gen = wgrad_generic_plan(sh.NV(), Cin, Cout, ntaps);
    p.part = tem_align_up(p.gen.db_floats, 64);
    int64_t bytes;   // of the regions behind p.part
    bool sums_shape = false;
    if (mode != TEM_ARITH_VALU && chan32) {
        p.zs = tem_zs_plan(sh);
        sums_shape = p.zs.use && tem_wgrad_sums_takes(sh);
        const int64_t zs_bytes =
            (p.zs.part_floats(sh) + p.zs.db_floats(sh) + (sums_shape ? tem_wgrad_sums_ws_floats(sh.N, sh.D, sh.H, Cin, Cout) : 0)) * 4 + 256;
        if (split && p.zs.use) {
            p.kernel = WK_ZS;
            bytes = zs_bytes;
        } else if (split) {
            p.kernel = WK_PATCH;
            p.wb = tem_wb_plan(sh);
            p.dbpart = p.part + tem_align_up((int64_t)p.wb.S * p.wb.ks2 * ntaps * Cin * Cout, 64);
            bytes = (p.dbpart - p.part) * 4 + (int64_t)p.wb.S * Cout * 4 + 256;
        } else {
            const bool tr = p.zs.use && p.zs.tr;
            p.kernel = tr && !c.stx && !c.sty && f.x_ld % 4 == 0 && f.g_ld % 4 == 0 && f.x16 && f.g16 ? WK_ZS : WK_PATCH_FP32;
            p.fp32 = tem_wgrad_fp32_plan(sh);
            p.dbpart = p.part + tem_align_up((int64_t)p.fp32.S * ntaps * Cin * Cout, 64);
            bytes = ((int64_t)p.fp32.S * ntaps * Cin * Cout + (int64_t)p.fp32.S * Cout) * 4 + 256;
            // alignment moves an exact-fp32 call between the transposing kernel and the patch kernel at launch time, which the
            // workspace query cannot know: sized for both
            if (tr && zs_bytes > bytes) bytes = zs_bytes;
        }
        if (p.kernel == WK_ZS) {
            p.dbpart = p.part + p.zs.part_floats(sh);
            p.extra = p.dbpart + p.zs.db_floats(sh);
        }
    } else {
        bytes = p.gen.part_floats * 4;
        if (Cin <= 4 && tem_conv_wgrad_cin1_ws(Cout, ntaps) > bytes) bytes = tem_conv_wgrad_cin1_ws(Cout, ntaps);
        if (ntaps == 1 && tem_conv1x1_proj_wgrad_ws(Cin, Cout) > bytes) bytes = tem_conv1x1_proj_wgrad_ws(Cin, Cout);
        if (mode == TEM_ARITH_VALU) {   // g (and the gnorm operands) in 16-byte rows / x without a pre-norm in 16-byte rows
            if (tem_conv_wgrad_cin1_takes(sh) && f.g_ld % 4 == 0 && f.g16 && !(f.gcoef && (f.gnx_ld % 4 || !f.gn16))) p.kernel = WK_CIN1;
            else if (ntaps == 1 && tem_conv1x1_proj_wgrad_takes(Cin, Cout) && !f.scale && f.x_ld % 4 == 0 && f.x16) p.kernel = WK_PROJ;
        }
    }
    p.ws_bytes = p.part * 4 + bytes + 256;
    const bool zs = p.kernel == WK_ZS;
    p.gmax = zs && p.kind == TEM_WG_BF16X3;
    p.f16x2 = zs && p.kind == TEM_WG_F16X2 && (!p.zs.teams || p.zs.tr);   // (k_conv_wgrad_zt has no fp16 2x1 variant)
    p.cs = zs && p.zs.tr && st != 0 && c.x_cs % 8 == 0;
    // exact fp32 delivers the sums where the data gradient that consumes them runs on the z-reuse kernel (option fp32_zr); an
    // fp32 call that alignment moves off the transposing kernel is refused below
    p.sums = sums_shape && (split || (mode == TEM_ARITH_FP32 && tem_option(TEM_OPT_FP32_ZR) && !c.stx && !c.sty && p.zs.tr));

    // by-products the planned kernel does not deliver
    if (c.g_amax_out && !p.gmax)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_gmax: tem_conv3d_wgrad_gmax_ok() == 0 for this layer");
    if (c.g_amax_in && !p.f16x2)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_gscaled: tem_conv3d_wgrad_gscaled_ok() == 0 for this layer");
    if (f.norm_sums && !(f.w && f.db && f.sd_layout && p.sums))
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_sums: norm_sums needs weights, a bias gradient and tem_conv3d_wgrad_sums_ok() != 0");
    if (f.gcoef && p.kernel != WK_CIN1)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_gnorm: only the small-Cin first-layer kernel applies a norm backward to g "
                                           "(tem_conv3d_wgrad_gnorm_ok() != 0; g / y / coefficients 16-byte aligned with ld %% 4 == 0)");
    if (f.ws_bytes < p.ws_bytes) return wgrad_refuse(p, TEM_EWS, "tem_conv3d_wgrad: workspace too small");
    if (c.x_cs && !p.cs)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_ex: a chunk stride (x_cs) needs 16-bit tensors on the transposing z-sliding "
                                           "kernel (use_mfma 5 / 7, tem_conv3d_wgrad_cs_ok() != 0), x_cs %% 8 == 0");
    if (mode == TEM_ARITH_VALU) return p;
    const char* const who = split ? "bf16x3" : "mfma";
    if (!chan32) return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): needs Cin%%32==0 and Cout%%32==0 (got %d,%d)", who, Cin, Cout);
    if (st != c.sty) return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): x and g must have the same storage type", who);
    if (!tem_wgrad_storage_ok(p.kind, st))
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): 16-bit storage goes with the one-term mode of the same type (fp16: "
                                           "use_mfma 5, bf16: use_mfma 7), got storage %d", who, st);
    if (f.x_ld % (st ? 8 : 4) || f.g_ld % (st ? 8 : 4) || !f.x16 || !f.g16)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): x / g must be 16-byte aligned with ld%%4==0 (16-bit storage: ld%%8==0)", who);
    if (!f.ss16) return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): scale/shift must be 16-byte aligned", who);
    if (p.kind == TEM_WG_F16X2 && !c.g_amax_in)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_gscaled: the fp16 2x1 arithmetic (use_mfma 8) needs g_amax");
    if (f.norm_sums && !zs)
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad_sums: only the z-sliding kernels deliver the norm sums (x / g need 16-byte rows)");
    if (zs) {
        if ((int64_t)sh.H * sh.W * (f.x_ld > f.g_ld ? f.x_ld : f.g_ld) * 4 >= (1ll << 31))
            return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): one z-plane of x / g must stay below 2 GiB (32-bit offsets inside a plane)", who);
        if (st && !p.zs.tr)
            return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad: 16-bit storage needs the transposing z-sliding kernel (option wgrad_zs = 3)");
    } else if (sh.key() != 7 && sh.key() != 3 && sh.key() != 0) {
        return wgrad_refuse(p, TEM_EINVAL, "tem_conv3d_wgrad(%s): kernel (%d,%d,%d) has no MFMA instantiation", who, sh.kd, sh.kh, sh.kw);
    }
    return p;
}

// The plan of a dense, 16-byte aligned launch of this shape with all the workspace it asks for, as the queries see it
static WgradPlan wgrad_query(const TemConvCall& c, const TemConvShape& sh, int mode) {
    const WgradFacts f = {sh.Cin, sh.Cout, sh.Cout, true, true, true, true, false, true, false, false, false, true, INT64_MAX};
    return wgrad_plan(c, sh, mode, f);
}

extern "C" int64_t tem_conv3d_wgrad_ws(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma) {
    // (the storage types do not change the workspace)
    return wgrad_query(TemConvCall{}, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma & 0xff).ws_bytes;
}

extern "C" int tem_conv3d_wgrad_sums_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma) {
    const TemConvCall c = conv_call(use_mfma);
    return wgrad_query(c, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma).sums;
}

extern "C" int tem_conv3d_wgrad_gmax_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma) {
    return wgrad_query(TemConvCall{}, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, use_mfma & 0xff).gmax;
}

extern "C" int tem_conv3d_wgrad_gscaled_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw) {
    return wgrad_query(TemConvCall{}, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, TEM_ARITH_F16X2).f16x2;
}

// x of storage type st with chunk stride x_cs, in the one-term mode of that type
extern "C" int tem_conv3d_wgrad_cs_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int st, int64_t x_cs) {
    TemConvCall c = {st, st};
    c.x_cs = x_cs;
    return wgrad_query(c, TemConvShape{N, D, H, W, Cin, Cout, kd, kh, kw}, st == TEM_ST_BF16 ? TEM_ARITH_BF16 : TEM_ARITH_F16).cs;
}

// tem_conv3d_wgrad_gnorm: the layers of the small-Cin first-layer kernel (whatever their extent)
extern "C" int tem_conv3d_wgrad_gnorm_ok(int Cin, int Cout, int kd, int kh, int kw, int use_mfma) {
    if (Cin <= 0 || Cout <= 0) return 0;
    return wgrad_query(TemConvCall{}, TemConvShape{1, 1, 1, 1, Cin, Cout, kd, kh, kw}, use_mfma & 0xff).kernel == WK_CIN1;
}

// the argument checks of every weight-gradient launch, shared by conv3d_wgrad_impl and the dispatch query of an actual launch
// (tem_conv3d_wgrad_path; outputs: the launch has dw and its workspace): a failed check leaves its message for tem_last_error()
static int wgrad_args_check(const TemConvCall& c, const void* x, int64_t x_ld, const void* scale, const void* shift, const void* g,
                            int64_t g_ld, bool outputs, const TemConvShape& sh, int use_mfma) {
    const int N = sh.N, D = sh.D, H = sh.H, W = sh.W, Cin = sh.Cin, Cout = sh.Cout, kd = sh.kd, kh = sh.kh, kw = sh.kw;
    TEM_REQUIRE(x && g && outputs, "tem_conv3d_wgrad: null pointer");
    TEM_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && x_ld >= (c.x_cs ? 32 : Cin) && g_ld >= Cout,
                "tem_conv3d_wgrad: bad shape");
    TEM_REQUIRE((kd == 1 || kd == 3) && (kh == 1 || kh == 3) && (kw == 1 || kw == 3),
                "tem_conv3d_wgrad: kernel size (%d,%d,%d) not supported (1 or 3 per axis)", kd, kh, kw);
    TEM_REQUIRE((scale == nullptr) == (shift == nullptr), "tem_conv3d_wgrad: scale and shift must both be given");
    const int stx = c.stx, sty = c.sty;
    TEM_REQUIRE(stx >= 0 && stx <= 2 && sty >= 0 && sty <= 2 && (stx == 0 || sty == 0 || stx == sty),
                "tem_conv3d_wgrad: unsupported storage types (x %d, g %d)", stx, sty);
    TEM_REQUIRE(!(stx || sty) || tem_arith(use_mfma).wgrad != TEM_WG_FP32,
                "tem_conv3d_wgrad: the exact-fp32 MFMA kernels take fp32 tensors only");
    return TEM_OK;
}
// ... and of tem_conv3d_wgrad_gnorm[_st] on top of them
static int wgrad_gnorm_args_check(const void* y, int64_t y_ld, const void* gcoef, int Cout) {
    TEM_REQUIRE(y && gcoef && y_ld >= Cout, "tem_conv3d_wgrad_gnorm: null pointer");
    return TEM_OK;
}

static int conv3d_wgrad_impl(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                             int64_t g_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int N, int D, int H,
                             int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma, int sd_layout,
                             const float* w_sd, const float* gamma, const float* beta, float* norm_sums,
                             const float* gnx, int64_t gnx_ld, const float* gcoef, tem_stream_t stream) {
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TEM_TRY(wgrad_args_check(c, x, x_ld, scale, shift, g, g_ld, dw && ws, sh, use_mfma));
    auto al16 = [](const void* ptr) { return (uintptr_t)ptr % 16 == 0; };
    const WgradFacts facts = {x_ld, g_ld, gnx_ld, al16(x), al16(g), al16(scale) && al16(shift), al16(gnx) && al16(gcoef),
                              scale != nullptr, db != nullptr, norm_sums != nullptr, w_sd != nullptr, gcoef != nullptr, sd_layout != 0,
                              ws_bytes};
    const WgradPlan p = wgrad_plan(c, sh, use_mfma, facts);
    if (p.kernel == WK_REFUSED) {
        tem_set_error("%s", p.error);
        return p.rc;
    }
    hipStream_t s = (hipStream_t)stream;
    float* const part = (float*)ws + p.part;
    float* const dbpart = db ? (float*)ws + p.dbpart : nullptr;
    static const char* const what[] = {"tem_conv3d_wgrad(generic)", "tem_conv3d_wgrad(cin1)", "tem_conv3d_wgrad(proj)",
                                       "tem_conv3d_wgrad(z-sliding)", "tem_conv3d_wgrad(bf16x3)", "tem_conv3d_wgrad(mfma)"};
    if (p.kernel == WK_ZS) {
        tem_conv_wgrad_zs(c, p.zs, p.kind, x, x_ld, scale, shift, g, g_ld, dw, db, part, dbpart, (float*)ws + p.extra, sh, sd_layout, w_sd,
                          gamma, beta, norm_sums, s);
    } else if (p.kernel == WK_PATCH) {
        tem_conv_wgrad_patch(c, p.wb, x, x_ld, scale, shift, g, g_ld, dw, db, part, dbpart, sh, sd_layout, s);
    } else if (p.kernel == WK_PATCH_FP32) {
        tem_conv_wgrad_mfma(p.fp32, x, x_ld, scale, shift, g, g_ld, dw, db, part, dbpart, sh, sd_layout, s);
    } else if (p.kernel == WK_CIN1) {
        tem_conv_wgrad_cin1(c, x, x_ld, scale, shift, g, g_ld, dw, db, part, sh, sd_layout, gnx, gnx_ld, gcoef, s);
    } else if (p.kernel == WK_PROJ) {
        tem_conv1x1_proj_wgrad(c, x, x_ld, g, g_ld, dw, db, part, sh.NV(), Cin, Cout, sd_layout, s);
    } else {
        const int64_t NV = sh.NV();
        const int ntaps = kd * kh * kw;
        if (db) {   // bias partials at the start of the workspace
            int Cb = Cout < 256 ? Cout : 256;
            int rows = 256 / Cb;
            int64_t vper = tem_cdiv(NV, p.gen.db_chunks);
            TEM_ST_SWITCH(c.sty, TG,
                          hipLaunchKernelGGL(k_colsum_partial<TG>, dim3(p.gen.db_chunks), dim3(256), (size_t)rows * Cb * sizeof(float), s,
                                             (const TG*)g, g_ld, NV, Cout, rows, vper, (float*)ws));
            tem_reduce_slabs((const float*)ws, p.gen.db_chunks, (int64_t)Cout, (int64_t)Cout, db, s);
        }
#define CALL(A, B, C) launch_wgrad_generic<A, B, C>(c, x, x_ld, scale, shift, g, g_ld, N, D, H, W, Cin, Cout, p.gen, part, s)
        DISPATCH_K(kd, kh, kw, CALL);
#undef CALL
        tem_reduce_slabs_w(part, p.gen.nchunks, ntaps, Cin, Cout, (int64_t)ntaps * Cin * Cout, dw, sd_layout, s);
    }
    TEM_CHECK_LAUNCH(what[p.kernel]);
    return TEM_OK;
}

extern "C" int tem_conv3d_wgrad(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                                int64_t g_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int N, int D, int H,
                                int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma, int sd_layout,
                                tem_stream_t stream) {
    const TemConvCall c = conv_call(use_mfma);
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw,
                             use_mfma, sd_layout, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, stream);
}

// The kernel wgrad_plan() names for a tem_conv3d_wgrad / _gnorm[_st] launch with exactly these arguments (tem_hip.h: TEM_WGRAD_*;
// launches nothing): the argument checks of conv3d_wgrad_impl, then the plan of the launch's real facts.  gnx / gcoef: the y and
// the coefficients of tem_conv3d_wgrad_gnorm (null: a plain tem_conv3d_wgrad)
extern "C" int tem_conv3d_wgrad_path(const void* x, int64_t x_ld, const void* scale, const void* shift, const void* g, int64_t g_ld,
                                     const void* gnx, int64_t gnx_ld, const void* gcoef, int has_db, int64_t ws_bytes, int N, int D,
                                     int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma, int sd_layout) {
    const TemConvCall c = conv_call(use_mfma);
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    if (wgrad_args_check(c, x, x_ld, scale, shift, g, g_ld, true, sh, use_mfma) != TEM_OK) return -1;
    if ((gnx || gcoef) && (use_mfma != TEM_ARITH_VALU || wgrad_gnorm_args_check(gnx, gnx_ld, gcoef, Cout) != TEM_OK)) return -1;
    auto al16 = [](const void* ptr) { return (uintptr_t)ptr % 16 == 0; };
    const WgradFacts facts = {x_ld, g_ld, gnx_ld, al16(x), al16(g), al16(scale) && al16(shift), al16(gnx) && al16(gcoef),
                              scale != nullptr, has_db != 0, false, false, gcoef != nullptr, sd_layout != 0, ws_bytes};
    const WgradPlan p = wgrad_plan(c, sh, use_mfma, facts);
    return p.kernel == WK_REFUSED ? -1 : (int)p.kernel;
}

// Backward of the network's output projection (out_conv: nn.Conv3d(features, out_channels, 1), reference model/unet.py:638)
// in ONE pass over its input x (a ReLU output): dw, db as tem_conv3d_wgrad AND the masked data gradient
// gx = (x > 0) * (g . w) as tem_conv3d_fwd(transposed pack, ref = x) -- two kernels that each read the 512 MB tensor before.
extern "C" int tem_conv1x1_out_bwd_ok(int Cin, int Cout) { return tem_conv1x1_out_bwd_takes(Cin, Cout); }
static int conv1x1_out_bwd_impl(const TemConvCall& c, const float* x, int64_t x_ld, const float* g, int64_t g_ld, const float* w,
                                float* gx, int64_t gx_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int64_t NV, int Cin,
                                int Cout, tem_stream_t stream) {
    TEM_REQUIRE(x && g && w && gx && dw && ws && NV > 0 && x_ld >= Cin && gx_ld >= Cin && g_ld >= Cout,
                "tem_conv1x1_out_bwd: bad arguments");
    TEM_REQUIRE(tem_conv1x1_out_bwd_ok(Cin, Cout), "tem_conv1x1_out_bwd: tem_conv1x1_out_bwd_ok() == 0 for %d -> %d", Cin, Cout);
    TEM_REQUIRE(ws_bytes >= tem_conv1x1_proj_wgrad_ws(Cin, Cout), "tem_conv1x1_out_bwd: workspace too small");
    TEM_REQUIRE(tem_st2_ok(c.stx, c.sty) && x_ld % 4 == 0 && gx_ld % 4 == 0 && ((uintptr_t)x | (uintptr_t)gx | (uintptr_t)w) % 16 == 0,
                "tem_conv1x1_out_bwd: x / gx / w need 16-byte alignment and ld %% 4 == 0");
    tem_conv1x1_out_bwd(c, x, x_ld, g, g_ld, w, gx, gx_ld, dw, db, (float*)ws, NV, Cin, Cout, 1, (hipStream_t)stream);
    TEM_CHECK_LAUNCH("tem_conv1x1_out_bwd");
    return TEM_OK;
}
extern "C" int tem_conv1x1_out_bwd(const float* x, int64_t x_ld, const float* g, int64_t g_ld, const float* w, float* gx,
                                   int64_t gx_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int64_t NV, int Cin,
                                   int Cout, tem_stream_t stream) {
    return conv1x1_out_bwd_impl(TemConvCall{}, x, x_ld, g, g_ld, w, gx, gx_ld, dw, db, ws, ws_bytes, NV, Cin, Cout, stream);
}
extern "C" int64_t tem_conv1x1_out_bwd_ws(int Cin, int Cout) { return tem_conv1x1_proj_wgrad_ws(Cin, Cout); }

// tem_conv1x1_out_bwd for x / gx of storage type st_x and g of storage type st_g (g is the gradient of the network output:
// normally fp32); out_amax (optional): device word that receives max |gx| (see tem_maxpool3d_bwd_st)
extern "C" int tem_conv1x1_out_bwd_st(const void* x, int64_t x_ld, const void* g, int64_t g_ld, const float* w, void* gx,
                                      int64_t gx_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int64_t NV, int Cin,
                                      int Cout, unsigned* out_amax, int st_x, int st_g, tem_stream_t stream) {
    TEM_REQUIRE(st_x >= 0 && st_x <= 2 && st_g >= 0 && st_g <= 2, "tem_conv1x1_out_bwd_st: unknown storage type");
    TemByproducts bp = {};
    bp.out_amax = out_amax;
    const TemConvCall c = {st_x, st_g, 0, 0, &bp};
    return conv1x1_out_bwd_impl(c, (const float*)x, x_ld, (const float*)g, g_ld, w, (float*)gx, gx_ld, dw, db, ws, ws_bytes, NV, Cin,
                                Cout, stream);
}

extern "C" int tem_conv3d_wgrad_gmax(const float* x, int64_t x_ld, const float* scale, const float* shift,
                                     const float* g, int64_t g_ld, const float* w, const float* gamma,
                                     const float* beta, float* dw, float* db, float* norm_sums, unsigned* g_amax,
                                     void* ws, int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd,
                                     int kh, int kw, int use_mfma, tem_stream_t stream) {
    TemConvCall c = conv_call(use_mfma);
    TEM_REQUIRE(g_amax, "tem_conv3d_wgrad_gmax: null g_amax");
    c.g_amax_out = g_amax;
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, use_mfma, 1,
                             norm_sums ? w : nullptr, gamma, beta, norm_sums, nullptr, 0, nullptr, stream);
}

// ---- weight gradient with 16-bit-class x^ and an 11-bit g (two MFMAs per product instead of three) -----------------------
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ x, int64_t ld, int cq, int64_t nq, unsigned* __restrict__ amax) {
    // nq = voxels * cq float4 items; max |x| as an integer max of the bit patterns (exact, order-independent; inf wins, NaNs are
    // skipped by v_max_f32 -- the consumers multiply the NaN itself through, so nothing is hidden)
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
        const int64_t v = i / cq;
        const int q = (int)(i - v * cq);
        typedef float f4n __attribute__((ext_vector_type(4)));
        const f4n t = __builtin_nontemporal_load(reinterpret_cast<const f4n*>(x + v * ld + q * 4));
        m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(t.x), __builtin_fabsf(t.y)),
                                               __builtin_fmaxf(__builtin_fabsf(t.z), __builtin_fabsf(t.w))));
    }
    unsigned u = __builtin_bit_cast(unsigned, m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, o, 64));
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = u;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax, max(max(red[0], red[1]), max(red[2], red[3])));
}

extern "C" int tem_absmax(const float* x, int64_t ld, int C, int64_t nvox, unsigned* amax, tem_stream_t stream) {
    TEM_REQUIRE(x && amax && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && ((uintptr_t)x % 16 == 0) && nvox >= 0,
                "tem_absmax: needs 16-byte aligned rows of C %% 4 == 0 floats");
    if (nvox == 0) return TEM_OK;
    const int64_t nq = nvox * (C / 4);
    int64_t nb = tem_cdiv(nq, 256 * 8);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_absmax, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, ld, C / 4, nq, amax);
    TEM_CHECK_LAUNCH("tem_absmax");
    return TEM_OK;
}

extern "C" int tem_conv3d_wgrad_gscaled(const float* x, int64_t x_ld, const float* scale, const float* shift,
                                        const float* g, int64_t g_ld, const float* w, const float* gamma,
                                        const float* beta, float* dw, float* db, float* norm_sums,
                                        const unsigned* g_amax, void* ws, int64_t ws_bytes, int N, int D, int H, int W,
                                        int Cin, int Cout, int kd, int kh, int kw, tem_stream_t stream) {
    TemConvCall c;
    TEM_REQUIRE(g_amax, "tem_conv3d_wgrad_gscaled: null g_amax");
    c.g_amax_in = g_amax;
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, TEM_ARITH_F16X2, 1,
                             norm_sums ? w : nullptr, gamma, beta, norm_sums, nullptr, 0, nullptr, stream);
}

// the argument checks of tem_conv3d_fwd_gscaled / _refnorm (also tem_conv3d_fwd_ex with in_amax / ref_coef).  Whether the launch
// then really takes the z-reuse kernel is the plan of its real arguments: conv3d_fwd_impl fails a call that carries one otherwise.
static int fwd_gscaled_check(const TemConvCall& c, const float* x, int64_t x_ld, const float* w_packed, const float* y, int64_t y_ld,
                             const float* ref, int64_t ref_ld, const TemConvShape& sh) {
    TEM_REQUIRE(c.in_amax, "tem_conv3d_fwd_gscaled: null in_amax");
    TEM_REQUIRE(fwd_query(c, sh, TEM_ARITH_F16X3, x_ld, y_ld, ref ? ref_ld : 0,
                          fwd_misaligned(x, nullptr, nullptr, w_packed, nullptr, y, ref)).family() == 3,
                "tem_conv3d_fwd_gscaled: only launches that tem_conv3d_fwd_kernel_ld() reports as 3 (z-reuse kernel) take a "
                "device-side prescale");
    return TEM_OK;
}
static int fwd_refnorm_check(const TemConvCall& c, const float* x, int64_t x_ld, const float* w_packed, const float* y, int64_t y_ld,
                             const float* ref, int64_t ref_ld, const TemConvShape& sh, int use_mfma) {
    TEM_REQUIRE(ref && c.ref_coef, "tem_conv3d_fwd_refnorm: null ref / coef");
    TEM_REQUIRE(fwd_query(c, sh, use_mfma, x_ld, y_ld, ref_ld,
                          fwd_misaligned(x, nullptr, nullptr, w_packed, c.ref_coef, y, ref)).family() == 3,
                "tem_conv3d_fwd_refnorm: only launches that tem_conv3d_fwd_kernel_ld() reports as 3 (z-reuse kernel) apply a "
                "norm backward in their epilogue");
    return TEM_OK;
}

extern "C" int tem_conv3d_fwd_gscaled(const float* x, int64_t x_ld, const float* w_packed, float* y, int64_t y_ld,
                                      const float* ref, int64_t ref_ld, const unsigned* in_amax, void* ws,
                                      int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                                      int kw, tem_stream_t stream) {
    TemConvCall c;
    c.in_amax = in_amax;
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TEM_TRY(fwd_gscaled_check(c, x, x_ld, w_packed, y, y_ld, ref, ref_ld, sh));
    return conv3d_fwd_impl(c, x, x_ld, nullptr, nullptr, w_packed, nullptr, y, y_ld, ref, ref_ld, ws, ws_bytes, sh, TEM_ACT_NONE,
                           TEM_ARITH_F16X3, nullptr, stream);
}

// Data gradient that lands behind a ReLU + norm: y = ref > 0 ? a*(conv) - m1 - (ref - mean)*m2r : 0 with coef[N][Cout][4] =
// (a, m1, m2r, mean) from tem_norm_bwd_coef -- the epilogue of the z-reuse kernel replaces tem_norm_bwd_from_sums' pass over
// g and ref.  Only for launches tem_conv3d_fwd_kernel_ld() reports as 3.
extern "C" int tem_conv3d_fwd_refnorm(const float* x, int64_t x_ld, const float* w_packed, float* y, int64_t y_ld,
                                      const float* ref, int64_t ref_ld, const float* coef, void* ws, int64_t ws_bytes,
                                      int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma,
                                      tem_stream_t stream) {
    TemConvCall c = conv_call(use_mfma);
    c.ref_coef = coef;
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TEM_TRY(fwd_refnorm_check(c, x, x_ld, w_packed, y, y_ld, ref, ref_ld, sh, use_mfma));
    return conv3d_fwd_impl(c, x, x_ld, nullptr, nullptr, w_packed, nullptr, y, y_ld, ref, ref_ld, ws, ws_bytes, sh, TEM_ACT_NONE,
                           use_mfma, nullptr, stream);
}

extern "C" int tem_conv3d_wgrad_sums(const float* x, int64_t x_ld, const float* scale, const float* shift,
                                     const float* g, int64_t g_ld, const float* w, const float* gamma,
                                     const float* beta, float* dw, float* db, float* norm_sums, void* ws,
                                     int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                                     int kw, int use_mfma, tem_stream_t stream) {
    const TemConvCall c = conv_call(use_mfma);
    TEM_REQUIRE(w && norm_sums && db, "tem_conv3d_wgrad_sums: null pointer (weights, sums and bias gradient are required)");
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, use_mfma, 1,
                             w, gamma, beta, norm_sums, nullptr, 0, nullptr, stream);
}

// ---- every variant and by-product of the forward / data-gradient convolution as explicit arguments (tem_hip.h) -----------------
static int fwd_ex_call(TemConvCall& c, const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                       const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, const TemConvShape& sh, int act,
                       int use_mfma, const unsigned* in_amax, const float* ref_coef, bool stat_part, int64_t x_cs, int64_t y_cs,
                       TemByproducts* bp);
extern "C" int tem_conv3d_fwd_ex(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w_packed,
                                 const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, void* ws,
                                 int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int act,
                                 int use_mfma, const unsigned* in_amax, const float* ref_coef, float* stat_part,
                                 int64_t stat_blocks, int64_t x_cs, int64_t y_cs, TemByproducts* bp, tem_stream_t stream) {
    TemConvCall c = conv_call(use_mfma);
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TEM_TRY(fwd_ex_call(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, act, use_mfma, in_amax, ref_coef,
                        stat_part != nullptr, x_cs, y_cs, bp));
    if (stat_part)
        TEM_TRY(fwd_stats_check(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, use_mfma, stat_part, stat_blocks));
    return conv3d_fwd_impl(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws, ws_bytes, sh, act, use_mfma, stat_part,
                           stream);
}

// The kernel of the matrix-core family and the instantiation a tem_conv3d_fwd_ex launch with exactly these arguments takes
// (tem_hip.h; launches nothing): the checks of tem_conv3d_fwd_ex and of conv3d_fwd_impl, the plan, and the family's own
// selector of its template arguments (*_describe: conv_internal.h)
extern "C" int tem_conv3d_fwd_mfma_path(const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                                        const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld,
                                        int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int act,
                                        int use_mfma, const void* in_amax, const void* ref_coef, int has_stat, int64_t x_cs,
                                        int64_t y_cs, const TemByproducts* bp, int* inst) {
    TemFwdInst in = {};
    auto report = [&] { for (int i = 0; inst && i < TEM_MFMA_INST_N; ++i) inst[i] = in.v[i]; };
    report();
    TemConvCall c = conv_call(use_mfma);
    const TemConvShape sh = {N, D, H, W, Cin, Cout, kd, kh, kw};
    TemByproducts asked = {};   // the request as the launch would see it: nothing delivered yet
    if (bp) {
        asked = *bp;
        asked.delivered = 0;
    }
    if (use_mfma == TEM_ARITH_VALU ||
        fwd_ex_call(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, sh, act, use_mfma, (const unsigned*)in_amax,
                    (const float*)ref_coef, has_stat != 0, x_cs, y_cs, bp ? &asked : nullptr) != TEM_OK)
        return -1;
    FwdPlan p;
    if (fwd_launch_plan(c, x, x_ld, scale, shift, w_packed, bias, y, y_ld, ref, ref_ld, ws_bytes, sh, act, use_mfma, has_stat != 0, p) != TEM_OK)
        return -1;
    if (has_stat && !p.stat_blocks) {   // (fwd_stats_check: the caller's rows must be the launch's)
        tem_set_error("tem_conv3d_fwd_stats: this launch writes no statistics rows");
        return -1;
    }
    switch (p.kernel) {
        case FK_ZR: tem_conv_fwd_zr_describe(c, p.zr, 0, sh, use_mfma, ref != nullptr, has_stat != 0, in); break;
        case FK_ZR_SPLITK: tem_conv_fwd_zr_describe(c, p.zr, p.ks, sh, use_mfma, ref != nullptr, has_stat != 0, in); break;
        case FK_PP: tem_conv_fwd_pp_describe(p.pp, sh, use_mfma, in); break;
        case FK_STREAM1X1: tem_conv1x1_stream_describe(c, sh, use_mfma, in); break;
        case FK_PATCH: tem_conv_fwd_bf16x3_describe(c, p.patch, p.ks, sh, use_mfma, in); break;
        case FK_PATCH_FP32: tem_fwd_mfma_describe(p.patch, p.ks, sh, x_ld, in); break;
        default: return -1;
    }
    report();
    return (int)p.kernel;   // FwdKernel IS TEM_MFMA_*
}

// the checks of tem_conv3d_fwd_ex on its variant arguments; fills the call
static int fwd_ex_call(TemConvCall& c, const void* x, int64_t x_ld, const void* scale, const void* shift, const void* w_packed,
                       const void* bias, const void* y, int64_t y_ld, const void* ref, int64_t ref_ld, const TemConvShape& sh, int act,
                       int use_mfma, const unsigned* in_amax, const float* ref_coef, bool stat_part, int64_t x_cs, int64_t y_cs,
                       TemByproducts* bp) {
    TEM_REQUIRE(!stat_part || (!in_amax && !ref_coef && !bp), "tem_conv3d_fwd_ex: stat_part excludes in_amax / ref_coef / by-products");
    TEM_REQUIRE(!(in_amax && ref_coef), "tem_conv3d_fwd_ex: in_amax and ref_coef exclude each other");
    TEM_REQUIRE(x_cs >= 0 && y_cs >= 0 && (!(x_cs || y_cs) || (!in_amax && !ref_coef && tem_arith_one_term(use_mfma))),
                "tem_conv3d_fwd_ex: chunk strides go with the one-term modes on 16-bit tensors (use_mfma 5 / 7), no in_amax / ref_coef");
    TEM_REQUIRE(!bp || (!bp->coef && (!bp->sums_part || (bp->sums_x && bp->sums_mean && bp->sums_rstd && bp->sums_G > 0 && bp->sums_nblk > 0))),
                "tem_conv3d_fwd_ex: bad by-product request (TEM_BP_NORM_COEF belongs to tem_conv3d_wgrad_ex; TEM_BP_NORM_SUMS needs "
                "sums_x / sums_mean / sums_rstd / sums_G / sums_nblk)");
    c.x_cs = x_cs;
    c.y_cs = y_cs;
    c.bp = bp;
    if (bp) bp->delivered = 0;
    if (in_amax) {
        TEM_REQUIRE(!scale && !shift && !bias && act == TEM_ACT_NONE && use_mfma == TEM_ARITH_F16X3,
                    "tem_conv3d_fwd_ex: in_amax (the fp16 two-term data gradient) takes use_mfma 4 and no scale / shift / bias / act");
        c.stx = c.sty = TEM_ST_F32;   // as tem_conv3d_fwd_gscaled: an fp32-tensor mode
        c.in_amax = in_amax;
        TEM_TRY(fwd_gscaled_check(c, (const float*)x, x_ld, (const float*)w_packed, (const float*)y, y_ld, (const float*)ref, ref_ld, sh));
    } else if (ref_coef) {
        TEM_REQUIRE(!scale && !shift && !bias && act == TEM_ACT_NONE, "tem_conv3d_fwd_ex: ref_coef takes no scale / shift / bias / act");
        c.ref_coef = ref_coef;
        TEM_TRY(fwd_refnorm_check(c, (const float*)x, x_ld, (const float*)w_packed, (const float*)y, y_ld, (const float*)ref, ref_ld, sh,
                                  use_mfma));
    }
    return TEM_OK;
}

extern "C" int tem_conv3d_wgrad_ex(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                                   int64_t g_ld, const float* w, const float* gamma, const float* beta, float* dw, float* db,
                                   float* norm_sums, const unsigned* g_amax_in, unsigned* g_amax_out, void* ws, int64_t ws_bytes,
                                   int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int use_mfma,
                                   int64_t x_cs, TemByproducts* bp, tem_stream_t stream) {
    TemConvCall c = conv_call(use_mfma);
    TEM_REQUIRE(!(g_amax_in && g_amax_out), "tem_conv3d_wgrad_ex: g_amax_in and g_amax_out exclude each other");
    TEM_REQUIRE(x_cs >= 0 && (!x_cs || (!g_amax_in && !g_amax_out && tem_arith_one_term(use_mfma))),
                "tem_conv3d_wgrad_ex: a chunk stride goes with the one-term modes on 16-bit tensors (use_mfma 5 / 7)");
    TEM_REQUIRE(!bp || (!bp->out_amax && !bp->sums_part && (!bp->coef || (norm_sums && bp->coef_mean && bp->coef_rstd && bp->coef_G > 0))),
                "tem_conv3d_wgrad_ex: bad by-product request (only TEM_BP_NORM_COEF, which needs norm_sums, coef_mean, coef_rstd, coef_G)");
    c.x_cs = x_cs;
    c.bp = bp;
    if (bp) bp->delivered = 0;
    if (g_amax_in) {
        TEM_REQUIRE(use_mfma == TEM_ARITH_F16X2, "tem_conv3d_wgrad_ex: g_amax_in (the fp16 2x1 arithmetic) takes use_mfma 8");
        c.stx = c.sty = TEM_ST_F32;   // as tem_conv3d_wgrad_gscaled: an fp32-tensor mode
        c.g_amax_in = g_amax_in;
    }
    c.g_amax_out = g_amax_out;
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, use_mfma, 1,
                             norm_sums ? w : nullptr, gamma, beta, norm_sums, nullptr, 0, nullptr, stream);   // (w, gamma, beta: read for the sums only)
}

// tem_conv3d_wgrad of a FIRST layer (small Cin, VALU kernel) whose output gradient g is still the raw data gradient
// behind the norm that follows this conv's ReLU: the norm backward (coefficients from tem_norm_bwd_coef) and the ReLU
// mask are applied while g is loaded -- y (this conv's output, the norm's input) is read instead of a rewritten g.
static int wgrad_gnorm_impl(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                            int64_t g_ld, const float* y, int64_t y_ld, const float* gcoef, float* dw, float* db, void* ws,
                            int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd_layout,
                            tem_stream_t stream) {
    TEM_TRY(wgrad_gnorm_args_check(y, y_ld, gcoef, Cout));
    return conv3d_wgrad_impl(c, x, x_ld, scale, shift, g, g_ld, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, TEM_ARITH_VALU,
                             sd_layout, nullptr, nullptr, nullptr, nullptr, y, y_ld, gcoef, stream);
}
extern "C" int tem_conv3d_wgrad_gnorm(const float* x, int64_t x_ld, const float* scale, const float* shift,
                                      const float* g, int64_t g_ld, const float* y, int64_t y_ld, const float* gcoef,
                                      float* dw, float* db, void* ws, int64_t ws_bytes, int N, int D, int H, int W,
                                      int Cin, int Cout, int kd, int kh, int kw, int sd_layout, tem_stream_t stream) {
    return wgrad_gnorm_impl(TemConvCall{}, x, x_ld, scale, shift, g, g_ld, y, y_ld, gcoef, dw, db, ws, ws_bytes, N, D, H, W, Cin, Cout,
                            kd, kh, kw, sd_layout, stream);
}

// tem_conv3d_wgrad_gnorm for x of storage type st_x and g / y of storage type st_g (TEM_ST_*)
extern "C" int tem_conv3d_wgrad_gnorm_st(const void* x, int64_t x_ld, const float* scale, const float* shift, const void* g,
                                         int64_t g_ld, const void* y, int64_t y_ld, const float* gcoef, float* dw, float* db,
                                         void* ws, int64_t ws_bytes, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                                         int kw, int sd_layout, int st_x, int st_g, tem_stream_t stream) {
    TEM_REQUIRE(st_x >= 0 && st_x <= 2 && st_g >= 0 && st_g <= 2, "tem_conv3d_wgrad_gnorm_st: unknown storage type");
    const TemConvCall c = {st_x, st_g};
    return wgrad_gnorm_impl(c, (const float*)x, x_ld, scale, shift, (const float*)g, g_ld, (const float*)y, y_ld, gcoef, dw, db, ws,
                            ws_bytes, N, D, H, W, Cin, Cout, kd, kh, kw, sd_layout, stream);
}
