// conv_internal.h -- C++-internal interface between conv.hip (entry points, VALU kernels)
// and conv_mfma.hip (v_mfma_f32_32x32x2_f32 implicit-GEMM kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tem_hip.h"
#include "tem_common.h"

// Everything a convolution launch needs beyond its tensors and its shape.  The extern "C" entry point (conv.hip) decodes its
// arguments into one of these; every launcher and dispatch query takes the call it answers for as its first argument.
struct TemConvCall {
    int stx = 0;   // TEM_ST_* of the input-side tensors  (forward: x;      weight gradient: x)
    int sty = 0;   // TEM_ST_* of the output-side tensors (forward: y, ref; weight gradient: g and the gnorm y)
    // Channel-CHUNK strides in elements (the *_ex calls; 0 = the channels of a voxel are contiguous): the 32-channel chunk k of a
    // voxel lives at base + k * stride + voxel * ld, so that the halves of a 2 x 32-channel concat are two DENSE planes of whole
    // 128-byte lines (DESIGN.md 6.R5 "half lines").  Only the z-reuse forward / data-gradient kernel and the transposing
    // z-sliding weight gradient on 16-bit tensors take them; every other launch site refuses a call that carries one.
    int64_t x_cs = 0, y_cs = 0;
    TemByproducts* bp = nullptr;           // by-products the caller asks for (tem_hip.h); the launch site sets `delivered`
    const unsigned* in_amax = nullptr;     // forward: device-side prescale of the input (TEM_ARITH_F16X3), z-reuse kernel only
    const float* ref_coef = nullptr;       // forward: coef[N][Cout][4], norm backward in the epilogue, z-reuse kernel only
    unsigned* g_amax_out = nullptr;        // weight gradient: largest |g| as a by-product of the z-sliding kernels
    const unsigned* g_amax_in = nullptr;   // weight gradient: prescale of g in the fp16 2x1 arithmetic (TEM_WG_F16X2)

    bool wants(unsigned bit) const {       // the call asks for by-product `bit` and no launch has delivered it yet
        if (!bp || (bp->delivered & bit)) return false;
        return bit == TEM_BP_NORM_COEF ? bp->coef != nullptr : bit == TEM_BP_NORM_SUMS ? bp->sums_part != nullptr : bp->out_amax != nullptr;
    }
    void delivered(unsigned bit) const { if (bp) bp->delivered |= bit; }
    unsigned* take_output_amax() const {   // "output amax" (tem_common.h): the caller's device word for the launch site that takes it
        if (!wants(TEM_BP_OUT_AMAX)) return nullptr;
        delivered(TEM_BP_OUT_AMAX);
        return bp->out_amax;
    }
};

// The shape of a convolution call: what the forward host functions pass around instead of nine ints
struct TemConvShape {
    int N, D, H, W, Cin, Cout, kd, kh, kw;
    int64_t V() const { return (int64_t)D * H * W; }
    int64_t NV() const { return (int64_t)N * D * H * W; }
    int key() const { return (kd == 3) * 4 + (kh == 3) * 2 + (kw == 3); }   // 7: 3x3x3, 3: 1x3x3, 0: 1x1x1
};

// ---- the forward / data-gradient dispatch: geometry helpers of the kernel files, called by the ONE plan function (conv.hip:
// fwd_plan), and the launchers that execute what it planned.  A launcher decides nothing: its caller holds a plan that names it.
// The team kernels (and the z-reuse split-K launch) address one halo / one patch with 32-bit byte offsets
inline bool tem_plane32_ok(const TemConvShape& sh, int64_t ld) { return (int64_t)sh.H * sh.W * 8 * 4 * ld < (1ll << 31); }
// units a launch needs for a team kernel: two per CU; option team_min_units replaces that, conv_fwd_variant == `forced` lifts it
inline long long tem_team_min_units(int forced) {
    const long long minu = tem_option(TEM_OPT_TEAM_MIN_UNITS);
    return tem_option(TEM_OPT_CONV_FWD_VARIANT) == forced ? 1 : (minu > 0 ? minu : 2ll * tem_ncu());
}
// patch kernels (split-precision: conv_bf16x3.hip, exact fp32: conv_mfma.hip): patch extent, 32-column tiles per workgroup,
// patches per sample, workgroups, and the split-K factor the grid asks for (1: none; 16 input channels per staged chunk)
struct TemPatchTiling {
    bool flat;
    int TZ, TY, TX, NR;
    int64_t per, nblk;
    int ks;
};
TemPatchTiling tem_fwd_patch_tiling(const TemConvShape& sh);
// conv_zr.hip: 4 x 16 x 8 tiles.  shape_ok: options, mode and shape admit the kernel; ok: ... with enough units for a direct launch
// pair: the two teams of a workgroup share one staged halo per chunk (sibling output-channel tiles: Cout % 64 == 0, a two-term
// split mode on fp32 tensors, option zr_pair) -- the direct launch and the split-K launch of this geometry both run k_conv_zr<.., PAIR>
struct ZrGeom {
    int shape_ok, ok;
    int nZ, nY, nX;
    int64_t nunits;
    int pair;
};
// conv_pp.hip
struct PpGeom {
    int variant;  // 0: not handled here; 1: ping-pong teams, 4 x 8 x 8 voxel patch per team
    int TZ, TY, TX, CT, WM;
    int nZ, nY, nX;
    int64_t nunits;
};

// conv_mfma.hip: the exact-fp32 patch kernel with ks slices of the input channels (> 1: partial sums in ws).  Raises on x /
// weights / scale it cannot load as 16-byte vectors
int tem_conv_fwd_mfma(const TemPatchTiling& t, int ks, const float* x, int64_t x_ld, const float* scale, const float* shift,
                      const float* w_packed, const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, void* ws,
                      const TemConvShape& sh, int act, hipStream_t s);

int64_t tem_conv_wgrad_mfma_ws(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
int tem_conv_wgrad_mfma(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                        int64_t g_ld, float* dw_tap_ci_co, float* db, void* ws, int64_t ws_bytes, int N, int D, int H,
                        int W, int Cin, int Cout, int kd, int kh, int kw, int sd_layout, hipStream_t s);

// conv_small.hip: HBM-bound special cases (return false when the shape is not covered)
bool tem_conv_fwd_cin1(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w,
                       const float* bias, float* y, int64_t y_ld, const float* ref, int N, int D, int H, int W,
                       int Cin, int Cout, int kd, int kh, int kw, int act, float* stat, hipStream_t s);
int64_t tem_conv_fwd_cin1_stat_blocks(int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
int64_t tem_conv_wgrad_cin1_ws(int Cout, int ntaps);
bool tem_conv_wgrad_cin1(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                         int64_t g_ld, float* dw, float* db, void* ws, int N, int D, int H, int W, int Cin, int Cout,
                         int kd, int kh, int kw, int sd_layout, const float* gnx, int64_t gnx_ld, const float* gcoef,
                         hipStream_t s);
bool tem_conv_fwd_cout1(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w,
                        const float* bias, float* y, int64_t y_ld, const float* ref, int N, int D, int H, int W,
                        int Cin, int Cout, int kd, int kh, int kw, int act, hipStream_t s);
bool tem_conv1x1_proj(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* w, const float* bias, float* y,
                      int64_t y_ld, const float* ref, int64_t NV, int Cin, int Cout, int act, hipStream_t s);
int64_t tem_conv1x1_proj_wgrad_ws(int Cin, int Cout);
bool tem_conv1x1_proj_wgrad(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* g, int64_t g_ld, float* dw,
                            float* db, void* ws, int64_t NV, int Cin, int Cout, int sd_layout, hipStream_t s);
bool tem_conv1x1_out_bwd(const TemConvCall& c, const float* x, int64_t x_ld, const float* g, int64_t g_ld, const float* w, float* gx, int64_t gx_ld,
                         float* dw, float* db, void* ws, int64_t NV, int Cin, int Cout, int sd_layout, hipStream_t s);
bool tem_conv1x1_expand(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* w, const float* bias, float* y,
                        int64_t y_ld, const float* ref, int64_t ref_ld, int64_t NV, int Cin, int Cout, int act,
                        hipStream_t s);
void tem_reduce_slabs_w(const float* part, int nchunks, int ntaps, int Cin, int Cout, int64_t chunk_stride, float* dw,
                        int sd_layout, hipStream_t s);
void tem_reduce_slabs_w_db(const float* part, int nchunks, int ntaps, int Cin, int Cout, int64_t chunk_stride, float* dw,
                           int sd_layout, const float* dbpart, int db_chunks, float* db, hipStream_t s, int64_t db_stride = 0);
void tem_reduce_slabs(const float* part, int nchunks, int64_t n, int64_t chunk_stride, float* out, hipStream_t s);

// conv_bf16x3.hip: split-bf16 ("bf16x3") MFMA path
// `mode` of the launchers and queries below: the arithmetic mode, TEM_ARITH_* (conv_arith.h says what each means)
// planes, kind: TemArith::planes / ::pack of the layout
int tem_pack_weights_bf16x3(const float* w, float* dst, int Cout, int Cin, int kd, int kh, int kw, int transpose,
                            int planes, int kind, hipStream_t s);
// the split-precision patch kernel, ks as tem_conv_fwd_mfma; stat (ks == 1 only): [N][t.per][Cout][2]
void tem_conv_fwd_bf16x3(const TemConvCall& c, const TemPatchTiling& t, int ks, const float* x, int64_t x_ld, const float* scale,
                         const float* shift, const float* wp, const float* bias, float* y, int64_t y_ld, const float* ref,
                         int64_t ref_ld, void* ws, const TemConvShape& sh, int act, int mode, float* stat, hipStream_t s);
// conv_pp.hip: ping-pong team kernel for the levels with many patches; stat: [N][nZ * nY * nX * WM][Cout][2]
PpGeom tem_pp_geometry(const TemConvCall& c, const TemConvShape& sh, int mode);
void tem_conv_fwd_pp(const PpGeom& g, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* wp,
                     const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, const TemConvShape& sh, int act,
                     int mode, float* stat, hipStream_t s);
// conv_zr.hip: z-reuse ping-pong kernel, 3x3x3 only; stat: [N][nZ * nY * nX * 4][Cout][2].  Honours c.in_amax, c.ref_coef, c.x_cs / y_cs
ZrGeom tem_zr_geometry(const TemConvCall& c, const TemConvShape& sh, int mode);
void tem_conv_fwd_zr(const TemConvCall& c, const ZrGeom& g, const float* x, int64_t x_ld, const float* scale, const float* shift,
                     const float* wp, const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld,
                     const TemConvShape& sh, int act, int mode, float* stat, hipStream_t s);
// ... with the input channels cut into ks slices, for a shape whose geometry g has too few units for a direct launch and that
// the ping-pong kernel does not take either (0: no split-K launch for this shape).  ws: ks * NV * Cout floats;
// stat: [N][tem_splitk_stat_blocks()][Cout][2], written by the summing epilogue
int tem_zr_splitk_ks(const TemConvCall& c, const ZrGeom& g, const TemConvShape& sh, int mode);
void tem_conv_fwd_zr_splitk(const TemConvCall& c, const ZrGeom& g, int ks, const float* x, int64_t x_ld, const float* scale,
                            const float* shift, const float* wp, const float* bias, float* y, int64_t y_ld, const float* ref,
                            int64_t ref_ld, void* ws, const TemConvShape& sh, int act, int mode, float* stat, hipStream_t s);
// conv1x1_stream.hip: 1x1x1 convolution / data gradient as a streaming GEMM: no pre-norm, no statistics, no sigmoid
void tem_conv1x1_stream(const TemConvCall& c, const float* x, int64_t x_ld, const float* wp, const float* bias, float* y, int64_t y_ld,
                        const float* ref, int64_t ref_ld, const TemConvShape& sh, int act, int mode, hipStream_t s);
// shared with conv_mfma.hip
int tem_fwd_ksplit(int64_t nblk, int nchunks);
void tem_splitk_epilogue(int sty, const float* part, int ksplit, int64_t NV, int Cout, const float* bias, int act,
                         const float* ref, int64_t ref_ld, float* y, int64_t y_ld, hipStream_t s);
// TEM_BP_NORM_SUMS of a call, as the split-K data gradient whose epilogue can deliver the rows reads it
struct TemDgradSumsReq {
    const void* x;       // input of the norm the gradient lands behind: [N*V][x_ld], element type of the gradient
    int64_t x_ld;
    const float* mean;
    const float* rstd;
    int G;
    float* part;         // [N][nblk][C][2]
    int64_t nblk;
};
void tem_splitk_epilogue_bwd_sums(int sty, const float* part, int ksplit, int N, int64_t V, int Cout, const float* bias, int act,
                                  const float* ref, int64_t ref_ld, float* y, int64_t y_ld, const TemDgradSumsReq& rq,
                                  hipStream_t s);
int64_t tem_splitk_stat_blocks(int64_t V, int Cout);
void tem_splitk_epilogue_stats(int sty, const float* part, int ksplit, int N, int64_t V, int Cout, const float* bias, int act,
                               const float* ref, int64_t ref_ld, float* y, int64_t y_ld, float* stat, hipStream_t s);
int64_t tem_conv_wgrad_bf16x3_ws(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
int tem_conv_wgrad_bf16x3(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                          int64_t g_ld, float* dw, float* db, void* ws, int64_t ws_bytes, int N, int D, int H, int W,
                          int Cin, int Cout, int kd, int kh, int kw, int sd_layout, int wg_kind /* TemWgradKind */, const float* w_sd,
                          const float* gamma, const float* beta, float* norm_sums, hipStream_t s);
// largest |g| as a by-product of the z-sliding weight gradient (tem_conv3d_wgrad_gmax: TemConvCall::g_amax_out)
int tem_conv_wgrad_gmax_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
// wg_kind TEM_WG_F16X2 of tem_conv_wgrad_bf16x3 ("fp16 2x1": x^ two fp16 terms, g one fp16 term prescaled from TemConvCall::g_amax_in)
int tem_conv_wgrad_gscaled_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
int tem_conv_wgrad_cs_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int st, int64_t x_cs);
int tem_conv_wgrad_tr_fp32_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);   // TEM_WG_FP32
// conv_wgrad_tr.hip: z-sliding weight gradient with a staging team and transposing LDS reads (option wgrad_zs = 3)
void tem_conv_wgrad_tr_launch(const TemConvCall& c, int wg_kind, unsigned nblk, const float* x, int64_t x_ld, const float* scale, const float* shift,
                              const float* g, int64_t g_ld, float* zpart, float* zdb, int N, int D, int H, int W, int Cin,
                              int Cout, int T, int nY, int nX, int zsegs, int Ss, int ncz, hipStream_t s);
// TEM_BP_NORM_COEF of a call, as tem_wgrad_sums_launch reads it (delivered when the layer's group layout allows it)
struct TemWgradCoefReq {
    int G;
    const float* mean;
    const float* rstd;
    float* coef;
};
// wgrad_sums.hip: norm-backward sums from the weight gradient
int tem_conv_wgrad_sums_ok(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int64_t x_cs);   // x_cs: the call's chunk stride of x
int64_t tem_wgrad_sums_ws_floats(int N, int D, int H, int Cin, int Cout);
void tem_wgrad_sums_launch(const TemConvCall& c, const float* zpart, int Ss, int ks2, const float* zdb, const float* g, int64_t g_ld,
                           const float* w, const float* gamma, const float* beta, float* dw, float* extra, int N, int D,
                           int H, int W, int Cin, int Cout, float* sums, int db_chunks, float* db, hipStream_t s);
