// conv_internal.h -- C++-internal interface between conv.hip (entry points, VALU kernels)
// and the kernel files (conv_mfma.hip, conv_bf16x3.hip, conv_zr.hip, conv_pp.hip, conv_wgrad_tr.hip, conv_small.hip, ...).
// Both dispatches are built the same way: ONE plan function in conv.hip (fwd_plan, wgrad_plan) decides which kernel a call takes,
// with which geometry and workspace regions; the kernel files export geometry helpers the plan calls and launchers that execute it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <set>
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

// The template arguments of the instantiation a planned launch runs, as tem_conv3d_fwd_mfma_path() reports them (tem_hip.h:
// TEM_MI_*).  Every family's *_describe() below fills them through the SAME host selector its launcher instantiates from.
struct TemFwdInst {
    int v[TEM_MFMA_INST_N];
    int& operator[](int i) { return v[i]; }
};
// the summing kernel behind a launch with split input channels (TEM_MI_EPILOGUE)
enum TemSplitkEpilogue { TEM_SKE_NONE = 0, TEM_SKE_PLAIN = 1, TEM_SKE_STATS = 2, TEM_SKE_BWD_SUMS = 3 };

// conv_mfma.hip: the exact-fp32 patch kernel with ks slices of the input channels (> 1: partial sums in ws).  Raises on x /
// weights / scale it cannot load as 16-byte vectors
int tem_conv_fwd_mfma(const TemPatchTiling& t, int ks, const float* x, int64_t x_ld, const float* scale, const float* shift,
                      const float* w_packed, const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, void* ws,
                      const TemConvShape& sh, int act, hipStream_t s);
// ... does that launch run the persistent variant (k_conv_fwd_mfma_p)?  Option fwd_persistent, the tile width, 32-bit halo offsets
bool tem_fwd_mfma_persistent(const TemPatchTiling& t, const TemConvShape& sh, int64_t x_ld);
void tem_fwd_mfma_describe(const TemPatchTiling& t, int ks, const TemConvShape& sh, int64_t x_ld, TemFwdInst& inst);

// conv_small.hip: the HBM-bound special cases of the VALU family (use_mfma 0).  As everywhere in this file: shape predicates
// that the ONE selector (conv.hip: fwd_valu_select) calls, and launchers that execute what it selected and decide nothing.
// The paths, as tem_conv3d_fwd_valu_path() reports them (tem_hip.h: TEM_VALU_*)
enum TemValuPath {
    TEM_VP_REFUSED = -1, TEM_VP_C1ROWS = 0, TEM_VP_CIN1, TEM_VP_COUT1, TEM_VP_PROJ_R, TEM_VP_PROJ, TEM_VP_EXPAND, TEM_VP_SMALLCOUT,
    TEM_VP_GENERIC
};
int tem_conv_fwd_cin1_takes(const TemConvShape& sh);      // 0: neither, 1: k_conv_fwd_cin1, 2: k_conv_fwd_c1rows
void tem_conv_fwd_cin1(const TemConvCall& c, bool rows, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* w,
                       const float* bias, float* y, int64_t y_ld, int N, int D, int H, int W,
                       int Cin, int Cout, int kd, int kh, int kw, int act, float* stat, hipStream_t s);
int64_t tem_conv_fwd_cin1_stat_blocks(int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
bool tem_conv_fwd_cout1_takes(const TemConvShape& sh);
void tem_conv_fwd_cout1(const TemConvCall& c, const float* x, int64_t x_ld, const float* w,
                        const float* bias, float* y, int64_t y_ld, int N, int D, int H, int W,
                        int Cin, int kd, int kh, int kw, int act, hipStream_t s);
int tem_conv1x1_proj_nj(int Cin, int Cout);               // NJ of k_conv1x1_proj_r, 0: k_conv1x1_proj, -1: none
void tem_conv1x1_proj(const TemConvCall& c, int nj, const float* x, int64_t x_ld, const float* w, const float* bias, float* y,
                      int64_t y_ld, int64_t NV, int Cin, int Cout, int act, hipStream_t s);
bool tem_conv1x1_expand_takes(int Cin, int Cout);
void tem_conv1x1_expand(const TemConvCall& c, const float* x, int64_t x_ld, const float* w, const float* bias, float* y,
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
void tem_conv_fwd_bf16x3_describe(const TemConvCall& c, const TemPatchTiling& t, int ks, const TemConvShape& sh, int mode, TemFwdInst& inst);
// conv_pp.hip: ping-pong team kernel for the levels with many patches; stat: [N][nZ * nY * nX * WM][Cout][2]
PpGeom tem_pp_geometry(const TemConvCall& c, const TemConvShape& sh, int mode);
void tem_conv_fwd_pp(const PpGeom& g, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* wp,
                     const float* bias, float* y, int64_t y_ld, const float* ref, int64_t ref_ld, const TemConvShape& sh, int act,
                     int mode, float* stat, hipStream_t s);
void tem_conv_fwd_pp_describe(const PpGeom& g, const TemConvShape& sh, int mode, TemFwdInst& inst);
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
// the instantiation of k_conv_zr of the direct launch (ks 0) or the split-K launch with ks slices, and the latter's epilogue;
// ref / stat: the launch carries them
void tem_conv_fwd_zr_describe(const TemConvCall& c, const ZrGeom& g, int ks, const TemConvShape& sh, int mode, bool ref, bool stat,
                              TemFwdInst& inst);
// conv1x1_stream.hip: 1x1x1 convolution / data gradient as a streaming GEMM: no pre-norm, no statistics, no sigmoid
void tem_conv1x1_stream(const TemConvCall& c, const float* x, int64_t x_ld, const float* wp, const float* bias, float* y, int64_t y_ld,
                        const float* ref, int64_t ref_ld, const TemConvShape& sh, int act, int mode, hipStream_t s);
void tem_conv1x1_stream_describe(const TemConvCall& c, const TemConvShape& sh, int mode, TemFwdInst& inst);
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

// ---- the weight-gradient dispatch: geometry helpers and shape predicates of the kernel files, plain functions of the shape that
// the ONE plan function (conv.hip: wgrad_plan) calls, and the launchers that execute what it planned.  As in the forward, a
// launcher decides and re-checks nothing: its caller holds a plan that names it, with the geometry and the workspace regions.
// z-sliding kernels (conv_bf16x3.hip: k_conv_wgrad_zs<1|2>, k_conv_wgrad_zt; conv_wgrad_tr.hip: k_conv_wgrad_tr), 3x3x3 only.
// Cin % 32 == 0 and Cout % 32 == 0 (this and the two patch plans divide by Cin / 32)
struct ZsPlan {
    bool use;     // option wgrad_zs, 3x3x3, D >= TEM_ZS_MIN_D
    bool teams;   // k_conv_wgrad_zt (staging team) instead of k_conv_wgrad_zs
    bool tr;      // k_conv_wgrad_tr (staging team + transposing LDS reads); same geometry as `teams`
    int nco, ks2, T, nY, nX, zsegs, S, Ss, ncz;
    int64_t part_floats(const TemConvShape& sh) const { return tem_align_up((int64_t)S * ks2 * 27 * sh.Cin * sh.Cout, 64); }   // slabs
    int64_t db_floats(const TemConvShape& sh) const { return tem_align_up((int64_t)S * sh.Cout, 64); }   // bias partials behind them
};
ZsPlan tem_zs_plan(const TemConvShape& sh);
// split-precision patch kernel (conv_bf16x3.hip: k_conv_wgrad_bf16x3), 3x3x3 / 1x3x3 / 1x1x1
struct WbPlan {
    int nco, ks2, T, S, P, nZ, nY, nX, ptz;
};
WbPlan tem_wb_plan(const TemConvShape& sh);
// exact-fp32 patch kernel (conv_mfma.hip: k_conv_wgrad_mfma), the same kernel sizes
struct WgradFp32Plan {
    int nco, T, S, P, nZ, nY, nX;
};
WgradFp32Plan tem_wgrad_fp32_plan(const TemConvShape& sh);
// conv_small.hip: the shapes its kernels take, and the bytes of their partial slabs
bool tem_conv_wgrad_cin1_takes(const TemConvShape& sh);   // small-Cin first layer, 3x3x3 / 1x3x3
int64_t tem_conv_wgrad_cin1_ws(int Cout, int ntaps);
bool tem_conv1x1_proj_wgrad_takes(int Cin, int Cout);     // 1x1x1 projection to a few channels
int64_t tem_conv1x1_proj_wgrad_ws(int Cin, int Cout);
bool tem_conv1x1_out_bwd_takes(int Cin, int Cout);        // ... fused with its masked data gradient (same slabs)
// wgrad_sums.hip: the z-sliding layers whose slab merge can also deliver the norm-backward sums (option wgrad_sums), and the
// floats of its region behind the bias partials
bool tem_wgrad_sums_takes(const TemConvShape& sh);
int64_t tem_wgrad_sums_ws_floats(int N, int D, int H, int Cin, int Cout);

// raise a kernel's dynamic-LDS limit to `bytes`, once per kernel
template <typename K>
inline void tem_raise_dynamic_lds(K kern, size_t bytes) {
    static std::set<const void*> sized;
    const void* key = reinterpret_cast<const void*>(kern);
    if (sized.insert(key).second) (void)hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// The launchers.  part / dbpart (null: no bias gradient) / extra: the plan's workspace regions; each enqueues its kernel and the
// merge of the partial slabs into dw / db.
// z-sliding.  wg_kind: TemWgradKind (TEM_WG_F16X2 reads c.g_amax_in; c.g_amax_out, c.x_cs as the plan admitted them).
// norm_sums (optional): the merge also delivers the norm-backward sums from w_sd / gamma / beta, through `extra`
void tem_conv_wgrad_zs(const TemConvCall& c, const ZsPlan& z, int wg_kind, const float* x, int64_t x_ld, const float* scale,
                       const float* shift, const float* g, int64_t g_ld, float* dw, float* db, float* part, float* dbpart, float* extra,
                       const TemConvShape& sh, int sd_layout, const float* w_sd, const float* gamma, const float* beta, float* norm_sums,
                       hipStream_t s);
void tem_conv_wgrad_patch(const TemConvCall& c, const WbPlan& p, const float* x, int64_t x_ld, const float* scale, const float* shift,
                          const float* g, int64_t g_ld, float* dw, float* db, float* part, float* dbpart, const TemConvShape& sh,
                          int sd_layout, hipStream_t s);
void tem_conv_wgrad_mfma(const WgradFp32Plan& p, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                         int64_t g_ld, float* dw, float* db, float* part, float* dbpart, const TemConvShape& sh, int sd_layout,
                         hipStream_t s);
// conv_wgrad_tr.hip: the main kernel of tem_conv_wgrad_zs for z.tr
void tem_conv_wgrad_tr_launch(const TemConvCall& c, int wg_kind, const ZsPlan& z, const float* x, int64_t x_ld, const float* scale,
                              const float* shift, const float* g, int64_t g_ld, float* zpart, float* zdb, const TemConvShape& sh,
                              hipStream_t s);
// gnx / gcoef (optional): the norm backward and ReLU mask applied to g while it is loaded (tem_conv3d_wgrad_gnorm)
void tem_conv_wgrad_cin1(const TemConvCall& c, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* g,
                         int64_t g_ld, float* dw, float* db, float* part, const TemConvShape& sh, int sd_layout, const float* gnx,
                         int64_t gnx_ld, const float* gcoef, hipStream_t s);
void tem_conv1x1_proj_wgrad(const TemConvCall& c, const float* x, int64_t x_ld, const float* g, int64_t g_ld, float* dw, float* db,
                            float* part, int64_t NV, int Cin, int Cout, int sd_layout, hipStream_t s);
void tem_conv1x1_out_bwd(const TemConvCall& c, const float* x, int64_t x_ld, const float* g, int64_t g_ld, const float* w, float* gx,
                         int64_t gx_ld, float* dw, float* db, float* part, int64_t NV, int Cin, int Cout, int sd_layout, hipStream_t s);
// TEM_BP_NORM_COEF of a call, as tem_wgrad_sums_launch reads it (delivered when the layer's group layout allows it)
struct TemWgradCoefReq {
    int G;
    const float* mean;
    const float* rstd;
    float* coef;
};
// wgrad_sums.hip: the z-sliding slab merge that also delivers the norm-backward sums
void tem_wgrad_sums_launch(const TemConvCall& c, const float* zpart, int Ss, int ks2, const float* zdb, const float* g, int64_t g_ld,
                           const float* w, const float* gamma, const float* beta, float* dw, float* extra, int N, int D,
                           int H, int W, int Cin, int Cout, float* sums, int db_chunks, float* db, hipStream_t s);
