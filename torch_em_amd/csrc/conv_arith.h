// conv_arith.h -- what an arithmetic mode of the convolutions (TEM_ARITH_*, the low byte of `use_mfma`: tem_hip.h) means to
// the packers, the launchers and the dispatch queries, stated ONCE.  Nothing else under csrc/ compares a mode with a number.
#pragma once
#include <type_traits>
#include "tem_common.h"
#include "conv_internal.h"

// how tem_conv_pack_weights* writes the planes of a weight (the `kind` word of the 56-byte pack descriptor: ABI values)
enum TemPackKind : int {
    TEM_PK_BF16 = 0,      // bf16 terms
    TEM_PK_F16 = 1,       // fp16 terms
    TEM_PK_F16_LO12 = 2,  // fp16 terms, the lo plane stored x 2^12 (conv_split.h: F16_LO_SCALE)
    TEM_PK_F16_PRE = 3,   // fp16 terms of the weight x 2^7 (conv_split.h: F16_W_PRESCALE)
    TEM_PK_FP32 = 4,      // the fp32 values themselves, two 64-lane groups per 16-channel chunk (tile kernel only)
};
enum TemElem : int { TEM_EL_F32, TEM_EL_F16, TEM_EL_BF16 };   // element type of the MFMA operands
// the arithmetic of the z-sliding weight-gradient kernels (k_conv_wgrad_zs / _zt / _tr<KIND>: template argument values)
enum TemWgradKind : int {
    TEM_WG_BF16X3 = 0,   // hi + lo planes, 3 MFMAs per product
    TEM_WG_F16 = 1,      // one fp16 term
    TEM_WG_BF16 = 2,     // one bf16 term
    TEM_WG_F16X2 = 3,    // fp16 2x1: x^ two fp16 terms, g one fp16 term prescaled from TemConvCall::g_amax_in
    TEM_WG_FP32 = 4,     // exact fp32 on k_conv_wgrad_tr where the plan (conv.hip: wgrad_plan) admits it, else on tem_conv_wgrad_mfma
    TEM_WG_NONE = -1,    // VALU kernels
};
constexpr int TEM_ST_NONE = -1;

struct TemArith {
    int planes;          // 16-bit planes per packed weight (TEM_PK_FP32: 64-lane groups); 0: the generic fp32 layout
    TemPackKind pack;
    TemElem elem;
    int st16;            // the 16-bit storage type (TEM_ST_*) whose stored values ARE the operands of this mode, or TEM_ST_NONE
    TemWgradKind wgrad;  // modes without a weight-gradient arithmetic of their own (bf16x6, fp16x3, fp16x3 prescaled) run exact fp32
    bool zr, pp, stream1x1;   // the forward kernel families with an instantiation for the mode (k_conv_zr also takes exact fp32
                              // under option fp32_zr: tem_zr_takes); every MFMA forward mode has the patch kernel
};
constexpr int TEM_ARITH_COUNT = 9;
constexpr TemArith TEM_ARITH_TABLE[TEM_ARITH_COUNT] = {
    /* VALU   */ {0, TEM_PK_BF16, TEM_EL_F32, TEM_ST_NONE, TEM_WG_NONE, false, false, false},
    /* FP32   */ {2, TEM_PK_FP32, TEM_EL_F32, TEM_ST_NONE, TEM_WG_FP32, false, false, false},
    /* BF16X3 */ {2, TEM_PK_BF16, TEM_EL_BF16, TEM_ST_NONE, TEM_WG_BF16X3, true, true, true},
    /* BF16X6 */ {3, TEM_PK_BF16, TEM_EL_BF16, TEM_ST_NONE, TEM_WG_FP32, false, false, true},
    /* F16X3  */ {2, TEM_PK_F16_LO12, TEM_EL_F16, TEM_ST_NONE, TEM_WG_FP32, true, true, false},
    /* F16    */ {1, TEM_PK_F16, TEM_EL_F16, TEM_ST_F16, TEM_WG_F16, true, true, true},
    /* F16X3S */ {2, TEM_PK_F16_PRE, TEM_EL_F16, TEM_ST_NONE, TEM_WG_FP32, false, false, false},
    /* BF16   */ {1, TEM_PK_BF16, TEM_EL_BF16, TEM_ST_BF16, TEM_WG_BF16, true, true, true},
    /* F16X2  */ {0, TEM_PK_F16, TEM_EL_F16, TEM_ST_NONE, TEM_WG_F16X2, false, false, false},   // weight gradient only: no pack, no forward
};
static_assert(TEM_ARITH_VALU == 0 && TEM_ARITH_FP32 == 1 && TEM_ARITH_BF16X3 == 2 && TEM_ARITH_BF16X6 == 3 && TEM_ARITH_F16X3 == 4 &&
                  TEM_ARITH_F16 == 5 && TEM_ARITH_F16X3S == 6 && TEM_ARITH_BF16 == 7 && TEM_ARITH_F16X2 == 8,
              "TEM_ARITH_TABLE is indexed by the mode");

constexpr bool tem_arith_known(int mode) { return mode >= 0 && mode < TEM_ARITH_COUNT; }
// an unknown mode reads the VALU row: no MFMA family takes it
constexpr const TemArith& tem_arith(int mode) { return TEM_ARITH_TABLE[tem_arith_known(mode) ? mode : TEM_ARITH_VALU]; }
// forward / data gradient on the matrix cores: every mode with a fragment pack
constexpr bool tem_arith_mfma_fwd(int mode) { return tem_arith(mode).planes != 0; }
// ... with 16-bit operands (tem_conv_fwd_bf16x3 and the kernels behind it)
constexpr bool tem_arith_split_fwd(int mode) { return tem_arith_mfma_fwd(mode) && tem_arith(mode).elem != TEM_EL_F32; }
// the one-term mixed-precision modes, whose tensors may be stored in the operand type
constexpr bool tem_arith_one_term(int mode) { return tem_arith(mode).st16 != TEM_ST_NONE; }
// weight gradient on the split-precision launchers (tem_conv_wgrad_zs / _patch) in the mode's own arithmetic
constexpr bool tem_arith_split_wgrad(int mode) { return tem_arith(mode).wgrad >= TEM_WG_BF16X3 && tem_arith(mode).wgrad <= TEM_WG_F16X2; }
// (layout -> mode is the identity: tem_hip.h defines TEM_WL_* as the modes)
constexpr bool tem_layout_is_split(int layout) { return tem_arith_split_fwd(layout); }

// tensors of storage type `st` (TEM_ST_*) go with the mode: fp32 always, a 16-bit type with the one-term mode of that type
constexpr bool tem_storage_ok(int mode, int st) { return st == TEM_ST_F32 || tem_arith(mode).st16 == st; }
constexpr bool tem_wgrad_storage_ok(TemWgradKind kind, int st) {
    return st == TEM_ST_F32 || (st == TEM_ST_F16 && kind == TEM_WG_F16) || (st == TEM_ST_BF16 && kind == TEM_WG_BF16);
}

// Which forward kernel family has an instantiation for this call's mode.  One definition each: the dispatch query and the
// launch both ask here (the shape conditions stay with the family's *_geometry()).
inline bool tem_zr_takes(int mode, const TemConvCall& c) {
    return tem_arith(mode).zr || (mode == TEM_ARITH_FP32 && tem_option(TEM_OPT_FP32_ZR) && c.stx == TEM_ST_F32);
}
// ... and, on 16-bit tensors, stages whole 64-byte records per phase: a one-term mode, 32-channel chunks
inline bool tem_zr_takes(int mode, const TemConvCall& c, int Cin) {
    return tem_zr_takes(mode, c) && (c.stx == TEM_ST_F32 || (Cin % 32 == 0 && tem_arith_one_term(mode)));
}
inline bool tem_pp_takes(int mode, const TemConvCall& c) {   // fp32 tensors only: the z-reuse / patch kernels carry the element type
    return tem_arith(mode).pp && c.stx == TEM_ST_F32 && c.sty == TEM_ST_F32;
}
constexpr bool tem_stream1x1_takes(int mode) { return tem_arith(mode).stream1x1; }

// Compile-time value of a runtime choice, for the variant selectors of the launchers: `sel(cond, [&](auto b) { f<b()>(...); })`
template <int V> using TemInt = std::integral_constant<int, V>;
template <bool V> using TemBool = std::integral_constant<bool, V>;
template <typename F> inline void tem_select_bool(bool v, F&& f) {
    if (v) f(TemBool<true>{});
    else f(TemBool<false>{});
}
