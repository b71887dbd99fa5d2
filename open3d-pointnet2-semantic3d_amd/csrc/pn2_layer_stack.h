// pn2_layer_stack.h -- the one reader of a fused MLP's layer tables (nlayers, widths[], w[], bias[]) for the host launchers of
// pn2_sa_fused.hip, pn2_sa_fused_bf16.hip and pn2_mlp_wide.hip.  Host code only: nothing here reaches a kernel.
//
// What a refused stack returns, in this order (the first fault wins; include/pn2_abi.h promises the codes):
//   1. nlayers < 1 or > rule.max_layers                 PN2_EUNSUP
//   2. widths, w or bias (the tables) NULL              PN2_ENULL
//   then per layer l = 0 .. nlayers-1, every check of layer l ahead of any check of layer l+1:
//   3. widths[l] off the width rule                     PN2_EUNSUP
//   4. w[l] or bias[l] NULL                             PN2_ENULL   (w[0] is exempt under rule.w0_may_be_null)
//   5. w[l] (and bias[l], under kPn2AlignWeightsAndBias) not 16-byte aligned   PN2_EUNSUP
// The entry points of the register-resident chains refuse nlayers <= 0 as PN2_EINVAL and the NULL tables as PN2_ENULL in their
// own leading argument checks, ahead of their shape and range checks; 1 and 2 then never fire for them and only keep the
// reader safe on its own.  Nothing is launched, queued or written before the reader has returned PN2_OK.
#pragma once
#include "pn2_common.h"

enum Pn2WidthRule {
    kPn2WidthsChain,  // a multiple of 32, at most 128: the chains whose weights stay resident in LDS
    kPn2WidthsWide,   // 128, 256 or 512: mlp_wide_kernel's column blocks of 128
};
enum Pn2AlignRule {
    kPn2AlignNone,              // weights staged with 4-byte loads (bf16 chain)
    kPn2AlignWeights,           // 16-byte weight staging, biases read float by float (fp32 chains)
    kPn2AlignWeightsAndBias,    // both read 16 bytes at a time (wide kernel)
};
struct Pn2LayerRule {
    int max_layers;       // <= 3
    Pn2WidthRule widths;
    Pn2AlignRule align;
    bool w0_may_be_null;  // the hoisted FP chain with c1 == 0 has no first-layer rows left: W[0] = bias[0], never read
};

// Fills p.w[], p.W[], p.bias[] of a kernel params struct and, when nt is given, nt[l] = widths[l] / 32 (0 past nlayers).
template <class Params>
inline int pn2_read_layers(Params& p, const Pn2LayerRule& rule, int nlayers, const int* widths, const float* const* w,
                           const float* const* bias, int* nt = nullptr) {
    if (nt) nt[0] = nt[1] = nt[2] = 0;
    if (nlayers < 1 || nlayers > rule.max_layers) return PN2_EUNSUP;
    if (!widths || !w || !bias) return PN2_ENULL;
    for (int l = 0; l < nlayers; ++l) {
        const int n = widths[l];
        const bool width_ok = rule.widths == kPn2WidthsWide ? (n == 128 || n == 256 || n == 512) : (n > 0 && n % 32 == 0 && n <= 128);
        if (!width_ok) return PN2_EUNSUP;
        const bool no_w = !w[l];
        if (!bias[l] || (no_w && !(l == 0 && rule.w0_may_be_null))) return PN2_ENULL;
        uintptr_t bits = rule.align == kPn2AlignNone ? 0 : (uintptr_t)w[l];
        if (rule.align == kPn2AlignWeightsAndBias) bits |= (uintptr_t)bias[l];
        if (bits & 15) return PN2_EUNSUP;
        p.w[l] = n; p.W[l] = no_w ? bias[l] : w[l]; p.bias[l] = bias[l];
        if (nt) nt[l] = n / 32;
    }
    return PN2_OK;
}
