// pn2_wave.h -- the wave64 primitives of the gfx950 kernels, once: lane id, wave-wide reductions, the FPS tie key.  pn2_common.h
// includes it.  The two families of reductions are NOT interchangeable: each comment says where the result lands, whether all 64
// lanes must be active (full EXEC), and what a lane with nothing to contribute holds.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int pn2_lane_id() {
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// ---- butterfly family: cross-lane shuffles, result in every lane ----
// v = op(v, the partner lane's v) over the xor tree 32, 16, .. 1 -- this order everywhere: with fmin / fmax it decides the sign
// of a zero result (pn2_wg.h), and the tests' exact models pin it.  Result: every lane.  Full EXEC: a switched-off partner hands
// a lane an undefined value, so call from uniform control flow.  A lane with nothing to contribute holds op's identity.
template <typename T, class Op>
__device__ __forceinline__ T pn2_wave_all(T v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}

// The combines in use: op(v, t), v = the lane's own value, t = its partner's.  Fmin / Fmax are fminf / fmaxf (fmin / fmax on
// double): they skip a NaN and do not order -0.0 against +0.0.  Min / Max are compare-and-select: a NaN partner never replaces v.
struct Pn2OpAdd { template <typename T> __device__ __forceinline__ T operator()(T v, T t) const { return v + t; } };
struct Pn2OpFmin {
    __device__ __forceinline__ float operator()(float v, float t) const { return fminf(v, t); }
    __device__ __forceinline__ double operator()(double v, double t) const { return fmin(v, t); }
};
struct Pn2OpFmax {
    __device__ __forceinline__ float operator()(float v, float t) const { return fmaxf(v, t); }
    __device__ __forceinline__ double operator()(double v, double t) const { return fmax(v, t); }
};
struct Pn2OpMin { template <typename T> __device__ __forceinline__ T operator()(T v, T t) const { return t < v ? t : v; } };
struct Pn2OpMax { template <typename T> __device__ __forceinline__ T operator()(T v, T t) const { return t > v ? t : v; } };

// sum / compare-select minimum / maximum (contract of pn2_wave_all)
template <typename T> __device__ __forceinline__ T pn2_wave_all_sum(T v) { return pn2_wave_all(v, Pn2OpAdd()); }
template <typename T> __device__ __forceinline__ T pn2_wave_all_min(T v) { return pn2_wave_all(v, Pn2OpMin()); }
template <typename T> __device__ __forceinline__ T pn2_wave_all_max(T v) { return pn2_wave_all(v, Pn2OpMax()); }

// Per-axis fmin of lo[3] and fmax of hi[3] (float or double): a wave's bounding box in every lane (contract of pn2_wave_all).
// Both values of an axis move in ONE step: two calls of pn2_wave_all give the same values and cost voxel_minmax_kernel a register.
template <typename T>
__device__ __forceinline__ void pn2_wave_all_box(T (&lo)[3], T (&hi)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = Pn2OpFmin()(lo[a], __shfl_xor(lo[a], o));
            hi[a] = Pn2OpFmax()(hi[a], __shfl_xor(hi[a], o));
        }
}

// ---- DPP family: one VALU per step, wave-uniform result in an SGPR; silently wrong unless all 64 lanes are active ----
// row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143 (gfx9 DPP).
// old == src and bound_ctrl=false: lanes without a valid source keep their value.
#define PN2_DPP_U32(v, ctrl, rmask) \
    ((unsigned)__builtin_amdgcn_update_dpp((int)(v), (int)(v), (ctrl), (rmask), 0xF, false))

// Unsigned maximum / minimum of the wave.  Result: an SGPR (lane 63).  Full EXEC required.
// A lane with nothing to contribute holds 0 (umax) or 0xFFFFFFFF (umin).
__device__ __forceinline__ unsigned pn2_wave_umax(unsigned v) {
    unsigned t;
    t = PN2_DPP_U32(v, 0x111, 0xF); v = v > t ? v : t;
    t = PN2_DPP_U32(v, 0x112, 0xF); v = v > t ? v : t;
    t = PN2_DPP_U32(v, 0x114, 0xF); v = v > t ? v : t;
    t = PN2_DPP_U32(v, 0x118, 0xF); v = v > t ? v : t;
    t = PN2_DPP_U32(v, 0x142, 0xA); v = v > t ? v : t;
    t = PN2_DPP_U32(v, 0x143, 0xC); v = v > t ? v : t;
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned pn2_wave_umin(unsigned v) { return ~pn2_wave_umax(~v); }

// Maximum of a 64-bit key over the 16 lanes of row 0.  Result: an SGPR pair (lane 15).  Lanes 0..15 must be active; lanes
// 16..63 are ignored.  A row-0 lane with nothing to contribute holds 0.
#define PN2_U64MAX_STEP(v, ctrl)                                        \
    do {                                                                \
        unsigned lo__ = (unsigned)(v), hi__ = (unsigned)((v) >> 32);    \
        unsigned tlo__ = PN2_DPP_U32(lo__, (ctrl), 0xF);                \
        unsigned thi__ = PN2_DPP_U32(hi__, (ctrl), 0xF);                \
        unsigned long long t__ = ((unsigned long long)thi__ << 32) | tlo__; \
        (v) = t__ > (v) ? t__ : (v);                                    \
    } while (0)

__device__ __forceinline__ unsigned long long pn2_row0_u64max(unsigned long long v) {
    PN2_U64MAX_STEP(v, 0x111);
    PN2_U64MAX_STEP(v, 0x112);
    PN2_U64MAX_STEP(v, 0x114);
    PN2_U64MAX_STEP(v, 0x118);
    unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 15);
    unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 15);
    return ((unsigned long long)hi << 32) | lo;
}

// The fused forms: one v_max / v_min with a DPP operand per step, written as asm; `s_nop 1` = the 2 wait states a DPP read
// needs after a VALU write of the same VGPR.  The FPS round loops are built on these, instruction for instruction.
//
// Signed maximum of the wave, IN PLACE (v is overwritten).  Result: an SGPR (lane 63).  Full EXEC required.  A lane with nothing
// to contribute holds a negative value (the keys are bits of distances >= +0, which order like ints; -1.0f is negative).
__device__ __forceinline__ int pn2_wave_imax(int v) {
    asm volatile(
        "s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n s_nop 1\n"
        : "+v"(v));
    return __builtin_amdgcn_readlane(v, 63);
}
// The same leaving `src` intact (for a value that lives on, like the candidates' td of pick_phase: in place it would cost a copy
// per call).  Result, EXEC and sentinel as pn2_wave_imax.
__device__ __forceinline__ int pn2_wave_imax_from(int src) {
    int v;
    asm volatile(
        "s_nop 1\n"
        "v_max_i32_dpp %0, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n"
        : "=&v"(v) : "v"(src));
    return __builtin_amdgcn_readlane(v, 63);
}
// Unsigned maximum of the wave, `src` left intact.  Result: an SGPR (lane 63).  Full EXEC required.  A lane with nothing to
// contribute holds 0.  The FPS tie paths use it, so clouds with many duplicated rows (every pick of a row that has a twin is a
// tie) pay 6 VALU instead of 6 cross-lane shuffles per tied pick.
__device__ __forceinline__ unsigned pn2_wave_umax_dpp(unsigned src) {
    unsigned v;
    asm volatile(
        "s_nop 1\n"
        "v_max_u32_dpp %0, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n s_nop 1\n"
        "v_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n"
        : "=&v"(v) : "v"(src));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// Signed maximum of each 16-lane row.  Result: a VGPR, valid in lane 15 of every row (lanes 15, 31, 47, 63).  The row's 16 lanes
// must be active.  A lane with nothing to contribute holds a negative value.
__device__ __forceinline__ int pn2_row_imax(int v) {
    asm volatile(
        "s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        : "+v"(v));
    return v;
}
// Signed maximum / unsigned minimum over lanes 0..15 (row 0).  Result: an SGPR (lane 15).  Lanes 0..15 must be active; lanes
// 16..63 are ignored.  A row-0 lane with nothing to contribute holds a negative value (imax) or 0xFFFFFFFF (umin).
__device__ __forceinline__ int pn2_row0_imax(int v) { return __builtin_amdgcn_readlane(pn2_row_imax(v), 15); }
__device__ __forceinline__ unsigned pn2_row0_umin(unsigned v) {
    asm volatile(
        "s_nop 1\n"
        "v_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        "v_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
        : "+v"(v));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 15);
}

// ---- the FPS tie key ----
// Tie-break of the reference (tf_sampling.cu:153-170: 512-thread strided scan with a strict '>', left-biased tree):
// among equal distances the lowest (k mod 512, k) wins.  Every point carries ~pn2_fps_tiekey(k) in the low word of its 64-bit
// key (td bits : ~tiekey), so a plain 64-bit max reproduces the reference's order.
__device__ __forceinline__ unsigned pn2_fps_tiekey(int k) { return (((unsigned)k & 511u) << 22) | ((unsigned)k >> 9); }
__device__ __forceinline__ int pn2_fps_untiekey(unsigned key) { return (int)(((key & 0x3FFFFFu) << 9) | (key >> 22)); }
