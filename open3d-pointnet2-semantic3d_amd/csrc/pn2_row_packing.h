// pn2_row_packing.h -- the row packer of the pooled K = 32 kernels (sa_fused_kernel's PACK, linear_pool_packed_kernel): one
// classifier, one tile decoder and one pooled epilogue, so that every packed kernel forms the same tiles from the same index rows.
//
// The ball query pads a short row with copies of its first hit.  A padded row's activation is a copy of row 0's, and a maximum
// does not count copies, so only the LIVE prefix of a centre's 32 rows needs the matrix pipe: live = 1 + the last position of
// the index row that differs from position 0 (NOT the number of distinct values: equal entries need not be contiguous).  A
// centre's class is the smallest s in {8, 16, 32} with live <= s.  A workgroup classifies a block of <= 64 consecutive centres
// and packs four class-8 or two class-16 centres into one 32-row tile; tiles are ordered class 32, then 16, then 8, and the last
// tile of a class may be short.  The host model of the same arithmetic: tools/sa_row_packing_stats.py::packed_tiles.
#pragma once

#include "pn2_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPn2PackBlockMax = 64;  // centres per block: one ballot
constexpr size_t kPn2PackLdsBytes = (kPn2PackBlockMax + kPn2PackBlockMax * 4) * sizeof(int);  // classes + tile list of one block

// the tiles of one classified block (wave-uniform)
struct Pn2PackBlock {
    int n32, t16, n16, n8;  // class-32 tiles; class-16 tiles and the centres in them; centres in class-8 tiles
    __device__ __forceinline__ int tiles() const { return n32 + t16 + ((n8 + 3) >> 2); }
};

// Classify the `cnt` (<= 64) centres [base, base + cnt) of idx (groups, 32) and write the block's tile list: s_desc[tile * 4 +
// slot] = centre.  Called by all NW waves of the workgroup (two barriers inside; the caller keeps the previous block's readers
// of s_desc behind a barrier of its own).  s_cls: 64 ints, s_desc: 64 x 4 ints of LDS.
template <int NW>
__device__ __forceinline__ Pn2PackBlock pn2_pack_classify(const int* __restrict__ idx, int base, int cnt, int wave, int lane,
                                                          int* s_cls, int* s_desc) {
    const int half = lane >> 5, l31 = lane & 31;
    // a half-wave reads one centre's 32 indices (128 bytes)
    for (int c0 = 2 * wave; c0 < cnt; c0 += 2 * NW) {
        const int cl = c0 + half;
        const int v = idx[(size_t)(base + (cl < cnt ? cl : c0)) * 32 + l31];
        const int first = __shfl(v, lane & 32);
        const unsigned long long diff = __ballot(v != first);
        const unsigned mine = (unsigned)(diff >> (lane & 32));
        const int live = 32 - __clz(mine | 1u);  // highest differing position + 1 (>= 1)
        if (l31 == 0 && cl < cnt) s_cls[cl] = live <= 8 ? 8 : (live <= 16 ? 16 : 32);
    }
    __syncthreads();
    const int cls = lane < cnt ? s_cls[lane] : 0;
    const unsigned long long m32 = __ballot(cls == 32), m16 = __ballot(cls == 16), m8 = __ballot(cls == 8);
    const int n16 = __popcll(m16), n8 = __popcll(m8);
    // an odd class-16 centre shares its tile with the last class-8 centre when that saves the class-8 tile it would open
    const int promote = ((n16 & 1) && (n8 & 3) == 1) ? 1 : 0;
    Pn2PackBlock b;
    b.n32 = __popcll(m32); b.n16 = n16 + promote; b.n8 = n8 - promote;
    b.t16 = (b.n16 + 1) >> 1;
    if (wave == 0 && lane < cnt) {
        const unsigned long long below = (1ull << lane) - 1ull;
        int tile, slot;
        if (cls == 32) { tile = __popcll(m32 & below); slot = 0; }
        else {
            int c = cls, r = __popcll((cls == 16 ? m16 : m8) & below);
            if (promote && c == 8 && r == n8 - 1) { c = 16; r = n16; }
            if (c == 16) { tile = b.n32 + (r >> 1); slot = r & 1; }
            else { tile = b.n32 + b.t16 + (r >> 2); slot = r & 3; }
        }
        s_desc[tile * 4 + slot] = base + lane;
    }
    __syncthreads();
    return b;
}

// tile g of a classified block -> log2(rows per slot), filled slots, and the centre of each of the four slots (an unfilled slot
// repeats slot 0's centre: its rows are computed and stored nowhere); all wave-uniform
__device__ __forceinline__ void pn2_pack_tile(const Pn2PackBlock& b, int g, const int* s_desc, int& sshift, int& nvalid, int (&gq)[4]) {
    if (g < b.n32) { sshift = 5; nvalid = 1; }
    else if (g < b.n32 + b.t16) { sshift = 4; nvalid = min(2, b.n16 - 2 * (g - b.n32)); }
    else { sshift = 3; nvalid = min(4, b.n8 - 4 * (g - b.n32 - b.t16)); }
#pragma unroll
    for (int q = 0; q < 4; ++q) gq[q] = __builtin_amdgcn_readfirstlane(s_desc[g * 4 + (q < nvalid ? q : 0)]);
}

// pooled epilogue of a PACKED tile: the tile holds 32 >> sshift slots of 1 << sshift rows, slot q = rows [q << sshift,
// (q + 1) << sshift) = accumulator registers [q << (sshift - 1), (q + 1) << (sshift - 1)) of both half-waves, and belongs to
// centre gq[q].  One maximum per slot, one half-wave exchange, then bias and ReLU; slots >= nvalid repeat slot 0's rows and store
// nothing.  A maximum does not depend on the order it is taken in, nor on how often a value occurs: same bits as the maximum over
// the centre's 32 rows when the dropped rows are copies of row 0.
template <int NT>
__device__ __forceinline__ void pool_store_packed(const f32x16 (&acc)[NT], const float* __restrict__ sbias, float* __restrict__ out,
                                                  int wout, int sshift, int nvalid, const int (&gq)[4], int half, int l31) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float bv = sbias[nt * 32 + l31];
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            v[q] = fmaxf(fmaxf(acc[nt][4 * q], acc[nt][4 * q + 1]), fmaxf(acc[nt][4 * q + 2], acc[nt][4 * q + 3]));
        if (sshift == 3) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float u = fmaxf(v[q], __shfl_xor(v[q], 32));
                if (half == 0 && q < nvalid) out[(size_t)gq[q] * wout + nt * 32 + l31] = fmaxf(u + bv, 0.f);
            }
        } else if (sshift == 4) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float u = fmaxf(v[2 * q], v[2 * q + 1]);
                u = fmaxf(u, __shfl_xor(u, 32));
                if (half == 0 && q < nvalid) out[(size_t)gq[q] * wout + nt * 32 + l31] = fmaxf(u + bv, 0.f);
            }
        } else {
            float u = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            u = fmaxf(u, __shfl_xor(u, 32));
            if (half == 0) out[(size_t)gq[0] * wout + nt * 32 + l31] = fmaxf(u + bv, 0.f);
        }
    }
}

}  // namespace
