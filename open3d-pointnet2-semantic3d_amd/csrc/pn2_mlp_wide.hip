// pn2_mlp_wide.hip -- the coarse levels' shared MLPs (SA4, FP2, FP3 of the SSG model: 4096 .. 16384 rows, layer widths
// 128 / 256 / 512) as ONE launch per level: up to three 1x1-conv layers (+bias, ReLU; inference BN folded by the host,
// util/tf_util.py:181-203, pointnet_util.py:150-170 and :312-325) chained inside a workgroup, optionally behind the SA
// front end (group_point + centre + concat, pointnet_util.py:39-54) or the FP front end (inverse-distance weights +
// three_interpolate + concat, pointnet_util.py:300-311), and in front of the max over the K = 32 neighbours.
//
// Why not the register-resident chain of pn2_sa_fused.hip: a 256-wide layer needs 256 KB of weights (LDS holds 160 KB) and
// 2 x 128 accumulator registers per 32-row tile.  Why not one pn2_linear per layer (round 1): each of those launches
// drains and refills the chip around ~7-10 us of MFMA work (8 - 55 % of the MFMA peak on these shapes).
//
// Mapping (v_mfma_f32_32x32x2_f32, exact fp32):
//   * a workgroup (4 waves) owns ONE 32-row tile through all layers; the tile's activations live in LDS
//     (act[row][k], row stride K+4 floats: conflict-free 16-byte reads), ping-pong between two buffers;
//   * a layer (K -> N, N in {128, 256, 512}) is cut into N/128 column blocks x 4/(N/128) slices of the contraction: every
//     wave owns a 32 x 128 accumulator block (four 32x32 tiles) for its K slice; the slices are added through LDS in a
//     fixed order (deterministic);
//   * A operand: one ds_read_b128 per 8 k (lane = row l&31, half-wave h reads k0+4h .. k0+4h+3);
//     B operand: straight from global memory / L2 -- lane (l&31, h) loads w[k0+4h+q][cb + 4*(l&31) .. +3] with one
//     16-byte load per k: the four floats are the B values of the wave's four accumulator tiles, i.e. tile t of a wave
//     holds the output columns cb + 4j + t (j = 0..31).  Four groups of 8 k are in flight under the 16 MFMAs of the
//     current one (an L2 round trip is ~1 us, a group's MFMAs ~0.4 us); the first groups of the NEXT layer are issued
//     before the current layer's epilogue (weights do not depend on it);
//   * the weights stream from L2 once per workgroup and layer (256 KB x rows/32: 64 MB per 256-wide layer at 8192 rows,
//     ~5 us of the XCDs' aggregate L2 bandwidth beside ~9 us of MFMA time).
//
// Host side (the end of this file): the five entry points (pn2_mlp_wide, pn2_sa_mlp_wide, pn2_fp_mlp_wide and the two *_pre
// forms with a hoisted first layer) keep their own argument checks and front-end fields; fill_wide reads the layer stack
// (pn2_layer_stack.h: 1 .. 3 layers of 128 / 256 / 512, weights and biases 16-byte aligned), checks the row count and fills
// what every mode shares; launch_mlp_wide lays out LDS and picks the kernel (plain / gather / gather + PACK / interp).
#include "pn2_common.h"
#include "pn2_layer_stack.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWideDepth = 4;  // groups of 8 k in flight per wave (2 / 6 / 8 measured the same or slower, EXPERIMENTS.md)

struct WideParams {
    int rows, cin, x_stride, nlayers, pool, relu_last;
    int w[3];
    const float* x;  // mode 0: (rows, x_stride) input rows
    // mode 1 (SA front end): rows = b*m*32 grouped neighbours, cin = 3 + c
    int n, m, c;
    const float* xyz;
    const float* new_xyz;
    const float* points;
    const int* idx;
    // mode 2 (FP front end): rows = b*n unknown points, cin = c2 + c1; idx / dist (b,n,3), points2 (b,m,c2) = `points`,
    // points1 (b,n,c1) or NULL
    const float* dist;
    const float* points1;
    int c1, c2;
    const float* W[3];
    const float* bias[3];
    float* y;
    // first layer hoisted by linearity (pn2_*_mlp_wide_pre): zpre = (source rows, w[0]) = points2 @ W0[interpolated rows]
    // (FP, b*m rows) or points @ W0[feature rows] (SA, b*n rows).  The layer-0 tile then holds only the skip-link channels
    // (FP: cin = c1) or dx dy dz (SA: cin = 3), and the layer-0 epilogue adds the blended / gathered rows of zpre.
    const float* zpre;
    int rowtab_off;     // floats from the start of LDS: the FP front end's 32 x 8 row table when zpre is set; PACK: kPackLdsInts
    int sa[2];          // row strides (floats) of the two activation buffers
    int scratch_off;    // floats from the start of LDS (dedicated scratch)
    int scratch_alias;  // 1: the K-slice partial sums are parked in the layer's (consumed) input buffer
};

// GATHER: the A tile of layer 0 is the SA front end, K order [features (c) | dx dy dz | zero pad to a multiple of 8]; the
// host hands over W0 with its rows in that order.
// INTERP: the A tile of layer 0 is the FP front end [three_interpolate(points2, idx, w(dist)) | points1]
// (pointnet_util.py:300-311), formed with the float expressions of fp_interp_concat_* / the reference ops.
//
// PACK (GATHER with pool == 32): the ball query pads a short index row with copies of its first hit, a padded row's MLP output is
// a copy too and the max does not count copies (pn2_sa_fused.hip, PACK).  A group's class is the smallest s in {8, 16, 32} with
// idx[j] == idx[0] for all j >= s; four class-8 or two class-16 groups share one 32-row tile.  A workgroup still carries ONE tile
// (a tile is ~27 us of matrix time on its CU: a loop over tiles would multiply the single-batch latency), so the packing is
// decided per chunk of kPackChunk consecutive groups, redundantly by every workgroup of the chunk: thread i classifies group i
// of the chunk, ranks come from ballots and popcounts through LDS, workgroup j of the chunk takes tile j of the chunk's list
// (class-32 tiles, then pairs of class 16, then fours of class 8) and the workgroups behind the list return.  No atomics, no
// second launch; the grid stays one workgroup per group.  The tile's 32 source rows (cloud base included: a tile may mix clouds)
// and its groups live in LDS, nothing of it in vector registers across the layer loop.  Every row keeps its own MFMA row and the
// contraction is cut and added as without PACK: same bits for any index table.
enum { kWidePlain = 0, kWideGather = 1, kWideInterp = 2 };
constexpr int kPackChunk = 256;  // groups per chunk = threads per workgroup
// PACK's LDS region (ints, at rowtab_off): source row of each tile row | groups of the slots | log2(slot rows), filled slots | counts
constexpr int kPackRows = 0, kPackGroups = 32, kPackMeta = 36, kPackCounts = 40, kPackLdsInts = 64;
template <int MODE, bool PACK = false>
__global__ void __launch_bounds__(256, 2)
mlp_wide_kernel(WideParams p) {
    constexpr bool GATHER = MODE == kWideGather;
    static_assert(!PACK || GATHER, "PACK: the pooled gather mode only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x;
    const int row0 = tile * 32;
    // LDS addresses are formed as smem + integer offset everywhere: selecting between POINTERS to the two buffers at run
    // time degrades them to generic pointers, the operand reads become flat_load, and flat loads (unordered against
    // global loads) force s_waitcnt vmcnt(0) in front of every group of MFMAs -- no load/MFMA overlap at all (measured).
    const int buf_off[2] = {0, 32 * p.sa[0]};
    float* const buf0 = smem;

    // ---- per-layer roles of this wave; the B operands (weights) of a layer go in flight before its input is ready ------
    struct LayerCfg { int N, wnt, ks_n, nq, ks, cb, g0, g1; const float* wcol; };
    auto make_cfg = [&](int l, int Kt) {
        LayerCfg c;
        c.N = p.w[l];
        c.wnt = c.N >> 7;        // column blocks of 128
        c.ks_n = 4 / c.wnt;      // slices of the contraction
        c.nq = wave % c.wnt;
        c.ks = wave / c.wnt;
        c.cb = c.nq * 128;
        const int ngroups = (Kt + 7) >> 3;
        c.g0 = (ngroups * c.ks) / c.ks_n;
        c.g1 = (ngroups * (c.ks + 1)) / c.ks_n;
        c.wcol = p.W[l] + c.cb + 4 * l31;
        return c;
    };
    f32x4 bq[kWideDepth][4];
    // W_l has round8(K_l) rows (the host pads with zero rows; in GATHER mode it also moves the three coordinate rows behind
    // the feature rows): no clamping or row mapping in the loop, four 16-byte loads off one pointer per group
    auto fetch_b = [&](const LayerCfg& c, int g, f32x4 (&b_)[4]) {
        const float* __restrict__ wp = c.wcol + (size_t)(8 * g + 4 * half) * c.N;
#pragma unroll
        for (int q = 0; q < 4; ++q) b_[q] = *reinterpret_cast<const f32x4*>(wp + (size_t)q * c.N);
    };
    auto prefetch_b = [&](const LayerCfg& c) {
#pragma unroll
        for (int u = 0; u < kWideDepth; ++u) fetch_b(c, c.g0 + u < c.g1 ? c.g0 + u : c.g1 - 1, bq[u]);
    };
    const LayerCfg first = make_cfg(0, p.cin);
    int* const pk = reinterpret_cast<int*>(smem + p.rowtab_off);  // PACK only
    (void)pk;
    if constexpr (PACK) {
        const int groups = p.rows >> 5;
        const int cbase = (tile / kPackChunk) * kPackChunk, mytile = tile - cbase;
        const int cnt = min(kPackChunk, groups - cbase);
        // classify: live slots = 1 + the last position that differs from position 0 (NOT the number of distinct values)
        int cls = 0;
        if (tid < cnt) {
            const int4* __restrict__ ip = reinterpret_cast<const int4*>(p.idx + (size_t)(cbase + tid) * 32);
            int4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ip[u];
            const int head = v[0].x;
            int live = 1;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (v[u].x != head) live = 4 * u + 1;
                if (v[u].y != head) live = 4 * u + 2;
                if (v[u].z != head) live = 4 * u + 3;
                if (v[u].w != head) live = 4 * u + 4;
            }
            cls = live <= 8 ? 8 : (live <= 16 ? 16 : 32);
        }
        const unsigned long long m32 = __ballot(cls == 32), m16 = __ballot(cls == 16), m8 = __ballot(cls == 8);
        if (lane == 0) {
            pk[kPackCounts + 3 * wave + 0] = __popcll(m32);
            pk[kPackCounts + 3 * wave + 1] = __popcll(m16);
            pk[kPackCounts + 3 * wave + 2] = __popcll(m8);
        }
        __syncthreads();
        int n32 = 0, n16 = 0, n8 = 0, b32 = 0, b16 = 0, b8 = 0;  // totals of the chunk, counts of the waves below this one
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c32 = pk[kPackCounts + 3 * w], c16 = pk[kPackCounts + 3 * w + 1], c8 = pk[kPackCounts + 3 * w + 2];
            n32 += c32; n16 += c16; n8 += c8;
            if (w < wave) { b32 += c32; b16 += c16; b8 += c8; }
        }
        n32 = __builtin_amdgcn_readfirstlane(n32); n16 = __builtin_amdgcn_readfirstlane(n16); n8 = __builtin_amdgcn_readfirstlane(n8);
        // an odd class-16 group shares its tile with the last class-8 group when that saves the class-8 tile it would open
        const int promote = ((n16 & 1) && (n8 & 3) == 1) ? 1 : 0;
        const int k16 = n16 + promote, k8 = n8 - promote, t16 = (k16 + 1) >> 1;
        const int ntiles = n32 + t16 + ((k8 + 3) >> 2);
        if (mytile >= ntiles) return;  // uniform: the chunk packed into fewer tiles than it has groups
        prefetch_b(first);  // after the decision (a returning workgroup streams no weights), in flight under the ranking and the staging
        if (cls != 0) {
            const unsigned long long below = (1ull << lane) - 1ull;
            int t, slot;
            if (cls == 32) { t = b32 + __popcll(m32 & below); slot = 0; }
            else {
                int c = cls, r = cls == 16 ? b16 + __popcll(m16 & below) : b8 + __popcll(m8 & below);
                if (promote && c == 8 && r == n8 - 1) { c = 16; r = n16; }
                if (c == 16) { t = n32 + (r >> 1); slot = r & 1; }
                else { t = n32 + t16 + (r >> 2); slot = r & 3; }
            }
            if (t == mytile) pk[kPackGroups + slot] = cbase + tid;
        }
        if (tid == 0) {  // tile `mytile` of the list: slot size and filled slots (the last tile of a class may be short)
            int sshift, nvalid;
            if (mytile < n32) { sshift = 5; nvalid = 1; }
            else if (mytile < n32 + t16) { sshift = 4; nvalid = min(2, k16 - 2 * (mytile - n32)); }
            else { sshift = 3; nvalid = min(4, k8 - 4 * (mytile - n32 - t16)); }
            pk[kPackMeta] = sshift; pk[kPackMeta + 1] = nvalid;
        }
        __syncthreads();
    } else {
        prefetch_b(first);
    }

    // ---- stage the input tile ------------------------------------------------------------------------------------
    const int K0 = (p.cin + 7) & ~7;
    // eight independent global loads in flight per thread (a plain load -> LDS store loop pays one L2 round trip per
    // iteration: measured 15 us of a 512-workgroup launch)
    auto stage4 = [&](int count4, int cv, int sa, auto src_of) {  // src_of(r, j) -> address of 4 floats
        for (int base = 0; base < count4; base += 256 * 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int e = base + u * 256 + tid;
                e = e < count4 ? e : count4 - 1;
                const int r = e / cv, j = e - r * cv;
                v[u] = *reinterpret_cast<const f32x4*>(src_of(r, j));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = base + u * 256 + tid;
                if (e < count4) {
                    const int r = e / cv, j = e - r * cv;
                    *reinterpret_cast<f32x4*>(buf0 + r * sa + 4 * j) = v[u];
                }
            }
        }
    };
    if constexpr (GATHER) {
        const int c = p.c, cv = c >> 2;  // c % 4 == 0
        const int bi = PACK ? 0 : tile / p.m;  // one tile = one centre (K = 32); PACK: the row table holds rows of (b*n, c)
        const float* __restrict__ pts = p.points + (size_t)bi * p.n * c;
        const int* __restrict__ idx = PACK ? pk + kPackRows : p.idx + (size_t)tile * 32;
        float* myrow = buf0 + (tid & 31) * p.sa[0];
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if constexpr (PACK) {
            // row r of the tile: slot r >> sshift, position r & (slot rows - 1) of that slot's group; the empty slots of a short
            // tile repeat the first group (their maxima are not stored)
            if (tid < 32) {
                const int sshift = pk[kPackMeta], nvalid = pk[kPackMeta + 1];
                const int q = tid >> sshift;
                const int g = pk[kPackGroups + (q < nvalid ? q : 0)];
                const int src = (g / p.m) * p.n + p.idx[(size_t)g * 32 + (tid & ((1 << sshift) - 1))];
                pk[kPackRows + tid] = src;
                const float* __restrict__ q3 = p.xyz + (size_t)src * 3;
                const float* __restrict__ ctr = p.new_xyz + (size_t)g * 3;
                dx = q3[0] - ctr[0]; dy = q3[1] - ctr[1]; dz = q3[2] - ctr[2];
            }
            __syncthreads();  // the row table is read by every thread (here or in the layer-0 epilogue)
        } else if (tid < 32) {
            const float* __restrict__ q = p.xyz + ((size_t)bi * p.n + idx[tid]) * 3;
            const float* __restrict__ ctr = p.new_xyz + (size_t)tile * 3;
            dx = q[0] - ctr[0]; dy = q[1] - ctr[1]; dz = q[2] - ctr[2];  // pointnet_util.py:44-46
        }
        if (p.zpre) {  // features hoisted: the tile is [dx dy dz | 0 0 0 0 0]
            if (tid < 32) {
                myrow[0] = dx; myrow[1] = dy; myrow[2] = dz;
                for (int k = 3; k < K0; ++k) myrow[k] = 0.f;
            }
        } else {
        stage4(32 * cv, cv, p.sa[0], [&](int r, int j) { return pts + (size_t)idx[r] * c + 4 * j; });
        if (tid < 32) {
            myrow[c] = dx; myrow[c + 1] = dy; myrow[c + 2] = dz;
            for (int k = c + 3; k < K0; ++k) myrow[k] = 0.f;
        }
        }
    } else if constexpr (MODE == kWideInterp) {
        const int c2 = p.c2, c1 = p.c1, cv2 = c2 >> 2, cv1 = c1 >> 2;  // both % 4 == 0
        const int bi = row0 / p.n;  // p.n % 32 == 0: a tile never straddles two clouds
        const float* __restrict__ p2 = p.points + (size_t)bi * p.m * c2;
        // 8 floats per row: w1 w2 w3 - | i1 i2 i3 -  (buffer 1 is idle until layer 0 ends; with zpre the table is still
        // needed in the layer-0 epilogue, which writes buffer 1: a region of its own)
        float* rowtab = smem + (p.zpre ? p.rowtab_off : buf_off[1]);
        if (tid < 32) {
            const size_t r = (size_t)row0 + tid;
            const float d1 = fmaxf(p.dist[r * 3 + 0], 1e-10f), d2 = fmaxf(p.dist[r * 3 + 1], 1e-10f);
            const float d3 = fmaxf(p.dist[r * 3 + 2], 1e-10f);
            const float r1 = 1.0f / d1, r2 = 1.0f / d2, r3 = 1.0f / d3;  // IEEE divisions (pointnet_util.py:300-303)
            const float norm = (r1 + r2) + r3;
            *reinterpret_cast<f32x4*>(rowtab + tid * 8) = f32x4{r1 / norm, r2 / norm, r3 / norm, 0.f};
            *reinterpret_cast<f32x4*>(rowtab + tid * 8 + 4) =
                f32x4{__int_as_float(p.idx[r * 3 + 0]), __int_as_float(p.idx[r * 3 + 1]), __int_as_float(p.idx[r * 3 + 2]), 0.f};
        }
        __syncthreads();
        const int count4 = p.zpre ? 0 : 32 * cv2;  // interpolated channels hoisted: nothing to stage for them
        for (int base = 0; base < count4; base += 256 * 4) {  // 4 elements x 3 gathers in flight per thread
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int e = base + u * 256 + tid;
                e = e < count4 ? e : count4 - 1;
                const int r = e / cv2, j = e - r * cv2;
                const f32x4 wq = *reinterpret_cast<const f32x4*>(rowtab + r * 8);
                const f32x4 iq = *reinterpret_cast<const f32x4*>(rowtab + r * 8 + 4);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(p2 + (size_t)__float_as_int(iq[0]) * c2 + 4 * j);
                const f32x4 x2 = *reinterpret_cast<const f32x4*>(p2 + (size_t)__float_as_int(iq[1]) * c2 + 4 * j);
                const f32x4 x3 = *reinterpret_cast<const f32x4*>(p2 + (size_t)__float_as_int(iq[2]) * c2 + 4 * j);
                v[u] = (x1 * wq[0] + x2 * wq[1]) + x3 * wq[2];  // tf_interpolate.cpp:322-324, unfused
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = base + u * 256 + tid;
                if (e < count4) {
                    const int r = e / cv2, j = e - r * cv2;
                    *reinterpret_cast<f32x4*>(buf0 + r * p.sa[0] + 4 * j) = v[u];
                }
            }
        }
        if (c1 > 0) {
            const float* __restrict__ p1 = p.points1 + (size_t)row0 * c1;
            for (int e = tid; e < 32 * cv1; e += 256) {
                const int r = e / cv1, j = e - r * cv1;
                *reinterpret_cast<f32x4*>(buf0 + r * p.sa[0] + (p.zpre ? 0 : c2) + 4 * j) = *reinterpret_cast<const f32x4*>(p1 + (size_t)r * c1 + 4 * j);
            }
        }
        if (K0 > p.cin) {
            const int padw = K0 - p.cin;
            for (int e = tid; e < 32 * padw; e += 256) buf0[(e / padw) * p.sa[0] + p.cin + e % padw] = 0.f;
        }
    } else {
        const float* __restrict__ x = p.x;
        if ((p.x_stride & 3) == 0 && (p.cin & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
            const int cv = p.cin >> 2;
            stage4(32 * cv, cv, p.sa[0], [&](int r, int j) {
                const int gr = row0 + r < p.rows ? row0 + r : p.rows - 1;
                return x + (size_t)gr * p.x_stride + 4 * j;
            });
            if (row0 + 32 > p.rows) {  // ragged last tile: rows past the end are zero
                __syncthreads();
                for (int e = tid; e < 32 * p.cin; e += 256) {
                    const int r = e / p.cin;
                    if (row0 + r >= p.rows) buf0[r * p.sa[0] + e - r * p.cin] = 0.f;
                }
            }
        } else {
            const int total = 32 * p.cin;
            for (int base = 0; base < total; base += 256 * 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int e = base + u * 256 + tid;
                    e = e < total ? e : total - 1;
                    const int r = e / p.cin, k = e - r * p.cin;
                    const int gr = row0 + r < p.rows ? row0 + r : p.rows - 1;
                    v[u] = x[(size_t)gr * p.x_stride + k];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = base + u * 256 + tid;
                    if (e < total) {
                        const int r = e / p.cin, k = e - r * p.cin;
                        buf0[r * p.sa[0] + k] = row0 + r < p.rows ? v[u] : 0.f;
                    }
                }
            }
        }
        if (K0 > p.cin) {
            const int padw = K0 - p.cin;
            for (int e = tid; e < 32 * padw; e += 256) buf0[(e / padw) * p.sa[0] + p.cin + e % padw] = 0.f;
        }
    }
    __syncthreads();

    // (the layer loop below starts with the B operands of layer 0 already in flight: see `prefetch_b` before the staging)
    LayerCfg cur = first;
#pragma unroll 1
    for (int l = 0; l < p.nlayers; ++l) {
        const int N = cur.N, wnt = cur.wnt, ks_n = cur.ks_n, nq = cur.nq, ks = cur.ks, cb = cur.cb, g0 = cur.g0, g1 = cur.g1;
        const int in_off = buf_off[l & 1];
        const int sin = p.sa[l & 1];
        const float* __restrict__ arow = smem + in_off + l31 * sin + 4 * half;

        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

        auto contract = [&](const f32x4& a_, const f32x4 (&b_)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_[q], b_[q][t], acc[t], 0, 0, 0);
        };
        if (g0 < g1) {
            const int last = g1 - 1;
            f32x4 aq[kWideDepth];
#pragma unroll
            for (int u = 0; u < kWideDepth; ++u) aq[u] = *reinterpret_cast<const f32x4*>(arow + 8 * (g0 + u < g1 ? g0 + u : last));
            int g = g0;
            // steady state: every refill is a real group (no clamping in the loop)
            for (; g + 2 * kWideDepth <= g1; g += kWideDepth) {
#pragma unroll
                for (int u = 0; u < kWideDepth; ++u) {
                    // sched_barrier: keep "16 MFMAs of slot u, then the refill of slot u" in program order.  Left alone the
                    // scheduler sinks all loads of the iteration below its 64 MFMAs and waits for them (vmcnt(0)) at the top
                    // of the next one: no load ever overlaps an MFMA (measured 48 % of the MFMA rate on an idle chip).
                    contract(aq[u], bq[u]);
                    __builtin_amdgcn_sched_barrier(0);
                    const int gn = g + kWideDepth + u;
                    aq[u] = *reinterpret_cast<const f32x4*>(arow + 8 * gn);
                    fetch_b(cur, gn, bq[u]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // drain: the slots hold groups g .. g+D-1 (those < g1 are real), rem more groups follow them
            const int rem = g1 - g - kWideDepth;  // < D
#pragma unroll
            for (int u = 0; u < kWideDepth; ++u) {
                if (g + u < g1) contract(aq[u], bq[u]);
                if (u < rem) {
                    aq[u] = *reinterpret_cast<const f32x4*>(arow + 8 * (g + kWideDepth + u));
                    fetch_b(cur, g + kWideDepth + u, bq[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kWideDepth - 1; ++u)
                if (u < rem) contract(aq[u], bq[u]);
        }
        // the next layer's weights do not depend on this layer's result: put them in flight under the epilogue
        const bool lastl = l == p.nlayers - 1;
        LayerCfg nxt = cur;
        if (!lastl) {
            nxt = make_cfg(l + 1, N);
            prefetch_b(nxt);
        }

        // ---- add the K slices (fixed order: 2,3 onto 0,1, then 1 onto 0), then the epilogue on the slice-0 waves ------
        if (ks_n > 1) {
            const int sc_off = p.scratch_alias ? in_off : p.scratch_off;
            if (p.scratch_alias) __syncthreads();  // every wave has finished reading the layer's input
            auto park = [&](int block) {
                float* dst = smem + sc_off + block * (64 * 64);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * 64 + lane] = acc[t][r];
            };
            auto add = [&](int block) {
                const float* src = smem + sc_off + block * (64 * 64);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] += src[(t * 16 + r) * 64 + lane];
            };
            if (ks_n == 4) {  // one column block, four slices
                if (ks >= 2) park(ks - 2);
                __syncthreads();
                if (ks < 2) add(ks);
                __syncthreads();
                if (ks == 1) park(0);
                __syncthreads();
                if (ks == 0) add(0);
            } else {          // two column blocks, two slices each
                if (ks == 1) park(nq);
                __syncthreads();
                if (ks == 0) add(nq);
            }
        }
        if (ks == 0 && l == 0 && p.zpre) {
            // hoisted part of layer 0: this lane's four output columns (cb + 4 l31 .. +3) of the source rows of zpre
            if constexpr (MODE == kWideInterp) {
                const float* __restrict__ zb = p.zpre + (size_t)(row0 / p.n) * p.m * N + cb + 4 * l31;
                const float* rowtab = smem + p.rowtab_off;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const f32x4 wq = *reinterpret_cast<const f32x4*>(rowtab + row * 8);
                    const f32x4 iq = *reinterpret_cast<const f32x4*>(rowtab + row * 8 + 4);
                    const f32x4 z1 = *reinterpret_cast<const f32x4*>(zb + (size_t)__float_as_int(iq[0]) * N);
                    const f32x4 z2 = *reinterpret_cast<const f32x4*>(zb + (size_t)__float_as_int(iq[1]) * N);
                    const f32x4 z3 = *reinterpret_cast<const f32x4*>(zb + (size_t)__float_as_int(iq[2]) * N);
                    const f32x4 z = (z1 * wq[0] + z2 * wq[1]) + z3 * wq[2];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t][r] += z[t];
                }
            } else if constexpr (MODE == kWideGather) {
                const float* __restrict__ zb = p.zpre + (PACK ? (size_t)0 : (size_t)(tile / p.m) * p.n * N) + cb + 4 * l31;
                const int* __restrict__ idx = PACK ? pk + kPackRows : p.idx + (size_t)tile * 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const f32x4 z = *reinterpret_cast<const f32x4*>(zb + (size_t)idx[row] * N);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t][r] += z[t];
                }
            }
        }
        if (ks == 0) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias[l] + cb + 4 * l31);
            const bool relu = !lastl || p.relu_last;
            if (!lastl) {
                float* __restrict__ out = smem + buf_off[(l + 1) & 1];
                const int so = p.sa[(l + 1) & 1];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    f32x4 v = {acc[0][r] + bv[0], acc[1][r] + bv[1], acc[2][r] + bv[2], acc[3][r] + bv[3]};
                    v = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    *reinterpret_cast<f32x4*>(out + row * so + cb + 4 * l31) = v;
                }
            } else if constexpr (PACK) {
                // segmented max: rows 8q .. 8q+7 are registers 4q .. 4q+3 of both half-waves; a slot of 8 / 16 / 32 rows is one /
                // two / four of these quarters.  A maximum does not depend on the order it is taken in, nor on how often a value
                // occurs: the bits of the un-packed epilogue over the group's 32 rows.
                const int sshift = __builtin_amdgcn_readfirstlane(pk[kPackMeta]);
                const int nvalid = __builtin_amdgcn_readfirstlane(pk[kPackMeta + 1]);
                f32x4 qm[4];  // qm[q][t]: quarter q of column tile t
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float mx = fmaxf(fmaxf(acc[t][4 * q], acc[t][4 * q + 1]), fmaxf(acc[t][4 * q + 2], acc[t][4 * q + 3]));
                        qm[q][t] = fmaxf(mx, __shfl_xor(mx, 32));
                    }
                auto store = [&](int slot, const f32x4& mx) {
                    if (half == 0 && slot < nvalid) {
                        f32x4 v = mx + bv;
                        if (relu) v = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                        const int g = pk[kPackGroups + slot];
                        *reinterpret_cast<f32x4*>(p.y + (size_t)g * N + cb + 4 * l31) = v;
                    }
                };
                auto vmax = [](const f32x4& a, const f32x4& b) {
                    return f32x4{fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3])};
                };
                if (sshift == 3) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) store(q, qm[q]);
                } else if (sshift == 4) {
                    store(0, vmax(qm[0], qm[1]));
                    store(1, vmax(qm[2], qm[3]));
                } else {
                    store(0, vmax(vmax(qm[0], qm[1]), vmax(qm[2], qm[3])));
                }
            } else if (p.pool == 32) {
                f32x4 v;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float mx = acc[t][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[t][r]);
                    mx = fmaxf(mx, __shfl_xor(mx, 32));
                    mx += bv[t];  // max_i relu(x_i + b) == relu(max_i(x_i) + b)
                    v[t] = relu ? fmaxf(mx, 0.f) : mx;
                }
                if (half == 0) *reinterpret_cast<f32x4*>(p.y + (size_t)tile * N + cb + 4 * l31) = v;
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    f32x4 v = {acc[0][r] + bv[0], acc[1][r] + bv[1], acc[2][r] + bv[2], acc[3][r] + bv[3]};
                    if (relu) v = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    if (row < p.rows) *reinterpret_cast<f32x4*>(p.y + (size_t)row * N + cb + 4 * l31) = v;
                }
            }
        }
        if (!lastl) __syncthreads();  // the next layer's input is complete; this layer's input and the scratch are free
        cur = nxt;
    }
}

template <int MODE, bool PACK = false>
int launch_mlp_wide_mode(const WideParams& p, size_t lds, hipStream_t st) {
    if (int e = pn2_allow_lds<mlp_wide_kernel<MODE, PACK>>(kPn2CuLdsBytes)) return e;
    mlp_wide_kernel<MODE, PACK><<<(p.rows + 31) / 32, 256, lds, st>>>(p);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

int launch_mlp_wide(WideParams& p, int mode, hipStream_t st) {
    // LDS: buffer 0 holds the layer-0 and layer-2 inputs, buffer 1 the layer-1 input
    const int k0 = (p.cin + 7) & ~7;
    int ka = k0, kb = 0;
    if (p.nlayers >= 2) kb = p.w[0];
    if (p.nlayers >= 3 && p.w[1] > ka) ka = p.w[1];
    p.sa[0] = ka + 4;
    p.sa[1] = kb + 4 > 8 ? kb + 4 : 8;  // >= 8: the FP front end parks its 32 x 8 row table there
    // K-slice partial sums: two 16 KB blocks; parked in the layer's consumed input buffer when every sliced layer's input
    // is that large, else in a region of their own
    bool sliced = false, alias_ok = true;
    int kin = k0;
    for (int l = 0; l < p.nlayers; ++l) {
        if (p.w[l] < 512) {
            sliced = true;
            if ((size_t)32 * p.sa[l & 1] < (size_t)2 * 64 * 64) alias_ok = false;
        }
        kin = p.w[l];
    }
    (void)kin;
    p.scratch_off = 32 * (p.sa[0] + p.sa[1]);
    p.scratch_alias = sliced && alias_ok;
    p.rowtab_off = p.scratch_off + (sliced && !alias_ok ? 2 * 64 * 64 : 0);
    // row packing (see the kernel): the pooled gather mode, the process-wide switch of the SA kernels read at launch (a captured
    // graph keeps what it was captured with); idx is read 16 bytes at a time and a source row is an int
    const bool pack = mode == kWideGather && p.pool == 32 && pn2_sa_row_packing_enabled() && (((uintptr_t)p.idx) & 15) == 0 &&
                      (long long)(p.rows / 32 / p.m) * p.n <= 0x7fffffffLL;
    const size_t lds = sizeof(float) * ((size_t)p.rowtab_off + (p.zpre && mode == kWideInterp ? 32 * 8 : 0) + (pack ? kPackLdsInts : 0));
    if (lds > kPn2CuLdsBytes) return PN2_EUNSUP;
    if (pack) return launch_mlp_wide_mode<kWideGather, true>(p, lds, st);
    if (mode == kWideGather) return launch_mlp_wide_mode<kWideGather>(p, lds, st);
    if (mode == kWideInterp) return launch_mlp_wide_mode<kWideInterp>(p, lds, st);
    return launch_mlp_wide_mode<kWidePlain>(p, lds, st);
}

constexpr Pn2LayerRule kWideLayers = {3, kPn2WidthsWide, kPn2AlignWeightsAndBias, false};

// What the five entry points fill the same way, behind their own argument checks: the layer stack (pn2_layer_stack.h holds the
// rule and the precedence of its refusals), then the row count -- handed over as long long, b * m * 32 is not formed in an int
// before it is known to fit -- and the fields of every mode.  `between`: the result of the checks an entry point ranks behind
// the layer stack's faults and ahead of PN2_ERANGE (pn2_mlp_wide's pool and y).
int fill_wide(WideParams& p, long long rows, int cin, int nlayers, const int* widths, const float* const* w,
              const float* const* bias, int pool, int relu_last, float* y, int between = PN2_OK) {
    if (int rc = pn2_read_layers(p, kWideLayers, nlayers, widths, w, bias)) return rc;
    if (between != PN2_OK) return between;
    if (rows + 64 > 0x7fffffffLL) return PN2_ERANGE;
    p.rows = (int)rows; p.cin = cin; p.nlayers = nlayers; p.pool = pool; p.relu_last = relu_last; p.y = y;
    return PN2_OK;
}

}  // namespace

extern "C" int pn2_mlp_wide(int rows, int cin, int x_stride, const float* x, int nlayers, const int* widths,
                            const float* const* w, const float* const* bias, int relu_last, int pool, float* y, void* stream) {
    if (rows <= 0 || cin <= 0 || x_stride < cin) return PN2_EINVAL;
    if (!x || !y) return PN2_ENULL;
    const int own = (pool != 0 && pool != 32) ? PN2_EUNSUP
                    : (pool == 32 && rows % 32 != 0) ? PN2_EINVAL
                    : (((uintptr_t)y) & 15) ? PN2_EUNSUP : PN2_OK;
    WideParams p = {};
    if (int rc = fill_wide(p, rows, cin, nlayers, widths, w, bias, pool, relu_last, y, own)) return rc;
    p.x_stride = x_stride; p.x = x;
    return launch_mlp_wide(p, kWidePlain, static_cast<hipStream_t>(stream));
}

extern "C" int pn2_sa_mlp_wide(int b, int n, int m, int nsample, int c, const float* xyz, const float* new_xyz,
                               const float* points, const int* idx, int nlayers, const int* widths, const float* const* w,
                               const float* const* bias, int pool, float* y, void* stream) {
    if (b <= 0 || n <= 0 || m <= 0 || c <= 0) return PN2_EINVAL;
    if (!xyz || !new_xyz || !points || !idx || !y) return PN2_ENULL;
    if (nsample != 32 || c % 4 != 0 || (((uintptr_t)points | (uintptr_t)y) & 15)) return PN2_EUNSUP;
    WideParams p = {};
    if (int rc = fill_wide(p, (long long)b * m * 32, 3 + c, nlayers, widths, w, bias, pool ? 32 : 0, 1, y)) return rc;
    p.n = n; p.m = m; p.c = c; p.xyz = xyz; p.new_xyz = new_xyz; p.points = points; p.idx = idx;
    return launch_mlp_wide(p, kWideGather, static_cast<hipStream_t>(stream));
}

extern "C" int pn2_fp_mlp_wide(int b, int n, int m, int c1, int c2, const float* dist, const int* idx, const float* points1,
                               const float* points2, int nlayers, const int* widths, const float* const* w,
                               const float* const* bias, float* y, void* stream) {
    if (b <= 0 || n <= 0 || m < 3 || c2 <= 0 || c1 < 0) return PN2_EINVAL;
    if (!dist || !idx || !points2 || !y || (c1 > 0 && !points1)) return PN2_ENULL;
    if (n % 32 != 0 || c2 % 4 != 0 || c1 % 4 != 0 || (((uintptr_t)points2 | (uintptr_t)points1 | (uintptr_t)y) & 15)) return PN2_EUNSUP;
    WideParams p = {};
    if (int rc = fill_wide(p, (long long)b * n, c2 + c1, nlayers, widths, w, bias, 0, 1, y)) return rc;
    p.n = n; p.m = m; p.c1 = c1; p.c2 = c2; p.dist = dist; p.idx = idx; p.points = points2; p.points1 = points1;
    return launch_mlp_wide(p, kWideInterp, static_cast<hipStream_t>(stream));
}

// pn2_fp_mlp_wide with the first layer's product with the interpolated channels hoisted by linearity (see
// pn2_fp_mlp_fused_pre): z = points2 @ W0[:c2] (b*m rows, widths[0] wide) replaces points2; w[0] = the c1 skip-link rows of
// the folded first-layer weight, zero-padded to a multiple of 8 rows.  c1 > 0, c1 % 4 == 0.
extern "C" int pn2_fp_mlp_wide_pre(int b, int n, int m, int c1, const float* dist, const int* idx, const float* points1,
                                   const float* z, int nlayers, const int* widths, const float* const* w,
                                   const float* const* bias, float* y, void* stream) {
    if (b <= 0 || n <= 0 || m < 3 || c1 <= 0) return PN2_EINVAL;
    if (!dist || !idx || !z || !y || !points1) return PN2_ENULL;
    if (n % 32 != 0 || c1 % 4 != 0 || (((uintptr_t)z | (uintptr_t)points1 | (uintptr_t)y) & 15)) return PN2_EUNSUP;
    WideParams p = {};
    if (int rc = fill_wide(p, (long long)b * n, c1, nlayers, widths, w, bias, 0, 1, y)) return rc;
    p.n = n; p.m = m; p.c1 = c1; p.c2 = 0; p.dist = dist; p.idx = idx; p.points1 = points1; p.zpre = z;
    return launch_mlp_wide(p, kWideInterp, static_cast<hipStream_t>(stream));
}

// pn2_sa_mlp_wide with the FEATURE part of the first layer hoisted (see pn2_sa_mlp_fused_pre): zf = points @ W0[3:] (b*n
// rows, widths[0] wide) replaces points; w[0] = the 3 xyz rows of the folded first-layer weight + 5 zero rows (8 x widths[0]).
extern "C" int pn2_sa_mlp_wide_pre(int b, int n, int m, int nsample, const float* xyz, const float* new_xyz, const float* zf,
                                   const int* idx, int nlayers, const int* widths, const float* const* w,
                                   const float* const* bias, int pool, float* y, void* stream) {
    if (b <= 0 || n <= 0 || m <= 0) return PN2_EINVAL;
    if (!xyz || !new_xyz || !zf || !idx || !y) return PN2_ENULL;
    if (nsample != 32 || (((uintptr_t)zf | (uintptr_t)y) & 15)) return PN2_EUNSUP;
    WideParams p = {};
    if (int rc = fill_wide(p, (long long)b * m * 32, 3, nlayers, widths, w, bias, pool ? 32 : 0, 1, y)) return rc;
    p.n = n; p.m = m; p.c = 4; p.xyz = xyz; p.new_xyz = new_xyz; p.points = zf; p.idx = idx; p.zpre = zf;
    return launch_mlp_wide(p, kWideGather, static_cast<hipStream_t>(stream));
}
