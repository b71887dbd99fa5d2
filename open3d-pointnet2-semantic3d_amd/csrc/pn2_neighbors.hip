// pn2_neighbors.hip -- fixed-radius neighbourhoods: per point the number of points within `radius` of it, the integer moments of
// that neighbourhood, its surface normal and its surface variation (what Open3D offers as estimate_normals with
// KDTreeSearchParamRadius and remove_radius_outlier).  The rules are in include/pn2_abi.h ("Fixed-radius neighbourhoods");
// tests/neighbors_ref.py is their numpy model, and everything here is compared with it for equality: a neighbourhood is a pure
// distance test, its sums are integer adds, and the eigen stage is pn2_eig3.h's fixed float64 sequence.
//
// pn2_radius_neighborhoods queues, on the caller's stream (eager only), six launches and one radix sort:
//   1 radius_init_kernel   : the scalars (a workspace arrives uninitialised; no memset node).
//   2 .. 5 CellGrid::build : pn2_cell_grid.h -- grid_min_kernel (the minimum of the valid points, their number), grid_key_kernel
//                            (the 63-bit cell key of every point at cell edge radius * (1 + 2^-20), x lowest; ~0 for an invalid
//                            point; status 1 for a cell coordinate >= 2^21), the radix sort of (key, point index) pairs,
//                            grid_gather_kernel (the sorted points as (x, y, z, index) rows; the fourth word is never read here).
//   6 radius_scan_kernel   : THE HOT ONE, below.
//   7 radius_header_kernel : the header from the scalars.
//
// THE SCAN.  One lane owns one SORTED point for the whole kernel: its count and its nine int64 sums live in the lane's registers,
// so there is no atomic and no LDS accumulation anywhere in it; the eigen stage runs as the kernel's tail on the lane's own sums,
// and the outputs are scattered to the point's original index.  The header's two counters are one atomic each per wave.
// Because a neighbour is decided by the distance test alone, ANY superset of the 27 cells around a point is a legal candidate
// set: a candidate from further away fails the test and changes nothing.  Two ways to enumerate one:
//   (a) the lane path.  Each lane walks the nine key ranges of its own cell: the rows y-1 .. y+1 of the layers z-1 .. z+1, x from
//       cx-1 to cx+1 (x is the lowest key field, so a row's three cells are one range of the sorted keys).  One binary search
//       and one stream of 16-byte loads per lane and range: pn2_cell_grid.h's grid_walk_rows with nrows = 9, end = n.
//   (b) the wave-uniform path, for a wave whose valid lanes lie in ONE row (cy, cz) with cx_max - cx_min <= kSpan (the sorted
//       order makes that common in a dense cloud: 64 consecutive keys).  The nine ranges are then the wave's own, x from
//       cx_min-1 to cx_max+1: lanes 0 .. 17 do the eighteen binary searches side by side, and the candidates are read in chunks
//       of 64 -- lane l loads spts[t0 + l] once, coalesced -- and handed round with v_readlane: the loop counter j is uniform, so
//       candidate j sits in scalar registers and costs no LDS and no per-lane load, and every lane tests the same candidate.
//       EVERY lane of the wave is a loader, whether or not its own point is valid or inside the cloud: no lane leaves before
//       the loop, and the loads are not under the query's mask.
//   A wave that is not eligible takes (a) as a whole.  Both give the same bits: the same tests on a superset, integer sums.
// In the loop the snap to the lattice multiplies by 1 / h (a power of two: exact) and rounds to nearest-even; |q| <= 2^20 fits
// an int32, so the six products are v_mad_i64_i32.
#include "pn2_cell_grid.h"  // kT, kCellBits, kCellLimit, kInvalidKey, GridScal, grid_scal_reset, key_cell, row_key, cell_in,
                            // lower_bound_key, grid_walk_rows, CellGrid
#include "pn2_common.h"
#include "pn2_eig3.h"       // eig3_axes, fix_sign
#include "pn2_wg.h"         // blocks_of, finite_host, refuse_capture, WsCarver

namespace {

constexpr int kChunk = 64;  // candidates per round of the wave-uniform path: one per lane
constexpr int kSpan = 8;    // the widest cx_max - cx_min of a wave that takes the wave-uniform path (measured: EXPERIMENTS.md,
                            // "Fixed-radius neighbourhoods")
// tuning hooks (pn2_debug_set(21, v), (22, v)): 21 = the variant, 0 = auto, 1 = the lane path only; 22 = kSpan (tools/neighbors_cost.py)
PN2_TUNABLE(int, g_radius_variant, 0)
PN2_TUNABLE(int, g_radius_span, kSpan)

// the scalars of one call, at the head of the workspace: the grid's, then
struct Scal : GridScal {
    int nok;       // points with count >= min_neighbors
    int maxcount;  // the largest count
};

struct Params {
    double r2;       // (double)radius * (double)radius
    double inv_h;    // 2^(Q - x)
    double h2;       // h * h
    double view[3];  // the viewpoint, copied from the host
    int has_view, min_neighbors, variant, span;
};

struct Ws {
    Scal* scal;
    CellGrid grid;
};
inline int ws_layout(int n, WsCarver& c, Ws* w) {
    w->scal = c.take<Scal>(1);
    w->grid.carve(c, (size_t)n);
    return w->grid.carve_tmp(c, n);
}

__global__ void radius_init_kernel(Scal* __restrict__ s) {
    if (threadIdx.x == 0) {
        grid_scal_reset(s);
        s->nok = s->maxcount = 0;
    }
}

// the count and the sums of one lane's own point
struct Sums {
    int count;
    long long s[9];  // S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz
};

// candidate (qx, qy, qz) against the lane's point: the NEIGHBOUR test of the header and, for a neighbour, the ten integer adds
__device__ __forceinline__ void test_candidate(bool valid, double px, double py, double pz, float qx, float qy, float qz, double r2,
                                               double inv_h, Sums& a) {
    const double dx = (double)qx - px, dy = (double)qy - py, dz = (double)qz - pz;
    if (valid && (dx * dx + dy * dy) + dz * dz <= r2) {
        // d / h: h is a power of two and |d| <= r (1 + 2^-51) < 2^x, so the product with 1 / h is the same double, |.| <= 2^Q
        const int ix = (int)__builtin_rint(dx * inv_h), iy = (int)__builtin_rint(dy * inv_h), iz = (int)__builtin_rint(dz * inv_h);
        a.count += 1;
        a.s[0] += ix; a.s[1] += iy; a.s[2] += iz;
        a.s[3] += (long long)ix * ix; a.s[4] += (long long)ix * iy; a.s[5] += (long long)ix * iz;
        a.s[6] += (long long)iy * iy; a.s[7] += (long long)iy * iz; a.s[8] += (long long)iz * iz;
    }
}

__global__ void __launch_bounds__(kT)
radius_scan_kernel(int n, const unsigned long long* __restrict__ keys, const int* __restrict__ order,
                   const float4* __restrict__ spts, Params P, Scal* __restrict__ s, int* __restrict__ count,
                   long long* __restrict__ moments, float* __restrict__ normals, float* __restrict__ curvature,
                   double* __restrict__ variance) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = t < n;
    const unsigned long long key = in ? keys[t] : kInvalidKey;
    const bool valid = key != kInvalidKey && s->status == 0;  // (the status is the same for every thread)
    const Cell own = key_cell(key);
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (valid) p = spts[t];
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    Sums a;
    a.count = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) a.s[j] = 0;

    // the valid lanes of a wave are consecutive sorted keys: the first and the last bound them all
    const unsigned long long any = __ballot(valid);
    bool uniform = false;
    int ux0 = 0, ux1 = 0, uy = 0, uz = 0;
    if (any != 0ull) {
        const int first = __ffsll((long long)any) - 1, last = 63 - __clzll((long long)any);
        const unsigned long long kf = __shfl(key, first), kl = __shfl(key, last);
        const int fx = (int)(kf & (kCellLimit - 1)), lx = (int)(kl & (kCellLimit - 1));
        uniform = P.variant == 0 && (kf >> kCellBits) == (kl >> kCellBits) && lx - fx <= P.span;
        ux0 = fx > 0 ? fx - 1 : 0;
        ux1 = lx < kCellLimit - 1 ? lx + 1 : lx;
        uy = (int)((kf >> kCellBits) & (kCellLimit - 1));
        uz = (int)((kf >> (2 * kCellBits)) & (kCellLimit - 1));
    }
    if (uniform) {
        // (b) lane 2r: where range r begins, lane 2r + 1: where it ends (the other lanes search along and are not read)
        const int r = (lane >> 1) % 9;
        const int z = uz - 1 + r / 3, y = uy - 1 + r % 3;
        int bound = 0;
        if (cell_in(z) && cell_in(y)) {
            const unsigned long long row = row_key(y, z);
            bound = lower_bound_key(keys, n, (lane & 1) ? (row | (unsigned long long)ux1) + 1ull : (row | (unsigned long long)ux0));
        }
        for (int rr = 0; rr < 9; ++rr) {
            const int lo = __builtin_amdgcn_readlane(bound, 2 * rr), hi = __builtin_amdgcn_readlane(bound, 2 * rr + 1);
            for (int t0 = lo; t0 < hi; t0 += kChunk) {  // (hi - t0 > 0: no overflow in the difference)
                const int left = hi - t0, chunk = left < kChunk ? left : kChunk;
                // every lane loads, valid or not: lane l holds candidate t0 + l
                float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (lane < chunk) c = spts[(size_t)t0 + lane];
                const int bx = __float_as_int(c.x), by = __float_as_int(c.y), bz = __float_as_int(c.z);
                for (int j = 0; j < chunk; ++j)  // j is uniform: the candidate arrives in scalar registers
                    test_candidate(valid, px, py, pz, __int_as_float(__builtin_amdgcn_readlane(bx, j)),
                                   __int_as_float(__builtin_amdgcn_readlane(by, j)),
                                   __int_as_float(__builtin_amdgcn_readlane(bz, j)), P.r2, P.inv_h, a);
            }
        }
    } else if (valid) {
        // (a) the nine rows around this lane's own cell, whole
        grid_walk_rows(keys, n, spts, own.x, own.y, own.z, 9,
                       [&](int, const float4& q) { test_candidate(true, px, py, pz, q.x, q.y, q.z, P.r2, P.inv_h, a); });
    }

    // the tail: covariance and axes of the lane's own sums (include/pn2_abi.h: m = count, upright = 0)
    const float nanf32 = __int_as_float(0x7FC00000);
    const double nan64 = __longlong_as_double(0x7FF8000000000000ll);
    float nrm[3] = {nanf32, nanf32, nanf32}, curv = nanf32;
    double var[3] = {nan64, nan64, nan64};
    const bool full = valid && a.count >= P.min_neighbors;
    if (full) {
        const double md = (double)a.count;
        const double sx = (double)a.s[0] / md, sy = (double)a.s[1] / md, sz = (double)a.s[2] / md;
        const double a00 = (double)a.s[3] / md - sx * sx, a01 = (double)a.s[4] / md - sx * sy, a02 = (double)a.s[5] / md - sx * sz;
        const double a11 = (double)a.s[6] / md - sy * sy, a12 = (double)a.s[7] / md - sy * sz, a22 = (double)a.s[8] / md - sz * sz;
        double lam[3], e0[3], e1[3], e2[3];
        eig3_axes(a00, a01, a02, a11, a12, a22, lam, e0, e1, e2);
        fix_sign(e2);
        if (P.has_view) {
            const double w = ((P.view[0] - px) * e2[0] + (P.view[1] - py) * e2[1]) + (P.view[2] - pz) * e2[2];
            if (w < 0.0) { e2[0] = -e2[0]; e2[1] = -e2[1]; e2[2] = -e2[2]; }  // a zero or NaN w changes nothing
        }
        const double tr = (lam[0] + lam[1]) + lam[2];
        const double c = lam[2] / tr;
        curv = (float)(c > 0.0 ? c : 0.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            nrm[k] = (float)e2[k];
            var[k] = lam[k] * P.h2;
        }
    }
    if (in) {
        const size_t i = (size_t)order[t];
        count[i] = a.count;
        if (moments) {
#pragma unroll
            for (int j = 0; j < 9; ++j) moments[i * 9 + j] = a.s[j];
        }
        normals[i * 3] = nrm[0]; normals[i * 3 + 1] = nrm[1]; normals[i * 3 + 2] = nrm[2];
        curvature[i] = curv;
        if (variance) { variance[i * 3] = var[0]; variance[i * 3 + 1] = var[1]; variance[i * 3 + 2] = var[2]; }
    }
    // the header's counters: one atomic each per wave
    const unsigned long long fulls = __ballot(full);
    const int most = pn2_wave_all_max(a.count);
    if (lane == 0 && any != 0ull) {
        if (fulls != 0ull) atomicAdd(&s->nok, __popcll(fulls));
        atomicMax(&s->maxcount, most);
    }
}

__global__ void radius_header_kernel(const Scal* __restrict__ s, int Q, int x, int* __restrict__ header) {
    if (threadIdx.x == 0) {
        const bool ok = s->status == 0;
        header[0] = s->status;
        header[1] = ok ? s->nvalid : 0;
        header[2] = ok ? s->nok : 0;
        header[3] = ok ? s->maxcount : 0;
        header[4] = ok ? Q : 0;
        header[5] = ok ? x : 0;
        header[6] = header[7] = 0;
    }
}

}  // namespace

#ifdef PN2_TUNING_HOOKS
extern "C" int pn2_debug_set_neighbors(int what, int value) {
    if (what == 21 && (value == 0 || value == 1)) { g_radius_variant = value; return 0; }
    if (what == 22 && value >= 0 && value < kCellLimit) { g_radius_span = value; return 0; }
    return -1;
}
#endif

extern "C" int pn2_radius_workspace_size(int n, unsigned long long* bytes) {
    if (n <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    const int rc = ws_layout(n, c, &w);
    if (rc != PN2_OK) return rc;
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_radius_neighborhoods(int n, const float* points, const int* labels, float radius, int min_neighbors,
                                        const double* viewpoint, int* count, long long* moments, float* normals, float* curvature,
                                        double* variance, int* header, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1 || !(radius > 0.0f) || !(radius <= 3.402823466e38f) || min_neighbors < 1) return PN2_EINVAL;
    if (viewpoint && !(finite_host(viewpoint[0]) && finite_host(viewpoint[1]) && finite_host(viewpoint[2]))) return PN2_EINVAL;
    if (!points || !count || !normals || !curvature || !header || !workspace) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)labels | (uintptr_t)count | (uintptr_t)normals | (uintptr_t)curvature | (uintptr_t)header) & 3) != 0 ||
        (((uintptr_t)moments | (uintptr_t)variance) & 7) != 0 || ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    const int rc = ws_layout(n, c, &w);  // too small: refused before the sort is asked for its share
    if (rc != PN2_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // it allocates nothing and would be capturable, but nothing in the project captures it: refused until a later change lifts
    // this together with a capture test
    if (const int refused = refuse_capture(st)) return refused;

    // THE LATTICE of this call: radius = f * 2^x, f in [0.5, 1); h = 2^(x - Q)
    int bitlen = 0;
    for (unsigned v = (unsigned)n; v != 0u; v >>= 1) ++bitlen;
    const int Q = (60 - bitlen) >> 1 < 20 ? (60 - bitlen) >> 1 : 20;
    int x = 0;
    (void)frexp((double)radius, &x);  // a float32 > 0 is a normal double: x in [-148, 128], Q in [14, 20]
    Params P;
    P.r2 = (double)radius * (double)radius;
    P.inv_h = ldexp(1.0, Q - x);
    P.h2 = ldexp(1.0, x - Q) * ldexp(1.0, x - Q);
    P.view[0] = viewpoint ? viewpoint[0] : 0.0;
    P.view[1] = viewpoint ? viewpoint[1] : 0.0;
    P.view[2] = viewpoint ? viewpoint[2] : 0.0;
    P.has_view = viewpoint ? 1 : 0;
    P.min_neighbors = min_neighbors;
    P.variant = g_radius_variant;
    P.span = g_radius_span;

    radius_init_kernel<<<1, 64, 0, st>>>(w.scal);
    const int built = w.grid.build(n, points, labels, radius, true, w.scal, st);
    if (built != PN2_OK) return built;
    radius_scan_kernel<<<blocks_of(n, kT), kT, 0, st>>>(n, w.grid.keys(), w.grid.order(), w.grid.spts, P, w.scal, count, moments,
                                                        normals, curvature, variance);
    radius_header_kernel<<<1, 64, 0, st>>>(w.scal, Q, x, header);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
