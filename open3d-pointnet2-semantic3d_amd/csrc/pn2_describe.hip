// pn2_describe.hip -- what each object of a clustered cloud looks like: member count, centroid, principal axes, variances and the
// oriented box around it (Open3D's get_oriented_bounding_box), and the box drawn as points for the renderer.  The rules are in
// include/pn2_abi.h (pn2_cluster_describe); tests/describe_ref.py is their numpy model, and everything here is compared with it
// for equality: every accumulation is an integer sum or an integer minimum / maximum, so the order of arrival cannot show.
//
// pn2_cluster_describe queues, on the caller's stream, seven launches and nothing else (no allocation, no host read, no memset):
//   1 describe_clear_kernel   : the accumulators of every cluster (a workspace arrives uninitialised).
//   2 describe_box_kernel     : per cluster the minimum and maximum x, y, z of its members as ordered uint32 (exact) and their
//                               number m.
//   3 describe_lattice_kernel : one thread per cluster: the origin o, the exponent x of the largest extent, Q, 1 / h.
//   4 describe_moments_kernel : THE HOT ONE.  Per member the lattice coordinates q and nine int64 adds: S_x S_y S_z, S_xx .. S_zz.
//   5 describe_axes_kernel    : one thread per cluster: centroid, covariance, the Jacobi sweeps, the axes; the moments row and
//                               desc[0..14].
//   6 describe_extent_kernel  : per member its three coordinates along the axes; minimum and maximum as ordered uint64.
//   7 describe_finish_kernel  : one thread per cluster: lo, hi and the box centre, desc[15..23].
//
// THE WAVE-LEVEL PRE-REDUCTION (passes 2, 4, 6; wave_peel).  A frame's largest object holds a quarter of its points, and a cloud
// that comes out of a sorted grid or a scan line has long runs of one id: one atomic per lane would send most of a frame's adds
// to a handful of addresses.  So a wave goes through the distinct ids among its members, at most kPeelRounds of them, one id at
// a time: the first remaining lane's id, a ballot of the lanes that hold it.  An id held by at least kPeelMinLanes lanes is
// reduced inside the wave -- an xor-shuffle tree over the values of exactly these lanes (the others contribute the identity) --
// and then lanes 0 .. 8 issue ONE atomic wave-instruction whose lanes address consecutive words of the cluster's accumulator
// row.  The lanes of an id held by fewer lanes, and those the rounds did not reach, issue their own atomics: their ids are spread
// over many rows, and there is no contention to speak of.  A round that reduces nothing costs a ballot and a few scalar
// instructions.  Because the sums are integers and minimum / maximum are associative and commutative, every such split gives
// the same bits.
//
// THE ACCUMULATORS.  Atomics execute at the memory side and drop the line from the L2 (MI355X: every atomic request leaves the
// L2 uncached), so what is only ever touched by atomics lives apart from what the point passes READ per member: one 128-byte row
// per cluster holds the nine sums, the six box keys and m (Acc), a second array the six extent keys (Ext, 64 bytes), and the
// values the moments and extent passes gather per member -- o and 1 / h (Lat), centroid and axes (desc itself) -- are written
// once by plain stores of the per-cluster kernels in between and stay cached.
#include "pn2_common.h"
#include "pn2_eig3.h"     // jacobi_rotate, fix_sign, eig3_axes
#include "pn2_ordered.h"  // ordered_key32, ordered_to_float, ordered_key, ordered_to_double
#include "pn2_wg.h"       // finite32, blocks_of, refuse_capture, WsCarver

namespace {

constexpr int kT = 256;      // threads of every workgroup here: one point (or one cluster) per thread, no loop over chunks
constexpr int kPeelRounds = 64;   // the most distinct ids of a wave that are looked at (64: all of them)
constexpr int kPeelMinLanes = 2;  // an id held by at least this many lanes of the wave is reduced inside the wave (measured:
                                  // EXPERIMENTS.md "Object description"; a lone lane gains nothing from a reduction)
// tuning hooks (pn2_debug_set(19, v), (20, v)): the two in force; rounds = 0 is one atomic per lane always (tools/describe_cost.py)
PN2_TUNABLE(int, g_describe_rounds, kPeelRounds)
PN2_TUNABLE(int, g_describe_min_lanes, kPeelMinLanes)
struct Peel {
    int rounds, min_lanes;
};

struct alignas(128) Acc {
    long long s[9];   // S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz
    unsigned lo[3];   // ordered uint32 of the members' minimum x, y, z
    unsigned hi[3];   // ... maximum
    int m;            // members
    int Q, x;         // written by the lattice kernel
};
struct Lat {          // what the moments pass reads per member
    double o[3];
    double inv_h;     // 2^(Q - x): a multiplication by it is the division by h, both exact
};
struct alignas(64) Ext {
    unsigned long long lo[3], hi[3];  // ordered uint64 of the members' minimum / maximum coordinate along a0, a1, a2
};

struct Ws {
    Acc* acc;
    Lat* lat;
    Ext* ext;
};
inline void ws_layout(int nclusters, WsCarver& c, Ws* w) {
    const size_t C = (size_t)nclusters;
    w->acc = c.take<Acc>(C);
    w->lat = c.take<Lat>(C);
    w->ext = c.take<Ext>(C);
}

// a MEMBER of cluster c: ids[i] == c, 0 <= c < nclusters, three finite coordinates.  -> c, or -1
__device__ __forceinline__ int member_of(int n, int nclusters, const float* __restrict__ points, const int* __restrict__ ids,
                                         long long i, float* p) {
    if (i >= n) return -1;
    const int c = ids[i];
    if (c < 0 || c >= nclusters) return -1;
    p[0] = points[(size_t)i * 3];
    p[1] = points[(size_t)i * 3 + 1];
    p[2] = points[(size_t)i * 3 + 2];
    return finite32(p[0]) && finite32(p[1]) && finite32(p[2]) ? c : -1;
}

// Goes through the distinct ids among the lanes that hold one (`in`), at most peel.rounds of them: reduce(v, mine) is called,
// by the whole wave, for every id v held by at least peel.min_lanes lanes (`mine`: this lane holds it).  -> whether this lane
// is left to issue its own atomics.  The loop is wave-uniform.
template <typename F>
__device__ __forceinline__ bool wave_peel(bool in, int c, Peel peel, F&& reduce) {
    unsigned long long todo = __ballot(in);
    bool self = false;
    for (int r = 0; todo != 0ull && r < peel.rounds; ++r) {
        const int v = __shfl(c, __ffsll((long long)todo) - 1);
        const bool mine = in && c == v;
        const unsigned long long same = __ballot(mine);
        if ((int)__popcll(same) >= peel.min_lanes) reduce(v, mine); else self = self || mine;
        todo &= ~same;
    }
    return self || (in && ((todo >> (threadIdx.x & 63)) & 1ull) != 0ull);
}

template <typename T>
__device__ __forceinline__ void atomic_add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void atomic_min(T* p, T v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void atomic_max(T* p, T v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// minima only fall and maxima only rise: a stale read costs an atomic, never a result (the per-lane path)
template <typename T>
__device__ __forceinline__ void lane_min(T* p, T v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) atomic_min(p, v);
}
template <typename T>
__device__ __forceinline__ void lane_max(T* p, T v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) atomic_max(p, v);
}

__global__ void __launch_bounds__(kT)
describe_clear_kernel(int nclusters, Acc* __restrict__ acc, Ext* __restrict__ ext) {
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= nclusters) return;
    const int c = (int)at;
    Acc a;
#pragma unroll
    for (int j = 0; j < 9; ++j) a.s[j] = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = 0xFFFFFFFFu;
        a.hi[j] = 0u;
    }
    a.m = a.Q = a.x = 0;
    acc[c] = a;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ext[c].lo[j] = ~0ull;
        ext[c].hi[j] = 0ull;
    }
}

__global__ void __launch_bounds__(kT)
describe_box_kernel(int n, int nclusters, Peel peel, const float* __restrict__ points, const int* __restrict__ ids,
                    Acc* __restrict__ acc) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    float p[3] = {0.0f, 0.0f, 0.0f};
    const int c = member_of(n, nclusters, points, ids, i, p);
    const bool in = c >= 0;
    const unsigned k0 = ordered_key32(p[0]), k1 = ordered_key32(p[1]), k2 = ordered_key32(p[2]);
    const bool self = wave_peel(in, c, peel, [&](int v, bool mine) {
        const unsigned l0 = pn2_wave_all_min(mine ? k0 : 0xFFFFFFFFu), l1 = pn2_wave_all_min(mine ? k1 : 0xFFFFFFFFu),
                       l2 = pn2_wave_all_min(mine ? k2 : 0xFFFFFFFFu);
        const unsigned h0 = pn2_wave_all_max(mine ? k0 : 0u), h1 = pn2_wave_all_max(mine ? k1 : 0u), h2 = pn2_wave_all_max(mine ? k2 : 0u);
        const int count = (int)__popcll(__ballot(mine));
        Acc* a = acc + v;
        // lanes 0 .. 5: the six consecutive box words; lane 6: the count
        if (lane < 3) atomic_min(&a->lo[lane], lane == 0 ? l0 : (lane == 1 ? l1 : l2));
        else if (lane < 6) atomic_max(&a->hi[lane - 3], lane == 3 ? h0 : (lane == 4 ? h1 : h2));
        else if (lane == 6) atomic_add(&a->m, count);
    });
    if (self) {
        Acc* a = acc + c;
        lane_min(&a->lo[0], k0); lane_min(&a->lo[1], k1); lane_min(&a->lo[2], k2);
        lane_max(&a->hi[0], k0); lane_max(&a->hi[1], k1); lane_max(&a->hi[2], k2);
        atomic_add(&a->m, 1);
    }
}

// 2^e as a double, e in the normal range
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }

__global__ void __launch_bounds__(kT)
describe_lattice_kernel(int nclusters, Acc* __restrict__ acc, Lat* __restrict__ lat) {
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= nclusters) return;
    const int c = (int)at;
    Acc* a = acc + c;
    const int m = a->m;
    Lat l = {{0.0, 0.0, 0.0}, 1.0};
    if (m > 0) {
        double E = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            l.o[j] = (double)ordered_to_float(a->lo[j]);
            const double e = (double)ordered_to_float(a->hi[j]) - l.o[j];
            E = e > E ? e : E;
        }
        const int bitlen = 32 - __clz(m);
        const int Q = (62 - bitlen) >> 1 < 20 ? (62 - bitlen) >> 1 : 20;
        // E is a difference of widened float32 values: 0 or at least 2^-149, a normal double, so frexp is its exponent field
        const int x = E > 0.0 ? (int)((__double_as_longlong(E) >> 52) & 0x7FF) - 1022 : Q;
        a->Q = Q;
        a->x = x;
        l.inv_h = pow2(Q - x);  // x in [-148, 129], Q in [15, 20]: normal
    }
    lat[c] = l;
}

__global__ void __launch_bounds__(kT)
describe_moments_kernel(int n, int nclusters, Peel peel, const float* __restrict__ points, const int* __restrict__ ids,
                        const Lat* __restrict__ lat, Acc* __restrict__ acc) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    float p[3] = {0.0f, 0.0f, 0.0f};
    const int c = member_of(n, nclusters, points, ids, i, p);
    const bool in = c >= 0;
    long long s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (in) {
        const Lat l = lat[c];
        // (p - o) / h: h is a power of two and the quotient is below 2^Q, so the product with 1 / h is the same double
        const long long qx = (long long)__builtin_rint(((double)p[0] - l.o[0]) * l.inv_h);
        const long long qy = (long long)__builtin_rint(((double)p[1] - l.o[1]) * l.inv_h);
        const long long qz = (long long)__builtin_rint(((double)p[2] - l.o[2]) * l.inv_h);
        s[0] = qx; s[1] = qy; s[2] = qz;
        s[3] = qx * qx; s[4] = qx * qy; s[5] = qx * qz;
        s[6] = qy * qy; s[7] = qy * qz; s[8] = qz * qz;
    }
    const bool self = wave_peel(in, c, peel, [&](int v, bool mine) {
        long long out = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const long long r = pn2_wave_all_sum(mine ? s[j] : 0ll);
            out = lane == j ? r : out;
        }
        if (lane < 9) atomic_add(&acc[v].s[lane], out);  // one wave-instruction, nine consecutive words of one row
    });
    if (self) {
#pragma unroll
        for (int j = 0; j < 9; ++j) atomic_add(&acc[c].s[j], s[j]);
    }
}

__global__ void __launch_bounds__(kT)
describe_axes_kernel(int nclusters, int upright, const Acc* __restrict__ acc, const Lat* __restrict__ lat,
                     long long* __restrict__ moments, double* __restrict__ desc) {
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= nclusters) return;
    const int c = (int)at;
    const Acc a = acc[c];
    long long* mo = moments + (size_t)c * 12;
    double* d = desc + (size_t)c * 24;
    if (a.m == 0) {
        for (int j = 0; j < 12; ++j) mo[j] = 0;
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        for (int j = 0; j < 24; ++j) d[j] = nan;
        return;
    }
    mo[0] = a.m;
    for (int j = 0; j < 9; ++j) mo[1 + j] = a.s[j];
    mo[10] = a.Q;
    mo[11] = a.x;
    const double h = pow2(a.x - a.Q), md = (double)a.m;
    const double sx = (double)a.s[0] / md, sy = (double)a.s[1] / md, sz = (double)a.s[2] / md;
    d[0] = lat[c].o[0] + sx * h;
    d[1] = lat[c].o[1] + sy * h;
    d[2] = lat[c].o[2] + sz * h;
    double a00 = (double)a.s[3] / md - sx * sx, a01 = (double)a.s[4] / md - sx * sy, a02 = (double)a.s[5] / md - sx * sz;
    double a11 = (double)a.s[6] / md - sy * sy, a12 = (double)a.s[7] / md - sy * sz, a22 = (double)a.s[8] / md - sz * sz;
    double e0[3], e1[3], e2[3], lam[3];
    if (upright) {
        double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0};  // the first two COLUMNS of V
        const double azz = a22;
        jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
        const bool swap = a00 < a11;  // descending, equal values keep the lower column first
        lam[0] = swap ? a11 : a00;
        lam[1] = swap ? a00 : a11;
        lam[2] = azz;
        for (int i = 0; i < 3; ++i) e0[i] = swap ? v1[i] : v0[i];
        fix_sign(e0);
        e1[0] = -e0[1]; e1[1] = e0[0]; e1[2] = 0.0;
        e2[0] = 0.0; e2[1] = 0.0; e2[2] = 1.0;
    } else {
        eig3_axes(a00, a01, a02, a11, a12, a22, lam, e0, e1, e2);
    }
    const double hh = h * h;
    for (int i = 0; i < 3; ++i) {
        d[3 + i] = lam[i] * hh;
        d[6 + i] = e0[i];
        d[9 + i] = e1[i];
        d[12 + i] = e2[i];
    }
}

__global__ void __launch_bounds__(kT)
describe_extent_kernel(int n, int nclusters, Peel peel, const float* __restrict__ points, const int* __restrict__ ids,
                       const double* __restrict__ desc, Ext* __restrict__ ext) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    float p[3] = {0.0f, 0.0f, 0.0f};
    const int c = member_of(n, nclusters, points, ids, i, p);
    const bool in = c >= 0;
    unsigned long long k[3] = {0ull, 0ull, 0ull};
    if (in) {
        const double* d = desc + (size_t)c * 24;
        const double dx = (double)p[0] - d[0], dy = (double)p[1] - d[1], dz = (double)p[2] - d[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) k[j] = ordered_key((d[6 + 3 * j] * dx + d[7 + 3 * j] * dy) + d[8 + 3 * j] * dz);
    }
    const bool self = wave_peel(in, c, peel, [&](int v, bool mine) {
        unsigned long long out = 0ull;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned long long lo = pn2_wave_all_min(mine ? k[j] : ~0ull), hi = pn2_wave_all_max(mine ? k[j] : 0ull);
            out = lane == j ? lo : (lane == 3 + j ? hi : out);
        }
        Ext* e = ext + v;
        if (lane < 3) atomic_min(&e->lo[lane], out);
        else if (lane < 6) atomic_max(&e->hi[lane - 3], out);
    });
    if (self) {
        Ext* e = ext + c;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            lane_min(&e->lo[j], k[j]);
            lane_max(&e->hi[j], k[j]);
        }
    }
}

__global__ void __launch_bounds__(kT)
describe_finish_kernel(int nclusters, const Acc* __restrict__ acc, const Ext* __restrict__ ext, double* __restrict__ desc) {
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= nclusters || acc[at].m == 0) return;  // a cluster without members: the axes kernel left a row of NaNs
    const int c = (int)at;
    double* d = desc + (size_t)c * 24;
    double g[3];
    for (int j = 0; j < 3; ++j) {
        const double lo = ordered_to_double(ext[c].lo[j]), hi = ordered_to_double(ext[c].hi[j]);
        d[15 + j] = lo;
        d[18 + j] = hi;
        g[j] = 0.5 * (lo + hi);
    }
    for (int j = 0; j < 3; ++j) d[21 + j] = d[j] + ((d[6 + j] * g[0] + d[9 + j] * g[1]) + d[12 + j] * g[2]);
}

// one thread per sample: point t = (cluster * 12 + edge) * per_edge + s
__global__ void __launch_bounds__(kT)
box_wireframe_kernel(int total, int per_edge, const double* __restrict__ desc, float* __restrict__ points, int* __restrict__ owner) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (t >= total) return;
    const int s = (int)(t % per_edge), edge = (int)((t / per_edge) % 12), c = (int)(t / per_edge / 12);
    const double* d = desc + (size_t)c * 24;
    // edge = 4 k + v: it runs along axis k; v holds the other two bits, the lower axis in its lower bit
    const int k = edge >> 2, v = edge & 3;
    const int u = k == 0 ? 1 : 0, w = k == 2 ? 1 : 2;
    const int ca = ((v & 1) << u) | ((v >> 1) << w), cb = ca | (1 << k);
    const double f = (double)s / (double)(per_edge - 1);
    for (int a = 0; a < 3; ++a) {
        double corner[2];
        for (int side = 0; side < 2; ++side) {
            const int j = side ? cb : ca;
            const double e0 = (j & 1) ? d[18] : d[15], e1 = (j & 2) ? d[19] : d[16], e2 = (j & 4) ? d[20] : d[17];
            corner[side] = d[a] + ((d[6 + a] * e0 + d[9 + a] * e1) + d[12 + a] * e2);
        }
        points[(size_t)t * 3 + a] = (float)(corner[0] + (corner[1] - corner[0]) * f);
    }
    owner[t] = c;
}

}  // namespace

#ifdef PN2_TUNING_HOOKS
extern "C" int pn2_debug_set_describe(int what, int value) {
    if (what == 19 && value >= 0 && value <= 64) { g_describe_rounds = value; return 0; }
    if (what == 20 && value >= 1 && value <= 64) { g_describe_min_lanes = value; return 0; }
    return -1;
}
#endif

extern "C" int pn2_cluster_describe_workspace_size(int nclusters, unsigned long long* bytes) {
    if (nclusters <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    ws_layout(nclusters, c, &w);
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_cluster_describe(int n, int nclusters, const float* points, const int* ids, int upright, long long* moments,
                                    double* desc, void* workspace, size_t workspace_bytes, void* stream) {
    if (n <= 0 || nclusters <= 0 || (upright != 0 && upright != 1)) return PN2_EINVAL;
    if (nclusters > n) return PN2_ERANGE;
    if (!points || !ids || !moments || !desc || !workspace) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)ids) & 3) != 0 || (((uintptr_t)moments | (uintptr_t)desc) & 7) != 0 ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    ws_layout(nclusters, c, &w);
    if (!c.fits()) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // capturable by construction, but nothing captures it yet: refused until a change lifts this together with a capture test
    if (const int refused = refuse_capture(st)) return refused;

    const Peel peel = {g_describe_rounds, g_describe_min_lanes};
    const int pblocks = blocks_of(n, kT), cblocks = blocks_of(nclusters, kT);
    describe_clear_kernel<<<cblocks, kT, 0, st>>>(nclusters, w.acc, w.ext);
    describe_box_kernel<<<pblocks, kT, 0, st>>>(n, nclusters, peel, points, ids, w.acc);
    describe_lattice_kernel<<<cblocks, kT, 0, st>>>(nclusters, w.acc, w.lat);
    describe_moments_kernel<<<pblocks, kT, 0, st>>>(n, nclusters, peel, points, ids, w.lat, w.acc);
    PN2_RETURN_IF_LAUNCH_FAILED();
    describe_axes_kernel<<<cblocks, kT, 0, st>>>(nclusters, upright, w.acc, w.lat, moments, desc);
    describe_extent_kernel<<<pblocks, kT, 0, st>>>(n, nclusters, peel, points, ids, desc, w.ext);
    describe_finish_kernel<<<cblocks, kT, 0, st>>>(nclusters, w.acc, w.ext, desc);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_box_wireframe(int nclusters, const double* desc, int per_edge, float* points, int* owner, void* stream) {
    if (nclusters <= 0 || per_edge < 2) return PN2_EINVAL;
    const long long total = (long long)nclusters * 12 * per_edge;
    if (total >= (1ll << 31)) return PN2_ERANGE;
    if (!desc || !points || !owner) return PN2_ENULL;
    if (((uintptr_t)desc & 7) != 0 || (((uintptr_t)points | (uintptr_t)owner) & 3) != 0) return PN2_EINVAL;
    box_wireframe_kernel<<<blocks_of(total, kT), kT, 0, static_cast<hipStream_t>(stream)>>>((int)total, per_edge, desc, points, owner);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
