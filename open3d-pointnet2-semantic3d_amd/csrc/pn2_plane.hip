// pn2_plane.hip -- plane segmentation by random sample consensus: the dominant plane of a cloud (the ground of a LiDAR frame, a
// floor, a facade), and the score of any set of plane hypotheses.  The rules are in include/pn2_abi.h ("Plane segmentation");
// tests/plane_ref.py is their numpy model, and everything here is compared with it for equality.
//
// pn2_plane_score queues
//   1 plane_clear_kernel   : counts[t] = 0.
//   2 plane_score_kernel   : a lane owns one plane -- its six doubles, thr2*nn and its count stay in registers -- and a workgroup
//                            256 planes.  The workgroup stages a chunk of kChunk points in LDS as doubles, an invalid point as
//                            NaNs (every comparison with it is false), and every lane then reads the SAME point per step: an LDS
//                            broadcast, no reduction inside the loop.  A workgroup walks the chunks blockIdx.y, + gridDim.y, ...
//                            and adds its count with one atomicAdd per lane at the end: integer adds, so nothing depends on the
//                            order of arrival.
// pn2_plane_ransac queues, with no allocation and no synchronisation:
//   1 plane_flag_kernel    : per block of 256 points the number of valid ones.
//   2 plane_offsets_kernel : one workgroup: the exclusive prefix of the block counts (chunks of 256 with a running carry, so any
//                            number of blocks); V; the scalars of the selection cleared.
//   3 plane_compact_kernel : valid[block offset + place in the block] = i (pn2_wg.h's scan): ascending point indices.
//   4 plane_hypo_kernel    : trial t -> its three ranks, the plane through the three points; a void plane, and one the axis
//                            constraint excludes, is stored as six zeros (nn == 0: it scores 0).  The non-void ones are counted.
//   5 the two kernels of pn2_plane_score over the trials.
//   6 plane_select_kernel  : atomicMax over (count << 32) | (0xFFFFFFFF - t): the largest count, the lowest t among equals.  A
//                            non-void trial scores at least 1 (its origin A is a valid point with e == 0, and 0 <= thr2*nn), a
//                            void one 0, so the trials with a count above 0 are the non-void ones.
//   7 plane_finish_kernel  : one lane: status, header, the oriented (a,b,c,d); the winner's six doubles for the mask.
//   8 plane_mask_kernel    : inlier[i] for every i.
// Every step after 2 reads V (and 7, 8 the status) from the workspace: a cloud with V < 3 or without a non-void trial runs the
// same launches and writes the outputs of its status.
#include "pn2_common.h"
#include "pn2_rng.h"
#include "pn2_wg.h"  // wg_excl_scan_flag, wg_excl_scan_int, finite64, point_valid, blocks_of, refuse_capture, WsCarver

namespace {

constexpr int kT = 256;        // threads of every workgroup here; planes per workgroup; points per scan block
constexpr int kW = kT / 64;
constexpr int kChunk = 1024;   // points staged per pass of the scoring kernel: 3 * 8 * 1024 = 24 KiB of LDS
constexpr int kScoreBlocks = 2048;  // the scoring grid aims at this many workgroups: 8 per CU
constexpr int kMaxTrials = 1 << 20;
constexpr int kMaxPlanes = 1 << 24;  // of one pn2_plane_score call
constexpr unsigned long long kRankTag = 1ull << 45;  // pn2_rng.h's index table

// the scalars of one pn2_plane_ransac call, at the head of the workspace
struct Scal {
    unsigned long long best;  // (count << 32) | (0xFFFFFFFF - t) of the winner, 0 without one
    int nvalid;
    int nonvoid;
    int status;
    double win[6];            // the winner's plane as scored
};

struct Ws {  // workspace carve-up
    Scal* scal;
    int *bcount, *valid;
    double* planes;
    int* counts;
};
inline size_t ws_layout(int n, int trials, unsigned char* base, Ws* w) {
    WsCarver c{base};
    w->scal = c.take<Scal>(1);
    w->bcount = c.take<int>((size_t)blocks_of(n, kT));
    w->valid = c.take<int>((size_t)n);
    w->planes = c.take<double>((size_t)trials * 6);
    w->counts = c.take<int>((size_t)trials);
    return c.used;
}

// nn of a plane when it is not void, -1 otherwise
__device__ __forceinline__ double plane_nn(double a, double b, double c) {
    const double nn = (a * a + b * b) + c * c;
    return finite64(nn) && nn > 0.0 ? nn : -1.0;
}

__device__ __forceinline__ bool plane_inlier(const double* __restrict__ pl, double lim, double x, double y, double z) {
    const double e = (pl[3] * (x - pl[0]) + pl[4] * (y - pl[1])) + pl[5] * (z - pl[2]);
    return e * e <= lim;
}

// ---- scoring -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) plane_clear_kernel(int nplanes, int* __restrict__ counts) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t < nplanes) counts[t] = 0;
}

__global__ void __launch_bounds__(kT)
plane_score_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, int nplanes,
                   const double* __restrict__ planes, double thr2, int nchunks, int* __restrict__ counts) {
    __shared__ double sx[kChunk], sy[kChunk], sz[kChunk];
    const int t = blockIdx.x * kT + threadIdx.x;
    double x0 = 0.0, y0 = 0.0, z0 = 0.0, a = 0.0, b = 0.0, c = 0.0;
    double lim = -1.0;  // a void plane: e*e is >= 0 or NaN, never <= -1
    if (t < nplanes) {
        const double* pl = planes + (size_t)t * 6;
        x0 = pl[0]; y0 = pl[1]; z0 = pl[2]; a = pl[3]; b = pl[4]; c = pl[5];
        const double nn = plane_nn(a, b, c);
        if (nn > 0.0) lim = thr2 * nn;
    }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int cnt = 0;
    for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        const long long base = (long long)chunk * kChunk;
        const int m = (int)((long long)n - base < kChunk ? (long long)n - base : kChunk);  // >= 1: chunk < nchunks
        __syncthreads();  // the pass before has read the stage
        for (int j = threadIdx.x; j < m; j += kT) {
            const long long i = base + j;
            const float* p = points + (size_t)i * 3;
            const float x = p[0], y = p[1], z = p[2];  // read once: the rule of point_valid on the values
            const bool ok = finite32(x) && finite32(y) && finite32(z) && (!labels || labels[i] >= 0);
            sx[j] = ok ? (double)x : nan;
            sy[j] = ok ? (double)y : nan;
            sz[j] = ok ? (double)z : nan;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double e = (a * (sx[j] - x0) + b * (sy[j] - y0)) + c * (sz[j] - z0);
            cnt += e * e <= lim ? 1 : 0;
        }
    }
    if (t < nplanes && cnt != 0) atomicAdd(counts + t, cnt);
}

inline void launch_score(int n, const float* points, const int* labels, int nplanes, const double* planes, float thr, int* counts,
                         hipStream_t st) {
    const int gx = (nplanes + kT - 1) / kT;  // nplanes <= kMaxPlanes: no overflow here or in the kernels' plane index
    const int nchunks = (int)(((long long)n + kChunk - 1) / kChunk);
    int gy = (kScoreBlocks + gx - 1) / gx;  // <= kScoreBlocks: inside the limit of a grid's y
    if (gy > nchunks) gy = nchunks;
    plane_clear_kernel<<<gx, kT, 0, st>>>(nplanes, counts);
    plane_score_kernel<<<dim3(gx, gy), kT, 0, st>>>(n, points, labels, nplanes, planes, (double)thr * (double)thr, nchunks, counts);
}

// ---- RANSAC --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
plane_flag_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, int* __restrict__ bcount) {
    __shared__ int wsum[kW];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    int total;
    wg_excl_scan_flag<kW>(i < n && point_valid(points, labels, i) ? 1 : 0, wsum, total);
    if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

// one workgroup: bcount -> its exclusive prefix, in chunks of kT with a running carry; the scalars
__global__ void __launch_bounds__(kT) plane_offsets_kernel(int nblocks, int* __restrict__ bcount, Scal* __restrict__ s) {
    __shared__ int wsum[kW];
    int carry = 0;
    for (int base = 0; base < nblocks; base += kT) {
        const int b = base + (int)threadIdx.x;
        const int v = b < nblocks ? bcount[b] : 0;
        int total;
        const int before = wg_excl_scan_int<kW>(v, wsum, total);
        if (b < nblocks) bcount[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        s->best = 0ull;
        s->nvalid = carry;
        s->nonvoid = 0;
        s->status = 0;
    }
}

__global__ void __launch_bounds__(kT)
plane_compact_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, const int* __restrict__ boffset,
                     int* __restrict__ valid) {
    __shared__ int wsum[kW];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool ok = i < n && point_valid(points, labels, i);
    int total;
    const int before = wg_excl_scan_flag<kW>(ok ? 1 : 0, wsum, total);
    if (ok) valid[boffset[blockIdx.x] + before] = (int)i;  // < V <= n
}

// the point index of sample point j of trial t; V >= 1
__device__ __forceinline__ int sample_index(unsigned long long h, int t, int j, int V, const int* __restrict__ valid) {
    const unsigned long long r = draw64(h, kRankTag + 3ull * (unsigned long long)t + (unsigned long long)j) % (unsigned long long)V;
    return valid[r];
}

struct Axis {
    double x, y, z, cos2;
    int on;
};

__global__ void __launch_bounds__(kT)
plane_hypo_kernel(int trials, unsigned long long seed, const float* __restrict__ points, const int* __restrict__ valid, Axis axis,
                  Scal* __restrict__ s, double* __restrict__ planes) {
    const int t = blockIdx.x * kT + threadIdx.x;
    const int V = s->nvalid;
    bool live = false;
    if (t < trials) {
        double pl[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (V >= 3) {
            const unsigned long long h = sample_stream(seed, 0ull, 0);
            const float* A = points + (size_t)sample_index(h, t, 0, V, valid) * 3;
            const float* B = points + (size_t)sample_index(h, t, 1, V, valid) * 3;
            const float* C = points + (size_t)sample_index(h, t, 2, V, valid) * 3;
            const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
            const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
            const double vx = (double)C[0] - ax, vy = (double)C[1] - ay, vz = (double)C[2] - az;
            const double a = uy * vz - uz * vy, b = uz * vx - ux * vz, c = ux * vy - uy * vx;
            const double nn = plane_nn(a, b, c);
            live = nn > 0.0;
            if (live && axis.on) {
                const double dt = (a * axis.x + b * axis.y) + c * axis.z;
                live = dt * dt >= (axis.cos2 * nn) * ((axis.x * axis.x + axis.y * axis.y) + axis.z * axis.z);
            }
            if (live) { pl[0] = ax; pl[1] = ay; pl[2] = az; pl[3] = a; pl[4] = b; pl[5] = c; }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) planes[(size_t)t * 6 + k] = pl[k];
    }
    const unsigned long long bal = __ballot(live);
    if (bal != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&s->nonvoid, __popcll(bal));
}

__global__ void __launch_bounds__(kT) plane_select_kernel(int trials, const int* __restrict__ counts, Scal* __restrict__ s) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t >= trials) return;
    const int cnt = counts[t];
    if (cnt > 0) atomicMax(&s->best, ((unsigned long long)(unsigned)cnt << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t));
}

__global__ void plane_finish_kernel(unsigned long long seed, const int* __restrict__ valid, const double* __restrict__ planes,
                                    Axis axis, Scal* __restrict__ s, double* __restrict__ plane, int* __restrict__ header) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int V = s->nvalid;
    const unsigned long long best = s->best;
    const int status = V < 3 ? 1 : (best == 0ull ? 2 : 0);
    s->status = status;
    header[0] = status;
    header[6] = V;
    header[7] = s->nonvoid;
    if (status != 0) {
        header[1] = 0; header[2] = 0; header[3] = -1; header[4] = -1; header[5] = -1;
        plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s->win[k] = 0.0;
        return;
    }
    const int t = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    header[1] = (int)(best >> 32);
    header[2] = t;
    const unsigned long long h = sample_stream(seed, 0ull, 0);
#pragma unroll
    for (int j = 0; j < 3; ++j) header[3 + j] = sample_index(h, t, j, V, valid);
    const double* pl = planes + (size_t)t * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) s->win[k] = pl[k];
    double a = pl[3], b = pl[4], c = pl[5];
    double d = -((a * pl[0] + b * pl[1]) + c * pl[2]);
    bool flip;
    if (axis.on) flip = (a * axis.x + b * axis.y) + c * axis.z < 0.0;
    else flip = c != 0.0 ? c < 0.0 : (b != 0.0 ? b < 0.0 : a < 0.0);
    if (flip) { a = -a; b = -b; c = -c; d = -d; }
    plane[0] = a; plane[1] = b; plane[2] = c; plane[3] = d;
}

__global__ void __launch_bounds__(kT)
plane_mask_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, double thr2, const Scal* __restrict__ s,
                  unsigned char* __restrict__ inlier) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    bool in = false;
    if (s->status == 0 && point_valid(points, labels, i)) {
        const double* pl = s->win;
        const float* p = points + (size_t)i * 3;
        in = plane_inlier(pl, thr2 * ((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5]), (double)p[0], (double)p[1], (double)p[2]);
    }
    inlier[i] = in ? 1 : 0;
}

inline bool thr_ok(float thr) { return thr > 0.0f && thr <= 3.402823466e38f; }

}  // namespace

extern "C" int pn2_plane_score(int n, const float* points, const int* labels, int nplanes, const double* planes, float thr,
                               int* counts, void* stream) {
    if (n < 1 || nplanes < 1 || nplanes > kMaxPlanes || !thr_ok(thr)) return PN2_EINVAL;
    if (!points || !planes || !counts) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)labels | (uintptr_t)counts) & 3) != 0 || ((uintptr_t)planes & 7) != 0) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = refuse_capture(st);  // allocation-free and capturable, but nothing captures it yet: include/pn2_abi.h
    if (rc != PN2_OK) return rc;
    launch_score(n, points, labels, nplanes, planes, thr, counts, st);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_plane_workspace_size(int n, int trials, unsigned long long* bytes) {
    if (n < 1 || trials < 1 || trials > kMaxTrials) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    Ws w;
    *bytes = (unsigned long long)ws_layout(n, trials, nullptr, &w);
    return PN2_OK;
}

extern "C" int pn2_plane_ransac(int n, const float* points, const int* labels, float thr, int trials, unsigned long long seed,
                                const double* axis, double cos2, unsigned char* inlier, double* plane, int* header, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (n < 1 || trials < 1 || trials > kMaxTrials || !thr_ok(thr)) return PN2_EINVAL;
    Axis ax = {0.0, 0.0, 0.0, 0.0, 0};
    if (axis) {
        if (!(cos2 >= 0.0 && cos2 <= 1.0)) return PN2_EINVAL;
        const double big = 1.7976931348623157e308;
        for (int k = 0; k < 3; ++k)
            if (!(axis[k] >= -big && axis[k] <= big)) return PN2_EINVAL;
        if (axis[0] == 0.0 && axis[1] == 0.0 && axis[2] == 0.0) return PN2_EINVAL;
        ax = {axis[0], axis[1], axis[2], cos2, 1};
    }
    if (!points || !inlier || !plane || !header || !workspace) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)labels | (uintptr_t)header) & 3) != 0 || ((uintptr_t)plane & 7) != 0 ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    Ws w;
    if (workspace_bytes < ws_layout(n, trials, static_cast<unsigned char*>(workspace), &w)) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = refuse_capture(st);  // as pn2_plane_score
    if (rc != PN2_OK) return rc;

    const int blocks = blocks_of(n, kT), tblocks = blocks_of(trials, kT);

    plane_flag_kernel<<<blocks, kT, 0, st>>>(n, points, labels, w.bcount);
    plane_offsets_kernel<<<1, kT, 0, st>>>(blocks, w.bcount, w.scal);
    plane_compact_kernel<<<blocks, kT, 0, st>>>(n, points, labels, w.bcount, w.valid);
    plane_hypo_kernel<<<tblocks, kT, 0, st>>>(trials, seed, points, w.valid, ax, w.scal, w.planes);
    PN2_RETURN_IF_LAUNCH_FAILED();
    launch_score(n, points, labels, trials, w.planes, thr, w.counts, st);
    plane_select_kernel<<<tblocks, kT, 0, st>>>(trials, w.counts, w.scal);
    plane_finish_kernel<<<1, 64, 0, st>>>(seed, w.valid, w.planes, ax, w.scal, plane, header);
    plane_mask_kernel<<<blocks, kT, 0, st>>>(n, points, labels, (double)thr * (double)thr, w.scal, inlier);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
