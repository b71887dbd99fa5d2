// pn2_cell_grid.h -- the sorted-key cell grid of the per-point neighbourhood passes (pn2_cluster.hip, pn2_neighbors.hip, pn2_icp.hip), in one
// copy: the minimum of the valid points, the 63-bit cell key of every point, and the search in the sorted keys.  The host half
// of a caller queues  its own init kernel (GridScal's fields as cluster_init_kernel sets them), cluster_min_kernel,
// cluster_key_kernel and one radix sort (pn2_sort.h) of (key, point index) pairs on key bits [0, 64).
//
// THE GRID.  h = eps * (1 + 2^-20) in float64, cell = floor(((double)x - (double)min_x) / h) per axis.  Why two points that pass
// the link test are never two cells apart on an axis: the test (dx*dx + dy*dy) + dz*dz <= eps*eps in float64 bounds |dx| by
// eps * (1 + 2^-51) (three roundings of 2^-53 each on the left, one on the right).  With a = x - min_x exact, the computed
// quotient q carries two roundings (the subtraction, the division): |q - a/h| <= 2.01 * 2^-53 * a/h, and a/h < 2^21 for every
// point that is not refused with status 1, so the error of a quotient is below 2^-31.  Then
//     q_i - q_j <= (a_i - a_j)/h + 2^-30 <= (1 + 2^-51) / (1 + 2^-20) + 2^-30 < 1 - 2^-21 < 1,
// and two numbers less than 1 apart have floors at most 1 apart.  (The hair is 2^-20, nine orders of magnitude above what the
// roundings need, and costs a 27-cell volume one part in 350 000.)
//
// Everything here has internal linkage: each including file gets its own kernels, under the same names.
#pragma once
#include "pn2_common.h"   // pn2_wave_umin
#include "pn2_ordered.h"  // ordered_key32, ordered_to_float
#include "pn2_wg.h"       // point_valid

namespace {

constexpr int kT = 256;            // threads of every workgroup here; also the scan block (points per block count)
constexpr int kW = kT / 64;
constexpr int kCellBits = 21;
constexpr int kCellLimit = 1 << kCellBits;
constexpr unsigned long long kInvalidKey = ~0ull;

// the grid's scalars of one call, at the head of the workspace (a caller's own scalars follow them: it derives from this)
struct GridScal {
    unsigned min_key[3];  // ordered uint32 of the minimum x, y, z over the valid points
    int status;
    int nvalid;
};

__global__ void __launch_bounds__(kT)
cluster_min_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, GridScal* __restrict__ s) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool ok = i < n && point_valid(points, labels, i);
    unsigned k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
    if (ok) {
        const float* p = points + (size_t)i * 3;
        k0 = ordered_key32(p[0]);
        k1 = ordered_key32(p[1]);
        k2 = ordered_key32(p[2]);
    }
    const unsigned long long bal = __ballot(ok);
    k0 = pn2_wave_umin(k0);
    k1 = pn2_wave_umin(k1);
    k2 = pn2_wave_umin(k2);
    if (bal != 0ull && (threadIdx.x & 63) == 0) {
        atomicMin(&s->min_key[0], k0);
        atomicMin(&s->min_key[1], k1);
        atomicMin(&s->min_key[2], k2);
        atomicAdd(&s->nvalid, __popcll(bal));
    }
}

__global__ void __launch_bounds__(kT)
cluster_key_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, double h, GridScal* __restrict__ s,
                   unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    unsigned long long key = kInvalidKey;
    if (point_valid(points, labels, i)) {
        const float* p = points + (size_t)i * 3;
        key = 0ull;
        bool far = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // >= 0: the minimum is the least of them and the subtraction is monotone
            const double q = __builtin_floor(((double)p[a] - (double)ordered_to_float(s->min_key[a])) / h);
            const bool in = q < (double)kCellLimit;  // tested in floating point before the conversion
            far = far || !in;
            key |= (unsigned long long)(in ? (long long)q : (long long)(kCellLimit - 1)) << (kCellBits * a);
        }
        if (far) atomicMax(&s->status, 1);
    }
    keys[i] = key;
    vals[i] = (int)i;
}

// first t in [0, hi) with keys[t] >= k
__device__ __forceinline__ int lower_bound_key(const unsigned long long* __restrict__ keys, int hi, unsigned long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace
