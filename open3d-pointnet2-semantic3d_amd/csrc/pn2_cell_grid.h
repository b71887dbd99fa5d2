// pn2_cell_grid.h -- the sorted-key cell grid of the per-point neighbourhood passes (pn2_cluster.hip, pn2_neighbors.hip,
// pn2_icp.hip), whole and in one copy.  Device half: the reset of the grid's scalars, the minimum of the valid points, the 63-bit
// cell key of every point, the gather of the sorted points into 16-byte rows, the key helpers, the search in the sorted keys and
// the walk over the rows around a cell.  Host half: CellGrid, which carves the grid's share of a caller's workspace and whose
// build() queues grid_min_kernel, grid_key_kernel, one radix sort (pn2_sort.h) of (key, point index) pairs on key bits [0, 64)
// and grid_gather_kernel, at the cell edge below.  A caller carves its scalars (a struct derived from GridScal) and its own
// arrays around it, resets the scalars in its init kernel (grid_scal_reset, then its own fields) and calls build() behind that
// launch: no file but this one names a grid kernel in a launch.
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
// THE WALK.  x is the lowest key field, so the three cells (cx-1 .. cx+1) of a row (y, z) are one range of the sorted keys.
// grid_walk_rows visits the first `nrows` of the nine rows around (cy, cz) in the order z = cz-1 + r/3, y = cy-1 + r%3, and of
// each only the sorted positions below `end`:
//   pn2_cluster.hip    (nrows = 5, end = the lane's own sorted position would be the rows IN FRONT of the point, its own up to
//                      itself; cluster_union_kernel keeps that loop written out: through the walker it measured 4 % slower)
//   pn2_neighbors.hip  nrows = 9, end = n (its lane path; the wave-uniform path searches the same rows with row_key / cell_in)
//   pn2_icp.hip        nrows = 9, end = nt, around the cell of a source point, which may lie one cell outside the grid
//
// Everything here has internal linkage: each including file gets its own kernels, under the same names.
#pragma once
#include "pn2_common.h"   // pn2_wave_umin
#include "pn2_ordered.h"  // ordered_key32, ordered_to_float
#include "pn2_sort.h"     // IndexSort
#include "pn2_wg.h"       // point_valid, blocks_of, WsCarver

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

// by one thread of a caller's init kernel, which sets its own fields behind it
__device__ __forceinline__ void grid_scal_reset(GridScal* __restrict__ s) {
    s->min_key[0] = s->min_key[1] = s->min_key[2] = 0xFFFFFFFFu;
    s->status = s->nvalid = 0;
}

__global__ void __launch_bounds__(kT)
grid_min_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, GridScal* __restrict__ s) {
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
grid_key_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, double h, GridScal* __restrict__ s,
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

// the sorted points as (x, y, z, w) rows; w = the point's original index (index_w) or its label (0 without labels)
__global__ void __launch_bounds__(kT)
grid_gather_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, const int* __restrict__ order,
                   bool index_w, float4* __restrict__ spts) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (t >= n) return;
    const int i = order[t];
    const float* p = points + (size_t)i * 3;
    spts[t] = make_float4(p[0], p[1], p[2], __int_as_float(index_w ? i : (labels ? labels[i] : 0)));
}

// ---- the key ---------------------------------------------------------------------------------------------------------------------
struct Cell {
    int x, y, z;
};
__device__ __forceinline__ Cell key_cell(unsigned long long key) {
    return {(int)(key & (kCellLimit - 1)), (int)((key >> kCellBits) & (kCellLimit - 1)),
            (int)((key >> (2 * kCellBits)) & (kCellLimit - 1))};
}
__device__ __forceinline__ unsigned long long row_key(int y, int z) {
    return ((unsigned long long)z << (2 * kCellBits)) | ((unsigned long long)y << kCellBits);
}
__device__ __forceinline__ bool cell_in(int c) { return c >= 0 && c < kCellLimit; }

// first t in [0, hi) with keys[t] >= k
__device__ __forceinline__ int lower_bound_key(const unsigned long long* __restrict__ keys, int hi, unsigned long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// THE WALK of the head comment, by one lane: visit(u, spts[u]) for every sorted position u < end in the cells cx-1 .. cx+1 of the
// rows r = 0 .. nrows-1 around (cy, cz), ascending within a row.  Rows outside the grid are skipped; x is clamped to the grid, so
// a cell one step outside it (cx = -1 or 2^21: pn2_icp.hip) still reaches the edge cells it touches.  One binary search and one
// stream of 16-byte loads per row.
template <typename Visit>
__device__ __forceinline__ void grid_walk_rows(const unsigned long long* __restrict__ keys, int end, const float4* __restrict__ spts,
                                               int cx, int cy, int cz, int nrows, Visit visit) {
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < kCellLimit - 1 ? cx + 1 : kCellLimit - 1;
    for (int r = 0; r < nrows; ++r) {
        const int z = cz - 1 + r / 3, y = cy - 1 + r % 3;
        if (!cell_in(z) || !cell_in(y)) continue;
        const unsigned long long row = row_key(y, z);
        const unsigned long long klo = row | (unsigned long long)x0, khi = row | (unsigned long long)x1;
        for (int u = lower_bound_key(keys, end, klo); u < end && keys[u] <= khi; ++u) visit(u, spts[u]);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The grid's share of a workspace and the launches that fill it.  A caller's ws_layout takes its scalars, calls carve(), takes
// its own arrays and ends with carve_tmp() (pn2_sort.h: the library's temporary storage is the last piece of a carve).
struct CellGrid {
    IndexSort<unsigned long long> sort;
    float4* spts;  // the sorted points

    void carve(WsCarver& c, size_t n) {
        sort.carve(c, n);
        spts = c.take<float4>(n);
    }
    int carve_tmp(WsCarver& c, int n) { return sort.carve_tmp(c, n, 0, 64); }

    const unsigned long long* keys() const { return sort.keys_out; }  // sorted; kInvalidKey last
    const int* order() const { return sort.vals_out; }                 // the original index of each sorted position

    // the cell edge of the head comment
    static double edge(float eps) { return (double)eps * (1.0 + 1.0 / 1048576.0); }

    // min, key, sort, gather on `st`, behind the caller's init kernel (scal reset).  PN2_OK or a hipError_t.
    int build(int n, const float* points, const int* labels, float eps, bool index_w, GridScal* scal, hipStream_t st) const {
        const int blocks = blocks_of(n, kT);
        grid_min_kernel<<<blocks, kT, 0, st>>>(n, points, labels, scal);
        grid_key_kernel<<<blocks, kT, 0, st>>>(n, points, labels, edge(eps), scal, sort.keys_in, sort.vals_in);
        PN2_RETURN_IF_LAUNCH_FAILED();
        const hipError_t e = sort.run(n, 0, 64, st);
        if (e != hipSuccess) return (int)e;
        grid_gather_kernel<<<blocks, kT, 0, st>>>(n, points, labels, sort.vals_out, index_w, spts);
        return PN2_OK;
    }
};

}  // namespace
