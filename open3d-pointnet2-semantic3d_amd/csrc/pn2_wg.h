// pn2_wg.h -- the workgroup primitives of the data-path kernels (pn2_scene.hip, pn2_dataset.hip, pn2_frame.hip, pn2_tile.hip,
// pn2_store.hip, pn2_cluster.hip, pn2_plane.hip, pn2_describe.hip, pn2_neighbors.hip, pn2_icp.hip) and the workspace carving of every host half that takes a
// workspace (those, and pn2_text.hip, pn2_scene_io.hip, pn2_grid_knn.h, pn2_fps_bucket.hip, pn2_augment.hip; pn2_sort.h carves the
// radix sort's share, pn2_cell_grid.h the cell grid's), and the prologue of the eager entry points: the block count
// (pn2_cluster.hip, pn2_neighbors.hip, pn2_icp.hip, pn2_plane.hip, pn2_describe.hip, pn2_cell_grid.h), the finite test of a host
// argument (pn2_neighbors.hip, pn2_icp.hip, pn2_tile.hip) and the refusal of a capturing stream (the first five).
// One copy of each.
//
// W is the number of waves of the CALLING workgroup (its threads / 64): a template parameter, because every file names its own
// thread count.  Every thread of the workgroup must reach a call (they hold barriers).
//
// The LDS contract, once: a scan or a sum takes an array of W elements (`wsum`, `red`) and holds TWO barriers -- one between the
// waves' stores and everybody's reads, one after the reads.  The second is what makes the array reusable: the next call, whose
// first act is a store into the same array, may follow at once.  wg_min3_stage holds only the first: its callers read smin
// afterwards and do not write it again.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/pn2_abi.h"  // PN2_OK, PN2_EUNSUP
#include "pn2_wave.h"

// ---- scans and sums ----------------------------------------------------------------------------------------------------------
// exclusive prefix of per-thread flags over the workgroup (thread order); `total` = workgroup sum.  wsum: W ints.
// The flag is an int on purpose (non-zero = set): taken as a bool, a flag formed inside a divergent branch stays a lane mask that
// is turned into a value and back behind the branch, on the serial path of every pass of scene_extract_kernel's slab loop
// (EXPERIMENTS.md: 4 to 5 us on a 0.53 ms batch)
template <int W>
__device__ __forceinline__ int wg_excl_scan_flag(int flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int v = wsum[w];
        if (w < wave) base += v;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return base + before;
}

// the same for per-thread counts
template <int W>
__device__ __forceinline__ int wg_excl_scan_int(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// workgroup sum of a per-thread value, returned to every thread; red: W elements
template <int W, typename T>
__device__ __forceinline__ T wg_sum(T v, T* red) {
    v = pn2_wave_all_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) t += red[w];
    __syncthreads();
    return t;
}

// ---- float64 x / y / z minimum -------------------------------------------------------------------------------------------------
// fmin does not order -0.0 against +0.0, so the ORDER of the folds decides the sign of a zero minimum, and that sign shows in
// z - min_z for z = -0.0.  The orders below are pinned by the exact models of the tests: none of them may change.
//
// the wave's minimum in every lane (xor-shuffle tree, 32 down to 1); lane 0 of each wave leaves it in smin[axis][wave]; a barrier
template <int W>
__device__ __forceinline__ void wg_min3_stage(double& m0, double& m1, double& m2, double (*smin)[W]) {
    m0 = pn2_wave_all(m0, Pn2OpFmin()); m1 = pn2_wave_all(m1, Pn2OpFmin()); m2 = pn2_wave_all(m2, Pn2OpFmin());
    if ((threadIdx.x & 63) == 0) { smin[0][threadIdx.x >> 6] = m0; smin[1][threadIdx.x >> 6] = m1; smin[2][threadIdx.x >> 6] = m2; }
    __syncthreads();
}

// the workgroup's minimum in every thread: each thread folds smin[axis][0 .. W), ascending, into its own wave's value
template <int W>
__device__ __forceinline__ void wg_min3(double& m0, double& m1, double& m2, double (*smin)[W]) {
    wg_min3_stage<W>(m0, m1, m2, smin);
    for (int w = 0; w < W; ++w) { m0 = fmin(m0, smin[0][w]); m1 = fmin(m1, smin[1][w]); m2 = fmin(m2, smin[2][w]); }
}

// ---- small things ------------------------------------------------------------------------------------------------------------
// first index i in [lo, hi) with x[3*i] >= v (np.searchsorted(points[:, 0], v), side='left'); rows [lo, hi) sorted by x
__device__ __forceinline__ int lower_bound_x(const double* __restrict__ pts, int lo, int hi, double v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pts[(size_t)mid * 3] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool finite64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ bool finite32(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }

// the VALID point of pn2_cluster_points and of the plane entry points (include/pn2_abi.h): three finite coordinates and, with
// labels, a label >= 0
__device__ __forceinline__ bool point_valid(const float* __restrict__ points, const int* __restrict__ labels, long long i) {
    const float* p = points + (size_t)i * 3;
    return finite32(p[0]) && finite32(p[1]) && finite32(p[2]) && (!labels || labels[i] >= 0);
}

// ---- host: the prologue of an eager entry point --------------------------------------------------------------------------------
// workgroups of `threads` that cover `items`
inline int blocks_of(long long items, int threads) { return (int)((items + threads - 1) / threads); }

// neither an infinity nor a NaN (a NaN fails the comparison)
inline bool finite_host(double v) { return v - v == 0.0; }

// PN2_OK when `st` is not capturing, PN2_EUNSUP when it is, or the query's hipError_t: the first act of an entry point that is
// eager only (pn2_cluster.hip, pn2_neighbors.hip, pn2_icp.hip, pn2_plane.hip, pn2_describe.hip), behind its argument checks and
// in front of its first launch.  Each call site says why it refuses.
inline int refuse_capture(hipStream_t st) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &capturing);
    if (e != hipSuccess) return (int)e;
    return capturing != hipStreamCaptureStatusNone ? PN2_EUNSUP : PN2_OK;
}

// ---- host: workspace carving ---------------------------------------------------------------------------------------------------
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// consecutive 256-byte-aligned pieces of a workspace.  base == nullptr measures: every piece comes back NULL, `used` still grows.
// Each file has ONE function that runs a carver over a struct of typed pointers; its size query calls it with a null base, its
// entry point with the caller's workspace and `limit` = the caller's workspace_bytes, and then asks fits().
struct WsCarver {
    unsigned char* base;
    size_t limit = ~(size_t)0;
    size_t used = 0;
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += al256(count * sizeof(T));
        return p;
    }
    bool fits() const { return used <= limit; }
};
