// pn2_cluster.hip -- Euclidean clustering: the points of a (labelled) cloud grouped into connected components of the graph that
// links two valid points of one label no more than eps apart.  The rules are in include/pn2_abi.h (pn2_cluster_points);
// tests/cluster_ref.py is their numpy model, and everything here is compared with it for equality.
//
// pn2_cluster_points queues, on the caller's stream (eager only: the host half of the caller reads the header afterwards):
//   1 cluster_init_kernel    : the scalars (ordered minima, counters, status); parent[i] = i, csize[i] = 0.
//   2 .. 5 CellGrid::build   : pn2_cell_grid.h -- grid_min_kernel (the minimum x, y, z of the valid points as ordered uint32: a
//                              float32 minimum is exact; the count of valid points), grid_key_kernel (the cell of every valid
//                              point and its 63-bit key, x lowest; an invalid point gets the key ~0, which sorts last and is never
//                              visited; a cell coordinate >= 2^21 raises the status), the radix sort of (key, point index) pairs,
//                              grid_gather_kernel (the sorted points as (x, y, z, label) rows).
//   6 cluster_union_kernel   : one sorted point per lane.  It visits the points IN FRONT of it in the sorted order that lie in the
//                              27 cells around its own -- five key ranges, because x is the lowest key field: the three rows
//                              (y-1, y, y+1) of the layer z-1, the row y-1 of its own layer, and its own row up to itself -- and
//                              unites itself with every one that is linked.  So each linked pair is tested once.
//   7 cluster_flatten_kernel : root[i] = the root of i (-1 for an invalid point), csize[root] += 1.
//   8 cluster_flag_kernel    : per scan block of 256 points the number of kept roots; components and kept points counted.
//   9 cluster_offsets_kernel : one workgroup: the exclusive prefix of the block counts, and the header.
//  10 cluster_number_kernel  : number[i] of a kept root = block offset + its place in the block (pn2_wg.h's scan), -1 otherwise.
//  11 cluster_ids_kernel     : ids[i] = number[root[i]], -1 without a root.
//
// THE GRID: pn2_cell_grid.h (the cell edge eps * (1 + 2^-20) and why the 27 cells around a point hold every linked partner).
//
// THE UNION-FIND.  parent[] over point indices; parent[i] <= i always, and a link always points from the higher root to the lower:
// a root is the lowest index of its tree, hence at the end the component's `first`.
//   * find walks down (parent[x] < x unless x is a root: strictly decreasing, bounded by its start) and halves the path with an
//     atomicMin on nodes that are no roots.  A node that has stopped being a root never becomes one again, so such a write can only
//     replace an ancestor by an ancestor.
//   * unite(a, b): find both; equal -> done; otherwise compare-and-swap parent[hi] from hi to lo.  The swap succeeds only while hi
//     is still its own parent, so no link is ever overwritten.  When it fails it returns the parent hi got meanwhile, old < hi, and
//     the pair (old, lo) carries the same obligation: it is united next.  max(a, b) falls strictly from one round to the next:
//     that is the loop's bound.
//   * parent[] is read with relaxed agent-scope atomic loads.  A stale value is an ancestor of an earlier time: it lengthens a walk
//     or fails a swap, and no loop's exit rests on it -- find ends on its own decreasing index, unite on the swap's answer.
// No kernel waits for another workgroup.
#include "pn2_cell_grid.h"  // kT, kW, kCellBits, kCellLimit, kInvalidKey, GridScal, grid_scal_reset, lower_bound_key, CellGrid
#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_key32, ordered_to_float
#include "pn2_wg.h"       // wg_excl_scan_flag, wg_excl_scan_int, wg_sum, point_valid, blocks_of, refuse_capture, WsCarver

namespace {

// the scalars of one call, at the head of the workspace: the grid's, then
struct Scal : GridScal {
    int ncomp;            // components before the size filter
    int nkeptpts;         // points in kept clusters
};

struct Ws {  // workspace carve-up
    Scal* scal;
    CellGrid grid;
    int *parent, *csize, *root, *number, *bcount;
};
inline int ws_layout(int n, WsCarver& c, Ws* w) {
    const size_t N = (size_t)n;
    w->scal = c.take<Scal>(1);
    w->grid.carve(c, N);
    w->parent = c.take<int>(N);
    w->csize = c.take<int>(N);
    w->root = c.take<int>(N);
    w->number = c.take<int>(N);
    w->bcount = c.take<int>((size_t)blocks_of(n, kT));
    return w->grid.carve_tmp(c, n);
}

__global__ void __launch_bounds__(kT)
cluster_init_kernel(int n, Scal* __restrict__ s, int* __restrict__ parent, int* __restrict__ csize) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i == 0) {
        grid_scal_reset(s);
        s->ncomp = s->nkeptpts = 0;
    }
    if (i < n) {
        parent[i] = (int)i;
        csize[i] = 0;
    }
}

__device__ __forceinline__ int load_parent(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x strictly decreases: parent[x] < x unless x is a root
__device__ __forceinline__ int uf_find(int* parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p >= x) return x;  // p == x: a root (p > x cannot be; it would end the walk all the same)
        const int g = load_parent(parent, p);
        if (g < p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // x is no root: halve
        x = p;
    }
}

// max(a, b) strictly decreases from round to round
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (seen >= hi) return;  // cannot be (a failed swap saw parent[hi] != hi, and parent[hi] <= hi): the bound, stated
        a = seen;  // hi was hooked by somebody else meanwhile: its new parent is united with lo instead
        b = lo;
    }
}

__global__ void __launch_bounds__(kT)
cluster_union_kernel(int n, const unsigned long long* __restrict__ keys, const int* __restrict__ order,
                     const float4* __restrict__ spts, double eps2, const Scal* __restrict__ s, int* parent) {
    const long long s0 = (long long)blockIdx.x * kT + threadIdx.x;
    if (s0 >= n || s->status != 0) return;
    const int me = (int)s0;
    const unsigned long long key = keys[me];
    if (key == kInvalidKey) return;
    const int cx = (int)(key & (kCellLimit - 1)), cy = (int)((key >> kCellBits) & (kCellLimit - 1)),
              cz = (int)((key >> (2 * kCellBits)) & (kCellLimit - 1));
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < kCellLimit - 1 ? cx + 1 : cx;
    const float4 p = spts[me];
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    const int label = __float_as_int(p.w);
    const int i = order[me];
    // the rows in front of this point: (z-1; y-1, y, y+1), (z; y-1), (z; y) up to the point itself.  The first five rows of
    // grid_walk_rows' order with end = me, written out: through the walker (row = r / 3, r % 3) this kernel measured 4 % slower
    // on a 1.5 M-point scene (EXPERIMENTS.md r13), so the loop keeps the shape it had
    for (int r = 0; r < 5; ++r) {
        const int z = r < 3 ? cz - 1 : cz;
        const int y = r < 3 ? cy - 1 + r : (r == 3 ? cy - 1 : cy);
        if (z < 0 || y < 0 || y >= kCellLimit) continue;
        const unsigned long long row = ((unsigned long long)z << (2 * kCellBits)) | ((unsigned long long)y << kCellBits);
        const unsigned long long klo = row | (unsigned long long)x0, khi = row | (unsigned long long)x1;
        // t rises to `me` at the most: only sorted positions in front of this one are visited
        for (int t = lower_bound_key(keys, me, klo); t < me && keys[t] <= khi; ++t) {
            const float4 q = spts[t];
            if (__float_as_int(q.w) != label) continue;
            const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
            if ((dx * dx + dy * dy) + dz * dz <= eps2) uf_unite(parent, i, order[t]);
        }
    }
}

// one atomic per distinct value among the lanes of a wave that hold one (`has`); at most 64 rounds, each retires a lane
__device__ __forceinline__ void wave_count_into(int* __restrict__ counts, bool has, int slot) {
    unsigned long long todo = __ballot(has);
    const int lane = threadIdx.x & 63;
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const int v = __shfl(slot, leader);
        const unsigned long long same = __ballot(has && slot == v) & todo;
        if (lane == leader) atomicAdd(counts + v, __popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(kT)
cluster_flatten_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, const int* __restrict__ parent,
                       const Scal* __restrict__ s, int* __restrict__ root, int* __restrict__ csize) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool ok = i < n && s->status == 0 && point_valid(points, labels, i);
    int r = -1;
    if (ok) {
        r = (int)i;
        for (int p = parent[r]; p < r; p = parent[r]) r = p;  // the union kernel is over: plain loads; r strictly decreases
    }
    if (i < n) root[i] = r;
    wave_count_into(csize, ok, r);
}

__device__ __forceinline__ bool size_kept(int size, int min_points, int max_points) {
    return size >= min_points && (max_points == 0 || size <= max_points);
}

__global__ void __launch_bounds__(kT)
cluster_flag_kernel(int n, const int* __restrict__ root, const int* __restrict__ csize, int min_points, int max_points,
                    Scal* __restrict__ s, int* __restrict__ bcount) {
    __shared__ int red[kW];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool is_root = i < n && root[i] == (int)i;
    const int size = is_root ? csize[i] : 0;
    const bool kept = is_root && size_kept(size, min_points, max_points);
    const int ncomp = wg_sum<kW>(is_root ? 1 : 0, red);
    const int nkept = wg_sum<kW>(kept ? 1 : 0, red);
    const int npts = wg_sum<kW>(kept ? size : 0, red);  // sizes sum to <= n: no overflow
    if (threadIdx.x == 0) {
        bcount[blockIdx.x] = nkept;
        if (ncomp) atomicAdd(&s->ncomp, ncomp);
        if (npts) atomicAdd(&s->nkeptpts, npts);
    }
}

// one workgroup: bcount -> its exclusive prefix, in chunks of kT with a running carry; then the header
__global__ void __launch_bounds__(kT)
cluster_offsets_kernel(int nblocks, int* __restrict__ bcount, const Scal* __restrict__ s, int* __restrict__ header) {
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
        const bool ok = s->status == 0;
        header[0] = s->status;
        header[1] = ok ? carry : 0;
        header[2] = ok ? s->ncomp : 0;
        header[3] = ok ? s->nvalid : 0;
        header[4] = ok ? s->nkeptpts : 0;
        header[5] = header[6] = header[7] = 0;
    }
}

__global__ void __launch_bounds__(kT)
cluster_number_kernel(int n, const int* __restrict__ root, const int* __restrict__ csize, int min_points, int max_points,
                      const int* __restrict__ boffset, int* __restrict__ number) {
    __shared__ int wsum[kW];
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const bool kept = i < n && root[i] == (int)i && size_kept(csize[i], min_points, max_points);
    int total;
    const int before = wg_excl_scan_flag<kW>(kept ? 1 : 0, wsum, total);
    if (i < n) number[i] = kept ? boffset[blockIdx.x] + before : -1;
}

__global__ void __launch_bounds__(kT)
cluster_ids_kernel(int n, const int* __restrict__ root, const int* __restrict__ number, int* __restrict__ ids) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    ids[i] = r >= 0 ? number[r] : -1;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
stats_init_kernel(int nclusters, int* __restrict__ first, int* __restrict__ size, unsigned* __restrict__ box) {
    const int c = blockIdx.x * kT + threadIdx.x;
    if (c >= nclusters) return;
    first[c] = 0x7FFFFFFF;
    size[c] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box[(size_t)c * 6 + a] = 0xFFFFFFFFu;
        box[(size_t)c * 6 + 3 + a] = 0u;
    }
}

__global__ void __launch_bounds__(kT)
stats_points_kernel(int n, int nclusters, const float* __restrict__ points, const int* __restrict__ ids, int* __restrict__ first,
                    int* __restrict__ size, unsigned* __restrict__ box) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int c = i < n ? ids[i] : -1;
    const bool in = c >= 0 && c < nclusters;  // an id outside the tables is never written
    wave_count_into(size, in, c);
    if (!in) return;
    // minima only fall and maxima only rise: a stale read costs an atomic, never a result
    if ((int)i < __hip_atomic_load(first + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) atomicMin(first + c, (int)i);
    unsigned* b = box + (size_t)c * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned k = ordered_key32(points[(size_t)i * 3 + a]);
        if (k < __hip_atomic_load(b + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) atomicMin(b + a, k);
        if (k > __hip_atomic_load(b + 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) atomicMax(b + 3 + a, k);
    }
}

__global__ void __launch_bounds__(kT)
stats_finish_kernel(int n, int nclusters, const int* __restrict__ labels, const int* __restrict__ first, int* __restrict__ label,
                    unsigned* __restrict__ box) {
    const int c = blockIdx.x * kT + threadIdx.x;
    if (c >= nclusters) return;
    const int f = first[c];
    label[c] = labels && f >= 0 && f < n ? labels[f] : 0;  // an empty cluster (an id the caller never used) keeps first = INT_MAX
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        unsigned* w = box + (size_t)c * 6 + a;
        *w = __float_as_uint(ordered_to_float(*w));
    }
}

// h = id * 0x9E3779B1; h ^= h >> 15; h *= 0x85EBCA77; h ^= h >> 13 (uint32); hue = h % 1536: six sectors of 256 steps
__global__ void __launch_bounds__(kT)
cluster_colors_kernel(int n, const int* __restrict__ ids, unsigned char* __restrict__ rgb) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    unsigned r = 96u, g = 96u, b = 96u;
    if (id >= 0) {
        unsigned h = (unsigned)id * 0x9E3779B1u;
        h ^= h >> 15;
        h *= 0x85EBCA77u;
        h ^= h >> 13;
        const unsigned hue = h % 1536u, f = hue & 255u;
        switch (hue >> 8) {
            case 0: r = 255u; g = f; b = 0u; break;
            case 1: r = 255u - f; g = 255u; b = 0u; break;
            case 2: r = 0u; g = 255u; b = f; break;
            case 3: r = 0u; g = 255u - f; b = 255u; break;
            case 4: r = f; g = 0u; b = 255u; break;
            default: r = 255u; g = 0u; b = 255u - f; break;
        }
    }
    unsigned char* out = rgb + (size_t)i * 3;
    out[0] = (unsigned char)r;
    out[1] = (unsigned char)g;
    out[2] = (unsigned char)b;
}

}  // namespace

extern "C" int pn2_cluster_workspace_size(int n, unsigned long long* bytes) {
    if (n <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    const int rc = ws_layout(n, c, &w);
    if (rc != PN2_OK) return rc;
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_cluster_points(int n, const float* points, const int* labels, float eps, int min_points, int max_points, int* ids,
                                  int* header, void* workspace, size_t workspace_bytes, void* stream) {
    if (n <= 0 || !(eps > 0.0f) || !(eps <= 3.402823466e38f) || min_points < 1 || max_points < 0) return PN2_EINVAL;
    if (!points || !ids || !header || !workspace) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)labels | (uintptr_t)ids | (uintptr_t)header) & 3) != 0 || ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    const int rc = ws_layout(n, c, &w);  // too small: refused before the sort is asked for its share
    if (rc != PN2_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // eager by nature: the caller reads the header (the number of clusters sizes what follows)
    if (const int refused = refuse_capture(st)) return refused;

    const double eps2 = (double)eps * (double)eps;
    const int blocks = blocks_of(n, kT);

    cluster_init_kernel<<<blocks, kT, 0, st>>>(n, w.scal, w.parent, w.csize);
    const int built = w.grid.build(n, points, labels, eps, false, w.scal, st);
    if (built != PN2_OK) return built;
    cluster_union_kernel<<<blocks, kT, 0, st>>>(n, w.grid.keys(), w.grid.order(), w.grid.spts, eps2, w.scal, w.parent);
    cluster_flatten_kernel<<<blocks, kT, 0, st>>>(n, points, labels, w.parent, w.scal, w.root, w.csize);
    cluster_flag_kernel<<<blocks, kT, 0, st>>>(n, w.root, w.csize, min_points, max_points, w.scal, w.bcount);
    cluster_offsets_kernel<<<1, kT, 0, st>>>(blocks, w.bcount, w.scal, header);
    cluster_number_kernel<<<blocks, kT, 0, st>>>(n, w.root, w.csize, min_points, max_points, w.bcount, w.number);
    cluster_ids_kernel<<<blocks, kT, 0, st>>>(n, w.root, w.number, ids);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_cluster_stats(int n, int nclusters, const float* points, const int* labels, const int* ids, int* first, int* size,
                                 int* label, float* bbox, void* stream) {
    if (n <= 0 || nclusters <= 0) return PN2_EINVAL;
    if (nclusters > n) return PN2_ERANGE;
    if (!points || !ids || !first || !size || !label || !bbox) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)labels | (uintptr_t)ids | (uintptr_t)first | (uintptr_t)size | (uintptr_t)label |
          (uintptr_t)bbox) & 3) != 0)
        return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned* box = reinterpret_cast<unsigned*>(bbox);
    const int cblocks = blocks_of(nclusters, kT);
    stats_init_kernel<<<cblocks, kT, 0, st>>>(nclusters, first, size, box);
    stats_points_kernel<<<blocks_of(n, kT), kT, 0, st>>>(n, nclusters, points, ids, first, size, box);
    stats_finish_kernel<<<cblocks, kT, 0, st>>>(n, nclusters, labels, first, label, box);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_cluster_colors(int n, const int* ids, uint8_t* rgb, void* stream) {
    if (n <= 0) return PN2_EINVAL;
    if (!ids || !rgb) return PN2_ENULL;
    if (((uintptr_t)ids & 3) != 0) return PN2_EINVAL;
    cluster_colors_kernel<<<blocks_of(n, kT), kT, 0, static_cast<hipStream_t>(stream)>>>(n, ids, rgb);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
