// pn2_grid_knn.h -- the scene-scale exact kNN search of pn2_label_interp.hip (dense labels, soft votes), in a header of its own
// so that other files can run it with their own tails: the points are binned into a uniform grid on the device (cell keys
// -> radix sort -> cell ranges) and every query searches growing cubic shells of cells until its knn-th neighbour is provably
// final.  Exact semantics: squared L2 in float64 from float32 coordinates, (dx*dx + dy*dy) + dz*dz, ascending, ties -> lowest
// index.  What a query does with its neighbours is a `Tail` (see li_query_kernel).  Everything here has internal linkage: each
// translation unit that includes the header gets its own copy of the kernels.
#pragma once
#include <math.h>

#include "pn2_bbox.h"  // bbox_init_kernel, bbox_kernel
#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_to_float
#include "pn2_sort.h"     // IndexSort
#include "pn2_wg.h"       // WsCarver

namespace {

constexpr int kLiMaxCells = 1 << 21;  // dense cell table (2 x 8 MiB of int32)
constexpr int kLiCellBits = 21;

struct LiParams {
    float lo[3], hi[3];
    float h, inv_h, slack;
    int n[3];
};

struct LiWs {  // workspace carve-up
    LiParams* prm;
    unsigned* bbox;  // 6 ordered keys (pn2_bbox.h)
    IndexSort<unsigned> sort;
    int *cell_start, *cell_end;  // kLiMaxCells each
    float4* sorted;
    size_t total;
};
inline void li_ws_layout(int ns, unsigned char* base, LiWs* w) {
    WsCarver c{base};
    const size_t n = ns > 0 ? (size_t)ns : 1;
    w->prm = c.take<LiParams>(1);
    w->bbox = c.take<unsigned>(6);
    w->sort.carve(c, n);
    w->cell_start = c.take<int>((size_t)kLiMaxCells);
    w->cell_end = c.take<int>((size_t)kLiMaxCells);
    w->sorted = c.take<float4>(n);
    (void)w->sort.carve_tmp(c, (int)n, 0, kLiCellBits);
    w->total = c.used;
}

// one thread: cell size so that the grid has about ns/2 cells (<= kLiMaxCells)
__global__ void li_params_kernel(int ns, const unsigned* __restrict__ bbox, LiParams* __restrict__ prm) {
    float lo[3], hi[3], ext[3], maxext = 0.f;
    for (int a = 0; a < 3; ++a) {
        lo[a] = ordered_to_float(bbox[a]);
        hi[a] = ordered_to_float(bbox[3 + a]);
        ext[a] = hi[a] - lo[a];
        maxext = fmaxf(maxext, ext[a]);
    }
    float h = 1.0f;
    int n[3] = {1, 1, 1};
    if (maxext > 0.f) {
        float target = (float)ns * 0.5f;
        target = target < 1.f ? 1.f : (target > (float)(kLiMaxCells / 2) ? (float)(kLiMaxCells / 2) : target);
        float vol = 1.f;
        for (int a = 0; a < 3; ++a) vol *= fmaxf(ext[a], maxext * 1e-3f);  // flat clouds: no zero-thickness axis
        h = cbrtf(vol / target);
        h = fmaxf(h, maxext * (1.0f / 2048.0f));
        for (int it = 0; it < 64; ++it) {
            long long tot = 1;
            for (int a = 0; a < 3; ++a) {
                n[a] = (int)floorf(ext[a] / h) + 1;
                tot *= n[a];
            }
            if (tot <= (long long)kLiMaxCells) break;
            h *= 1.26f;
        }
    }
    for (int a = 0; a < 3; ++a) { prm->lo[a] = lo[a]; prm->hi[a] = hi[a]; prm->n[a] = n[a]; }
    prm->h = h;
    prm->inv_h = 1.0f / h;
    prm->slack = 1e-6f * (maxext + h);  // >> the rounding of (x - lo) * inv_h at a cell boundary
}

// the ONE cell-coordinate function (points and queries): monotone in x
__device__ __forceinline__ int li_cell(float x, float lo, float inv_h, int n) {
    int c = (int)floorf((x - lo) * inv_h);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

__global__ void __launch_bounds__(256)
li_keys_kernel(int ns, const float* __restrict__ pts, const LiParams* __restrict__ prm, unsigned* __restrict__ keys,
               int* __restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const int cx = li_cell(pts[(size_t)i * 3 + 0], prm->lo[0], prm->inv_h, prm->n[0]);
    const int cy = li_cell(pts[(size_t)i * 3 + 1], prm->lo[1], prm->inv_h, prm->n[1]);
    const int cz = li_cell(pts[(size_t)i * 3 + 2], prm->lo[2], prm->inv_h, prm->n[2]);
    keys[i] = (unsigned)((cz * prm->n[1] + cy) * prm->n[0] + cx);
    vals[i] = i;
}

__global__ void __launch_bounds__(256)
li_bounds_kernel(int ns, const float* __restrict__ pts, const unsigned* __restrict__ keys, const int* __restrict__ vals,
                 int* __restrict__ cell_start, int* __restrict__ cell_end, float4* __restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const unsigned k = keys[i];
    if (i == 0 || keys[i - 1] != k) cell_start[k] = i;
    if (i == ns - 1 || keys[i + 1] != k) cell_end[k] = i + 1;
    const int src = vals[i];  // stable sort: ascending original index inside a cell
    sorted[i] = make_float4(pts[(size_t)src * 3 + 0], pts[(size_t)src * 3 + 1], pts[(size_t)src * 3 + 2],
                            __int_as_float(src));
}

// one thread per dense point: the shell search, then the tail
template <int KMAX, class Tail>
__global__ void __launch_bounds__(256)
li_query_kernel(int nd, int kf, const LiParams* __restrict__ prm, const int* __restrict__ cell_start,
                const int* __restrict__ cell_end, const float4* __restrict__ sorted, const float* __restrict__ dense,
                const Tail tail) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd) return;
    const float qxf = dense[(size_t)j * 3 + 0], qyf = dense[(size_t)j * 3 + 1], qzf = dense[(size_t)j * 3 + 2];
    const double qx = qxf, qy = qyf, qz = qzf;
    const int nx = prm->n[0], ny = prm->n[1], nz = prm->n[2];
    // cell of the query CLAMPED into the box: the shell bound below is about that point
    const int cx = li_cell(fminf(fmaxf(qxf, prm->lo[0]), prm->hi[0]), prm->lo[0], prm->inv_h, nx);
    const int cy = li_cell(fminf(fmaxf(qyf, prm->lo[1]), prm->hi[1]), prm->lo[1], prm->inv_h, ny);
    const int cz = li_cell(fminf(fmaxf(qzf, prm->lo[2]), prm->hi[2]), prm->lo[2], prm->inv_h, nz);
    // squared distance from the query to the bounding box of the sparse points (0 inside)
    double o2 = 0.0;
    {
        const float q[3] = {qxf, qyf, qzf};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float c = fminf(fmaxf(q[a], prm->lo[a]), prm->hi[a]);
            const double o = (double)q[a] - (double)c;
            o2 += o * o;
        }
    }
    const double h = prm->h, slack = prm->slack;
    double bd[KMAX];
    int bi[KMAX];
#pragma unroll
    for (int p = 0; p < KMAX; ++p) { bd[p] = INFINITY; bi[p] = 0x7fffffff; }
    int cnt = 0;
    auto visit = [&](int x, int y, int z) {
        const int cell = (z * ny + y) * nx + x;
        const int e = cell_end[cell];
        for (int p = cell_start[cell]; p < e; ++p) {
            const float4 pt = sorted[p];
            const double dx = qx - (double)pt.x, dy = qy - (double)pt.y, dz = qz - (double)pt.z;
            const double d = (dx * dx + dy * dy) + dz * dz;  // contraction is off
            const int id = __float_as_int(pt.w);
            // keep the kf smallest by (distance, index)
            const bool room = cnt < kf;
            bool better = false;
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s == kf - 1) better = d < bd[s] || (d == bd[s] && id < bi[s]);
            if (!room && !better) continue;
            const int pos = room ? cnt : kf - 1;
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s == pos) { bd[s] = d; bi[s] = id; }
            cnt += room ? 1 : 0;
#pragma unroll
            for (int s = KMAX - 1; s > 0; --s) {
                if (s < cnt && (bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bi[s] < bi[s - 1]))) {
                    const double td = bd[s]; bd[s] = bd[s - 1]; bd[s - 1] = td;
                    const int ti = bi[s]; bi[s] = bi[s - 1]; bi[s - 1] = ti;
                }
            }
        }
    };
    int maxr = cx;
    maxr = max(maxr, nx - 1 - cx); maxr = max(maxr, cy); maxr = max(maxr, ny - 1 - cy);
    maxr = max(maxr, cz); maxr = max(maxr, nz - 1 - cz);
    for (int r = 0; r <= maxr; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= nz) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= ny) continue;
                const bool face = (dz == -r || dz == r || dy == -r || dy == r);
                if (face) {
                    const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
                    for (int x = x0; x <= x1; ++x) visit(x, y, z);
                } else {
                    if (cx - r >= 0) visit(cx - r, y, z);
                    if (cx + r < nx) visit(cx + r, y, z);  // r > 0 here
                }
            }
        }
        if (cnt == kf) {
            // every unvisited cell is >= r+1 cells away: its points are farther than r*h (minus the
            // boundary rounding) from the clamped query, plus the query's own offset from the box
            const double rb = (double)r * h - slack;
            double worst = 0.0;
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s == kf - 1) worst = bd[s];
            if (rb > 0.0 && worst < o2 + rb * rb) break;
        }
    }
    tail.template finish<KMAX>(j, cnt, bi);
}

struct LiGrid {  // what the query kernels read, inside the caller's workspace
    const LiParams* prm;
    const int *cell_start, *cell_end;
    const float4* sorted;
};

// The uniform grid over the sparse points, queued on `st`: shared by both entry points.  ns > 0, the workspace checked.
int li_build_grid(int ns, const float* sparse_points, const LiWs& w, hipStream_t st, LiGrid* g) {
    const int sgrid = (ns + 255) / 256;

    bbox_init_kernel<<<1, 64, 0, st>>>(1, w.bbox);
    bbox_kernel<<<sgrid < 1024 ? sgrid : 1024, 256, 0, st>>>(ns, sparse_points, w.bbox);
    li_params_kernel<<<1, 1, 0, st>>>(ns, w.bbox, w.prm);
    li_keys_kernel<<<sgrid, 256, 0, st>>>(ns, sparse_points, w.prm, w.sort.keys_in, w.sort.vals_in);
    PN2_RETURN_IF_LAUNCH_FAILED();
    hipError_t e = w.sort.run(ns, 0, kLiCellBits, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(w.cell_start, 0, (size_t)kLiMaxCells * 4, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(w.cell_end, 0, (size_t)kLiMaxCells * 4, st);
    if (e != hipSuccess) return (int)e;
    li_bounds_kernel<<<sgrid, 256, 0, st>>>(ns, sparse_points, w.sort.keys_out, w.sort.vals_out, w.cell_start, w.cell_end, w.sorted);
    g->prm = w.prm; g->cell_start = w.cell_start; g->cell_end = w.cell_end; g->sorted = w.sorted;
    return PN2_OK;
}

}  // namespace
