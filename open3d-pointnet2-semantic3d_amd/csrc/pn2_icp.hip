// pn2_icp.hip -- rigid registration of two clouds by iterative closest point, point-to-point (Horn's quaternion) and
// point-to-plane (one Gauss-Newton step per iteration), and the rigid transform of a cloud: what Open3D offers as
// registration_icp, evaluate_registration and PointCloud.transform.  The rules are in include/pn2_abi.h ("Rigid registration
// (ICP)"); tests/icp_ref.py is their numpy model, and everything here is compared with it for equality.
//
// pn2_icp queues, on the caller's stream (eager only), with max_iteration = K:
//   1 icp_init_kernel      : the scalars (a workspace arrives uninitialised; no memset node), T_0 = init, the trace zeroed.
//   2 icp_count_kernel     : the valid source points.
//   3 icp_labels_kernel    : point-to-plane only -- the target's labels with -1 where a normal is not finite, so that the grid
//                            below sees the VALID rule of this call through its one `labels` argument.
//   4 CellGrid::build      : pn2_cell_grid.h -- grid_min_kernel, grid_key_kernel, one radix sort, grid_gather_kernel: the TARGET's
//                            grid at cell edge max_distance * (1 + 2^-20), built once; the sorted target points as (x, y, z,
//                            original index) rows.
//   5 K + 1 times: icp_match_kernel (THE HOT ONE), icp_step_kernel (one workgroup).
// Nothing is read by the host: the stop is a `done` word in the scalars, and every launch behind the stop returns at once.
//
// THE MATCH.  One lane owns one source point, in the source's own order (lane = block * 256 + thread: the sums are a fixed tree
// over that index, so nothing is sorted on this side).  The lane transforms its point, walks the nine key ranges around its cell
// of the target's grid (pn2_cell_grid.h's grid_walk_rows with nrows = 9, end = nt, as the lane path (a) of pn2_neighbors.hip),
// keeps the nearest candidate in registers, and forms its row of the normal equations in registers (17 doubles point-to-point,
// 29 point-to-plane).  The rows are added in float64: xor butterflies inside the wave, ((w0 + w1) + w2) + w3 across the four
// waves through LDS, one row of partials per workgroup; icp_step_kernel adds those rows in ascending order.  No atomic on a sum.
// The two estimators are two instantiations, so that the point-to-point kernel does not carry the other's registers.
#include "pn2_cell_grid.h"  // kT, kW, kCellLimit, GridScal, grid_scal_reset, grid_walk_rows, CellGrid
#include "pn2_common.h"
#include "pn2_eig4.h"       // eig4_largest
#include "pn2_wg.h"         // WsCarver, point_valid, finite32, blocks_of, finite_host, refuse_capture

namespace {

constexpr int kRow = 32;    // doubles per row of partials (17 or 29 in use)
constexpr int kNvPoint = 17, kNvPlane = 29;

// the scalars of one call, at the head of the workspace: the grid's, then
struct Scal : GridScal {
    int ns_valid;   // valid source points
    int done;       // set by the step that stops: every later launch returns at once
    int updates;    // transformations applied
    int converged;
    double T[16];   // the current transformation, row-major
    double prev_fitness, prev_rmse;
};

struct Init {
    double T[16];
};

struct Ws {
    Scal* scal;
    int* eff;  // the target's labels of a point-to-plane call
    CellGrid grid;  // the target's
    double* partials;
};
inline int ws_layout(int ns, int nt, WsCarver& c, Ws* w) {
    w->scal = c.take<Scal>(1);
    w->eff = c.take<int>((size_t)nt);
    w->grid.carve(c, (size_t)nt);
    w->partials = c.take<double>((size_t)blocks_of(ns, kT) * kRow);
    return w->grid.carve_tmp(c, nt);
}

__global__ void __launch_bounds__(kT)
icp_init_kernel(Scal* __restrict__ s, Init init, double* __restrict__ trace, long long trace_doubles) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i == 0) {
        grid_scal_reset(s);
        s->ns_valid = s->done = s->updates = s->converged = 0;
        for (int j = 0; j < 16; ++j) s->T[j] = init.T[j];
        s->prev_fitness = s->prev_rmse = 0.0;
    }
    if (trace && i < trace_doubles) trace[i] = 0.0;
}

__global__ void __launch_bounds__(kT)
icp_count_kernel(int n, const float* __restrict__ points, const int* __restrict__ labels, Scal* __restrict__ s) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const unsigned long long bal = __ballot(i < n && point_valid(points, labels, i));
    if (bal != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&s->ns_valid, __popcll(bal));
}

__global__ void __launch_bounds__(kT)
icp_labels_kernel(int n, const int* __restrict__ labels, const float* __restrict__ normals, int* __restrict__ eff) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float* v = normals + (size_t)i * 3;
    eff[i] = finite32(v[0]) && finite32(v[1]) && finite32(v[2]) ? (labels ? labels[i] : 0) : -1;
}

// the TRANSFORMED SOURCE POINT of the header: float64, rounded to float32 once
__device__ __forceinline__ float transform_axis(const double* __restrict__ T, int a, double x, double y, double z) {
    return (float)(((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3]);
}

// EST: 0 point-to-point, 1 point-to-plane
template <int EST>
__global__ void __launch_bounds__(kT)
icp_match_kernel(int ns, const float* __restrict__ source, const int* __restrict__ slabels, int nt,
                 const unsigned long long* __restrict__ keys, const float4* __restrict__ spts,
                 const float* __restrict__ tnormals, double r2, double h, const Scal* __restrict__ s, int* __restrict__ corr,
                 double* __restrict__ partials) {
    constexpr int NV = EST ? kNvPlane : kNvPoint;
    __shared__ double red[kW][NV];
    if (s->done) return;  // (the same for every thread of the launch)
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool search = i < ns && s->status == 0 && point_valid(source, slabels, i);
    float sp[3] = {0.0f, 0.0f, 0.0f};
    double o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (double)ordered_to_float(s->min_key[a]);
    int cell[3] = {0, 0, 0};
    if (search) {
        const float* p = source + (size_t)i * 3;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sp[a] = transform_axis(s->T, a, x, y, z);
            // (a NaN quotient -- a non-finite s', or no valid target point at all -- fails both comparisons)
            const double q = __builtin_floor(((double)sp[a] - o[a]) / h);
            const bool in = finite32(sp[a]) && q >= -1.0 && q <= (double)kCellLimit;  // in floating point, before the conversion
            search = search && in;
            cell[a] = in ? (int)q : 0;
        }
    }
    const double sx = (double)sp[0], sy = (double)sp[1], sz = (double)sp[2];
    double bd = r2;          // the best d2 so far; a candidate needs d2 <= r2
    int bi = 0x7FFFFFFF;     // its target index
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
    if (search) {
        grid_walk_rows(keys, nt, spts, cell[0], cell[1], cell[2], 9, [&](int, const float4& q) {
            const double dx = (double)q.x - sx, dy = (double)q.y - sy, dz = (double)q.z - sz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const int idx = __float_as_int(q.w);
            if (d2 < bd || (d2 == bd && idx < bi)) {
                bd = d2; bi = idx; bx = q.x; by = q.y; bz = q.z;
            }
        });
    }
    const bool paired = bi != 0x7FFFFFFF;
    if (i < ns) corr[i] = paired ? bi : -1;

    // the lane's row: [0] m, [1] d2, then the estimator's sums; +0.0 without a partner
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    if (paired) {
        v[0] = 1.0;
        v[1] = bd;
        const double pa[3] = {sx - o[0], sy - o[1], sz - o[2]};
        if constexpr (EST == 0) {
            const double ta[3] = {(double)bx - o[0], (double)by - o[1], (double)bz - o[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[2 + a] = pa[a];
                v[5 + a] = ta[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) v[8 + 3 * a + b] = pa[a] * ta[b];
            }
        } else {
            const float* nf = tnormals + (size_t)bi * 3;
            const double n0 = (double)nf[0], n1 = (double)nf[1], n2 = (double)nf[2];
            const double e0 = sx - (double)bx, e1 = sy - (double)by, e2 = sz - (double)bz;
            const double rho = (e0 * n0 + e1 * n1) + e2 * n2;
            const double J[6] = {pa[1] * n2 - pa[2] * n1, pa[2] * n0 - pa[0] * n2, pa[0] * n1 - pa[1] * n0, n0, n1, n2};
            int at = 2;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) v[at++] = J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[23 + a] = J[a] * rho;
        }
    }
    // the tree: every lane of every wave is here (full EXEC)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const double w = pn2_wave_all_sum<double>(v[j]);
        if (lane == 0) red[wave][j] = w;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int j = threadIdx.x;
        partials[(size_t)blockIdx.x * kRow + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}

// R = the quadratic form of the quaternion (w, x, y, z) divided by its squared norm
__device__ void rotation_of(double w, double x, double y, double z, double (&R)[3][3]) {
    const double nn = ((w * w + x * x) + y * y) + z * z;
    R[0][0] = (((w * w + x * x) - y * y) - z * z) / nn;
    R[0][1] = (2.0 * (x * y - w * z)) / nn;
    R[0][2] = (2.0 * (x * z + w * y)) / nn;
    R[1][0] = (2.0 * (x * y + w * z)) / nn;
    R[1][1] = (((w * w - x * x) + y * y) - z * z) / nn;
    R[1][2] = (2.0 * (y * z - w * x)) / nn;
    R[2][0] = (2.0 * (x * z - w * y)) / nn;
    R[2][1] = (2.0 * (y * z + w * x)) / nn;
    R[2][2] = (((w * w - x * x) - y * y) + z * z) / nn;
}

// POINT-TO-POINT of the header: S = the summed row, m >= 3 -> R, t
__device__ void solve_point(const double* S, const double* o, double (&R)[3][3], double* t) {
    const double m = S[0];
    double sm[3], tm[3], M[3][3];
    for (int a = 0; a < 3; ++a) { sm[a] = S[2 + a] / m; tm[a] = S[5 + a] / m; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] = S[8 + 3 * a + b] / m - sm[a] * tm[b];
    double N[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    N[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    N[0][1] = N[1][0] = M[1][2] - M[2][1];
    N[0][2] = N[2][0] = M[2][0] - M[0][2];
    N[0][3] = N[3][0] = M[0][1] - M[1][0];
    N[1][2] = N[2][1] = M[0][1] + M[1][0];
    N[1][3] = N[3][1] = M[2][0] + M[0][2];
    N[2][3] = N[3][2] = M[1][2] + M[2][1];
    double q[4];
    eig4_largest(N, q);
    rotation_of(q[0], q[1], q[2], q[3], R);
    double c[3];
    for (int a = 0; a < 3; ++a) c[a] = sm[a] + o[a];
    for (int a = 0; a < 3; ++a) t[a] = (tm[a] + o[a]) - ((R[a][0] * c[0] + R[a][1] * c[1]) + R[a][2] * c[2]);
}

// POINT-TO-PLANE of the header: S = the summed row, m >= 6 -> R, t; false for a pivot that is not > 0
__device__ bool solve_plane(const double* S, const double* o, double (&R)[3][3], double* t) {
    double A[6][6], L[6][6], y[6], x[6];
    int at = 2;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[a][b] = A[b][a] = S[at]; ++at; }
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0)) return false;
        L[j][j] = __builtin_sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = -S[23 + i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    rotation_of(1.0, x[0] / 2.0, x[1] / 2.0, x[2] / 2.0, R);
    for (int a = 0; a < 3; ++a) t[a] = (o[a] + x[3 + a]) - ((R[a][0] * o[0] + R[a][1] * o[1]) + R[a][2] * o[2]);
    return true;
}

// evaluation k: the rows of partials added in ascending order, fitness and rmse, the stop, or T_(k+1) = U_k * T_k
__global__ void __launch_bounds__(64)
icp_step_kernel(int k, int max_iteration, int est, int rows, double rel_fitness, double rel_rmse,
                const double* __restrict__ partials, Scal* __restrict__ s, double* __restrict__ result,
                double* __restrict__ trace, int* __restrict__ header) {
    __shared__ double S[kRow];
    if (s->done) return;
    const int nv = est ? kNvPlane : kNvPoint;
    if ((int)threadIdx.x < kRow) {
        double t = 0.0;
        if ((int)threadIdx.x < nv)
            for (int b = 0; b < rows; ++b) t += partials[(size_t)b * kRow + threadIdx.x];
        S[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double m = S[0], sum_d2 = S[1];
    const double fitness = s->ns_valid > 0 ? m / (double)s->ns_valid : 0.0;
    const double rmse = m > 0.0 ? __builtin_sqrt(sum_d2 / m) : 0.0;
    if (trace) {
        double* row = trace + (size_t)k * 20;
        row[0] = m; row[1] = fitness; row[2] = rmse; row[3] = 0.0;
        for (int j = 0; j < 16; ++j) row[4 + j] = s->T[j];
    }
    int status = s->status;
    bool stop = status != 0;
    if (!stop && k >= 1 && __builtin_fabs(fitness - s->prev_fitness) < rel_fitness &&
        __builtin_fabs(rmse - s->prev_rmse) < rel_rmse) {
        s->converged = 1;
        stop = true;
    }
    if (!stop && k == max_iteration) stop = true;
    if (!stop) {
        double o[3], R[3][3], t[3];
        for (int a = 0; a < 3; ++a) o[a] = (double)ordered_to_float(s->min_key[a]);
        bool ok;
        if (est == 0) {
            ok = m >= 3.0;
            if (ok) solve_point(S, o, R, t);
        } else {
            ok = m >= 6.0 && solve_plane(S, o, R, t);
        }
        if (!ok) {
            status = 2;
            stop = true;
        } else {
            // T_(k+1) = U * T_k, U = [R t; 0 0 0 1]: rows 0..2 in the written association, row 3 kept
            double Tn[12];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 4; ++b)
                    Tn[4 * a + b] = ((R[a][0] * s->T[b] + R[a][1] * s->T[4 + b]) + R[a][2] * s->T[8 + b]) + t[a] * s->T[12 + b];
            for (int j = 0; j < 12; ++j) s->T[j] = Tn[j];
            s->updates += 1;
            s->prev_fitness = fitness;
            s->prev_rmse = rmse;
        }
    }
    if (stop) {
        const bool grid = status == 1;  // the cloud did not fit the grid: T = init, zeros behind it
        for (int j = 0; j < 16; ++j) result[j] = s->T[j];
        result[16] = grid ? 0.0 : fitness;
        result[17] = grid ? 0.0 : rmse;
        result[18] = grid ? 0.0 : sum_d2;
        result[19] = 0.0;
        header[0] = status;
        header[1] = grid ? 0 : s->ns_valid;
        header[2] = grid ? 0 : s->nvalid;
        header[3] = grid ? 0 : (int)m;
        header[4] = grid ? 0 : s->updates;
        header[5] = grid ? 0 : s->converged;
        header[6] = header[7] = 0;
        s->status = status;
        s->done = 1;
    }
}

__global__ void __launch_bounds__(kT)
transform_points_kernel(int n, const float* points, Init T, float* out) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float* p = points + (size_t)i * 3;
    const float x = p[0], y = p[1], z = p[2];
    float r0 = x, r1 = y, r2 = z;  // an invalid row passes through as it is
    if (finite32(x) && finite32(y) && finite32(z)) {
        r0 = transform_axis(T.T, 0, (double)x, (double)y, (double)z);
        r1 = transform_axis(T.T, 1, (double)x, (double)y, (double)z);
        r2 = transform_axis(T.T, 2, (double)x, (double)y, (double)z);
    }
    out[(size_t)i * 3] = r0;
    out[(size_t)i * 3 + 1] = r1;
    out[(size_t)i * 3 + 2] = r2;
}

inline bool finite16(const double* T) {
    for (int j = 0; j < 16; ++j)
        if (!finite_host(T[j])) return false;
    return true;
}

}  // namespace

extern "C" int pn2_icp_workspace_size(int ns, int nt, int max_iteration, unsigned long long* bytes) {
    if (ns < 1 || nt < 1 || max_iteration < 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    const int rc = ws_layout(ns, nt, c, &w);
    if (rc != PN2_OK) return rc;
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_icp(int ns, const float* source, const int* source_labels, int nt, const float* target,
                       const int* target_labels, const float* target_normals, float max_distance, int estimation,
                       const double* init, int max_iteration, double relative_fitness, double relative_rmse, int* correspondence,
                       double* result, double* trace, int* header, void* workspace, size_t workspace_bytes, void* stream) {
    if (ns < 1 || nt < 1 || !(max_distance > 0.0f) || !(max_distance <= 3.402823466e38f) || (estimation != 0 && estimation != 1) ||
        max_iteration < 0 || !(relative_fitness >= 0.0) || !(relative_rmse >= 0.0))
        return PN2_EINVAL;
    if (init && !finite16(init)) return PN2_EINVAL;
    if (!source || !target || !correspondence || !result || !header || !workspace || (estimation == 1 && !target_normals))
        return PN2_ENULL;
    if ((((uintptr_t)source | (uintptr_t)source_labels | (uintptr_t)target | (uintptr_t)target_labels | (uintptr_t)target_normals |
          (uintptr_t)correspondence | (uintptr_t)header) & 3) != 0 ||
        (((uintptr_t)result | (uintptr_t)trace) & 7) != 0 || ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    const int rc = ws_layout(ns, nt, c, &w);  // too small: refused before the sort is asked for its share
    if (rc != PN2_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the loop's length is data, so a capture would record all max_iteration + 1 rounds; nothing in the project captures it
    if (const int refused = refuse_capture(st)) return refused;

    Init T0;
    for (int j = 0; j < 16; ++j) T0.T[j] = init ? init[j] : (j % 5 == 0 ? 1.0 : 0.0);
    const double r = (double)max_distance;
    const double cell = CellGrid::edge(max_distance);
    const int bs = blocks_of(ns, kT), bt = blocks_of(nt, kT);
    const long long trace_doubles = trace ? ((long long)max_iteration + 1) * 20 : 0;
    const int binit = trace_doubles > kT ? (int)((trace_doubles + kT - 1) / kT) : 1;
    const int* tlabels = target_labels;

    icp_init_kernel<<<binit, kT, 0, st>>>(w.scal, T0, trace, trace_doubles);
    icp_count_kernel<<<bs, kT, 0, st>>>(ns, source, source_labels, w.scal);
    if (estimation == 1) {
        icp_labels_kernel<<<bt, kT, 0, st>>>(nt, target_labels, target_normals, w.eff);
        tlabels = w.eff;
    }
    const int built = w.grid.build(nt, target, tlabels, max_distance, true, w.scal, st);
    if (built != PN2_OK) return built;
    for (int k = 0; k <= max_iteration; ++k) {
        if (estimation == 0)
            icp_match_kernel<0><<<bs, kT, 0, st>>>(ns, source, source_labels, nt, w.grid.keys(), w.grid.spts, target_normals, r * r, cell,
                                                   w.scal, correspondence, w.partials);
        else
            icp_match_kernel<1><<<bs, kT, 0, st>>>(ns, source, source_labels, nt, w.grid.keys(), w.grid.spts, target_normals, r * r, cell,
                                                   w.scal, correspondence, w.partials);
        icp_step_kernel<<<1, 64, 0, st>>>(k, max_iteration, estimation, bs, relative_fitness, relative_rmse, w.partials, w.scal, result,
                                          trace, header);
    }
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_transform_points(int n, const float* points, const double* transform, float* out, void* stream) {
    if (n < 1) return PN2_EINVAL;
    if (!points || !transform || !out) return PN2_ENULL;
    if (!finite16(transform) || (((uintptr_t)points | (uintptr_t)out) & 3) != 0) return PN2_EINVAL;
    Init T;
    for (int j = 0; j < 16; ++j) T.T[j] = transform[j];
    transform_points_kernel<<<blocks_of(n, kT), kT, 0, static_cast<hipStream_t>(stream)>>>(n, points, T, out);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
