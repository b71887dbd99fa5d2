// pn2_label_interp.hip -- InterpolateLabelWithColor for gfx950: the dense-label kNN vote that follows the
// SA/FP stack in the reference's inference pipeline (tf_ops/tf_interpolate.cpp:71-115, callers
// interpolate.py:35-44, predict.py:40-42, kitti_predict.py:61-63).  The reference builds an Open3D/FLANN
// KD-tree over the sparse points on the CPU and queries it per dense point under OpenMP; here the sparse
// points are binned into a uniform grid on the device (cell keys -> radix sort -> cell ranges) and every
// dense point searches growing cubic shells of cells until its knn-th neighbour is provably final.
// Exact semantics (same as oracle_interpolate_label_with_color): squared L2 in float64,
// ((0+dx*dx)+dy*dy)+dz*dz, ascending, ties -> lowest index; vote of :96-107; colours of :45-47.
// pn2_interpolate_scores is the same grid and the same search with another tail: instead of counting the neighbours' labels it
// sums their int64 score rows (include/pn2_abi.h, "Soft voting").
// The grid and the search live in pn2_grid_knn.h; this file holds the two tails and the entry points.
#include "pn2_grid_knn.h"

namespace {

__device__ __forceinline__ void li_color(int label, uint8_t* __restrict__ c) {
    // tf_interpolate.cpp:45-47
    constexpr unsigned lut[9] = {0xffffffu, 0xff0000u, 0x000080u, 0xff00ffu, 0x008000u,
                                 0x0000ffu, 0x800080u, 0x800000u, 0x008080u};  // 0xBBGGRR
    const unsigned v = (label >= 0 && label < 9) ? lut[label] : 0u;
    c[0] = (uint8_t)(v & 0xff); c[1] = (uint8_t)((v >> 8) & 0xff); c[2] = (uint8_t)((v >> 16) & 0xff);
}

// What a dense point does with its neighbours, bi[0 .. cnt): the kf nearest sparse points by (distance, index) ascending.
// The label tail: the vote of tf_interpolate.cpp:96-107, a label wins when its running count exceeds the running maximum.
struct LiLabelTail {
    const int* __restrict__ labels;
    int* __restrict__ out_labels;
    uint8_t* __restrict__ out_colors;
    template <int KMAX>
    __device__ __forceinline__ void finish(int j, int cnt, const int (&bi)[KMAX]) const {
        int lab[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) lab[s] = s < cnt ? labels[bi[s]] : -1;
        int best = -1, max_count = 0;
#pragma unroll
        for (int a = 0; a < KMAX; ++a) {
            if (a < cnt) {
                int c = 0;
#pragma unroll
                for (int e = 0; e < KMAX; ++e) c += (e <= a && lab[e] == lab[a]) ? 1 : 0;
                if (c > max_count) { best = lab[a]; max_count = c; }
            }
        }
        out_labels[j] = best;
        li_color(best, out_colors + (size_t)j * 3);
    }
};

// The score tail: S_c = the int64 sum of the neighbours' score rows, class by class with a running best, so that num_class
// costs no registers: the <= 16 rows are read again for every class (consecutive 8-byte words of the same few cache lines).
struct LiScoreTail {
    int num_class;
    const long long* __restrict__ scores;
    int* __restrict__ out_labels;
    uint8_t* __restrict__ out_colors;
    float* __restrict__ out_confidence;
    template <int KMAX>
    __device__ __forceinline__ void finish(int j, int cnt, const int (&bi)[KMAX]) const {
        int best = 0;
        long long top = 0, total = 0;
        for (int c = 0; c < num_class; ++c) {
            long long sum = 0;
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s < cnt) sum += scores[(size_t)bi[s] * num_class + c];
            total += sum;
            if (c == 0 || sum > top) { top = sum; best = c; }  // strictly greater: the first maximal class; all zero: 0
        }
        out_labels[j] = best;
        li_color(best, out_colors + (size_t)j * 3);
        if (out_confidence) out_confidence[j] = total == 0 ? 0.0f : (float)((double)top / (double)total);
    }
};

__global__ void __launch_bounds__(256)
li_fill_kernel(int nd, int* __restrict__ out_labels, uint8_t* __restrict__ out_colors, float* __restrict__ out_confidence) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd) return;
    out_labels[j] = -1;
    out_colors[(size_t)j * 3 + 0] = 0; out_colors[(size_t)j * 3 + 1] = 0; out_colors[(size_t)j * 3 + 2] = 0;
    if (out_confidence) out_confidence[j] = 0.0f;
}

}  // namespace

extern "C" size_t pn2_interpolate_label_workspace_bytes(int num_sparse_points) {
    if (num_sparse_points < 0) return 0;
    LiWs w;
    li_ws_layout(num_sparse_points, nullptr, &w);
    return w.total;
}

extern "C" int pn2_interpolate_label_with_color(int num_sparse_points, int num_dense_points,
                                                const float* sparse_points, const int* sparse_labels,
                                                const float* dense_points, int* dense_labels,
                                                uint8_t* dense_colors, int knn, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    if (num_sparse_points < 0 || num_dense_points < 0 || knn <= 0) return PN2_EINVAL;
    if (num_dense_points == 0) return PN2_OK;
    if (!dense_points || !dense_labels || !dense_colors) return PN2_ENULL;
    if (knn > 16) return PN2_EUNSUP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nd = num_dense_points, ns = num_sparse_points;
    const int qgrid = (nd + 255) / 256;
    if (ns == 0) {
        li_fill_kernel<<<qgrid, 256, 0, st>>>(nd, dense_labels, dense_colors, nullptr);
        PN2_RETURN_IF_LAUNCH_FAILED();
        return PN2_OK;
    }
    if (!sparse_points || !sparse_labels || !workspace) return PN2_ENULL;
    LiWs w;
    li_ws_layout(ns, static_cast<unsigned char*>(workspace), &w);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255) != 0) return PN2_EINVAL;
    LiGrid g;
    const int rc = li_build_grid(ns, sparse_points, w, st, &g);
    if (rc != PN2_OK) return rc;
    const int kf = knn < ns ? knn : ns;
    const LiLabelTail tail{sparse_labels, dense_labels, dense_colors};
    if (knn <= 4)
        li_query_kernel<4><<<qgrid, 256, 0, st>>>(nd, kf, g.prm, g.cell_start, g.cell_end, g.sorted, dense_points, tail);
    else
        li_query_kernel<16><<<qgrid, 256, 0, st>>>(nd, kf, g.prm, g.cell_start, g.cell_end, g.sorted, dense_points, tail);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_interpolate_scores(int ns, int nd, int num_class, const float* sparse_points, const long long* sparse_scores,
                                      const float* dense_points, int* dense_labels, uint8_t* dense_colors,
                                      float* dense_confidence, int knn, void* workspace, size_t workspace_bytes, void* stream) {
    if (ns < 0 || nd < 0 || num_class <= 0 || knn <= 0) return PN2_EINVAL;
    if (num_class > 64 || knn > 16) return PN2_EUNSUP;
    if (nd == 0) return PN2_OK;
    if (!dense_points || !dense_labels || !dense_colors) return PN2_ENULL;
    if (ns > 0 && (!sparse_points || !sparse_scores || !workspace)) return PN2_ENULL;
    if ((((uintptr_t)sparse_points | (uintptr_t)dense_points | (uintptr_t)dense_labels | (uintptr_t)dense_confidence) & 3) != 0 ||
        ((uintptr_t)sparse_scores & 7) != 0)
        return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int qgrid = (nd + 255) / 256;
    if (ns == 0) {
        li_fill_kernel<<<qgrid, 256, 0, st>>>(nd, dense_labels, dense_colors, dense_confidence);
        PN2_RETURN_IF_LAUNCH_FAILED();
        return PN2_OK;
    }
    if (((uintptr_t)workspace & 255) != 0) return PN2_EINVAL;
    LiWs w;
    li_ws_layout(ns, static_cast<unsigned char*>(workspace), &w);
    if (workspace_bytes < w.total) return PN2_EINVAL;
    LiGrid g;
    const int rc = li_build_grid(ns, sparse_points, w, st, &g);
    if (rc != PN2_OK) return rc;
    const int kf = knn < ns ? knn : ns;
    const LiScoreTail tail{num_class, sparse_scores, dense_labels, dense_colors, dense_confidence};
    if (knn <= 4)
        li_query_kernel<4><<<qgrid, 256, 0, st>>>(nd, kf, g.prm, g.cell_start, g.cell_end, g.sorted, dense_points, tail);
    else
        li_query_kernel<16><<<qgrid, 256, 0, st>>>(nd, kf, g.prm, g.cell_start, g.cell_end, g.sorted, dense_points, tail);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
