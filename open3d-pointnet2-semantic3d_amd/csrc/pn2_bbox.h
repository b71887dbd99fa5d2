// pn2_bbox.h -- the float32 bounding boxes of a batch of clouds, as ordered keys (pn2_ordered.h): bbox[cloud * 6 + 0..2] the
// minima, + 3..5 the maxima.  One kernel pair for pn2_grid_knn.h (one cloud, gridDim.y == 1) and pn2_fps_bucket.hip (gridDim.y
// == b).  Internal linkage: each translation unit that includes the header gets its own copy of the kernels.
#pragma once
#include "pn2_common.h"   // pn2_wave_umin, pn2_wave_umax
#include "pn2_ordered.h"  // ordered_key32

namespace {

// running minima all ones, running maxima zero; one lane per word
__global__ void bbox_init_kernel(int b, unsigned* bbox) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b * 6) bbox[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
}

// cloud blockIdx.y of n points each: a strided pass, then one atomicMin / atomicMax per axis per wave
__global__ void __launch_bounds__(256)
bbox_kernel(int n, const float* __restrict__ xyz_all, unsigned* __restrict__ bbox_all) {
    const float* __restrict__ xyz = xyz_all + (size_t)blockIdx.y * n * 3;
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned o = ordered_key32(xyz[(size_t)i * 3 + a]);
            mn[a] = o < mn[a] ? o : mn[a];
            mx[a] = o > mx[a] ? o : mx[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned wmn = pn2_wave_umin(mn[a]);
        const unsigned wmx = pn2_wave_umax(mx[a]);
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&bbox_all[blockIdx.y * 6 + a], wmn);
            atomicMax(&bbox_all[blockIdx.y * 6 + 3 + a], wmx);
        }
    }
}

}  // namespace
