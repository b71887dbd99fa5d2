// pn2_color.h -- the one colour rule the scene-file writers share (pn2_scene_io.hip's .pcd rows, pn2_records.hip's records).
#pragma once
#include <hip/hip_runtime.h>

// floor(c * 255.0) clipped to [0, 255], the host writers' np.clip(np.floor(c * 255.0), 0, 255); a NaN gives 0.  Needs IEEE fp64
// multiply (no fast-math, no contraction).
__host__ __device__ __forceinline__ unsigned unit_to_byte(double c) {
    const double t = __builtin_floor(c * 255.0);
    return t >= 255.0 ? 255u : (t > 0.0 ? (unsigned)t : 0u);
}
