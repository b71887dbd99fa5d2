// pn2_ordered.h -- float <-> unsigned key with the same order: k(a) < k(b) <=> a < b for every pair of non-NaN values (-0.0 sorts
// directly below +0.0).  Minima / maxima go through integer atomics on it, and a radix sort on it is a sort by value.  One copy:
//   float64 <-> 64 bits: pn2_dataset.hip, pn2_scene.hip, pn2_store.hip, pn2_tile.hip, pn2_describe.hip;
//   float32 <-> 32 bits: pn2_bbox.h (pn2_grid_knn.h, pn2_fps_bucket.hip), pn2_cluster.hip, pn2_render.hip, pn2_describe.hip.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long ordered_key(double v) {
    unsigned long long k = (unsigned long long)__double_as_longlong(v);
    return (k >> 63) ? ~k : (k | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_to_double(unsigned long long k) {
    k = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)k);
}

// all bits of a negative float flipped, the sign bit of a non-negative one set: -0.0f -> 0x7fffffff, +0.0f -> 0x80000000
__device__ __forceinline__ unsigned ordered_key32(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
