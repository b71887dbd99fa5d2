// pn2_ordered.h -- float64 <-> unsigned 64-bit key with the same order: k(a) < k(b) <=> a < b for every pair of non-NaN
// doubles (-0.0 sorts directly below +0.0).  float64 minima / maxima go through 64-bit integer atomics on it, and a radix
// sort on it is a sort by value.  One copy for pn2_dataset.hip, pn2_scene.hip and pn2_store.hip.
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
