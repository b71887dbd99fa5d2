// pn2_rng.h -- the counter-based random numbers of the dataset sampler (pn2_dataset.hip) and the augmenter (pn2_augment.hip).
// A draw is a hash of (seed, batch counter, cloud, index): nothing is kept between draws, so any thread forms any draw and a
// captured call replays into fresh numbers once its device counter has advanced.  tests/test_dataset_stream_gpu.py pins the
// values: none of these functions may change.
//
// Index space of draw64(h, i), per stream h = sample_stream(seed, counter, cloud):
//   [0, 2^40)            pn2_dataset.hip: the subset key of the point at scene-local index i
//   2^40 + 0, 1, 2       pn2_dataset.hip: scene, centre, angle of the sample
//   [2^41, 2^45)         pn2_augment.hip (its own tags are listed there): a dataset and an augmenter that share a seed and a
//                        counter value share no draw
//   [2^45, 2^46)         pn2_plane.hip: 2^45 + 3t + j is the rank draw of sample point j of RANSAC trial t (stream
//                        sample_stream(seed, 0, 0))
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long fmix64(unsigned long long x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}
// counter-based stream of (seed, batch counter, sample); one more mix per draw index
__device__ __forceinline__ unsigned long long sample_stream(unsigned long long seed, unsigned long long ctr, int s) {
    unsigned long long h = fmix64(seed + 0x9E3779B97F4A7C15ull);
    h = fmix64(h ^ (ctr * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull));
    return fmix64(h ^ ((unsigned long long)(unsigned)s * 0xAEF17502108EF2D9ull + 0x632BE59BD9B4E019ull));
}
// draw i of stream h
__device__ __forceinline__ unsigned long long draw64(unsigned long long h, unsigned long long i) {
    return fmix64(h ^ fmix64(i + 0x8CB92BA72F3D8DD7ull));
}
__device__ __forceinline__ double unit53(unsigned long long k) { return (double)(k >> 11) * 0x1.0p-53; }  // [0, 1)
