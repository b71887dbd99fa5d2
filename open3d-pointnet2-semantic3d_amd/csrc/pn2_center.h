// pn2_center.h -- the one-workgroup tail of the fixed-size samplers: _get_fix_sized_sample_mask + _center_box
// (dataset/semantic_dataset.py:90-121 of the reference) for scene_sample_kernel (pn2_scene.hip: positions map through the
// column's index list) and fs_finish_kernel (pn2_frame.hip: positions are rows).  W = the workgroup's waves; every thread calls.
#pragma once
#include "pn2_wg.h"

// cnt > npts: the reference's shuffled boolean mask.  sel = the set positions, ascending, through map[] (NULL: themselves); returns
// how many are set -- the caller rejects anything but npts (:96-100).  wsum: W ints
template <int W>
__device__ __forceinline__ int center_select_mask(int cnt, int npts, const unsigned char* __restrict__ mask,
                                                  const int* __restrict__ map, int* __restrict__ sel, int* wsum) {
    int count = 0;
    for (int base = 0; base < cnt; base += W * 64) {
        const int i = base + threadIdx.x;
        const bool in = (i < cnt) && mask[i] != 0;
        int tot;
        const int off = wg_excl_scan_flag<W>(in, wsum, tot);
        if (in && count + off < npts) sel[count + off] = map ? map[i] : i;
        count += tot;
    }
    return count;
}

// cnt <= npts: arange(cnt) doubled until it reaches npts, then cut (:102-106) == j mod cnt
template <int W>
__device__ __forceinline__ void center_select_repeat(int cnt, int npts, const int* __restrict__ map, int* __restrict__ sel) {
    for (int j = threadIdx.x; j < npts; j += W * 64) sel[j] = map ? map[j % cnt] : j % cnt;
}

struct CenterShift { double s0, s1, s2; };

// box_min = np.min(points, axis=0) over the SAMPLED points (:111), then the shift (:112-118), float64.  sel must be visible to the
// workgroup (a barrier after its writes).  smin: 3 x W doubles
template <int W>
__device__ __forceinline__ CenterShift center_shift(int npts, const double* __restrict__ pts, const int* __restrict__ sel, double hx,
                                                    double hy, double (*smin)[W]) {
    double m0 = 1.0e300, m1 = 1.0e300, m2 = 1.0e300;
    for (int j = threadIdx.x; j < npts; j += W * 64) {
        const size_t k = (size_t)sel[j];
        m0 = fmin(m0, pts[k * 3]); m1 = fmin(m1, pts[k * 3 + 1]); m2 = fmin(m2, pts[k * 3 + 2]);
    }
    wg_min3<W>(m0, m1, m2, smin);
    return {m0 + hx, m1 + hy, m2};
}

// row j of the sample = point k: centred (one float64 subtraction, one rounding: :119 then astype(float32)) and raw (NULL: none)
__device__ __forceinline__ void center_put(const double* __restrict__ pts, size_t k, int j, const CenterShift& sh,
                                           float* __restrict__ cen, double* __restrict__ raw) {
    const double x = pts[k * 3], y = pts[k * 3 + 1], z = pts[k * 3 + 2];
    cen[j * 3 + 0] = (float)(x - sh.s0); cen[j * 3 + 1] = (float)(y - sh.s1); cen[j * 3 + 2] = (float)(z - sh.s2);
    if (raw) { raw[j * 3 + 0] = x; raw[j * 3 + 1] = y; raw[j * 3 + 2] = z; }
}
