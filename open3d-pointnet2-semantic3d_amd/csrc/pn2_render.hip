// pn2_render.hip -- a headless renderer: a point cloud with per-point colours or labels becomes an image on the device.  The
// rules are in include/pn2_abi.h (pn2_render_splat); tests/render_ref.py is their numpy model.
//
//   pn2_label_colors   : one point per lane, the table staged in LDS: the label's colour, 0,0,0 and a count for a label outside it.
//   pn2_render_splat   : one point per lane.  The point is projected in float64 by a 3x4 matrix passed by value, culled in floating
//                        point before any conversion to an integer, and its size x size pixels clipped to the image.  The z-buffer
//                        holds one 64-bit key per pixel, (ordered float32 depth << 32) | global point index, and takes the
//                        unsigned minimum: nearest depth, then lowest index, whatever the order of arrival.  A pixel is read
//                        with a plain load first and the atomic skipped where the stored key is already smaller: keys only
//                        fall, so a stale (larger) value costs an atomic and never a result.  In an x-sorted scene seen from
//                        above the lanes of a wave land on neighbouring or identical pixels, and most of them lose.
//   pn2_render_resolve : one pixel per lane: key -> index, depth, colour.
// All accumulation is an integer minimum or an integer count: no result depends on the order of lanes, waves or launches.
#include <string.h>

#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_key32, ordered_to_float

namespace {

constexpr int kT = 256;
constexpr unsigned long long kEmpty = ~0ull;
constexpr double kPixelLimit = 1073741824.0;  // 2^30: |u|, |v| beyond it are culled before the conversion to int

struct RenderView {
    double m[12];  // row-major 3x4
};

struct RenderBackground {
    unsigned char c[3];
};

__global__ void __launch_bounds__(kT)
label_colors_kernel(int n, int num_class, const int* __restrict__ labels, const unsigned char* __restrict__ palette,
                    unsigned char* __restrict__ colors, unsigned long long* __restrict__ bad) {
    __shared__ unsigned char table[256 * 3];
    for (int k = threadIdx.x; k < num_class * 3; k += kT) table[k] = palette[k];
    __syncthreads();
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    bool outside = false;
    if (i < n) {
        const int l = labels[i];
        outside = l < 0 || l >= num_class;
        unsigned char* out = colors + (size_t)i * 3;
        out[0] = outside ? 0 : table[l * 3 + 0];
        out[1] = outside ? 0 : table[l * 3 + 1];
        out[2] = outside ? 0 : table[l * 3 + 2];
    }
    const unsigned long long b = __ballot(outside);
    if (bad && b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(bad, (unsigned long long)__popcll(b));
}

template <typename T>
__global__ void __launch_bounds__(kT)
render_splat_kernel(int n, int index0, const T* __restrict__ points, RenderView view, int perspective, int width, int height,
                    int size, unsigned long long* __restrict__ zbuf, unsigned long long* __restrict__ culled) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    bool out = false;
    if (i < n) {
        const T* __restrict__ p = points + (size_t)i * 3;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const double* m = view.m;
        const double t0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        const double t1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        const double d = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        double u = t0, v = t1;
        bool ok = true;
        if (perspective) {
            ok = d > 0.0;
            u = t0 / d;
            v = t1 / d;
        }
        // a NaN fails every comparison, an infinite u or v the range; d must be finite by its own test
        ok = ok && u >= -kPixelLimit && u < kPixelLimit && v >= -kPixelLimit && v < kPixelLimit && __builtin_fabs(d) <= 1.7976931348623157e308;
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        if (ok) {
            const int px = (int)__builtin_floor(u), py = (int)__builtin_floor(v);  // in [-2^30, 2^30)
            x0 = px - size / 2;
            y0 = py - size / 2;
            x1 = x0 + size < width ? x0 + size : width;
            y1 = y0 + size < height ? y0 + size : height;
            x0 = x0 > 0 ? x0 : 0;
            y0 = y0 > 0 ? y0 : 0;
            ok = x0 < x1 && y0 < y1;
        }
        out = !ok;
        if (ok) {
            const float f = (float)d + 0.0f;  // to nearest; -0 -> +0
            const unsigned long long key = ((unsigned long long)ordered_key32(f) << 32) | (unsigned)(index0 + (int)i);
            for (int py = y0; py < y1; ++py) {
                unsigned long long* row = zbuf + (size_t)py * width;
                for (int px = x0; px < x1; ++px) {
#ifdef PN2_RENDER_ALWAYS_ATOMIC  // the other arm of tools/render_cost.py --ab-library: every pixel visit is an atomic
                    atomicMin(row + px, key);
#else
                    // a plain load: what it returns is the pixel's key now or an earlier, larger one
                    const unsigned long long seen = __hip_atomic_load(row + px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    if (key < seen) atomicMin(row + px, key);
#endif
                }
            }
        }
    }
    const unsigned long long b = __ballot(out);
    if (culled && b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(culled, (unsigned long long)__popcll(b));
}

__global__ void __launch_bounds__(kT)
render_resolve_kernel(int npixels, const unsigned long long* __restrict__ zbuf, int npoints, const unsigned char* __restrict__ colors,
                      RenderBackground background, unsigned char* __restrict__ image, float* __restrict__ depth,
                      int* __restrict__ index) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    if (p >= npixels) return;
    const unsigned long long key = zbuf[p];
    const bool empty = key == kEmpty;
    const unsigned at = (unsigned)key;
    if (index) index[p] = empty ? -1 : (int)at;
    if (depth) depth[p] = empty ? __builtin_inff() : ordered_to_float((unsigned)(key >> 32));
    if (image) {
        unsigned char r = background.c[0], g = background.c[1], b = background.c[2];
        if (!empty && at < (unsigned)npoints) {  // an index beyond the colours is never read
            const unsigned char* c = colors + (size_t)at * 3;
            r = c[0];
            g = c[1];
            b = c[2];
        }
        unsigned char* out = image + (size_t)p * 3;
        out[0] = r;
        out[1] = g;
        out[2] = b;
    }
}

}  // namespace

extern "C" int pn2_label_colors(int n, int num_class, const int* labels, const uint8_t* palette, uint8_t* colors, long long* bad,
                                void* stream) {
    if (n <= 0 || num_class <= 0) return PN2_EINVAL;
    if (num_class > 256) return PN2_EUNSUP;
    if (!labels || !palette || !colors) return PN2_ENULL;
    if (((uintptr_t)labels & 3) != 0 || ((uintptr_t)bad & 7) != 0) return PN2_EINVAL;
    label_colors_kernel<<<(int)(((long long)n + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(
        n, num_class, labels, palette, colors, reinterpret_cast<unsigned long long*>(bad));
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_render_splat(int n, int index0, const void* points, int points_f64, const double* view, int perspective,
                                int width, int height, int size, unsigned long long* zbuf, long long* culled, void* stream) {
    if (n <= 0 || width <= 0 || height <= 0 || size <= 0 || (points_f64 & ~1) != 0 || (perspective & ~1) != 0) return PN2_EINVAL;
    if (index0 < 0 || (long long)index0 + n > 2147483647ll || (long long)width * height >= 2147483648ll) return PN2_ERANGE;
    if (size > 16) return PN2_EUNSUP;
    if (!points || !view || !zbuf) return PN2_ENULL;
    if (((uintptr_t)points & (points_f64 ? 7 : 3)) != 0 || (((uintptr_t)zbuf | (uintptr_t)culled) & 7) != 0) return PN2_EINVAL;
    RenderView m;
    memcpy(m.m, view, sizeof(m.m));  // by value into the launch: frozen at capture
    const int blocks = (int)(((long long)n + kT - 1) / kT);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(culled);
    if (points_f64)
        render_splat_kernel<double><<<blocks, kT, 0, s>>>(n, index0, static_cast<const double*>(points), m, perspective, width,
                                                          height, size, zbuf, count);
    else
        render_splat_kernel<float><<<blocks, kT, 0, s>>>(n, index0, static_cast<const float*>(points), m, perspective, width,
                                                         height, size, zbuf, count);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_render_resolve(int width, int height, const unsigned long long* zbuf, int npoints, const uint8_t* colors,
                                  const uint8_t* background, uint8_t* image, float* depth, int* index, void* stream) {
    if (width <= 0 || height <= 0 || npoints < 0) return PN2_EINVAL;
    if ((long long)width * height >= 2147483648ll) return PN2_ERANGE;
    if (!zbuf || (!image && !depth && !index) || (image && (!background || (!colors && npoints > 0)))) return PN2_ENULL;
    if (((uintptr_t)zbuf & 7) != 0 || (((uintptr_t)depth | (uintptr_t)index) & 3) != 0) return PN2_EINVAL;
    RenderBackground bg = {{0, 0, 0}};
    if (image) memcpy(bg.c, background, 3);
    const int npixels = width * height;
    render_resolve_kernel<<<(int)(((long long)npixels + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(
        npixels, zbuf, npoints, colors, bg, image, depth, index);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
