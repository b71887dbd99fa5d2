// pn2_augment.hip -- util/provider.py of the reference as one pipeline on a device-resident batch: shuffle, rotation (axis and
// / or small-angle perturbation, normals too), scale, shift, jitter, dropout.  The contract -- stage order, the arithmetic
// rule, how every draw is formed -- is written in include/pn2_abi.h; this file is its mechanism.
//
// Three launches per call, no host synchronisation:
//   1 aug_prologue : one workgroup.  Device mode: reads the batch counter ONCE, snapshots it into the workspace, advances it,
//                    and forms the per-cloud parameters (matrix, scale, shift, ratio; float64) from the snapshot.  Replay
//                    mode: copies the given parameters.  With in == out and dropout it also keeps row 0 of every cloud.
//   2 aug_perm     : only with the shuffle.  perm[rank of i among the 64-bit keys, ties by index] = i.  A rank count: the
//                    keys are hashes, so every workgroup forms them tile by tile in LDS (256 keys, read back as broadcasts)
//                    instead of sorting: 64 indices per workgroup, a quarter of every tile per wave, n^2 / 64 hashes and
//                    n^2 compares -- 67 M compares at n = 8192, 4.3 G at 65536 -- no key buffer, no LDS limit on n.
//   3 aug_rows     : grid (row tiles, b), 256 lanes, one row per lane, 64-bit row offsets.  C == 6 rows (24 bytes) on an
//                    8-byte aligned address move as one 16-byte and one 8-byte piece; everything else as plain elements, so
//                    any element-aligned base works.
#include "pn2_common.h"
#include "pn2_rng.h"
#include "pn2_wg.h"  // al256

namespace {

constexpr int kT = 256;
constexpr int kPermIdx = 64;        // indices a workgroup of the permutation launch ranks
constexpr int kP = PN2_AUG_PARAMS;  // doubles per cloud: R (9), scale, shift (3), ratio, 0, 0
constexpr unsigned long long kTag = 1ull << 41;
constexpr unsigned long long kTagAngle = kTag, kTagPerturb = kTag + 2, kTagScale = kTag + 8, kTagShift = kTag + 9,
                             kTagRatio = kTag + 12, kTagJitter = 2 * kTag, kTagDrop = 4 * kTag, kTagPerm = 8 * kTag;

// workspace: [counter snapshot | params (b, kP) f64 | row 0 of every cloud (b, PN2_AUG_INPLACE_MAX_C) f32]
inline size_t ws_params_off() { return 256; }
inline size_t ws_row0_off(int b) { return 256 + al256((size_t)b * kP * 8); }
inline size_t ws_bytes(int b) { return ws_row0_off(b) + al256((size_t)b * PN2_AUG_INPLACE_MAX_C * 4); }

struct Aug {
    int b, n, c, flags, axis, cj;
    double p_sigma, p_clip, s_lo, s_hi, t_range, j_sigma, j_clip, d_max;
    unsigned long long seed;
    const int* perm;  // the permutation the rows read: draw_perm (replay) or out_perm
    const double* matrix;
    const double* scale;
    const double* shift;
    const double* noise;
    const double* ratio;
    const double* u;
};

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }  // np.clip
__device__ __forceinline__ double normal_draw(unsigned long long h, unsigned long long i) {
    const double u1 = unit53(draw64(h, i)), u2 = unit53(draw64(h, i + 1));
    return sqrt(-2.0 * log(1.0 - u1)) * cos((u2 * 2.0) * M_PI);
}
// c = a . b (3x3, row-major), np.dot's result in the plain order
__device__ __forceinline__ void mat3(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// ---- launch 1 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
aug_prologue_kernel(Aug a, long long* __restrict__ counter, long long* __restrict__ snap, double* __restrict__ params,
                    double* __restrict__ out_params, const float* __restrict__ in, float* __restrict__ row0) {
    const int tid = threadIdx.x;
    const bool replay = a.flags & PN2_AUG_REPLAY;
    unsigned long long ctr = 0;
    if (!replay) {
        ctr = (unsigned long long)counter[0];  // every thread reads it, the barrier follows, then one thread advances it
        __syncthreads();
        if (tid == 0) { snap[0] = (long long)ctr; counter[0] = (long long)(ctr + 1); }
    }
    for (int s = tid; s < a.b; s += kT) {
        double p[kP] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0};
        if (replay) {
            if (a.flags & (PN2_AUG_ROTATE | PN2_AUG_PERTURB))
                for (int k = 0; k < 9; ++k) p[k] = a.matrix[(size_t)s * 9 + k];
            if (a.flags & PN2_AUG_SCALE) p[9] = a.scale[s];
            if (a.flags & PN2_AUG_SHIFT)
                for (int k = 0; k < 3; ++k) p[10 + k] = a.shift[(size_t)s * 3 + k];
            if (a.flags & PN2_AUG_DROPOUT) p[13] = a.ratio[s];
        } else {
            const unsigned long long h = sample_stream(a.seed, ctr, s);
            double ra[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            if (a.flags & PN2_AUG_ROTATE) {  // provider.py: np.random.uniform() * 2 * np.pi, the reference's matrix per axis
                const double ang = (unit53(draw64(h, kTagAngle)) * 2.0) * M_PI;
                const double cs = cos(ang), sn = sin(ang);
                if (a.axis == 0) { ra[4] = cs; ra[5] = sn; ra[7] = -sn; ra[8] = cs; }
                else if (a.axis == 1) { ra[0] = cs; ra[2] = sn; ra[6] = -sn; ra[8] = cs; }
                else { ra[0] = cs; ra[1] = sn; ra[3] = -sn; ra[4] = cs; }
            }
            if (a.flags & PN2_AUG_PERTURB) {
                double g[3];
                for (int k = 0; k < 3; ++k)
                    g[k] = clipd(a.p_sigma * normal_draw(h, kTagPerturb + 2 * k), -a.p_clip, a.p_clip);
                const double rx[9] = {1, 0, 0, 0, cos(g[0]), -sin(g[0]), 0, sin(g[0]), cos(g[0])};
                const double ry[9] = {cos(g[1]), 0, sin(g[1]), 0, 1, 0, -sin(g[1]), 0, cos(g[1])};
                const double rz[9] = {cos(g[2]), -sin(g[2]), 0, sin(g[2]), cos(g[2]), 0, 0, 0, 1};
                double ryx[9], rp[9];
                mat3(ry, rx, ryx);
                mat3(rz, ryx, rp);
                if (a.flags & PN2_AUG_ROTATE) mat3(ra, rp, p);
                else
                    for (int k = 0; k < 9; ++k) p[k] = rp[k];
            } else {
                for (int k = 0; k < 9; ++k) p[k] = ra[k];
            }
            if (a.flags & PN2_AUG_SCALE) p[9] = a.s_lo + (a.s_hi - a.s_lo) * unit53(draw64(h, kTagScale));
            if (a.flags & PN2_AUG_SHIFT)
                for (int k = 0; k < 3; ++k)
                    p[10 + k] = -a.t_range + (a.t_range - (-a.t_range)) * unit53(draw64(h, kTagShift + k));
            if (a.flags & PN2_AUG_DROPOUT) p[13] = unit53(draw64(h, kTagRatio)) * a.d_max;
        }
        for (int k = 0; k < kP; ++k) {
            params[(size_t)s * kP + k] = p[k];
            if (out_params) out_params[(size_t)s * kP + k] = p[k];
        }
    }
    if (row0)  // in == out with dropout (c <= PN2_AUG_INPLACE_MAX_C): the rows launch overwrites row 0 while others still need it
        for (int i = tid; i < a.b * a.c; i += kT) {
            const int s = i / a.c, ch = i - s * a.c;
            row0[(size_t)s * PN2_AUG_INPLACE_MAX_C + ch] = in[(size_t)s * a.n * a.c + ch];
        }
}

// ---- launch 2 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
aug_perm_kernel(Aug a, const long long* __restrict__ snap, int* __restrict__ out_perm) {
    __shared__ unsigned long long tile[kT];
    __shared__ int part[kT];
    const int tid = threadIdx.x, n = a.n, lane = tid & 63, wave = tid >> 6;
    if (a.flags & PN2_AUG_REPLAY) {  // the given permutation is also the output
        const long long i = (long long)blockIdx.x * kPermIdx + tid;
        if (tid < kPermIdx && i < n) out_perm[i] = a.perm[i];
        return;
    }
    // a workgroup ranks kPermIdx = 64 indices: lane l of every wave holds index 64 * block + l, wave w counts the keys of its
    // quarter [64 w, 64 w + 64) of each tile (every lane of a wave reads the same LDS word: a broadcast), the four partial
    // counts meet in LDS.  A slot past n holds the largest key: no key is below it, and at equal keys its index is above i.
    const long long i = (long long)blockIdx.x * kPermIdx + lane;
    const unsigned long long h = sample_stream(a.seed, (unsigned long long)snap[0], -1);
    const unsigned long long ka = i < n ? draw64(h, kTagPerm + (unsigned long long)i) : 0ull;
    int rank = 0;
    for (long long t0 = 0; t0 < n; t0 += kT) {
        tile[tid] = t0 + tid < n ? draw64(h, kTagPerm + (unsigned long long)(t0 + tid)) : ~0ull;
        __syncthreads();
        // the 64 slots of this wave's quarter are this workgroup's own indices, or all below them, or all above them (both
        // ranges start at multiples of 64): only the first case needs the index in the compare
        const long long q0 = t0 + wave * 64, own = (long long)blockIdx.x * kPermIdx;
        const unsigned long long* __restrict__ tq = tile + wave * 64;
        if (q0 == own) {
#pragma unroll 16
            for (int q = 0; q < 64; ++q) rank += (tq[q] < ka) || (tq[q] == ka && q0 + q < i);
        } else if (q0 < own) {
#pragma unroll 16
            for (int q = 0; q < 64; ++q) rank += tq[q] <= ka;
        } else {
#pragma unroll 16
            for (int q = 0; q < 64; ++q) rank += tq[q] < ka;
        }
        __syncthreads();
    }
    part[tid] = rank;
    __syncthreads();
    if (wave == 0 && i < n)  // (key, index) is a strict total order: the ranks of [0, n) are [0, n)
        out_perm[part[lane] + part[64 + lane] + part[128 + lane] + part[192 + lane]] = (int)i;
}

// ---- launch 3 --------------------------------------------------------------------------------------------------------
// the first m (<= 6) channels of a row; 24-byte rows move as 16 + 8 bytes when the address allows it
__device__ __forceinline__ void load_head(const float* __restrict__ r, int c, int m, float* f) {
    const uintptr_t ad = (uintptr_t)r;
    if (c == 6 && (ad & 7) == 0) {
        if ((ad & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(r);
            const float2 w = *reinterpret_cast<const float2*>(r + 4);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; f[4] = w.x; f[5] = w.y;
        } else {
            const float2 w = *reinterpret_cast<const float2*>(r);
            const float4 v = *reinterpret_cast<const float4*>(r + 2);
            f[0] = w.x; f[1] = w.y; f[2] = v.x; f[3] = v.y; f[4] = v.z; f[5] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) f[k] = k < m ? r[k] : 0.f;
    }
}
__device__ __forceinline__ void store_head(float* __restrict__ o, int c, int m, const float* f) {
    const uintptr_t ad = (uintptr_t)o;
    if (c == 6 && (ad & 7) == 0) {
        if ((ad & 15) == 0) {
            *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
            *reinterpret_cast<float2*>(o + 4) = make_float2(f[4], f[5]);
        } else {
            *reinterpret_cast<float2*>(o) = make_float2(f[0], f[1]);
            *reinterpret_cast<float4*>(o + 2) = make_float4(f[2], f[3], f[4], f[5]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < m) o[k] = f[k];
    }
}

// clip(sigma * z) of row jn, channel ch of cloud s (ch < cj)
__device__ __forceinline__ double jitter_of(const Aug& a, unsigned long long h, int s, long long jn, int ch) {
    const long long at = jn * a.cj + ch;
    const double z = (a.flags & PN2_AUG_REPLAY) ? a.noise[(size_t)s * a.n * a.cj + at]
                                                : normal_draw(h, kTagJitter + 2ull * (unsigned long long)at);
    return clipd(a.j_sigma * z, -1 * a.j_clip, a.j_clip);
}

__global__ void __launch_bounds__(kT)
aug_rows_kernel(Aug a, const long long* __restrict__ snap, const double* __restrict__ params, const float* __restrict__ row0,
                const float* in, const int* in_labels, const float* in_weights, float* out, int* out_labels,
                float* out_weights) {
    const int s = blockIdx.y, n = a.n, c = a.c, fl = a.flags;
    const long long j = (long long)blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const bool replay = fl & PN2_AUG_REPLAY;
    const unsigned long long h = replay ? 0ull : sample_stream(a.seed, (unsigned long long)snap[0], s);
    double p[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) p[k] = params[(size_t)s * kP + k];
    const size_t cloud = (size_t)s * n;
    long long src = j;
    if (fl & PN2_AUG_SHUFFLE) {
        const int q = a.perm[j];
        if ((unsigned)q < (unsigned)n) src = q;
    }
    if (out_labels) out_labels[cloud + j] = in_labels[cloud + src];
    if (out_weights) out_weights[cloud + j] = in_weights[cloud + src];
    // the row whose stages 1-4 this lane computes: its own, or row 0 of the cloud when it is dropped
    long long jn = j;
    const float* r = in + (cloud + src) * c;
    if ((fl & PN2_AUG_DROPOUT) && j != 0) {
        const double u = replay ? a.u[cloud + j] : unit53(draw64(h, kTagDrop + (unsigned long long)j));
        if (u <= p[13]) {
            jn = 0;
            if (row0) {
                r = row0 + (size_t)s * PN2_AUG_INPLACE_MAX_C;
            } else {
                long long s0 = 0;
                if (fl & PN2_AUG_SHUFFLE) {
                    const int q = a.perm[0];
                    if ((unsigned)q < (unsigned)n) s0 = q;
                }
                r = in + (cloud + s0) * c;
            }
        }
    }
    float* o = out + (cloud + j) * c;
    const int m = c < 6 ? c : 6;
    float f[6];
    load_head(r, c, m, f);  // (a kept row 0 starts a 256-byte slot of the workspace)
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = (double)f[k];
    if (fl & (PN2_AUG_ROTATE | PN2_AUG_PERTURB)) {
        const double x = v[0], y = v[1], z = v[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (x * p[k] + y * p[3 + k]) + z * p[6 + k];
        if (fl & PN2_AUG_ROTATE_NORMALS) {
            const double nx = v[3], ny = v[4], nz = v[5];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 + k] = (nx * p[k] + ny * p[3 + k]) + nz * p[6 + k];
        }
    }
    if (fl & PN2_AUG_SCALE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] * p[9];
    }
    if (fl & PN2_AUG_SHIFT) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] + p[10 + k];
    }
    if (fl & PN2_AUG_JITTER) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < a.cj && k < m) v[k] = v[k] + jitter_of(a, h, s, jn, k);
    }
    // channels past the sixth: copied, or jittered with PN2_AUG_JITTER_ALL.  Read before this row's head is stored (in == out)
    const bool jall = (fl & PN2_AUG_JITTER) && a.cj == c;
    float g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = (float)v[k];
    for (int k = 6; k < c; ++k) {
        double w = (double)r[k];
        if (jall) w = w + jitter_of(a, h, s, jn, k);
        o[k] = (float)w;
    }
    store_head(o, c, m, g);
}

}  // namespace

extern "C" int pn2_augment_workspace_bytes(int b, unsigned long long* bytes) {
    if (b <= 0 || b > 65535) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    *bytes = (unsigned long long)ws_bytes(b);
    return PN2_OK;
}

extern "C" int pn2_augment(int b, int n, int c, int flags, int rotate_axis, double perturb_sigma, double perturb_clip,
                           double scale_lo, double scale_hi, double shift_range, double jitter_sigma, double jitter_clip,
                           double dropout_max, unsigned long long seed, long long* counter, const int* draw_perm,
                           const double* draw_matrix, const double* draw_scale, const double* draw_shift,
                           const double* draw_noise, const double* draw_ratio, const double* draw_u, const float* in,
                           const int* in_labels, const float* in_weights, void* workspace, size_t workspace_bytes,
                           double* out_params, int* out_perm, float* out, int* out_labels, float* out_weights, void* stream) {
    constexpr int kAll = PN2_AUG_SHUFFLE | PN2_AUG_ROTATE | PN2_AUG_PERTURB | PN2_AUG_SCALE | PN2_AUG_SHIFT | PN2_AUG_JITTER |
                         PN2_AUG_DROPOUT | PN2_AUG_ROTATE_NORMALS | PN2_AUG_JITTER_ALL | PN2_AUG_REPLAY;
    if (b <= 0 || n <= 0 || c < 3 || b > 65535 || (flags & ~kAll)) return PN2_EINVAL;
    const bool replay = flags & PN2_AUG_REPLAY, rot = flags & (PN2_AUG_ROTATE | PN2_AUG_PERTURB);
    if ((flags & PN2_AUG_ROTATE_NORMALS) && c < 6) return PN2_EINVAL;
    if (!replay) {  // the parameters the device draws from
        if ((flags & PN2_AUG_ROTATE) && (rotate_axis < 0 || rotate_axis > 2)) return PN2_EINVAL;
        if ((flags & PN2_AUG_PERTURB) && !(perturb_sigma >= 0 && perturb_clip > 0)) return PN2_EINVAL;
        if ((flags & PN2_AUG_SCALE) && !(scale_lo <= scale_hi)) return PN2_EINVAL;
        if ((flags & PN2_AUG_SHIFT) && !(shift_range >= 0)) return PN2_EINVAL;
        if ((flags & PN2_AUG_DROPOUT) && !(dropout_max >= 0 && dropout_max <= 1)) return PN2_EINVAL;
    }
    if ((flags & PN2_AUG_JITTER) && !(jitter_sigma >= 0 && jitter_clip > 0)) return PN2_EINVAL;
    if ((flags & PN2_AUG_SHUFFLE) && in && (const void*)in == (const void*)out) return PN2_EINVAL;
    if ((in_labels == nullptr) != (out_labels == nullptr) || (in_weights == nullptr) != (out_weights == nullptr)) return PN2_EINVAL;
    if ((long long)n * c >= (1ll << 40)) return PN2_ERANGE;  // the jitter indices of a cloud stay inside their tag space
    if (!in || !out || !workspace) return PN2_ENULL;
    if (!replay && !counter) return PN2_ENULL;
    if ((flags & PN2_AUG_SHUFFLE) && (!out_perm || (replay && !draw_perm))) return PN2_ENULL;
    if (replay && ((rot && !draw_matrix) || ((flags & PN2_AUG_SCALE) && !draw_scale) || ((flags & PN2_AUG_SHIFT) && !draw_shift) ||
                   ((flags & PN2_AUG_JITTER) && !draw_noise) || ((flags & PN2_AUG_DROPOUT) && (!draw_ratio || !draw_u))))
        return PN2_ENULL;
    if (workspace_bytes < ws_bytes(b) || ((uintptr_t)workspace & 255) != 0) return PN2_EINVAL;
    const bool keep_row0 = (flags & PN2_AUG_DROPOUT) && in == out;
    if (keep_row0 && c > PN2_AUG_INPLACE_MAX_C) return PN2_EUNSUP;
    unsigned char* base = static_cast<unsigned char*>(workspace);
    long long* snap = reinterpret_cast<long long*>(base);
    double* params = reinterpret_cast<double*>(base + ws_params_off());
    float* row0 = keep_row0 ? reinterpret_cast<float*>(base + ws_row0_off(b)) : nullptr;
    Aug a;
    a.b = b; a.n = n; a.c = c; a.flags = flags; a.axis = rotate_axis;
    a.cj = (flags & PN2_AUG_JITTER_ALL) ? c : 3;
    a.p_sigma = perturb_sigma; a.p_clip = perturb_clip; a.s_lo = scale_lo; a.s_hi = scale_hi; a.t_range = shift_range;
    a.j_sigma = jitter_sigma; a.j_clip = jitter_clip; a.d_max = dropout_max; a.seed = seed;
    a.perm = replay ? draw_perm : out_perm;
    a.matrix = draw_matrix; a.scale = draw_scale; a.shift = draw_shift; a.noise = draw_noise; a.ratio = draw_ratio; a.u = draw_u;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    aug_prologue_kernel<<<1, kT, 0, sm>>>(a, counter, snap, params, out_params, in, row0);
    if (flags & PN2_AUG_SHUFFLE) aug_perm_kernel<<<(n + kPermIdx - 1) / kPermIdx, kT, 0, sm>>>(a, snap, out_perm);
    aug_rows_kernel<<<dim3((n + kT - 1) / kT, b), kT, 0, sm>>>(a, snap, params, row0, in, in_labels, in_weights, out, out_labels,
                                                               out_weights);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
