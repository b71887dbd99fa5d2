// pn2_store.hip -- one scene of the SemanticDataset store built on the device: SemanticFileData.__init__
// (dataset/semantic_dataset.py:84-88 of the reference: sort by x, gather points / labels / colours) and what
// SemanticDataset.__init__ (:214-290) takes from the sorted scene (scene_z_size, the label histogram), written straight into
// the scene's slice of the resident store.  The rule is in include/pn2_abi.h (pn2_scene_ingest).
//
//   1 ingest_key_kernel    : one row per lane; key = ordered_key(x) with -0.0 folded onto +0.0, payload = row index; a
//                            non-finite x, y or z raises bit 0 of the flags (one atomic per wave that saw one);
//   2 hipcub radix sort    : 64 key bits, pairs, stable: ties in x keep their input order (np.argsort(kind="stable"));
//   3 ingest_gather_kernel : one OUTPUT row per lane: perm, 24-byte point row, 3 colours float64 -> float32, label -> uint8;
//                            z min / max as ordered keys (wave, LDS, one atomicMin / atomicMax per workgroup), the label
//                            histogram (ballots, LDS, one 64-bit atomic per non-zero bin per workgroup), the label range
//                            (a ballot; bit 1 of the flags);
//   4 ingest_finish_kernel : keys -> out_zrange, flags -> status.
// Every reduction is in integers or ordered keys: no result depends on the order in which workgroups arrive.
//
// What bounds the gather: its writes are coalesced (24 + 12 + 1 + 4 bytes per row, consecutive lanes consecutive rows), its
// reads are not: each lane reads a 24-byte point row, a 24-byte colour row and a 4-byte label at a random row of the input, so
// each wave-instruction touches up to 64 different 128-byte lines of which it uses 8 bytes (a row straddles two lines one time
// in 16 * 3).  The input of a scene (tens of MB) sits in the Infinity Cache after the key kernel's pass, so the kernel runs at
// the rate the memory system turns random 64-byte requests around, not at the HBM byte rate; nine independent loads per lane
// and eight waves per SIMD are what hides their latency.
#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_key, ordered_to_double
#include "pn2_sort.h"     // IndexSort
#include "pn2_wg.h"       // finite64, WsCarver

namespace {

constexpr int kT = 256;  // threads per workgroup: one row per lane
constexpr int kWaves = kT / 64;
constexpr int kHistBins = 9;
enum { FLAG_NONFINITE = 1, FLAG_LABEL = 2 };

struct Scal {  // the scalars the kernels reduce into (workspace)
    unsigned long long zmin, zmax;  // ordered keys
    unsigned flags;
};

struct Ws {  // workspace carve-up
    IndexSort<unsigned long long> sort;
    Scal* scal;
};
inline int ws_layout(int n, WsCarver& c, Ws* w) {
    w->sort.carve(c, (size_t)n);
    w->scal = c.take<Scal>(1);
    return w->sort.carve_tmp(c, n, 0, 64);
}

__global__ void __launch_bounds__(kT)
ingest_key_kernel(int n, const double* __restrict__ pts, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                  Scal* __restrict__ scal) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const double x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        bad = !(finite64(x) && finite64(y) && finite64(z));
        keys[i] = ordered_key(x == 0.0 ? 0.0 : x);  // -0.0 == +0.0: one key for both
        vals[i] = (int)i;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&scal->flags, (unsigned)FLAG_NONFINITE);
}

__global__ void __launch_bounds__(kT)
ingest_gather_kernel(int n, const int* __restrict__ perm, const double* __restrict__ pts, const double* __restrict__ col,
                     const int* __restrict__ lab, double* __restrict__ out_pts, float* __restrict__ out_col,
                     unsigned char* __restrict__ out_lab, int* __restrict__ out_perm, unsigned long long* __restrict__ out_hist,
                     Scal* __restrict__ scal) {
    __shared__ unsigned long long s_min[kWaves], s_max[kWaves];
    __shared__ unsigned s_hist[kHistBins];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * kT + tid;
    const bool live = i < n;
    if (tid < kHistBins) s_hist[tid] = 0u;
    __syncthreads();
    unsigned long long kmin = ~0ull, kmax = 0ull;
    int bin = -1;  // histogram bin of this row's label; -1: counted nowhere
    bool bad_label = false;
    if (live) {
        const long long src = perm[i];
        const double x = pts[src * 3], y = pts[src * 3 + 1], z = pts[src * 3 + 2];
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if (col) { c0 = col[src * 3]; c1 = col[src * 3 + 1]; c2 = col[src * 3 + 2]; }
        const int L = lab ? lab[src] : 0;
        out_pts[i * 3] = x; out_pts[i * 3 + 1] = y; out_pts[i * 3 + 2] = z;
        if (col) { out_col[i * 3] = (float)c0; out_col[i * 3 + 1] = (float)c1; out_col[i * 3 + 2] = (float)c2; }
        out_lab[i] = (unsigned char)L;
        if (out_perm) out_perm[i] = (int)src;
        kmin = kmax = ordered_key(z);
        bad_label = L < 0 || L > 255;
        bin = (L >= 0 && L <= 9) ? (L < 9 ? L : 8) : -1;  // np.histogram(labels, range(10)): the last bin is [8, 9]
    }
    // label histogram: per bin one ballot per wave, counted into LDS by the wave's first lane
#pragma unroll
    for (int b = 0; b < kHistBins; ++b) {
        const unsigned long long m = __ballot(bin == b);
        if (lane == 0 && m != 0ull) atomicAdd(&s_hist[b], (unsigned)__popcll(m));
    }
    const unsigned long long anybad = __ballot(bad_label);
    if (lane == 0 && anybad != 0ull) atomicOr(&scal->flags, (unsigned)FLAG_LABEL);
    // z range
    kmin = pn2_wave_all_min(kmin); kmax = pn2_wave_all_max(kmax);
    if (lane == 0) { s_min[wave] = kmin; s_max[wave] = kmax; }
    __syncthreads();
    if (tid == 0) {  // every workgroup holds at least one live row
        unsigned long long lo = s_min[0], hi = s_max[0];
        for (int w = 1; w < kWaves; ++w) { lo = s_min[w] < lo ? s_min[w] : lo; hi = s_max[w] > hi ? s_max[w] : hi; }
        atomicMin(&scal->zmin, lo);
        atomicMax(&scal->zmax, hi);
    }
    if (tid < kHistBins && s_hist[tid] != 0u) atomicAdd(&out_hist[tid], (unsigned long long)s_hist[tid]);
}

__global__ void ingest_finish_kernel(const Scal* __restrict__ scal, double* __restrict__ out_zrange, int* __restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out_zrange[0] = ordered_to_double(scal->zmin);
    out_zrange[1] = ordered_to_double(scal->zmax);
    const unsigned f = scal->flags;
    *status = (f & FLAG_NONFINITE) ? 1 : ((f & FLAG_LABEL) ? 2 : 0);
}

}  // namespace

extern "C" int pn2_scene_ingest_workspace_size(int n, unsigned long long* bytes) {
    if (n <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    const int rc = ws_layout(n, c, &w);
    if (rc != PN2_OK) return rc;
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_scene_ingest(int n, const double* points, const double* colors, const int* labels, double* out_points,
                                float* out_colors, unsigned char* out_labels, int* out_perm, double* out_zrange,
                                long long* out_hist, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (n <= 0) return PN2_EINVAL;
    if (!points || !out_points || !out_labels || !out_zrange || !out_hist || !status || !workspace) return PN2_ENULL;
    if (colors && !out_colors) return PN2_ENULL;
    if ((((uintptr_t)points | (uintptr_t)colors | (uintptr_t)out_points | (uintptr_t)out_zrange | (uintptr_t)out_hist) & 7) != 0 ||
        (((uintptr_t)labels | (uintptr_t)out_colors | (uintptr_t)out_perm | (uintptr_t)status) & 3) != 0 ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    const int rc = ws_layout(n, c, &w);  // too small: refused before the sort is asked for its share
    if (rc != PN2_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scal* scal = w.scal;
    hipError_t e = hipMemsetAsync(&scal->zmin, 0xFF, sizeof(unsigned long long), st);  // running minimum: all ones
    if (e == hipSuccess) e = hipMemsetAsync(&scal->zmax, 0, sizeof(Scal) - offsetof(Scal, zmax), st);  // maximum, flags
    if (e == hipSuccess) e = hipMemsetAsync(out_hist, 0, kHistBins * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    const int blocks = (int)(((long long)n + kT - 1) / kT);
    ingest_key_kernel<<<blocks, kT, 0, st>>>(n, points, w.sort.keys_in, w.sort.vals_in, scal);
    e = w.sort.run(n, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    ingest_gather_kernel<<<blocks, kT, 0, st>>>(n, w.sort.vals_out, points, colors, labels, out_points, colors ? out_colors : nullptr,
                                                out_labels, out_perm, reinterpret_cast<unsigned long long*>(out_hist), scal);
    ingest_finish_kernel<<<1, 64, 0, st>>>(scal, out_zrange, status);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
