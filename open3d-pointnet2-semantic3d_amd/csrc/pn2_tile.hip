// pn2_tile.hip -- the tiled cover of one scene of the SemanticDataset store: every point of the scene predicted once per pass
// (the whole-scene evaluation of PointNet++'s ScanNet code, on the columns this network is trained on).  The rule is in
// include/pn2_abi.h (pn2_tile_plan).
//
//   pn2_tile_plan   : rules 1-3.  The scene's tiles, the order of its points by tile, the table of samples.
//     1 tp_ymin_kernel   : one row per lane; min y as an ordered key (wave, LDS, one atomicMin per workgroup); a non-finite x or y
//                          raises bit 0 of the flags;
//     2 tp_key_kernel    : key = (i << 32) | j, i = floor((x - ox) / box_size_x), j likewise: float64 subtraction, float64
//                          DIVISION, floor; an index outside [0, 2^31) raises bit 1 and takes key 0; payload = scene position;
//     3 hipcub radix sort: 64 key bits, pairs, stable: equal tiles keep ascending scene position.  Its payload output IS `order`;
//     4 tp_head_count    : per chunk of kChunk sorted positions, how many start a tile (key differs from its predecessor's);
//     5 tp_scan_kernel   : one workgroup: the chunk counts -> exclusive prefixes, the total -> n_tiles;
//     6 tp_head_emit     : the tile starts, ascending, by an ordered in-chunk compaction (ballots);
//     7 tp_tile_count    : per chunk of kChunk TILES the sum of S = ceil(m / npts) (0 below min_points); the skipped points;
//     8 tp_scan_kernel   : again, over those sums -> n_samples;
//     9 tp_rows_emit     : the table rows [a, m, s, S] of every tile at its prefix; the header.
//   pn2_tile_gather : rule 4.  kGatherSplit-or-fewer workgroups per sample: each takes the float64 minimum over the sample's live
//                     rows (the refill rows repeat them), then writes its share of the rows.
//   pn2_tile_vote   : rule 5.  One batch row per lane, one integer atomic per counted row.
//   pn2_tile_labels : rule 6.  One point per lane.
// Every reduction is in integers or ordered keys: no result depends on the order in which workgroups arrive.
//
// What bounds the gather: as in pn2_store.hip, the writes are coalesced (consecutive lanes, consecutive 12- or 24-byte rows) and
// the reads are not -- a lane reads `order` at stride S ints, then a 24-byte point row and a 12-byte colour row where that entry
// points.  The members of a tile lie in the x-slab of its column (the store is sorted by x), interleaved with the slab's other
// tiles, so a sample's rows come from a few MB that the key and sort passes of the plan left in the Infinity Cache; the kernel
// runs at the rate the memory system turns those small requests around.  Rows go through registers: a row is far shorter than
// the 1 KiB pieces for which staging an indexed gather in LDS pays, and nothing reads a row twice.
#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_key, ordered_to_double
#include "pn2_sort.h"     // IndexSort
#include "pn2_wg.h"       // wg_sum, wg_excl_scan_flag, wg_excl_scan_int, finite64, finite_host, WsCarver

namespace {

constexpr int kT = 256;          // threads per workgroup of the chunked launches
constexpr int kWaves = kT / 64;
constexpr int kChunk = 1024;     // sorted positions (launches 4, 6) or tiles (7, 9) per chunk: 4 ordered passes of kT
constexpr int kScanT = 256;      // threads of the one-workgroup scan over the chunks: ceil(chunks / kScanT) chunks per thread
constexpr int kInlineRows = 4;   // a tile of at most this many samples has its table rows written by its own lane
constexpr int kGatherSplit = 8;  // most workgroups that share one sample of the gather
constexpr int kGatherRows = 1024;  // rows per workgroup before a sample is split
enum { FLAG_NONFINITE = 1, FLAG_INDEX = 2 };

struct Scal {  // the scalars the kernels reduce into (workspace; cleared by the call)
    unsigned long long ymin;  // ordered key
    unsigned flags;
    int n_tiles, n_samples, skipped;
};

inline int chunks_of(int n) { return (n + kChunk - 1) / kChunk; }

struct Ws {  // workspace carve-up
    IndexSort<unsigned long long> sort;  // its sorted row indices are the caller's `order`
    int *tile_start, *chunk_a, *chunk_b;
    Scal* scal;
};
inline int ws_layout(int n, int* order, WsCarver& c, Ws* w) {
    w->sort.carve_into(c, (size_t)n, order);
    w->tile_start = c.take<int>((size_t)n);
    w->chunk_a = c.take<int>((size_t)chunks_of(n));
    w->chunk_b = c.take<int>((size_t)chunks_of(n));
    w->scal = c.take<Scal>(1);
    return w->sort.carve_tmp(c, n, 0, 64);
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
tp_ymin_kernel(int n, const double* __restrict__ pts, Scal* __restrict__ scal) {
    __shared__ unsigned long long s_min[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * kT + tid;
    unsigned long long kmin = ~0ull;
    bool bad = false;
    if (i < n) {
        const double x = pts[i * 3], y = pts[i * 3 + 1];
        bad = !(finite64(x) && finite64(y));
        kmin = ordered_key(y);  // -0.0 directly below +0.0
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&scal->flags, (unsigned)FLAG_NONFINITE);
    kmin = pn2_wave_all_min(kmin);
    if (lane == 0) s_min[wave] = kmin;
    __syncthreads();
    if (tid == 0) {  // every workgroup holds at least one live row
        unsigned long long lo = s_min[0];
        for (int w = 1; w < kWaves; ++w) lo = s_min[w] < lo ? s_min[w] : lo;
        atomicMin(&scal->ymin, lo);
    }
}

__global__ void __launch_bounds__(kT)
tp_key_kernel(int n, const double* __restrict__ pts, double bx, double by, double phase_x, double phase_y,
              unsigned long long* __restrict__ keys, int* __restrict__ vals, Scal* __restrict__ scal) {
    const long long p = (long long)blockIdx.x * kT + threadIdx.x;
    bool bad = false;
    if (p < n) {
        const double ox = pts[0] - phase_x;                          // the scene is sorted by x: its first row holds the minimum
        const double oy = ordered_to_double(scal->ymin) - phase_y;
        const double fi = floor((pts[p * 3] - ox) / bx);             // a division, never a product with 1 / box
        const double fj = floor((pts[p * 3 + 1] - oy) / by);
        bad = !(fi >= 0.0 && fi < 2147483648.0 && fj >= 0.0 && fj < 2147483648.0);  // (a NaN fails every comparison)
        keys[p] = bad ? 0ull : (((unsigned long long)(unsigned)(int)fi << 32) | (unsigned long long)(unsigned)(int)fj);
        vals[p] = (int)p;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&scal->flags, (unsigned)FLAG_INDEX);
}

__device__ __forceinline__ bool is_head(int n, const unsigned long long* __restrict__ keys, int p) {
    return p < n && (p == 0 || keys[p] != keys[p - 1]);
}

__global__ void __launch_bounds__(kT)
tp_head_count_kernel(int n, const unsigned long long* __restrict__ keys, int* __restrict__ chunk_cnt) {
    __shared__ int red[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int it = 0; it < kChunk / kT; ++it) mine += is_head(n, keys, ch * kChunk + it * kT + tid);
    const int tot = wg_sum<kWaves>(mine, red);
    if (tid == 0) chunk_cnt[ch] = tot;
}

// one workgroup: v[0 .. items) -> its exclusive prefixes, in place; *total = the sum.  Thread t owns the `per` consecutive items
// from t * per.
__global__ void __launch_bounds__(kScanT)
tp_scan_kernel(int items, int* __restrict__ v, int* __restrict__ total) {
    __shared__ int wsum[kScanT / 64];
    const int tid = threadIdx.x;
    const int per = (items + kScanT - 1) / kScanT;
    const int lo = tid * per < items ? tid * per : items;
    const int hi = lo + per < items ? lo + per : items;
    int mine = 0;
    for (int k = lo; k < hi; ++k) mine += v[k];
    int tot;
    int run = wg_excl_scan_int<kScanT / 64>(mine, wsum, tot);
    for (int k = lo; k < hi; ++k) {
        const int c = v[k];
        v[k] = run;
        run += c;
    }
    if (tid == 0) *total = tot;
}

__global__ void __launch_bounds__(kT)
tp_head_emit_kernel(int n, const unsigned long long* __restrict__ keys, const int* __restrict__ chunk_off,
                    int* __restrict__ tile_start) {
    __shared__ int wsum[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x;
    int run = chunk_off[ch];  // tiles that start before this chunk
    for (int it = 0; it < kChunk / kT; ++it) {
        const int p = ch * kChunk + it * kT + tid;
        const bool head = is_head(n, keys, p);
        int tot;
        const int off = wg_excl_scan_flag<kWaves>(head, wsum, tot);
        if (head) tile_start[run + off] = p;  // run + off <= p < n: at most p tiles start before position p
        run += tot;
    }
}

// tile t of nt: its start a, its size m, its sample count S (0: below min_points)
__device__ __forceinline__ void tile_of(int n, int nt, const int* __restrict__ tile_start, int t, int npts, int min_points,
                                        int& a, int& m, int& S) {
    a = m = S = 0;
    if (t >= nt) return;
    a = tile_start[t];
    m = (t + 1 < nt ? tile_start[t + 1] : n) - a;
    S = m < min_points ? 0 : (m + npts - 1) / npts;  // m, npts <= PN2_FRAME_MAX_ROWS: the sum fits
}

__global__ void __launch_bounds__(kT)
tp_tile_count_kernel(int n, int npts, int min_points, const int* __restrict__ tile_start, int* __restrict__ chunk_cnt,
                     Scal* __restrict__ scal) {
    __shared__ int red[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x;
    const int nt = scal->n_tiles;
    int samples = 0, skipped = 0;
    if (ch * kChunk < nt) {
#pragma unroll
        for (int it = 0; it < kChunk / kT; ++it) {
            int a, m, S;
            tile_of(n, nt, tile_start, ch * kChunk + it * kT + tid, npts, min_points, a, m, S);
            samples += S;
            skipped += S == 0 ? m : 0;
        }
    }
    const int tot = wg_sum<kWaves>(samples, red);
    const int skp = wg_sum<kWaves>(skipped, red);
    if (tid == 0) {
        chunk_cnt[ch] = tot;  // (a chunk beyond the last tile: 0, the scan reads every entry)
        if (skp) atomicAdd(&scal->skipped, skp);
    }
}

__device__ __forceinline__ void put_row(int* __restrict__ samples, int cap, int q, int a, int m, int s, int S) {
    if (q < cap) *reinterpret_cast<int4*>(samples + (size_t)q * 4) = make_int4(a, m, s, S);
}

__global__ void __launch_bounds__(kT)
tp_rows_emit_kernel(int n, int npts, int min_points, int sample_cap, const int* __restrict__ tile_start,
                    const int* __restrict__ chunk_off, const Scal* __restrict__ scal, int* __restrict__ samples,
                    int* __restrict__ header) {
    __shared__ int wsum[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nt = scal->n_tiles;
    if (ch == 0 && tid == 0) {
        const unsigned f = scal->flags;
        const int ns = scal->n_samples;
        header[0] = nt; header[1] = ns; header[2] = scal->skipped;
        header[3] = (f & FLAG_NONFINITE) ? 1 : ((f & FLAG_INDEX) ? 2 : (ns > sample_cap ? 3 : 0));
        header[4] = header[5] = header[6] = header[7] = 0;
    }
    if (ch * kChunk >= nt) return;  // (uniform over the workgroup)
    int run = chunk_off[ch];        // samples of the tiles before this chunk
    for (int it = 0; it < kChunk / kT; ++it) {
        int a, m, S;
        tile_of(n, nt, tile_start, ch * kChunk + it * kT + tid, npts, min_points, a, m, S);
        int tot;
        const int q = run + wg_excl_scan_int<kWaves>(S, wsum, tot);
        if (S <= kInlineRows)
            for (int s = 0; s < S; ++s) put_row(samples, sample_cap, q + s, a, m, s, S);
        // a tile of many samples (a dense tile, a small npts): its rows are spread over the wave
        unsigned long long big = __ballot(S > kInlineRows);
        while (big != 0ull) {
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1ull;
            const int a_ = __shfl(a, src), m_ = __shfl(m, src), S_ = __shfl(S, src), q_ = __shfl(q, src);
            for (int s = lane; s < S_; s += 64) put_row(samples, sample_cap, q_ + s, a_, m_, s, S_);
        }
        run += tot;
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
tg_gather_kernel(int npts, int q0, int use_color, const double* __restrict__ pts, const float* __restrict__ col,
                 const int* __restrict__ order, const int* __restrict__ samples, const int* __restrict__ header, double hx,
                 double hy, float* __restrict__ out_data, int* __restrict__ out_sel, int* __restrict__ out_live) {
    __shared__ unsigned long long s_min[3][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = blockIdx.y;
    const int ch = use_color ? 6 : 3;
    float* __restrict__ data = out_data + (size_t)slot * npts * ch;
    int* __restrict__ sel = out_sel + (size_t)slot * npts;
    const int ns = header[3] == 0 ? header[1] : 0;  // a plan that was refused (or cut short) has no sample to offer
    if (ns <= 0) {
        for (int k = blockIdx.x * kT + tid; k < npts; k += gridDim.x * kT) {
            for (int c = 0; c < ch; ++c) data[(size_t)k * ch + c] = 0.f;
            sel[k] = -1;
        }
        if (blockIdx.x == 0 && tid == 0) out_live[slot] = 0;
        return;
    }
    const long long q = (long long)q0 + slot;
    const int4 row = *reinterpret_cast<const int4*>(samples + (size_t)(q < ns ? q : ns - 1) * 4);
    const int a = row.x, m = row.y, s = row.z, S = row.w;
    const int c = (m - s + S - 1) / S;  // live rows: the members of rank s, s + S, ...
    const int* __restrict__ mine = order + a + s;
    // box_min over the live rows (the refill rows repeat them), as ordered keys
    unsigned long long k0 = ~0ull, k1 = ~0ull, k2 = ~0ull;
    for (int k = tid; k < c; k += kT) {
        const size_t pos = (size_t)mine[(size_t)k * S];
        const unsigned long long x = ordered_key(pts[pos * 3]), y = ordered_key(pts[pos * 3 + 1]), z = ordered_key(pts[pos * 3 + 2]);
        k0 = x < k0 ? x : k0; k1 = y < k1 ? y : k1; k2 = z < k2 ? z : k2;
    }
    k0 = pn2_wave_all_min(k0); k1 = pn2_wave_all_min(k1); k2 = pn2_wave_all_min(k2);
    if (lane == 0) { s_min[0][wave] = k0; s_min[1][wave] = k1; s_min[2][wave] = k2; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        k0 = s_min[0][w] < k0 ? s_min[0][w] : k0; k1 = s_min[1][w] < k1 ? s_min[1][w] : k1; k2 = s_min[2][w] < k2 ? s_min[2][w] : k2;
    }
    const double sh0 = ordered_to_double(k0) + hx, sh1 = ordered_to_double(k1) + hy, sh2 = ordered_to_double(k2);  // _center_box
    for (int k = blockIdx.x * kT + tid; k < npts; k += gridDim.x * kT) {
        const int at = mine[(size_t)(k % c) * S];
        const size_t pos = (size_t)at;
        const double x = pts[pos * 3], y = pts[pos * 3 + 1], z = pts[pos * 3 + 2];
        float* __restrict__ d = data + (size_t)k * ch;
        d[0] = (float)(x - sh0); d[1] = (float)(y - sh1); d[2] = (float)(z - sh2);  // float64 subtraction, one rounding
        if (use_color) { d[3] = col[pos * 3]; d[4] = col[pos * 3 + 1]; d[5] = col[pos * 3 + 2]; }
        sel[k] = at;
    }
    if (blockIdx.x == 0 && tid == 0) out_live[slot] = q < ns ? c : 0;
}

// ---- vote, labels ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
tv_vote_kernel(long long rows, int npts, int num_class, const int* __restrict__ sel, const int* __restrict__ live,
               const int* __restrict__ pred, int* __restrict__ votes, unsigned long long* __restrict__ dropped) {
    const long long r = (long long)blockIdx.x * kT + threadIdx.x;
    bool drop = false;
    if (r < rows) {
        const int q = (int)(r / npts), k = (int)(r % npts);
        if (k < live[q]) {
            const int p = pred[r], at = sel[r];
            if (p >= 0 && p < num_class && at >= 0) atomicAdd(&votes[(size_t)at * num_class + p], 1);
            else drop = true;
        }
    }
    const unsigned long long d = __ballot(drop);
    if (dropped && d != 0ull && (threadIdx.x & 63) == 0) atomicAdd(dropped, (unsigned long long)__popcll(d));
}

__global__ void __launch_bounds__(kT)
tv_labels_kernel(int n, int num_class, const int* __restrict__ votes, int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int* __restrict__ v = votes + (size_t)i * num_class;
    int best = 0, bv = v[0];
    for (int c = 1; c < num_class; ++c) {
        const int x = v[c];
        if (x > bv) { bv = x; best = c; }  // strictly greater: the first maximal class; no vote at all: 0
    }
    labels[i] = best;
}

}  // namespace

extern "C" int pn2_tile_plan_workspace_size(int n, unsigned long long* bytes) {
    if (n <= 0) return PN2_EINVAL;
    if (n > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!bytes) return PN2_ENULL;
    WsCarver c{nullptr};
    Ws w;
    const int rc = ws_layout(n, nullptr, c, &w);
    if (rc != PN2_OK) return rc;
    *bytes = (unsigned long long)c.used;
    return PN2_OK;
}

extern "C" int pn2_tile_plan(int n, const double* points, double box_size_x, double box_size_y, double phase_x, double phase_y,
                             int npts, int min_points, int sample_cap, int* order, int* samples, int* header, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (n <= 0 || npts <= 0 || min_points < 1 || sample_cap < 0) return PN2_EINVAL;
    if (!(box_size_x > 0) || !(box_size_y > 0) || !finite_host(box_size_x) || !finite_host(box_size_y)) return PN2_EINVAL;
    if (!(phase_x >= 0) || !(phase_y >= 0) || !finite_host(phase_x) || !finite_host(phase_y)) return PN2_EINVAL;
    if (n > PN2_FRAME_MAX_ROWS || npts > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!points || !order || !header || !workspace || (sample_cap > 0 && !samples)) return PN2_ENULL;
    if (((uintptr_t)points & 7) != 0 || (((uintptr_t)order | (uintptr_t)header) & 3) != 0 || ((uintptr_t)samples & 15) != 0 ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    WsCarver c{static_cast<unsigned char*>(workspace), workspace_bytes};
    Ws w;
    const int rc = ws_layout(n, order, c, &w);  // too small: refused before the sort is asked for its share
    if (rc != PN2_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scal* scal = w.scal;
    hipError_t e = hipMemsetAsync(&scal->ymin, 0xFF, sizeof(unsigned long long), st);  // running minimum: all ones
    if (e == hipSuccess) e = hipMemsetAsync(&scal->flags, 0, sizeof(Scal) - offsetof(Scal, flags), st);
    if (e != hipSuccess) return (int)e;
    const int blocks = (int)(((long long)n + kT - 1) / kT);
    const int nch = chunks_of(n);  // chunks of positions; tiles number at most n, so it bounds their chunks as well
    tp_ymin_kernel<<<blocks, kT, 0, st>>>(n, points, scal);
    tp_key_kernel<<<blocks, kT, 0, st>>>(n, points, box_size_x, box_size_y, phase_x, phase_y, w.sort.keys_in,
                                         w.sort.vals_in, scal);
    e = w.sort.run(n, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    tp_head_count_kernel<<<nch, kT, 0, st>>>(n, w.sort.keys_out, w.chunk_a);
    tp_scan_kernel<<<1, kScanT, 0, st>>>(nch, w.chunk_a, &scal->n_tiles);
    tp_head_emit_kernel<<<nch, kT, 0, st>>>(n, w.sort.keys_out, w.chunk_a, w.tile_start);
    tp_tile_count_kernel<<<nch, kT, 0, st>>>(n, npts, min_points, w.tile_start, w.chunk_b, scal);
    tp_scan_kernel<<<1, kScanT, 0, st>>>(nch, w.chunk_b, &scal->n_samples);
    tp_rows_emit_kernel<<<nch, kT, 0, st>>>(n, npts, min_points, sample_cap, w.tile_start, w.chunk_b, scal, samples, header);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_tile_gather(int b, int npts, int q0, int use_color, const double* points, const float* colors,
                               const int* order, const int* samples, const int* header, double box_size_x, double box_size_y,
                               float* out_data, int* out_sel, int* out_live, void* stream) {
    if (b <= 0 || npts <= 0 || q0 < 0) return PN2_EINVAL;
    if (!(box_size_x > 0) || !(box_size_y > 0) || !finite_host(box_size_x) || !finite_host(box_size_y)) return PN2_EINVAL;
    if (npts > PN2_FRAME_MAX_ROWS || b > 65535 || (long long)b * npts > 2147483647ll) return PN2_ERANGE;
    if (!points || !order || !samples || !header || !out_data || !out_sel || !out_live) return PN2_ENULL;
    if (use_color && !colors) return PN2_ENULL;
    if (((uintptr_t)points & 7) != 0 || ((uintptr_t)samples & 15) != 0 ||
        (((uintptr_t)colors | (uintptr_t)order | (uintptr_t)header | (uintptr_t)out_data | (uintptr_t)out_sel | (uintptr_t)out_live) & 3) != 0)
        return PN2_EINVAL;
    int split = (npts + kGatherRows - 1) / kGatherRows;
    split = split > kGatherSplit ? kGatherSplit : split;
    tg_gather_kernel<<<dim3(split, b), kT, 0, static_cast<hipStream_t>(stream)>>>(
        npts, q0, use_color ? 1 : 0, points, colors, order, samples, header, box_size_x / 2, box_size_y / 2, out_data, out_sel,
        out_live);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_tile_vote(int b, int npts, int num_class, const int* sel, const int* live, const int* pred, int* votes,
                             long long* dropped, void* stream) {
    if (b <= 0 || npts <= 0 || num_class <= 0) return PN2_EINVAL;
    if ((long long)b * npts > 2147483647ll) return PN2_ERANGE;
    if (num_class > 64) return PN2_EUNSUP;
    if (!sel || !live || !pred || !votes) return PN2_ENULL;
    if ((((uintptr_t)sel | (uintptr_t)live | (uintptr_t)pred | (uintptr_t)votes) & 3) != 0 || ((uintptr_t)dropped & 7) != 0)
        return PN2_EINVAL;
    const long long rows = (long long)b * npts;
    tv_vote_kernel<<<(int)((rows + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(
        rows, npts, num_class, sel, live, pred, votes, reinterpret_cast<unsigned long long*>(dropped));
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_tile_labels(int n, int num_class, const int* votes, int* labels, void* stream) {
    if (n <= 0 || num_class <= 0) return PN2_EINVAL;
    if (num_class > 64) return PN2_EUNSUP;
    if (!votes || !labels) return PN2_ENULL;
    if ((((uintptr_t)votes | (uintptr_t)labels) & 3) != 0) return PN2_EINVAL;
    tv_labels_kernel<<<(int)(((long long)n + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(n, num_class, votes, labels);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
