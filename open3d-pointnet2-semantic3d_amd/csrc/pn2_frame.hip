// pn2_frame.hip -- the per-frame front end of the KITTI flow (dataset/kitti_dataset.py of the reference) on the device:
//   pn2_frame_crop   : KittiFileData.__init__ :15-26, the box crop of a raw float32 frame as an ordered stream compaction
//                      (two launches: per-chunk counts; per-chunk prefix + in-chunk ordered scan, as pn2_dataset.hip emits);
//   pn2_frame_sample : get_batch_of_one_z_box_from_origin :40-54 = _get_fix_sized_sample_mask + gather + _center_box
//                      (semantic_dataset.py:90-121) over the WHOLE cropped, x-sorted frame: one sample of npts points.
// The x-sort between the two is pn2_scene_ingest (csrc/pn2_store.hip).
//
// pn2_frame_sample is, for one cloud whose count is a host integer, two things that exist per batch elsewhere, and it runs the same
// code as they do: the mask / repeat / centre tail of scene_sample_kernel (pn2_center.h; the scene kernel maps positions through an
// index list and leaves a rejected sample unwritten, this one takes positions as rows and zero-fills) and the "npts smallest 64-bit
// keys, exactly" of pn2_dataset.hip (pn2_subset.h; there the members are a column of a multi-scene store found by binary search).
// Its own are the launches, the workspace and the status codes.  The stream is pn2_rng.h's: subset keys
// draw64(sample_stream(seed, *counter, 0), i) for i in [0, cnt), the index space pn2_dataset.hip uses for them.
#include "pn2_center.h"
#include "pn2_common.h"
#include "pn2_rng.h"
#include "pn2_subset.h"
#include "pn2_wg.h"

namespace {

constexpr int kT = 256;             // threads per workgroup of the chunked launches
constexpr int kWaves = kT / 64;
constexpr int kChunk = 1024;        // rows per chunk (4 ordered passes of kT)
constexpr int kFinT = 1024;         // threads of the one-workgroup finishing launch
constexpr int kFinW = kFinT / 64;
enum { M_T, M_NEED, M_INTS };       // meta words fs_select leaves for fs_emit

inline int chunks_of(int n) { return (n + kChunk - 1) / kChunk; }

// ---- crop ------------------------------------------------------------------------------------------------------------
struct Box { double lo0, lo1, lo2, hi0, hi1, hi2; };

// lo <= p <= hi on every axis, in float64: a NaN fails every comparison, +-inf fails one of the pair
__device__ __forceinline__ bool in_box(const Box& b, const float* __restrict__ frame, int ld, int n, int i) {
    if (i >= n) return false;
    const float* p = frame + (size_t)i * ld;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    return (x >= b.lo0) & (x <= b.hi0) & (y >= b.lo1) & (y <= b.hi1) & (z >= b.lo2) & (z <= b.hi2);
}

__global__ void __launch_bounds__(kT)
fc_count_kernel(int n, const float* __restrict__ frame, int ld, Box box, int* __restrict__ chunk_cnt) {
    __shared__ int red[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int it = 0; it < kChunk / kT; ++it) mine += in_box(box, frame, ld, n, ch * kChunk + it * kT + tid);
    const int tot = wg_sum<kWaves>(mine, red);
    if (tid == 0) chunk_cnt[ch] = tot;
}

__global__ void __launch_bounds__(kT)
fc_emit_kernel(int n, const float* __restrict__ frame, int ld, Box box, const int* __restrict__ chunk_cnt,
               double* __restrict__ out_points, int* __restrict__ out_src, int* __restrict__ out_count) {
    __shared__ int red[kWaves];
    __shared__ int wsum[kWaves];
    const int ch = blockIdx.x, tid = threadIdx.x;
    int part = 0;
    for (int k = tid; k < ch; k += kT) part += chunk_cnt[k];
    const int prefix = wg_sum<kWaves>(part, red);  // rows kept before this chunk
    int run = 0;
    for (int it = 0; it < kChunk / kT; ++it) {
        const int i = ch * kChunk + it * kT + tid;
        const bool in = in_box(box, frame, ld, n, i);
        int tot;
        const int off = wg_excl_scan_flag<kWaves>(in, wsum, tot);
        if (in) {
            const size_t pos = (size_t)(prefix + run + off);  // < n: at most i rows are kept before row i
            const float* p = frame + (size_t)i * ld;
            out_points[pos * 3 + 0] = (double)p[0]; out_points[pos * 3 + 1] = (double)p[1]; out_points[pos * 3 + 2] = (double)p[2];
            out_src[pos] = i;
        }
        run += tot;
    }
    if (ch == (int)gridDim.x - 1 && tid == 0) out_count[0] = prefix + run;
}

// ---- sample ----------------------------------------------------------------------------------------------------------
struct SampleWs {  // workspace carve-up; hist and ncand are cleared by the call itself
    unsigned* hist;                // kBins
    unsigned* ncand;               // 1 (directly behind hist: one memset clears both)
    unsigned long long* cand_key;  // kCandCap
    int* cand_idx;                 // kCandCap
    int* defcnt;                   // chunks
    int* meta;                     // M_INTS
};
inline size_t sample_ws_layout(int cnt, unsigned char* base, SampleWs* w) {
    WsCarver c{base};
    SampleWs t;
    t.hist = c.take<unsigned>((size_t)kBins + 1);
    t.ncand = t.hist + kBins;
    t.cand_key = c.take<unsigned long long>((size_t)kCandCap);
    t.cand_idx = c.take<int>((size_t)kCandCap);
    t.defcnt = c.take<int>((size_t)chunks_of(cnt));
    t.meta = c.take<int>((size_t)M_INTS);
    if (w) *w = t;
    return c.used;
}

// launch 1 (device mode, cnt > npts): histogram of the top kBinBits bits of every point's key
__global__ void __launch_bounds__(kT)
fs_hist_kernel(int cnt, unsigned long long seed, const long long* __restrict__ counter, SampleWs ws) {
    __shared__ unsigned lhist[kBins];
    const int tid = threadIdx.x;
    const unsigned long long h = sample_stream(seed, (unsigned long long)counter[0], 0);
    for (int j = tid; j < kBins; j += kT) lhist[j] = 0;
    __syncthreads();
    for (int ch = blockIdx.x; ch * kChunk < cnt; ch += gridDim.x)
        for (int it = 0; it < kChunk / kT; ++it) {
            const int i = ch * kChunk + it * kT + tid;
            if (i < cnt) atomicAdd(&lhist[subset_bin(draw64(h, (unsigned long long)i))], 1u);
        }
    __syncthreads();
    for (int j = tid; j < kBins; j += kT)
        if (lhist[j]) atomicAdd(&ws.hist[j], lhist[j]);
}

// launch 2: the bin T holding the npts-th smallest key; per chunk the count of points below T; points in T become candidates
__global__ void __launch_bounds__(kT)
fs_select_kernel(int cnt, int npts, unsigned long long seed, const long long* __restrict__ counter, SampleWs ws) {
    __shared__ int red[kWaves];
    __shared__ int sums[kT];
    __shared__ int s_T, s_below;
    const int ch = blockIdx.x, tid = threadIdx.x;
    const unsigned long long h = sample_stream(seed, (unsigned long long)counter[0], 0);
    subset_find_bin<kT>(ws.hist, npts, sums, &s_T, &s_below);  // cnt > npts: there is such a bin
    const int T = s_T;
    if (ch == 0 && tid == 0) { ws.meta[M_T] = T; ws.meta[M_NEED] = npts - s_below; }
    int chosen = 0;
    for (int it = 0; it < kChunk / kT; ++it) {
        const int i = ch * kChunk + it * kT + tid;
        if (i >= cnt) continue;
        chosen += subset_below_or_push(draw64(h, (unsigned long long)i), i, T, ws.ncand, ws.cand_key, ws.cand_idx);
    }
    const int tot = wg_sum<kWaves>(chosen, red);
    if (tid == 0) ws.defcnt[ch] = tot;
}

// launch 3: the exact cut inside T (the candidate of rank need - 1 in (key, index) order), every chosen index in ascending order
__global__ void __launch_bounds__(kT)
fs_emit_kernel(int cnt, int npts, unsigned long long seed, const long long* __restrict__ counter, SampleWs ws,
               int* __restrict__ sel, int* __restrict__ status) {
    __shared__ int red[kWaves];
    __shared__ int wsum[kWaves];
    __shared__ unsigned long long cut_key;
    __shared__ int cut_idx;
    const int ch = blockIdx.x, tid = threadIdx.x;
    const unsigned long long h = sample_stream(seed, (unsigned long long)counter[0], 0);
    const int T = ws.meta[M_T], need = ws.meta[M_NEED];
    const int nc = (int)ws.ncand[0];
    if (nc > kCandCap || need > nc || need < 1) {  // candidate list full (a frame far beyond PN2_FRAME_MAX_ROWS would need it)
        if (ch == 0 && tid == 0) status[0] = PN2_FRAME_ST_CAND;
        return;
    }
    const unsigned long long* __restrict__ ck = ws.cand_key;
    const int* __restrict__ ci = ws.cand_idx;
    subset_find_cut<kT>(ck, ci, nc, need, &cut_key, &cut_idx);
    const unsigned long long cutk = cut_key;
    const int cuti = cut_idx;
    const int start = ch * kChunk;
    int part = 0;
    for (int k = tid; k < ch; k += kT) part += ws.defcnt[k];
    part += subset_cands_before<kT>(ck, ci, nc, start, cutk, cuti);
    const int prefix = wg_sum<kWaves>(part, red);  // chosen points before this chunk
    int run = 0;
    for (int it = 0; it < kChunk / kT; ++it) {
        const int i = start + it * kT + tid;
        const bool win = i < cnt && subset_wins(draw64(h, (unsigned long long)i), i, T, cutk, cuti);
        int tot;
        const int off = wg_excl_scan_flag<kWaves>(win, wsum, tot);
        const int pos = prefix + run + off;
        if (win && pos < npts) sel[pos] = i;
        run += tot;
    }
}

enum { MODE_REPEAT, MODE_MASK, MODE_KEYS };

// last launch, one workgroup: the index list of the repeat / mask modes, box_min over the SAMPLED points, the shift, the gathers
__global__ void __launch_bounds__(kFinT)
fs_finish_kernel(int mode, int cnt, int npts, const double* __restrict__ pts, const unsigned char* __restrict__ mask, double hx,
                 double hy, long long* __restrict__ counter, int* __restrict__ sel, float* __restrict__ cen,
                 double* __restrict__ raw, int* __restrict__ status) {
    __shared__ int wsum[kFinW];
    __shared__ double smin[3][kFinW];
    const int tid = threadIdx.x;
    if (tid == 0 && counter) counter[0] = counter[0] + 1;  // the next call draws fresh keys (graph replays included)
    int st = mode == MODE_KEYS ? status[0] : PN2_FRAME_ST_OK;
    if (mode == MODE_MASK) {  // the reference's shuffled boolean mask: the set positions, ascending
        if (center_select_mask<kFinW>(cnt, npts, mask, nullptr, sel, wsum) != npts) st = PN2_FRAME_ST_MASK;
    } else if (mode == MODE_REPEAT) {
        center_select_repeat<kFinW>(cnt, npts, nullptr, sel);
    } else if (st == PN2_FRAME_ST_OK) {  // fs_emit wrote every entry; nothing below gathers through one that is not a row
        int bad = 0;
        for (int j = tid; j < npts; j += kFinT) bad |= (unsigned)sel[j] >= (unsigned)cnt;
        if (__syncthreads_or(bad)) st = PN2_FRAME_ST_CAND;
    }
    if (tid == 0) status[0] = st;
    if (st != PN2_FRAME_ST_OK) {  // a rejected frame comes back zero-filled, never as stale memory
        for (int j = tid; j < npts; j += kFinT) {
            sel[j] = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { cen[j * 3 + a] = 0.f; raw[j * 3 + a] = 0.0; }
        }
        return;
    }
    __syncthreads();
    const CenterShift sh = center_shift<kFinW>(npts, pts, sel, hx, hy, smin);
    for (int j = tid; j < npts; j += kFinT) center_put(pts, (size_t)sel[j], j, sh, cen, raw);
}

}  // namespace

extern "C" int pn2_frame_crop_workspace_size(int n, unsigned long long* bytes) {
    if (n <= 0) return PN2_EINVAL;
    if (n > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!bytes) return PN2_ENULL;
    *bytes = (unsigned long long)al256((size_t)chunks_of(n) * 4);
    return PN2_OK;
}

extern "C" int pn2_frame_crop(int n, const float* frame, int row_floats, double lo_x, double lo_y, double lo_z, double hi_x,
                              double hi_y, double hi_z, double* out_points, int* out_src, int* out_count, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (n <= 0 || row_floats < 3) return PN2_EINVAL;
    if (n > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!frame || !out_points || !out_src || !out_count || !workspace) return PN2_ENULL;
    const int nch = chunks_of(n);
    if (workspace_bytes < al256((size_t)nch * 4) || ((uintptr_t)workspace & 255) != 0) return PN2_EINVAL;
    const Box box{lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    int* chunk_cnt = static_cast<int*>(workspace);
    hipStream_t sm = static_cast<hipStream_t>(stream);
    fc_count_kernel<<<nch, kT, 0, sm>>>(n, frame, row_floats, box, chunk_cnt);
    fc_emit_kernel<<<nch, kT, 0, sm>>>(n, frame, row_floats, box, chunk_cnt, out_points, out_src, out_count);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_frame_sample_workspace_size(int cnt, unsigned long long* bytes) {
    if (cnt <= 0) return PN2_EINVAL;
    if (cnt > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!bytes) return PN2_ENULL;
    *bytes = (unsigned long long)sample_ws_layout(cnt, nullptr, nullptr);
    return PN2_OK;
}

extern "C" int pn2_frame_sample(int cnt, int npts, const double* points, const unsigned char* mask, double box_size_x,
                                double box_size_y, unsigned long long seed, long long* counter, void* workspace,
                                size_t workspace_bytes, int* out_sel, float* out_centered, double* out_raw, int* status,
                                void* stream) {
    if (cnt <= 0 || npts <= 0 || !(box_size_x > 0) || !(box_size_y > 0)) return PN2_EINVAL;
    if (cnt > PN2_FRAME_MAX_ROWS || npts > PN2_FRAME_MAX_ROWS) return PN2_ERANGE;
    if (!points || !out_sel || !out_centered || !out_raw || !status || !workspace) return PN2_ENULL;
    if (!mask && !counter) return PN2_ENULL;
    SampleWs ws;
    if (workspace_bytes < sample_ws_layout(cnt, static_cast<unsigned char*>(workspace), &ws) ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const double hx = box_size_x / 2, hy = box_size_y / 2;
    int mode = MODE_REPEAT;
    if (cnt > npts) mode = mask ? MODE_MASK : MODE_KEYS;
    if (mode == MODE_KEYS) {
        hipError_t e = hipMemsetAsync(ws.hist, 0, (size_t)(kBins + 1) * 4, sm);
        if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int), sm);
        if (e != hipSuccess) return (int)e;
        const int nch = chunks_of(cnt);
        fs_hist_kernel<<<nch < 256 ? nch : 256, kT, 0, sm>>>(cnt, seed, counter, ws);
        fs_select_kernel<<<nch, kT, 0, sm>>>(cnt, npts, seed, counter, ws);
        fs_emit_kernel<<<nch, kT, 0, sm>>>(cnt, npts, seed, counter, ws, out_sel, status);
    }
    fs_finish_kernel<<<1, kFinT, 0, sm>>>(mode, cnt, npts, points, mask, hx, hy, mask ? nullptr : counter, out_sel,
                                          out_centered, out_raw, status);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
