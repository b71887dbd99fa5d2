// pn2_dataset.hip -- SemanticDataset.sample_batch_in_all_files (dataset/semantic_dataset.py:214-343 of the reference) on a
// device-resident multi-scene store: scene pick, column crop, exact-N random subset, centring, z-rotation augmentation
// and per-point label weights in FOUR launches per batch, with no host synchronisation and no (B, capacity) buffer.
//
// Store: every scene x-sorted in its own segment of one (total, 3) float64 array; colours float32 (the reference casts
// the same float64 once when it builds the batch), labels uint8; per scene its offset, the float64 CDF np.random.choice
// builds (cdf = p.cumsum(); cdf /= cdf[-1]) and scene_z_size = max z - min z.
//
// One batch, grid (kG, B) for the first three launches: every sample's x-slab is cut into chunks of kChunk points and the
// kG workgroups of a sample stride over them.
//   1 ds_count   : draws (scene, centre, angle), the slab by binary search, per-chunk member counts and a histogram of
//                  the top kBinBits bits of each member's 64-bit subset key;
//   2 ds_select  : the column count, the histogram bin T holding the N-th smallest key; members below T are chosen,
//                  members in T become candidates (a short list); per-chunk counts of the chosen;
//   3 ds_emit    : the exact cut inside T (rank among the candidates, ties broken by point index), every chosen member
//                  written in scene order (per-chunk prefix + in-chunk ordered scan), float64 column minimum by atomics;
//   4 ds_write   : interleaved float32 rows [xyz | rgb], int32 labels, float32 weights; resets the zero-kept
//                  workspace and advances the batch counter.
// The N smallest of cnt i.i.d. keys are a uniform random N-subset; keys are 64-bit, so a tie (broken by index) has
// probability ~cnt^2 / 2^65 per column.  Replay mode takes the reference's draws instead (scene, centre, its shuffled
// boolean mask, cos / sin computed by numpy) and reproduces its batch bit for bit.
#include "pn2_common.h"
#include "pn2_ordered.h"  // ordered_key, ordered_to_double
#include "pn2_rng.h"
#include "pn2_subset.h"  // the exact-N key selection of launches 1-3: kBinBits, kBins, kCandCap, subset_*
#include "pn2_wg.h"

namespace {

constexpr int kT = 256;             // threads per workgroup
constexpr int kWaves = kT / 64;
constexpr int kChunk = 1024;        // slab points per chunk (4 ordered passes of kT)
constexpr int kG = 64;              // workgroups per sample in launches 1-3
constexpr int kInfo = 8;            // ints per sample: scene, centre, cnt, slab lo, slab hi, T, need, status
constexpr int kFInfo = 3;           // doubles per sample: angle, cos, sin
enum { I_SCENE, I_CENTER, I_CNT, I_LO, I_HI, I_T, I_NEED, I_STATUS };

// status per sample (also in include/pn2_abi.h)
enum { ST_OK = 0, ST_EMPTY = 1, ST_CAP = 2, ST_MASK = 3, ST_CAND = 4, ST_CHUNKS = 5 };

struct Ws {  // workspace carve-up; hist and ncand are kept zero between batches (ds_write resets them)
    unsigned* hist;                  // b * kBins
    unsigned* ncand;                 // b
    unsigned long long* cand_key;    // b * kCandCap
    int* cand_idx;                   // b * kCandCap
    int* memcnt;                     // b * max_chunks
    int* defcnt;                     // b * max_chunks
    unsigned long long* mins;        // b * 3 ordered float64 keys
};
inline size_t ws_layout(int b, int max_chunks, unsigned char* base, Ws* w) {
    WsCarver c{base};
    Ws t;
    t.hist = c.take<unsigned>((size_t)b * kBins);
    t.ncand = c.take<unsigned>((size_t)b);
    t.cand_key = c.take<unsigned long long>((size_t)b * kCandCap);
    t.cand_idx = c.take<int>((size_t)b * kCandCap);
    t.memcnt = c.take<int>((size_t)b * max_chunks);
    t.defcnt = c.take<int>((size_t)b * max_chunks);
    t.mins = c.take<unsigned long long>((size_t)b * 3);
    if (w) *w = t;
    return c.used;
}

struct Store {
    const double* pts;        // (total, 3) float64, each scene x-sorted in its segment
    const float* col;         // (total, 3) float32 or NULL
    const unsigned char* lab; // (total) or NULL
    const int* off;           // (ns + 1) scene offsets
    const double* cdf;        // (ns) normalised cumulative scene probabilities
    const double* zsize;      // (ns) scene_z_size
    int ns;
};

struct Draws {  // replay inputs (all NULL: device random numbers from seed and *counter)
    const int* scene;
    const int* center;
    const unsigned char* mask;
    int mask_cap;
    const double* rot;  // (b, 3): angle, cos, sin
};

// fmix64, sample_stream, draw64, unit53: csrc/pn2_rng.h.  Tags of the per-sample draws live above every point index
constexpr unsigned long long kTagScene = 1ull << 40, kTagCenter = kTagScene + 1, kTagAngle = kTagScene + 2;

struct Column {
    int scene, center, lo, hi;        // scene, scene-local centre index, global slab [lo, hi)
    double b0, b1, b2, e0, e1, e2;    // box_min / box_max (semantic_dataset.py:133-142), float64
    unsigned long long h;             // the sample's random stream (device mode)
};

// the sample's draws and its slab; every workgroup of the sample computes the same values
__device__ Column make_column(const Store& st, const Draws& dr, unsigned long long seed, const long long* counter, int s,
                              double hx, double hy) {
    Column c;
    const bool replay = dr.scene != nullptr;
    c.h = replay ? 0ull : sample_stream(seed, (unsigned long long)counter[0], s);
    if (replay) {
        c.scene = dr.scene[s];
        c.center = 0;
    } else {  // np.random.choice(k, p): cdf.searchsorted(uniform, side='right')
        const double u = unit53(draw64(c.h, kTagScene));
        int k = 0;
        while (k < st.ns && st.cdf[k] <= u) ++k;
        c.scene = k < st.ns ? k : st.ns - 1;
    }
    c.lo = c.hi = 0;
    c.b0 = c.b1 = c.b2 = c.e0 = c.e1 = c.e2 = 0.0;
    if (c.scene < 0 || c.scene >= st.ns) return c;  // a bad replayed draw: empty slab, the sample is rejected (status 1)
    const int o0 = st.off[c.scene], n = st.off[c.scene + 1] - o0;
    c.center = replay ? dr.center[s] : (int)__umul64hi(draw64(c.h, kTagCenter), (unsigned long long)n);  // randint(0, n)
    if (c.center < 0 || c.center >= n) return c;
    const double* p = st.pts + (size_t)(o0 + c.center) * 3;
    const double z = st.zsize[c.scene];
    c.b0 = p[0] - hx; c.b1 = p[1] - hy; c.b2 = p[2] - z;
    c.e0 = p[0] + hx; c.e1 = p[1] + hy; c.e2 = p[2] + z;
    c.lo = lower_bound_x(st.pts, o0, o0 + n, c.b0);   // :144
    c.hi = lower_bound_x(st.pts, c.lo, o0 + n, c.e0); // :145 (x == box_max[0] stays outside)
    return c;
}

__device__ __forceinline__ bool in_column(const Column& c, const double* __restrict__ pts, int i) {
    if (i >= c.hi) return false;
    const double x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    return (x >= c.b0) & (x <= c.e0) & (y >= c.b1) & (y <= c.e1) & (z >= c.b2) & (z <= c.e2);  // :146-153
}


__device__ __forceinline__ int num_chunks(const Column& c) { return (c.hi - c.lo + kChunk - 1) / kChunk; }

// ---- launch 1 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
ds_count_kernel(Store st, Draws dr, unsigned long long seed, const long long* __restrict__ counter, int augment, double hx,
                double hy, int max_chunks, Ws ws, int* __restrict__ info, double* __restrict__ finfo) {
    __shared__ unsigned lhist[kBins];
    __shared__ long long red[kWaves];
    const int s = blockIdx.y, tid = threadIdx.x;
    const Column c = make_column(st, dr, seed, counter, s, hx, hy);
    const bool replay = dr.scene != nullptr;
    int nch = num_chunks(c);
    if (blockIdx.x == 0 && tid == 0) {
        int* in = info + s * kInfo;
        in[I_SCENE] = c.scene; in[I_CENTER] = c.center; in[I_CNT] = 0; in[I_LO] = c.lo; in[I_HI] = c.hi;
        in[I_T] = 0; in[I_NEED] = 0; in[I_STATUS] = nch > max_chunks ? ST_CHUNKS : ST_OK;
        double ang = 0.0, cs = 1.0, sn = 0.0;
        if (augment) {
            if (replay) {
                ang = dr.rot[s * 3 + 0]; cs = dr.rot[s * 3 + 1]; sn = dr.rot[s * 3 + 2];
            } else {  // provider.py: np.random.uniform() * 2 * np.pi, then np.cos / np.sin in float64
                ang = unit53(draw64(c.h, kTagAngle)) * 2.0 * M_PI;
                cs = cos(ang); sn = sin(ang);
            }
        }
        finfo[s * kFInfo + 0] = ang; finfo[s * kFInfo + 1] = cs; finfo[s * kFInfo + 2] = sn;
#pragma unroll
        for (int a = 0; a < 3; ++a) ws.mins[s * 3 + a] = ~0ull;  // reset for launch 3's atomicMin
    }
    if (nch > max_chunks) return;
    for (int j = tid; j < kBins; j += kT) lhist[j] = 0;
    __syncthreads();
    const int o0 = nch > 0 ? st.off[c.scene] : 0;
    bool any = false;
    for (int ch = blockIdx.x; ch < nch; ch += kG) {
        int mine = 0;
        for (int it = 0; it < kChunk / kT; ++it) {
            const int i = c.lo + ch * kChunk + it * kT + tid;
            if (in_column(c, st.pts, i)) {
                ++mine;
                if (!replay) atomicAdd(&lhist[subset_bin(draw64(c.h, (unsigned long long)(i - o0)))], 1u);
            }
        }
        const long long tot = wg_sum<kWaves, long long>(mine, red);
        if (tid == 0) ws.memcnt[s * max_chunks + ch] = (int)tot;
        any = any || tot > 0;
    }
    __syncthreads();
    if (!replay && any) {
        unsigned* gh = ws.hist + (size_t)s * kBins;
        for (int j = tid; j < kBins; j += kT)
            if (lhist[j]) atomicAdd(&gh[j], lhist[j]);
    }
}

// ---- launch 2 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
ds_select_kernel(Store st, Draws dr, unsigned long long seed, const long long* __restrict__ counter, int npts, double hx,
                 double hy, int max_chunks, Ws ws, int* __restrict__ info) {
    __shared__ long long red[kWaves];
    __shared__ int wsum[kWaves];
    __shared__ int sums[kT];
    __shared__ int s_T, s_below;
    const int s = blockIdx.y, tid = threadIdx.x;
    const Column c = make_column(st, dr, seed, counter, s, hx, hy);
    const bool replay = dr.scene != nullptr;
    const int nch = num_chunks(c);
    if (nch > max_chunks) return;
    const int* __restrict__ mc = ws.memcnt + s * max_chunks;
    long long part = 0;
    for (int ch = tid; ch < nch; ch += kT) part += mc[ch];
    const int cnt = (int)wg_sum<kWaves, long long>(part, red);
    const bool subset = cnt > npts;
    int T = kBins, below = 0;
    if (subset && !replay) {
        subset_find_bin<kT>(ws.hist + (size_t)s * kBins, npts, sums, &s_T, &s_below);
        T = s_T; below = s_below;
    }
    if (blockIdx.x == 0 && tid == 0) {
        int* in = info + s * kInfo;
        in[I_CNT] = cnt; in[I_T] = T; in[I_NEED] = subset && !replay ? npts - below : 0;
        if (cnt <= 0) in[I_STATUS] = ST_EMPTY;
        else if (replay && subset && cnt > dr.mask_cap) in[I_STATUS] = ST_CAP;
    }
    const int o0 = nch > 0 ? st.off[c.scene] : 0;
    const unsigned char* __restrict__ mask = replay && subset ? dr.mask + (size_t)s * dr.mask_cap : nullptr;
    int prefix = 0;  // members before the current chunk (replay: the mask is indexed by column position)
    if (mask)
        for (int k = 0; k < (int)blockIdx.x && k < nch; ++k) prefix += mc[k];
    int prev = blockIdx.x;
    for (int ch = blockIdx.x; ch < nch; ch += kG) {
        if (mask) { for (int k = prev; k < ch; ++k) prefix += mc[k]; prev = ch; }
        int run = 0, chosen = 0;
        for (int it = 0; it < kChunk / kT; ++it) {
            const int i = c.lo + ch * kChunk + it * kT + tid;
            const bool in = in_column(c, st.pts, i);
            bool win = false;
            if (!subset) {
                win = in;
            } else if (mask) {
                int tot;
                const int off = wg_excl_scan_flag<kWaves>(in, wsum, tot);
                const int p = prefix + run + off;
                win = in && p < dr.mask_cap && mask[p] != 0;
                run += tot;
            } else if (in) {
                win = subset_below_or_push(draw64(c.h, (unsigned long long)(i - o0)), i, T, &ws.ncand[s],
                                           ws.cand_key + (size_t)s * kCandCap, ws.cand_idx + (size_t)s * kCandCap);
            }
            chosen += win;
        }
        const long long tot = wg_sum<kWaves, long long>(chosen, red);
        if (tid == 0) ws.defcnt[s * max_chunks + ch] = (int)tot;
    }
}

// ---- launch 3 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
ds_emit_kernel(Store st, Draws dr, unsigned long long seed, const long long* __restrict__ counter, int npts, double hx,
               double hy, int max_chunks, Ws ws, int* __restrict__ info, int* __restrict__ sel_all) {
    __shared__ long long red[kWaves];
    __shared__ int wsum[kWaves];
    __shared__ unsigned long long cut_key;
    __shared__ int cut_idx;
    __shared__ double smin[3][kWaves];
    const int s = blockIdx.y, tid = threadIdx.x;
    int* in = info + s * kInfo;
    if (in[I_STATUS] != ST_OK) return;
    const Column c = make_column(st, dr, seed, counter, s, hx, hy);
    const bool replay = dr.scene != nullptr;
    const int nch = num_chunks(c);
    const int cnt = in[I_CNT], T = in[I_T], need = in[I_NEED];
    const bool subset = cnt > npts;
    const int ncap = subset ? npts : cnt;
    const bool cands = subset && !replay;
    const int* __restrict__ mc = ws.memcnt + s * max_chunks;
    const int* __restrict__ dc = ws.defcnt + s * max_chunks;
    const unsigned long long* __restrict__ ck = ws.cand_key + (size_t)s * kCandCap;
    const int* __restrict__ ci = ws.cand_idx + (size_t)s * kCandCap;
    int nc = 0;
    if (cands) {
        nc = (int)ws.ncand[s];
        if (nc > kCandCap || need > nc) {
            if (blockIdx.x == 0 && tid == 0) in[I_STATUS] = ST_CAND;
            return;
        }
        subset_find_cut<kT>(ck, ci, nc, need, &cut_key, &cut_idx);
    }
    if (replay && subset && blockIdx.x == 0) {  // the reference's mask must select exactly npts members (:96-100)
        long long part = 0;
        for (int ch = tid; ch < nch; ch += kT) part += dc[ch];
        const long long tot = wg_sum<kWaves, long long>(part, red);
        if (tid == 0 && tot != npts) in[I_STATUS] = ST_MASK;  // ds_write zero-fills the sample
    }
    const unsigned long long cutk = cands ? cut_key : 0ull;
    const int cuti = cands ? cut_idx : 0;
    const int o0 = st.off[c.scene];
    const unsigned char* __restrict__ mask = replay && subset ? dr.mask + (size_t)s * dr.mask_cap : nullptr;
    int* __restrict__ sel = sel_all + (size_t)s * npts;
    double m0 = 1.0e300, m1 = 1.0e300, m2 = 1.0e300;
    for (int ch = blockIdx.x; ch < nch; ch += kG) {
        const int start = c.lo + ch * kChunk;
        // chosen members before this chunk: per-chunk counts of launch 2 + candidates at or under the cut before it
        long long part = 0, mpart = 0;
        for (int k = tid; k < ch; k += kT) { part += dc[k]; mpart += mc[k]; }
        if (cands) part += subset_cands_before<kT>(ck, ci, nc, start, cutk, cuti);
        const int prefix = (int)wg_sum<kWaves, long long>(part, red);
        const int mprefix = mask ? (int)wg_sum<kWaves, long long>(mpart, red) : 0;
        int run = 0, mrun = 0;
        for (int it = 0; it < kChunk / kT; ++it) {
            const int i = start + it * kT + tid;
            const bool inc = in_column(c, st.pts, i);
            bool win = false;
            if (!subset) {
                win = inc;
            } else if (mask) {
                int tot;
                const int off = wg_excl_scan_flag<kWaves>(inc, wsum, tot);
                const int p = mprefix + mrun + off;
                win = inc && p < dr.mask_cap && mask[p] != 0;
                mrun += tot;
            } else if (inc) {
                win = subset_wins(draw64(c.h, (unsigned long long)(i - o0)), i, T, cutk, cuti);
            }
            int tot;
            const int off = wg_excl_scan_flag<kWaves>(win, wsum, tot);
            const int pos = prefix + run + off;
            if (win && pos < ncap) {
                sel[pos] = i;
                m0 = fmin(m0, st.pts[(size_t)i * 3]); m1 = fmin(m1, st.pts[(size_t)i * 3 + 1]);
                m2 = fmin(m2, st.pts[(size_t)i * 3 + 2]);
            }
            run += tot;
        }
    }
    // box_min = np.min(points, axis=0) over the selected points (_center_box, :111); duplicates (cnt <= npts) change nothing
    wg_min3_stage<kWaves>(m0, m1, m2, smin);
    if (tid < 3) {  // (its own tail: from smin[a][0] upwards, then across workgroups as ordered keys)
        double v = smin[tid][0];
        for (int w = 1; w < kWaves; ++w) v = fmin(v, smin[tid][w]);
        if (v < 1.0e300) atomicMin(&ws.mins[s * 3 + tid], ordered_key(v));
    }
}

// ---- launch 4 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT)
ds_write_kernel(Store st, int npts, int use_color, int augment, double hx, double hy, const float* __restrict__ lw, int nlw,
                Ws ws, long long* __restrict__ counter, const int* __restrict__ info, const double* __restrict__ finfo,
                int* __restrict__ sel_all, float* __restrict__ data, int* __restrict__ out_lab,
                float* __restrict__ out_w) {
    const int s = blockIdx.y, tid = threadIdx.x;
    // keep the workspace zero for the next batch (nothing in this launch reads hist / ncand)
    unsigned* gh = ws.hist + (size_t)s * kBins;
    for (int j = blockIdx.x * kT + tid; j < kBins; j += gridDim.x * kT) gh[j] = 0u;
    if (blockIdx.x == 0 && tid == 0) {
        ws.ncand[s] = 0u;
        if (s == 0 && counter) counter[0] = counter[0] + 1;  // the next batch draws fresh numbers (graph replays included)
    }
    const int* in = info + s * kInfo;
    const int status = in[I_STATUS], cnt = in[I_CNT];
    const int ncap = cnt > npts ? npts : cnt;
    const int C = use_color ? 6 : 3;
    const double cs = finfo[s * kFInfo + 1], sn = finfo[s * kFInfo + 2];
    double sh0 = 0.0, sh1 = 0.0, sh2 = 0.0;
    if (status == ST_OK) {  // shift (:112-118), float64
        sh0 = ordered_to_double(ws.mins[s * 3 + 0]) + hx;
        sh1 = ordered_to_double(ws.mins[s * 3 + 1]) + hy;
        sh2 = ordered_to_double(ws.mins[s * 3 + 2]);
    }
    int* __restrict__ sel = sel_all + (size_t)s * npts;
    for (int j = blockIdx.x * kT + tid; j < npts; j += gridDim.x * kT) {
        float* row = data + ((size_t)s * npts + j) * C;
        const size_t r = (size_t)s * npts + j;
        if (status != ST_OK) {  // a rejected sample comes back zero-filled, never as stale memory
            for (int a = 0; a < C; ++a) row[a] = 0.f;
            out_lab[r] = 0;
            out_w[r] = 0.f;
            sel[j] = -1;
            continue;
        }
        const int k = sel[j < ncap ? j : j % ncap];  // cnt <= npts: the index list repeated (:102-106) == i mod cnt
        if (j >= ncap) sel[j] = k;  // (entries below ncap are only read in this launch)
        const double x = st.pts[(size_t)k * 3] - sh0, y = st.pts[(size_t)k * 3 + 1] - sh1, z = st.pts[(size_t)k * 3 + 2] - sh2;
        if (augment) {  // p @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] in float64 (provider.py rotate_*point_cloud), then float32
            row[0] = (float)((x * cs + y * (-sn)) + z * 0.0);
            row[1] = (float)((x * sn + y * cs) + z * 0.0);
            row[2] = (float)((x * 0.0 + y * 0.0) + z * 1.0);
        } else {
            row[0] = (float)x; row[1] = (float)y; row[2] = (float)z;
        }
        if (use_color) {
#pragma unroll
            for (int a = 0; a < 3; ++a) row[3 + a] = st.col ? st.col[(size_t)k * 3 + a] : 0.f;
        }
        const int L = st.lab ? (int)st.lab[k] : 0;
        out_lab[r] = L;
        out_w[r] = (lw && L < nlw) ? lw[L] : 0.f;  // label_weights[labels]
    }
}

}  // namespace

extern "C" int pn2_dataset_workspace_size(int b, int max_chunks, unsigned long long* bytes) {
    if (b <= 0 || max_chunks <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    *bytes = (unsigned long long)ws_layout(b, max_chunks, nullptr, nullptr);
    return PN2_OK;
}

extern "C" int pn2_dataset_sample(int b, int npts, int num_scenes, int max_chunks, int use_color, int augment,
                                  const double* points, const float* colors, const unsigned char* labels,
                                  const int* scene_offsets, const double* scene_cdf, const double* scene_z_size,
                                  const float* label_weights, int num_label_weights, double half_x, double half_y,
                                  unsigned long long seed, long long* counter, const int* draw_scene,
                                  const int* draw_center, const unsigned char* draw_mask, int mask_cap,
                                  const double* draw_rot, void* workspace, size_t workspace_bytes, int* out_info,
                                  double* out_finfo, int* out_sel, float* out_data, int* out_labels, float* out_weights,
                                  void* stream) {
    if (b <= 0 || npts <= 0 || num_scenes <= 0 || max_chunks <= 0 || num_label_weights < 0 || !(half_x > 0) ||
        !(half_y > 0) || b > 65535)
        return PN2_EINVAL;
    const bool replay = draw_scene != nullptr;
    if (replay && (!draw_center || mask_cap < 0 || (augment && !draw_rot))) return PN2_EINVAL;
    if (!replay && (draw_center || draw_mask || draw_rot)) return PN2_EINVAL;  // all draws or none
    if (!points || !scene_offsets || !scene_cdf || !scene_z_size || !workspace || !out_info || !out_finfo || !out_sel ||
        !out_data || !out_labels || !out_weights)
        return PN2_ENULL;
    if (!replay && !counter) return PN2_ENULL;
    if (num_label_weights > 0 && !label_weights) return PN2_ENULL;
    Ws ws;
    if (workspace_bytes < ws_layout(b, max_chunks, static_cast<unsigned char*>(workspace), &ws) ||
        ((uintptr_t)workspace & 255) != 0)
        return PN2_EINVAL;
    const Store st{points, colors, labels, scene_offsets, scene_cdf, scene_z_size, num_scenes};
    const Draws dr{draw_scene, draw_center, draw_mask, mask_cap, draw_rot};
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const dim3 grid(kG, b), gridw((npts + kT - 1) / kT, b);
    ds_count_kernel<<<grid, kT, 0, sm>>>(st, dr, seed, counter, augment, half_x, half_y, max_chunks, ws, out_info, out_finfo);
    ds_select_kernel<<<grid, kT, 0, sm>>>(st, dr, seed, counter, npts, half_x, half_y, max_chunks, ws, out_info);
    ds_emit_kernel<<<grid, kT, 0, sm>>>(st, dr, seed, counter, npts, half_x, half_y, max_chunks, ws, out_info, out_sel);
    ds_write_kernel<<<gridw, kT, 0, sm>>>(st, npts, use_color, augment, half_x, half_y, label_weights, num_label_weights, ws,
                                          replay ? nullptr : counter, out_info, out_finfo, out_sel, out_data, out_labels,
                                          out_weights);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
