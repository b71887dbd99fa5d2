// pn2_scene_io.hip -- scene files written and read on the device (include/pn2_abi.h "scene files"): the reference writes labels
// with one "%d\n" % l per point (util/point_cloud_util.py:60-63) and goes through Open3D for its .pcd files.  Here
//   * an int32 table becomes the text pn2_text_parse reads back (one row per lane: lengths, a scan of the workgroup totals, emit
//     through LDS so that the workgroup's contiguous span leaves in 16-byte stores);
//   * the rows of a binary .pcd payload (float32 x y z [+ rgb packed in a word]) are packed from and unpacked into the arrays the
//     pipeline holds, one row per lane.
// Built like the rest of the library: no fast-math (the colour rule needs IEEE fp64 multiply and divide), no inline assembly.
#include <hipcub/hipcub.hpp>

#include "pn2_color.h"  // unit_to_byte
#include "pn2_common.h"
#include "pn2_itoa.h"
#include "pn2_wg.h"  // WsCarver

namespace {

constexpr int kFmtT = PN2_TEXT_FORMAT_ROWS;                       // rows per workgroup, one per lane
constexpr int kRowMax = PN2_TEXT_MAX_COLS * PN2_TEXT_I32_CHARS;   // longest row: every token 11 characters and its separator
constexpr int kStageBytes = kFmtT * kRowMax + 16;                 // + the span's offset inside its first 16-byte piece
static_assert(kFmtT == 256, "four waves per workgroup");
static_assert(kStageBytes % 16 == 0 && kStageBytes <= 64 * 1024, "staged in 16-byte pieces of static LDS");

// bytes of the row: its tokens, ncols - 1 spaces and the '\n'
__device__ __forceinline__ int row_chars(const int* __restrict__ row, int ncols) {
    int n = ncols;
    for (int k = 0; k < ncols; ++k) n += pn2_i32_chars(row[k]);
    return n;
}

__global__ void __launch_bounds__(kFmtT)
format_count_kernel(const int* __restrict__ values, int nrows, int ncols, int* __restrict__ wg_total) {
    __shared__ int wsum[kFmtT / 64];
    const int row = blockIdx.x * kFmtT + threadIdx.x;
    int c = row < nrows ? row_chars(values + (size_t)row * ncols, ncols) : 0;
    c = pn2_wave_all_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) wg_total[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// wg_base: the exclusive scan of wg_total.  The workgroup's rows are the bytes [base, base + total) of the full text; only
// those below cap are stored.  The span is staged at its own offset inside a 16-byte piece (origin = base rounded down), so
// every piece that lies wholly inside the span and below cap is one aligned 16-byte store; the pieces at the two ends, shared
// with the neighbouring workgroups or cut by cap, go out byte by byte, each byte by the workgroup that owns it.
__global__ void __launch_bounds__(kFmtT)
format_emit_kernel(const int* __restrict__ values, int nrows, int ncols, const int* __restrict__ wg_base,
                   unsigned char* __restrict__ text, int cap, unsigned long long* __restrict__ out_bytes) {
    __shared__ __align__(16) unsigned char s_out[kStageBytes];
    __shared__ int wsum[kFmtT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x * kFmtT + tid;
    const int* __restrict__ v = values + (size_t)row * ncols;
    const int len = row < nrows ? row_chars(v, ncols) : 0;
    int incl = len;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kFmtT / 64; ++w) {
        const int c = wsum[w];
        if (w < wave) before += c;
        total += c;
    }
    const int base = wg_base[blockIdx.x];
    const int origin = base & ~15;
    if (row < nrows) {
        int at = base - origin + before + incl - len;
        auto put = [&](int p, unsigned char c) { s_out[p] = c; };
        for (int k = 0; k < ncols; ++k) {
            at = pn2_i32_emit(v[k], at, put);
            s_out[at++] = k + 1 < ncols ? ' ' : '\n';
        }
    }
    __syncthreads();
    const int end = base + total;
    const int lim = end < cap ? end : cap;
    for (int o = tid * 16; origin + o < lim; o += kFmtT * 16) {  // o + 16 <= kStageBytes: 15 + total <= kStageBytes - 1
        const int g = origin + o;
        if (g >= base && g + 16 <= lim) {
            *reinterpret_cast<uint4*>(text + g) = *reinterpret_cast<const uint4*>(s_out + o);
        } else {
            for (int j = 0; j < 16; ++j)
                if (g + j >= base && g + j < lim) text[g + j] = s_out[o + j];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *out_bytes = (unsigned long long)end;
}

struct FormatWs {  // workspace carve-up
    int nwg;
    int *wg_total, *wg_base;  // per workgroup
    void* scan_tmp;
    size_t scan_bytes, bytes;
};
inline hipError_t format_ws_layout(int nrows, unsigned char* base, FormatWs* w) {
    WsCarver c{base};
    w->nwg = (nrows + kFmtT - 1) / kFmtT;
    w->wg_total = c.take<int>((size_t)w->nwg);
    w->wg_base = c.take<int>((size_t)w->nwg);
    w->scan_bytes = 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, w->scan_bytes, (const int*)nullptr, (int*)nullptr, w->nwg);
    w->scan_tmp = c.take<unsigned char>(w->scan_bytes);
    w->bytes = c.used;
    return e;
}

// ---- binary .pcd rows ---------------------------------------------------------------------------------------------------------
constexpr int kPcdT = 256;

template <class P>
__global__ void __launch_bounds__(kPcdT)
pcd_pack_kernel(const P* __restrict__ points, const void* __restrict__ colors, int color_kind, int n,
                unsigned* __restrict__ rows) {
    const int i = blockIdx.x * kPcdT + threadIdx.x;
    if (i >= n) return;
    const P* __restrict__ p = points + (size_t)i * 3;
    const unsigned x = __float_as_uint((float)p[0]), y = __float_as_uint((float)p[1]), z = __float_as_uint((float)p[2]);
    if (color_kind == PN2_PCD_COLOR_NONE) {
        unsigned* __restrict__ r = rows + (size_t)i * 3;
        r[0] = x;
        r[1] = y;
        r[2] = z;
        return;
    }
    unsigned cr, cg, cb;
    if (color_kind == PN2_PCD_COLOR_U8) {
        const unsigned char* __restrict__ c = static_cast<const unsigned char*>(colors) + (size_t)i * 3;
        cr = c[0]; cg = c[1]; cb = c[2];
    } else {
        const double* __restrict__ c = static_cast<const double*>(colors) + (size_t)i * 3;
        cr = unit_to_byte(c[0]); cg = unit_to_byte(c[1]); cb = unit_to_byte(c[2]);
    }
    reinterpret_cast<uint4*>(rows)[i] = make_uint4(x, y, z, (cr << 16) | (cg << 8) | cb);
}

__device__ __forceinline__ unsigned pick(const uint4& w, int k) { return k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w)); }

__global__ void __launch_bounds__(kPcdT)
pcd_unpack_kernel(const unsigned* __restrict__ rows, int n, int nfields, int ix, int iy, int iz, int irgb,
                  double* __restrict__ points, double* __restrict__ colors) {
    const int i = blockIdx.x * kPcdT + threadIdx.x;
    if (i >= n) return;
    unsigned x, y, z, rgb = 0;
    if (nfields == 4) {
        const uint4 w = reinterpret_cast<const uint4*>(rows)[i];
        x = pick(w, ix); y = pick(w, iy); z = pick(w, iz);
        if (irgb >= 0) rgb = pick(w, irgb);
    } else {
        const unsigned* __restrict__ r = rows + (size_t)i * nfields;
        x = r[ix]; y = r[iy]; z = r[iz];
        if (irgb >= 0) rgb = r[irgb];
    }
    double* __restrict__ p = points + (size_t)i * 3;
    p[0] = (double)__uint_as_float(x);
    p[1] = (double)__uint_as_float(y);
    p[2] = (double)__uint_as_float(z);
    if (colors) {  // byte / 255.0: the IEEE quotient, as the host reader's; zeros without an rgb field
        double* __restrict__ c = colors + (size_t)i * 3;
        c[0] = (double)((rgb >> 16) & 255u) / 255.0;
        c[1] = (double)((rgb >> 8) & 255u) / 255.0;
        c[2] = (double)(rgb & 255u) / 255.0;
    }
}

}  // namespace

extern "C" int pn2_text_format_workspace_bytes(int nrows, unsigned long long* bytes) {
    if (nrows <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    if ((long long)nrows * PN2_TEXT_I32_CHARS > PN2_TEXT_MAX_BYTES) return PN2_ERANGE;
    FormatWs w;
    const hipError_t e = format_ws_layout(nrows, nullptr, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = w.bytes;
    return PN2_OK;
}

extern "C" int pn2_text_format_i32(const int* values, int nrows, int ncols, unsigned char* text, size_t text_cap,
                                   unsigned long long* out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (nrows <= 0 || ncols <= 0 || ncols > PN2_TEXT_MAX_COLS) return PN2_EINVAL;
    if (!values || !text || !out_bytes || !workspace) return PN2_ENULL;
    const long long worst = (long long)nrows * ncols * PN2_TEXT_I32_CHARS;
    if (worst > PN2_TEXT_MAX_BYTES) return PN2_ERANGE;
    if (((uintptr_t)text & 15) != 0 || ((uintptr_t)workspace & 255) != 0 || ((uintptr_t)values & 3) != 0) return PN2_EINVAL;
    FormatWs w;
    hipError_t e = format_ws_layout(nrows, static_cast<unsigned char*>(workspace), &w);
    if (e != hipSuccess) return (int)e;
    if (workspace_bytes < w.bytes) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cap = text_cap < (size_t)worst ? (int)text_cap : (int)worst;  // no row ends past `worst`
    format_count_kernel<<<w.nwg, kFmtT, 0, st>>>(values, nrows, ncols, w.wg_total);
    e = hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, w.scan_bytes, w.wg_total, w.wg_base, w.nwg, st);
    if (e != hipSuccess) return (int)e;
    format_emit_kernel<<<w.nwg, kFmtT, 0, st>>>(values, nrows, ncols, w.wg_base, text, cap, out_bytes);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_pcd_pack(const void* points, int point_kind, const void* colors, int color_kind, int n, unsigned int* rows,
                            void* stream) {
    if (n <= 0 || (point_kind != PN2_PCD_F32 && point_kind != PN2_PCD_F64) || color_kind < PN2_PCD_COLOR_NONE ||
        color_kind > PN2_PCD_COLOR_U8)
        return PN2_EINVAL;
    if (!points || !rows || (color_kind != PN2_PCD_COLOR_NONE && !colors)) return PN2_ENULL;
    if (n > PN2_PCD_MAX_ROWS) return PN2_ERANGE;
    const uintptr_t point_mask = point_kind == PN2_PCD_F64 ? 7 : 3, color_mask = color_kind == PN2_PCD_COLOR_F64 ? 7 : 0;
    if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)points & point_mask) != 0 || ((uintptr_t)colors & color_mask) != 0)
        return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = (n + kPcdT - 1) / kPcdT;
    if (point_kind == PN2_PCD_F64)
        pcd_pack_kernel<double><<<grid, kPcdT, 0, st>>>(static_cast<const double*>(points), colors, color_kind, n, rows);
    else
        pcd_pack_kernel<float><<<grid, kPcdT, 0, st>>>(static_cast<const float*>(points), colors, color_kind, n, rows);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_pcd_unpack(const unsigned int* rows, int n, int nfields, int ix, int iy, int iz, int irgb, double* points,
                              double* colors, void* stream) {
    if (n <= 0 || nfields < 3 || nfields > PN2_PCD_MAX_FIELDS) return PN2_EINVAL;
    if (ix < 0 || ix >= nfields || iy < 0 || iy >= nfields || iz < 0 || iz >= nfields || irgb < -1 || irgb >= nfields)
        return PN2_EINVAL;
    if (!rows || !points) return PN2_ENULL;
    if (n > PN2_PCD_MAX_ROWS) return PN2_ERANGE;
    if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)points & 7) != 0 || ((uintptr_t)colors & 7) != 0) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    pcd_unpack_kernel<<<(n + kPcdT - 1) / kPcdT, kPcdT, 0, st>>>(rows, n, nfields, ix, iy, iz, irgb, points, colors);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
