// pn2_records.hip -- rows of any byte stride with typed fields at any byte offset (include/pn2_abi.h "records"): the payload of a
// binary .ply and of a .pcd whose fields are not all 4 bytes wide.  Open3D's read_point_cloud takes such files in the
// reference; here the rows are unpacked into, and packed from, the arrays the pipeline holds.
//   * plain form: a row per lane, every field read from (written to) global memory -- with one access of its own size where
//     every row puts it at a multiple of that size (stride and offset both multiples), else byte by byte, assembled in registers;
//   * staged form: a workgroup's rows are one contiguous span that starts at a multiple of 16 bytes (rows per workgroup is a
//     multiple of 64), so it moves between global memory and LDS in aligned 16-byte pieces, and the lanes pick (place) their
//     fields in LDS with the same code.  A span too long for kStageBytes at 64 rows stays on the plain form.
// Both forms give the same bytes.  Global memory is touched with naturally aligned accesses only; unpack reads no byte at or
// past n * stride rounded up to 16, pack writes none at or past n * stride.  No fast-math (the colour rules need IEEE fp64
// multiply and divide), no inline assembly.
#include "pn2_color.h"  // unit_to_byte
#include "pn2_common.h"

namespace {

constexpr int kRecT = 256;                        // lanes per workgroup, a row each
constexpr int kStageBytes = PN2_REC_STAGE_BYTES;  // static LDS of the staged form
static_assert(kStageBytes % 16 == 0 && kStageBytes <= 64 * 1024, "staged in 16-byte pieces of static LDS");
static_assert(kStageBytes / 64 >= 31, "every layout pn2_record_pack writes is staged");

enum Slot { kX, kY, kZ, kC0, kC1, kC2, kLabel, kSlots };
static_assert(kSlots == PN2_REC_SLOTS, "seven slots");

struct RecLayout {
    int off[kSlots], type[kSlots];  // byte offset (-1: absent or not wanted) and PN2_REC_* of each slot
    int stride, colour_kind, big;
};

__host__ __device__ constexpr int type_size(int t) { return t <= PN2_REC_I8 ? 1 : (t <= PN2_REC_I16 ? 2 : (t <= PN2_REC_F32 ? 4 : 8)); }
__host__ __device__ constexpr bool is_float(int t) { return t >= PN2_REC_F32; }

// rows per workgroup of the staged form: a multiple of 64, at most kRecT; 0: the stride stays on the plain form
inline int staged_rows(int stride) {
    const int r = (kStageBytes / stride) & ~63;
    return r > kRecT ? kRecT : r;
}

// The S bytes at p as an unsigned number.  `natural`: p is a multiple of S (the caller proves it for every row at once).
template <int S>
__device__ __forceinline__ unsigned long long load_bytes(const unsigned char* p, bool natural, bool big) {
    unsigned long long v = 0;
    if (natural) {
        if (S == 1) v = *p;
        if (S == 2) v = *reinterpret_cast<const unsigned short*>(p);
        if (S == 4) v = *reinterpret_cast<const unsigned*>(p);
        if (S == 8) v = *reinterpret_cast<const unsigned long long*>(p);
        if (big && S == 2) v = __builtin_bswap16((unsigned short)v);
        if (big && S == 4) v = __builtin_bswap32((unsigned)v);
        if (big && S == 8) v = __builtin_bswap64(v);
        return v;
    }
#pragma unroll
    for (int k = 0; k < S; ++k) v |= (unsigned long long)p[k] << (8 * (big ? S - 1 - k : k));
    return v;
}

// the raw bits of the field of `type` at byte `off` of the row, zero-extended
__device__ __forceinline__ unsigned long long load_field(const unsigned char* row, int off, int type, int stride, bool big) {
    const int size = type_size(type);
    const bool natural = ((stride | off) & (size - 1)) == 0;  // the span starts at a multiple of 16
    const unsigned char* p = row + off;
    return size == 1 ? load_bytes<1>(p, true, big)
                     : (size == 2 ? load_bytes<2>(p, natural, big)
                                  : (size == 4 ? load_bytes<4>(p, natural, big) : load_bytes<8>(p, natural, big)));
}

// the field's value, exactly: every type is a subset of float64
__device__ __forceinline__ double field_value(unsigned long long raw, int type) {
    switch (type) {
        case PN2_REC_I8: return (double)(signed char)raw;
        case PN2_REC_I16: return (double)(short)raw;
        case PN2_REC_I32: return (double)(int)raw;
        case PN2_REC_F32: return (double)__uint_as_float((unsigned)raw);
        case PN2_REC_F64: return __longlong_as_double((long long)raw);
        default: return (double)(unsigned)raw;  // U8, U16, U32
    }
}

// one colour channel: U8 byte / 255.0 and U16 v / 65535.0, the IEEE quotients; a float field is the colour itself
__device__ __forceinline__ double channel_value(unsigned long long raw, int type) {
    if (type == PN2_REC_U8) return (double)(unsigned)raw / 255.0;
    if (type == PN2_REC_U16) return (double)(unsigned)raw / 65535.0;
    return field_value(raw, type);
}

// row: the lane's row, in global memory or in LDS.  -> the label field is a float that is no int32 (label 0)
__device__ __forceinline__ bool unpack_row(const unsigned char* row, const RecLayout& L, size_t i, double* __restrict__ points,
                                           double* __restrict__ colors, int* __restrict__ labels) {
    const bool big = L.big != 0;
    double* __restrict__ p = points + i * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = field_value(load_field(row, L.off[a], L.type[a], L.stride, big), L.type[a]);
    if (colors) {
        double* __restrict__ c = colors + i * 3;
        if (L.colour_kind == PN2_REC_COLOUR_THREE) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
                c[a] = channel_value(load_field(row, L.off[kC0 + a], L.type[kC0 + a], L.stride, big), L.type[kC0 + a]);
        } else {  // one word 0x00RRGGBB; zeros without colour
            const unsigned w = L.colour_kind == PN2_REC_COLOUR_PACKED
                                   ? (unsigned)load_field(row, L.off[kC0], L.type[kC0], L.stride, big) : 0u;
            c[0] = (double)((w >> 16) & 255u) / 255.0;
            c[1] = (double)((w >> 8) & 255u) / 255.0;
            c[2] = (double)(w & 255u) / 255.0;
        }
    }
    bool bad = false;
    if (labels) {
        const int t = L.type[kLabel];
        const unsigned long long raw = load_field(row, L.off[kLabel], t, L.stride, big);
        int v;
        if (is_float(t)) {  // finite, integral and inside int32, else 0 and counted
            const double d = field_value(raw, t);
            bad = !(d >= -2147483648.0 && d <= 2147483647.0 && d == __builtin_floor(d));
            v = bad ? 0 : (int)d;
        } else {
            v = t == PN2_REC_I8 ? (int)(signed char)raw : (t == PN2_REC_I16 ? (int)(short)raw : (int)(unsigned)raw);
        }
        labels[i] = v;
    }
    return bad;
}

// every lane of the workgroup arrives here
__device__ __forceinline__ void count_invalid(bool bad, unsigned long long* __restrict__ invalid) {
    const unsigned long long mask = __ballot(bad);
    if (mask != 0 && (threadIdx.x & 63) == 0) atomicAdd(invalid, (unsigned long long)__popcll(mask));
}

__global__ void __launch_bounds__(kRecT)
record_unpack_plain_kernel(const unsigned char* __restrict__ rows, int n, RecLayout L, double* __restrict__ points,
                           double* __restrict__ colors, int* __restrict__ labels, unsigned long long* __restrict__ invalid) {
    const int i = blockIdx.x * kRecT + threadIdx.x;
    bool bad = false;
    if (i < n) bad = unpack_row(rows + (size_t)i * L.stride, L, (size_t)i, points, colors, labels);
    if (labels && is_float(L.type[kLabel])) count_invalid(bad, invalid);
}

// rows_per_wg: staged_rows(stride).  The workgroup's span [row0 * stride, ...) starts at a multiple of 64 bytes and is read in
// whole 16-byte pieces, the last of which ends at most at n * stride rounded up to 16.
__global__ void __launch_bounds__(kRecT)
record_unpack_staged_kernel(const unsigned char* __restrict__ rows, int n, int rows_per_wg, RecLayout L,
                            double* __restrict__ points, double* __restrict__ colors, int* __restrict__ labels,
                            unsigned long long* __restrict__ invalid) {
    __shared__ __align__(16) unsigned char s_rows[kStageBytes];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * rows_per_wg;
    const int m = n - row0 < rows_per_wg ? n - row0 : rows_per_wg;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(rows + (size_t)row0 * L.stride);
    const int pieces = (m * L.stride + 15) >> 4;  // <= kStageBytes / 16
    for (int q = tid; q < pieces; q += kRecT) reinterpret_cast<uint4*>(s_rows)[q] = src[q];
    __syncthreads();
    bool bad = false;
    if (tid < m) bad = unpack_row(s_rows + tid * L.stride, L, (size_t)row0 + tid, points, colors, labels);
    if (labels && is_float(L.type[kLabel])) count_invalid(bad, invalid);
}

// ---- pack: x y z [red green blue] [label], tightly packed, little-endian ------------------------------------------------------
template <int S>
__device__ __forceinline__ void store_bytes(unsigned char* p, unsigned long long v, bool natural) {
    if (natural) {
        if (S == 1) *p = (unsigned char)v;
        if (S == 4) *reinterpret_cast<unsigned*>(p) = (unsigned)v;
        if (S == 8) *reinterpret_cast<unsigned long long*>(p) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < S; ++k) p[k] = (unsigned char)(v >> (8 * k));
}

struct PackArgs {
    const void* points;
    const void* colors;
    const int* labels;
    int point_f64, coord_f64, color_kind, stride;
};

// row: where the lane's row goes, in global memory or in LDS
__device__ __forceinline__ void pack_row(unsigned char* row, const PackArgs& A, size_t i) {
    double p[3];
    if (A.point_f64) {
        const double* __restrict__ s = static_cast<const double*>(A.points) + i * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    } else {
        const float* __restrict__ s = static_cast<const float*>(A.points) + i * 3;
        p[0] = (double)s[0]; p[1] = (double)s[1]; p[2] = (double)s[2];
    }
    int at = 0;
    if (A.coord_f64) {
        const bool natural = (A.stride & 7) == 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) store_bytes<8>(row + 8 * a, (unsigned long long)__double_as_longlong(p[a]), natural);
        at = 24;
    } else {  // (float)p: a float32 point went to float64 and comes back unchanged
        const bool natural = (A.stride & 3) == 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) store_bytes<4>(row + 4 * a, __float_as_uint((float)p[a]), natural);
        at = 12;
    }
    if (A.color_kind == PN2_PCD_COLOR_U8) {
        const unsigned char* __restrict__ c = static_cast<const unsigned char*>(A.colors) + i * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) row[at + a] = c[a];
        at += 3;
    } else if (A.color_kind == PN2_PCD_COLOR_F64) {
        const double* __restrict__ c = static_cast<const double*>(A.colors) + i * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) row[at + a] = (unsigned char)unit_to_byte(c[a]);
        at += 3;
    }
    if (A.labels) store_bytes<4>(row + at, (unsigned)A.labels[i], ((A.stride | at) & 3) == 0);
}

__global__ void __launch_bounds__(kRecT) record_pack_plain_kernel(PackArgs A, int n, unsigned char* __restrict__ rows) {
    const int i = blockIdx.x * kRecT + threadIdx.x;
    if (i < n) pack_row(rows + (size_t)i * A.stride, A, (size_t)i);
}

// kRecT rows per workgroup: the span starts at a multiple of 16 bytes.  Whole 16-byte pieces leave in one store; the piece
// that n * stride cuts goes out byte by byte, so no byte at or past n * stride is written.
__global__ void __launch_bounds__(kRecT) record_pack_staged_kernel(PackArgs A, int n, unsigned char* __restrict__ rows) {
    __shared__ __align__(16) unsigned char s_rows[kRecT * 32];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kRecT;
    const int m = n - row0 < kRecT ? n - row0 : kRecT;
    if (tid < m) pack_row(s_rows + tid * A.stride, A, (size_t)row0 + tid);
    __syncthreads();
    unsigned char* __restrict__ dst = rows + (size_t)row0 * A.stride;
    const int bytes = m * A.stride;
    for (int o = tid * 16; o < bytes; o += kRecT * 16) {
        if (o + 16 <= bytes) {
            *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(s_rows + o);
        } else {
            for (int j = o; j < bytes; ++j) dst[j] = s_rows[j];
        }
    }
}

inline bool natural(const void* p, int size) { return ((uintptr_t)p & (uintptr_t)(size - 1)) == 0; }

}  // namespace

extern "C" int pn2_record_unpack(const void* rows, int n, int stride, const int* offsets, const int* types, int colour_kind,
                                 int flags, double* points, double* colors, int* labels, long long* invalid, void* stream) {
    if (n <= 0 || stride < 1 || colour_kind < PN2_REC_COLOUR_NONE || colour_kind > PN2_REC_COLOUR_PACKED ||
        (flags & ~(PN2_REC_BIG_ENDIAN | PN2_REC_FORM_PLAIN)) != 0)
        return PN2_EINVAL;
    if (stride > PN2_REC_MAX_STRIDE) return PN2_EUNSUP;
    if (!rows || !offsets || !types || !points) return PN2_ENULL;
    if ((long long)n * stride > PN2_REC_MAX_BYTES) return PN2_ERANGE;
    // the slots this call reads: x y z, the colour slots when colours are written, the label when labels are
    RecLayout L;
    const int ncolour = !colors ? 0 : (colour_kind == PN2_REC_COLOUR_THREE ? 3 : (colour_kind == PN2_REC_COLOUR_PACKED ? 1 : 0));
    for (int s = 0; s < kSlots; ++s) {
        const bool wanted = s < kC0 || (s < kLabel ? s - kC0 < ncolour : labels != nullptr);
        L.off[s] = wanted ? offsets[s] : -1;
        L.type[s] = wanted ? types[s] : PN2_REC_U8;
        if (!wanted) continue;
        if (L.type[s] < PN2_REC_U8 || L.type[s] > PN2_REC_F64) return PN2_EINVAL;
        if (L.off[s] < 0 || L.off[s] + type_size(L.type[s]) > stride) return PN2_EINVAL;  // absent, or it reaches past the row
        for (int t = 0; t < s; ++t)
            if (L.off[t] >= 0 && L.off[s] < L.off[t] + type_size(L.type[t]) && L.off[t] < L.off[s] + type_size(L.type[s]))
                return PN2_EINVAL;  // two wanted fields overlap
    }
    for (int s = kC0; s < kC0 + ncolour; ++s) {
        const int t = L.type[s];
        if (colour_kind == PN2_REC_COLOUR_PACKED ? type_size(t) != 4
                                                 : (t != PN2_REC_U8 && t != PN2_REC_U16 && !is_float(t)))
            return PN2_EUNSUP;
    }
    const bool counts = labels && is_float(L.type[kLabel]);
    if (counts && !invalid) return PN2_ENULL;
    if (!natural(rows, 16) || !natural(points, 8) || !natural(colors, 8) || !natural(labels, 4) || !natural(invalid, 8))
        return PN2_EINVAL;
    L.stride = stride;
    L.colour_kind = colors ? colour_kind : PN2_REC_COLOUR_NONE;
    L.big = (flags & PN2_REC_BIG_ENDIAN) != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char* r = static_cast<const unsigned char*>(rows);
    unsigned long long* inv = reinterpret_cast<unsigned long long*>(invalid);
    const int per_wg = (flags & PN2_REC_FORM_PLAIN) ? 0 : staged_rows(stride);
    if (per_wg)
        record_unpack_staged_kernel<<<(n + per_wg - 1) / per_wg, kRecT, 0, st>>>(r, n, per_wg, L, points, colors, labels, inv);
    else
        record_unpack_plain_kernel<<<(n + kRecT - 1) / kRecT, kRecT, 0, st>>>(r, n, L, points, colors, labels, inv);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_record_pack(const void* points, int point_kind, const void* colors, int color_kind, const int* labels, int n,
                               int coord_type, int flags, void* rows, void* stream) {
    if (n <= 0 || (point_kind != PN2_PCD_F32 && point_kind != PN2_PCD_F64) || color_kind < PN2_PCD_COLOR_NONE ||
        color_kind > PN2_PCD_COLOR_U8 || (coord_type != PN2_REC_F32 && coord_type != PN2_REC_F64) ||
        (flags & ~PN2_REC_FORM_PLAIN) != 0)
        return PN2_EINVAL;
    if (!points || !rows || (color_kind != PN2_PCD_COLOR_NONE && !colors)) return PN2_ENULL;
    PackArgs A;
    A.points = points;
    A.colors = colors;
    A.labels = labels;
    A.point_f64 = point_kind == PN2_PCD_F64;
    A.coord_f64 = coord_type == PN2_REC_F64;
    A.color_kind = color_kind;
    A.stride = (A.coord_f64 ? 24 : 12) + (color_kind != PN2_PCD_COLOR_NONE ? 3 : 0) + (labels ? 4 : 0);
    if ((long long)n * A.stride > PN2_REC_MAX_BYTES) return PN2_ERANGE;
    if (!natural(rows, 16) || !natural(points, A.point_f64 ? 8 : 4) ||
        !natural(colors, color_kind == PN2_PCD_COLOR_F64 ? 8 : 1) || !natural(labels, 4))
        return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* r = static_cast<unsigned char*>(rows);
    const int grid = (n + kRecT - 1) / kRecT;
    if (flags & PN2_REC_FORM_PLAIN)
        record_pack_plain_kernel<<<grid, kRecT, 0, st>>>(A, n, r);
    else
        record_pack_staged_kernel<<<grid, kRecT, 0, st>>>(A, n, r);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
