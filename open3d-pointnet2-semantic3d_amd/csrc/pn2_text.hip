// pn2_text.hip -- raw ASCII scans on the device (include/pn2_abi.h "raw ASCII scans"): the reference's preprocess.py:40-46
// walks every line of <scene>.txt in Python (tokens[3] = str(int(float(tokens[3])))) and util/point_cloud_util.py:53-57
// calls int(line) per label.  Here a chunk of text lies in device memory and is parsed in two stages:
//   1. line index: '\n' counted per tile of PN2_TEXT_TILE_BYTES, an exclusive scan of the tile counts, then every line's start
//      offset written in file order (ballot + population-count prefix inside a tile);
//   2. field parse: one line per lane, the workgroup's contiguous span of text staged in LDS first.
// The number rule needs IEEE fp64 multiply and divide, each rounded once: this file is built like the rest of the library, -O3
// -ffp-contract=off and no fast-math flag, and must stay so (a reciprocal-multiply division would break float(token) equality).
#include <hipcub/hipcub.hpp>

#include "pn2_common.h"
#include "pn2_wg.h"  // WsCarver

namespace {

constexpr int kTile = PN2_TEXT_TILE_BYTES;
constexpr int kIdxT = kTile / 16;  // lanes of an index workgroup: one 16-byte load each
static_assert(kIdxT == 256 && kTile % 16 == 0, "the index kernels assume 4 waves per tile");

// bit j (0..3) = byte j of x is '\n'; exact (no borrow between bytes)
__device__ __forceinline__ unsigned newline_nibble(unsigned x) {
    x ^= 0x0A0A0A0Au;
    const unsigned t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where the byte was zero
    return ((t >> 7) * ((1u << 24) | (1u << 17) | (1u << 10) | (1u << 3))) >> 24 & 0xFu;
}

// bit j = byte p + j is a '\n' that begins another line, i.e. lies below `last` = nbytes - 1: the one that is the chunk's
// last byte ends the last line and starts none.  p is a multiple of 16; bytes at or past nbytes are never read.
__device__ __forceinline__ unsigned newline_mask(const unsigned char* __restrict__ text, int p, int nbytes) {
    unsigned m = 0;
    if (p + 16 <= nbytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + p);
        m = newline_nibble(v.x) | (newline_nibble(v.y) << 4) | (newline_nibble(v.z) << 8) | (newline_nibble(v.w) << 12);
    } else {  // the tail of the last partial tile
        for (int j = 0; p + j < nbytes; ++j) m |= (unsigned)(text[p + j] == '\n') << j;
    }
    const int keep = nbytes - 1 - p;  // bits below `keep` count
    if (keep < 16) m &= keep <= 0 ? 0u : (1u << keep) - 1u;
    return m;
}

__global__ void __launch_bounds__(kIdxT)
text_count_kernel(const unsigned char* __restrict__ text, int nbytes, int* __restrict__ tile_count) {
    __shared__ int wsum[kIdxT / 64];
    const int p = blockIdx.x * kTile + threadIdx.x * 16;
    int c = __popc(newline_mask(text, p, nbytes));
    c = pn2_wave_all_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// line 0 starts at byte 0; the k-th counted '\n' (k from 0, file order) at byte q starts line k + 1 at q + 1
__global__ void __launch_bounds__(kIdxT)
text_starts_kernel(const unsigned char* __restrict__ text, int nbytes, const int* __restrict__ tile_base,
                   int* __restrict__ line_start, int cap, int* __restrict__ out_count) {
    __shared__ int wsum[kIdxT / 64];
    const int p = blockIdx.x * kTile + threadIdx.x * 16;
    unsigned m = newline_mask(text, p, nbytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // line breaks in the lanes below this one: per byte position one ballot (64 bits wide) and the population count of its
    // lower lanes.  A lane's own 16 bytes follow those of every lower lane in the file.
    const unsigned long long below = (1ull << lane) - 1ull;
    int before = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned long long bal = __ballot((m >> j) & 1u);
        before += __popcll(bal & below);
        wave_total += __popcll(bal);
    }
    if (lane == 0) wsum[wave] = wave_total;
    __syncthreads();
    const int tile0 = tile_base[blockIdx.x];
    int base = tile0, tile_total = 0;
#pragma unroll
    for (int w = 0; w < kIdxT / 64; ++w) {
        const int c = wsum[w];
        if (w < wave) base += c;
        tile_total += c;
    }
    int r = base + before + 1;
    while (m) {
        const int j = __ffs((int)m) - 1;
        m &= m - 1u;
        if (r < cap) line_start[r] = p + j + 1;
        ++r;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const int nlines = tile0 + tile_total + 1;
        *out_count = nlines;
        if (cap > 0) line_start[0] = 0;
        if (nlines < cap) line_start[nlines] = text[nbytes - 1] == '\n' ? nbytes : nbytes + 1;
    }
}

struct IndexWs {  // workspace carve-up
    int ntiles;
    int *count, *base;  // per tile
    void* scan_tmp;
    size_t scan_bytes, total;
};
inline hipError_t index_ws_layout(int nbytes, unsigned char* base, IndexWs* w) {
    WsCarver c{base};
    w->ntiles = (nbytes + kTile - 1) / kTile;
    w->count = c.take<int>((size_t)w->ntiles);
    w->base = c.take<int>((size_t)w->ntiles);
    w->scan_bytes = 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, w->scan_bytes, (const int*)nullptr, (int*)nullptr, w->ntiles);
    w->scan_tmp = c.take<unsigned char>(w->scan_bytes);
    w->total = c.used;
    return e;
}

// ---- field parse --------------------------------------------------------------------------------------------------------------
constexpr int kParseT = 256;           // lines per workgroup, one per lane
constexpr int kSpanBytes = 24 * 1024;  // text a workgroup stages in LDS: 96 bytes per line on average (a Semantic3D line has
                                       // about 45), six workgroups per CU; a longer span is read from global memory
static_assert(kSpanBytes % 16 == 0, "staged in 16-byte pieces");

__device__ const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                      1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};  // all exact in fp64

struct GlobalBytes {  // the chunk where it lies
    const unsigned char* __restrict__ p;
    __device__ __forceinline__ unsigned operator[](int i) const { return p[i]; }
};
struct LdsBytes {  // the workgroup's staged span: s[0] is byte `origin` of the chunk
    const unsigned char* s;
    int origin;
    __device__ __forceinline__ unsigned operator[](int i) const { return s[i - origin]; }
};

__device__ __forceinline__ bool is_blank(unsigned c) { return c == ' ' || c == '\t' || c == '\r'; }

enum { kFast = 0, kSlow = 1, kBad = 2 };

// [i, b) spells nan, inf or infinity in any case
template <class Bytes>
__device__ bool is_special(const Bytes& t, int i, int b) {
    const char* word = nullptr;
    const int len = b - i;
    const unsigned c0 = t[i] | 0x20u;
    if (len == 3) word = c0 == 'n' ? "nan" : "inf";
    else if (len == 8) word = "infinity";
    else return false;
    for (int k = 0; k < len; ++k)
        if ((t[i + k] | 0x20u) != (unsigned)word[k]) return false;
    return true;
}

// the float token [a, b), a < b: kFast with its value, kSlow (valid, left to the caller) or kBad
template <class Bytes>
__device__ int parse_float(const Bytes& t, int a, int b, double& out) {
    int i = a;
    unsigned c = t[i];
    const bool neg = c == '-';
    if (c == '+' || c == '-') ++i;
    if (i >= b) return kBad;
    c = t[i] | 0x20u;
    if (c == 'n' || c == 'i') return is_special(t, i, b) ? kSlow : kBad;
    unsigned long long w = 0;  // the mantissa digits as an integer while they fit: 19 significant digits < 2^64
    int nsig = 0, ndig = 0, nfrac = 0;
    for (; i < b; ++i) {
        const unsigned d = t[i] - '0';
        if (d > 9u) break;
        ++ndig;
        if (nsig | (int)d) {  // leading zeros are stripped
            if (nsig < 19) w = w * 10ull + d;
            ++nsig;
        }
    }
    if (i < b && t[i] == '.') {
        for (++i; i < b; ++i) {
            const unsigned d = t[i] - '0';
            if (d > 9u) break;
            ++ndig;
            ++nfrac;
            if (nsig | (int)d) {
                if (nsig < 19) w = w * 10ull + d;
                ++nsig;
            }
        }
    }
    if (ndig == 0) return kBad;
    long long ex = 0;
    if (i < b && (t[i] | 0x20u) == 'e') {
        ++i;
        bool eneg = false;
        if (i < b && (t[i] == '+' || t[i] == '-')) { eneg = t[i] == '-'; ++i; }
        int ned = 0;
        for (; i < b; ++i) {
            const unsigned d = t[i] - '0';
            if (d > 9u) break;
            ++ned;
            if (ex < (1ll << 40)) ex = ex * 10 + d;  // saturates far above any fraction length: such a token is slow
        }
        if (ned == 0) return kBad;
        if (eneg) ex = -ex;
    }
    if (i != b) return kBad;
    const long long e10 = ex - nfrac;
    if (nsig > 19 || w > (1ull << 53) || e10 > 22 || e10 < -22) return kSlow;
    const double v = e10 >= 0 ? (double)w * kPow10[e10] : (double)w / kPow10[-e10];  // exact operands, one IEEE rounding
    out = neg ? -v : v;  // -0.0 keeps its sign
    return kFast;
}

// the int token [a, b), a < b: [+-]?digits+ in int32
template <class Bytes>
__device__ bool parse_int(const Bytes& t, int a, int b, int& out) {
    int i = a;
    const unsigned c = t[i];
    const bool neg = c == '-';
    if (c == '+' || c == '-') ++i;
    if (i >= b) return false;
    long long v = 0;
    for (; i < b; ++i) {
        const unsigned d = t[i] - '0';
        if (d > 9u) return false;
        if (v < (1ll << 40)) v = v * 10 + d;  // saturates outside int32
    }
    if (neg) v = -v;
    if (v < -2147483648ll || v > 2147483647ll) return false;
    out = (int)v;
    return true;
}

// kinds4 / slots4: 4 bits per column -- its PN2_TEXT_* kind, and its column in the output it writes to
template <class Bytes>
__device__ unsigned parse_line(const Bytes& t, int lo, int hi, int ncols, unsigned kinds4, unsigned slots4,
                               double* __restrict__ f64_row, int* __restrict__ i32_row) {
    unsigned flags = 0;
    int i = lo, k = 0;
    for (;;) {
        while (i < hi && is_blank(t[i])) ++i;
        if (i >= hi) break;
        const int a = i;
        while (i < hi && !is_blank(t[i])) ++i;
        if (k >= ncols) { ++k; break; }  // one token too many
        const unsigned kind = (kinds4 >> (4 * k)) & 0xFu, slot = (slots4 >> (4 * k)) & 0xFu;
        if (kind == PN2_TEXT_I32) {
            int v;
            if (parse_int(t, a, i, v)) i32_row[slot] = v; else flags |= PN2_TEXT_MALFORMED;
        } else if (kind != PN2_TEXT_SKIP) {
            double v;
            const int r = parse_float(t, a, i, v);
            if (r == kBad) flags |= PN2_TEXT_MALFORMED;
            else if (r == kSlow) flags |= 1u << k;
            else if (kind == PN2_TEXT_F64) f64_row[slot] = v;
            else if (v > -2147483648.0 && v < 2147483648.0) i32_row[slot] = (int)v;  // toward zero; v is finite here
            else flags |= PN2_TEXT_MALFORMED;
        }
        ++k;
    }
    if (k != ncols) flags |= PN2_TEXT_MALFORMED;  // also a line of nothing but whitespace: k == 0
    return flags;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kParseT)
text_parse_kernel(const unsigned char* __restrict__ text, int nbytes, const int* __restrict__ line_start, int nlines, int ncols,
                  unsigned kinds4, unsigned slots4, int nf, int ni, double* __restrict__ out_f64, int* __restrict__ out_i32,
                  unsigned char* __restrict__ flags_out, int* __restrict__ status) {
    __shared__ __align__(16) unsigned char s_text[kSpanBytes];
    const int tid = threadIdx.x;
    const int l0 = blockIdx.x * kParseT;
    const int l1 = l0 + kParseT < nlines ? l0 + kParseT : nlines;
    // the lines of a workgroup are one contiguous span of the chunk.  Offsets are clamped into the chunk: an index that is not
    // this chunk's gives wrong values, never a read outside the text or the staged span.
    const int span_lo = clampi(line_start[l0], 0, nbytes);
    const int span_hi = clampi(line_start[l1] - 1, span_lo, nbytes);
    const int origin = span_lo & ~15;
    const bool staged = span_hi - origin <= kSpanBytes;  // uniform over the workgroup
    if (staged) {
        for (int o = tid * 16; origin + o < span_hi; o += kParseT * 16) {  // o + 16 <= kSpanBytes: both multiples of 16
            const int p = origin + o;
            if (p + 16 <= nbytes) {
                *reinterpret_cast<uint4*>(s_text + o) = *reinterpret_cast<const uint4*>(text + p);
            } else {
                for (int j = 0; p + j < nbytes; ++j) s_text[o + j] = text[p + j];
            }
        }
        __syncthreads();
    }
    const int line = l0 + tid;
    if (line >= l1) return;
    const int lo = clampi(line_start[line], span_lo, span_hi);
    const int hi = clampi(line_start[line + 1] - 1, lo, span_hi);
    double* f64_row = out_f64 + (size_t)line * nf;
    int* i32_row = out_i32 + (size_t)line * ni;
    const unsigned fl = staged ? parse_line(LdsBytes{s_text, origin}, lo, hi, ncols, kinds4, slots4, f64_row, i32_row)
                               : parse_line(GlobalBytes{text}, lo, hi, ncols, kinds4, slots4, f64_row, i32_row);
    flags_out[line] = (unsigned char)fl;
    if (fl & PN2_TEXT_MALFORMED) {
        atomicMin(status, line);
        atomicAdd(status + 1, 1);
    } else if (fl) {
        atomicAdd(status + 2, __popc(fl));
    }
}

}  // namespace

extern "C" int pn2_text_index_workspace_bytes(int nbytes, unsigned long long* bytes) {
    if (nbytes <= 0) return PN2_EINVAL;
    if (!bytes) return PN2_ENULL;
    if (nbytes > PN2_TEXT_MAX_BYTES) return PN2_ERANGE;
    IndexWs w;
    const hipError_t e = index_ws_layout(nbytes, nullptr, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = w.total;
    return PN2_OK;
}

extern "C" int pn2_text_index_lines(const unsigned char* text, int nbytes, int* line_start, int line_cap, int* out_count,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (nbytes <= 0 || line_cap <= 0) return PN2_EINVAL;
    if (!text || !line_start || !out_count || !workspace) return PN2_ENULL;
    if (nbytes > PN2_TEXT_MAX_BYTES) return PN2_ERANGE;
    if (((uintptr_t)text & 15) != 0 || ((uintptr_t)workspace & 255) != 0) return PN2_EINVAL;
    IndexWs w;
    hipError_t e = index_ws_layout(nbytes, static_cast<unsigned char*>(workspace), &w);
    if (e != hipSuccess) return (int)e;
    if (workspace_bytes < w.total) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    text_count_kernel<<<w.ntiles, kIdxT, 0, st>>>(text, nbytes, w.count);
    e = hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, w.scan_bytes, w.count, w.base, w.ntiles, st);
    if (e != hipSuccess) return (int)e;
    text_starts_kernel<<<w.ntiles, kIdxT, 0, st>>>(text, nbytes, w.base, line_start, line_cap, out_count);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_text_parse(const unsigned char* text, int nbytes, const int* line_start, int nlines, const int* kinds,
                              int ncols, double* out_f64, int* out_i32, unsigned char* flags, int* status, void* stream) {
    if (nbytes <= 0 || nlines <= 0 || ncols <= 0 || ncols > PN2_TEXT_MAX_COLS) return PN2_EINVAL;
    if (!text || !line_start || !kinds || !flags || !status) return PN2_ENULL;
    if (nbytes > PN2_TEXT_MAX_BYTES) return PN2_ERANGE;
    unsigned kinds4 = 0, slots4 = 0;
    int nf = 0, ni = 0;
    for (int k = 0; k < ncols; ++k) {
        const int kind = kinds[k];
        if (kind < PN2_TEXT_F64 || kind > PN2_TEXT_SKIP) return PN2_EINVAL;
        if (k == 7 && (kind == PN2_TEXT_F64 || kind == PN2_TEXT_TRUNC_I32)) return PN2_EUNSUP;  // its slow bit is PN2_TEXT_MALFORMED
        const int slot = kind == PN2_TEXT_F64 ? nf++ : (kind == PN2_TEXT_SKIP ? 0 : ni++);
        kinds4 |= (unsigned)kind << (4 * k);
        slots4 |= (unsigned)slot << (4 * k);
    }
    if ((nf && !out_f64) || (ni && !out_i32)) return PN2_ENULL;
    if (((uintptr_t)text & 15) != 0) return PN2_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(status), 0x7fffffff, 1, st);
    if (e == hipSuccess) e = hipMemsetAsync(status + 1, 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    text_parse_kernel<<<(nlines + kParseT - 1) / kParseT, kParseT, 0, st>>>(text, nbytes, line_start, nlines, ncols, kinds4, slots4,
                                                                           nf, ni, out_f64, out_i32, flags, status);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
