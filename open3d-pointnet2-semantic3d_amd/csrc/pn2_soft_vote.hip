// pn2_soft_vote.hip -- soft voting: class scores from the network's logits to a label per point.  The rule is in
// include/pn2_abi.h (pn2_softmax_scores); tests/soft_vote_ref.py is its numpy model.
//
//   pn2_softmax_scores   : one logit row per lane.  Float64 softmax (max, exp, a sum in class order, a division), then
//                          q = rint(p * 2^30): a row of int32 in units of 2^-30.  Three passes over the row, the exponentials formed
//                          twice, so that num_class = 64 holds no row in registers; the row's cache lines stay in L1 between passes.
//   pn2_tile_vote_scores : the soft twin of pn2_tile_vote.  A batch row takes P = the power of two >= num_class consecutive lanes
//                          of one wave, lane c of the group class c: the loads of q and the 64-bit atomics of a row are
//                          consecutive addresses.  One ballot tells every lane of the group whether its row holds a negative
//                          entry.  A zero adds nothing and is not sent.
//   pn2_score_labels     : one point per lane: the first maximal class, top / total as the confidence.
// All accumulation is in integers: no result depends on the order in which lanes, waves or launches arrive.
#include <math.h>

#include "pn2_common.h"

namespace {

constexpr int kT = 256;
constexpr double kScoreOne = 1073741824.0;  // 2^30

__global__ void __launch_bounds__(kT)
sv_softmax_kernel(int rows, int num_class, const float* __restrict__ logits, int* __restrict__ q,
                  unsigned long long* __restrict__ invalid) {
    const long long r = (long long)blockIdx.x * kT + threadIdx.x;
    bool bad = false;
    if (r < rows) {
        const float* __restrict__ x = logits + (size_t)r * num_class;
        int* __restrict__ out = q + (size_t)r * num_class;
        float mf = x[0];
        bool nan = mf != mf;
        for (int c = 1; c < num_class; ++c) {
            const float v = x[c];
            nan = nan || v != v;
            mf = v > mf ? v : mf;
        }
        bad = nan || mf == INFINITY || mf == -INFINITY;
        if (bad) {
            for (int c = 0; c < num_class; ++c) out[c] = 0;
        } else {
            const double m = (double)mf;
            double s = 0.0;
            for (int c = 0; c < num_class; ++c) s += exp((double)x[c] - m);  // class order
            for (int c = 0; c < num_class; ++c) {
                const double p = exp((double)x[c] - m) / s;
                out[c] = (int)rint(p * kScoreOne);  // half to even; p <= 1: at most 2^30
            }
        }
    }
    const unsigned long long b = __ballot(bad);
    if (invalid && b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(invalid, (unsigned long long)__popcll(b));
}

// P lanes per batch row (a power of two, num_class <= P <= 64): kT / P rows per workgroup
__global__ void __launch_bounds__(kT)
sv_vote_kernel(long long rows, int npts, int num_class, int lg_p, const int* __restrict__ sel, const int* __restrict__ live,
               const int* __restrict__ q, long long* __restrict__ scores, unsigned long long* __restrict__ dropped) {
    const int P = 1 << lg_p;
    const int c = threadIdx.x & (P - 1);
    const long long r = (((long long)blockIdx.x * kT) >> lg_p) + (threadIdx.x >> lg_p);
    bool is_live = false;
    int at = -1, v = 0;
    if (r < rows) {
        const int s = (int)(r / npts), k = (int)(r % npts);
        is_live = k < live[s];
        if (is_live) {
            at = sel[r];
            if (c < num_class) v = q[(size_t)r * num_class + c];
        }
    }
    // the negative entries of the wave, then of this lane's row
    const unsigned long long neg = __ballot(v < 0);
    const int group = (threadIdx.x & 63) >> lg_p;
    const unsigned long long mine = P == 64 ? neg : (neg >> (group * P)) & ((1ull << P) - 1ull);
    const bool drop = is_live && (at < 0 || mine != 0ull);
    if (is_live && !drop && v > 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(scores) + ((size_t)at * num_class + c), (unsigned long long)v);
    const unsigned long long d = __ballot(drop && c == 0);  // one lane per dropped row
    if (dropped && d != 0ull && (threadIdx.x & 63) == 0) atomicAdd(dropped, (unsigned long long)__popcll(d));
}

__global__ void __launch_bounds__(kT)
sv_labels_kernel(int n, int num_class, const long long* __restrict__ scores, int* __restrict__ labels,
                 float* __restrict__ confidence) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const long long* __restrict__ v = scores + (size_t)i * num_class;
    int best = 0;
    long long top = v[0], total = v[0];
    for (int c = 1; c < num_class; ++c) {
        const long long x = v[c];
        total += x;
        if (x > top) { top = x; best = c; }  // strictly greater: the first maximal class; an all-zero row: 0
    }
    labels[i] = best;
    if (confidence) confidence[i] = total == 0 ? 0.0f : (float)((double)top / (double)total);
}

}  // namespace

extern "C" int pn2_softmax_scores(int rows, int num_class, const float* logits, int* q, long long* invalid, void* stream) {
    if (rows <= 0 || num_class <= 0) return PN2_EINVAL;
    if (num_class > 64) return PN2_EUNSUP;
    if (!logits || !q) return PN2_ENULL;
    if ((((uintptr_t)logits | (uintptr_t)q) & 3) != 0 || ((uintptr_t)invalid & 7) != 0) return PN2_EINVAL;
    sv_softmax_kernel<<<(int)(((long long)rows + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(
        rows, num_class, logits, q, reinterpret_cast<unsigned long long*>(invalid));
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_tile_vote_scores(int b, int npts, int num_class, const int* sel, const int* live, const int* q,
                                    long long* scores, long long* dropped, void* stream) {
    if (b <= 0 || npts <= 0 || num_class <= 0) return PN2_EINVAL;
    if ((long long)b * npts > 2147483647ll) return PN2_ERANGE;
    if (num_class > 64) return PN2_EUNSUP;
    if (!sel || !live || !q || !scores) return PN2_ENULL;
    if ((((uintptr_t)sel | (uintptr_t)live | (uintptr_t)q) & 3) != 0 || (((uintptr_t)scores | (uintptr_t)dropped) & 7) != 0)
        return PN2_EINVAL;
    int lg_p = 0;
    while ((1 << lg_p) < num_class) ++lg_p;
    const long long rows = (long long)b * npts;
    const long long per_wg = kT >> lg_p;  // at most 2^31 / 4 workgroups
    sv_vote_kernel<<<(int)((rows + per_wg - 1) / per_wg), kT, 0, static_cast<hipStream_t>(stream)>>>(
        rows, npts, num_class, lg_p, sel, live, q, scores, reinterpret_cast<unsigned long long*>(dropped));
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

extern "C" int pn2_score_labels(int n, int num_class, const long long* scores, int* labels, float* confidence, void* stream) {
    if (n <= 0 || num_class <= 0) return PN2_EINVAL;
    if (num_class > 64) return PN2_EUNSUP;
    if (!scores || !labels) return PN2_ENULL;
    if (((uintptr_t)scores & 7) != 0 || (((uintptr_t)labels | (uintptr_t)confidence) & 3) != 0) return PN2_EINVAL;
    sv_labels_kernel<<<(int)(((long long)n + kT - 1) / kT), kT, 0, static_cast<hipStream_t>(stream)>>>(n, num_class, scores, labels,
                                                                                                       confidence);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
