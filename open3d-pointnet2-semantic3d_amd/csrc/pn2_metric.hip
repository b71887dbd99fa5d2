// pn2_metric.hip -- the per-batch metrics of the reference's train_one_epoch / eval_one_epoch (train.py:199-331) on the
// device: argmax of the logits (np.argmax(pred_val, 2)) and the confusion matrix of util/metric.py's ConfusionMatrix, plus
// the running sum of the step losses.  Nothing is read back per batch: the counts stay in device memory until an epoch ends,
// so the update can sit inside the captured training step.
//
// One 256-thread workgroup per CU at most, grid-stride over rows, one row per lane.  Each workgroup counts into a private
// uint32 histogram of C*C bins in LDS (C <= 64: 16 KB), counts out-of-range labels with a wave ballot, and at the end adds
// every non-zero bin to the global int64 matrix with one device-scope atomic.  Integer counts: the result is exact and does
// not depend on the order in which workgroups arrive.
#include "pn2_common.h"

namespace {

constexpr int kMetricMaxClasses = 64;  // = kCeMaxClasses of pn2_train.hip
constexpr int kMetricThreads = 256;
constexpr int kMetricMaxBlocks = 256;  // MI355X: 256 CUs

// np.argmax semantics: the first maximal index wins ties; a NaN counts as the maximum and the first NaN wins; +-inf
// compare as ordinary values.
__device__ __forceinline__ int row_argmax(const float* __restrict__ z, int C) {
    float bv = z[0];
    int best = 0;
    if (bv != bv) return 0;
    for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (v != v) return c;
        if (v > bv) {
            bv = v;
            best = c;
        }
    }
    return best;
}

template <typename LabelT>
__global__ void __launch_bounds__(kMetricThreads)
confusion_update_kernel(int rows, int C, const float* __restrict__ logits, const LabelT* __restrict__ labels,
                        int* __restrict__ pred, unsigned long long* __restrict__ confusion,
                        unsigned long long* __restrict__ invalid, const float* __restrict__ loss,
                        double* __restrict__ loss_acc) {
    __shared__ unsigned hist[kMetricMaxClasses * kMetricMaxClasses];
    __shared__ unsigned s_invalid;
    const int bins = C * C;
    if (confusion) {
        for (int i = threadIdx.x; i < bins; i += kMetricThreads) hist[i] = 0u;
    }
    if (threadIdx.x == 0) s_invalid = 0u;
    __syncthreads();

    const int lane = threadIdx.x & (PN2_WAVE - 1);
    unsigned my_invalid = 0u;  // kept by lane 0 of each wave
    // the loop bound is uniform per wave (rows rounded up to whole waves), so every lane takes part in the ballot
    const long long span = ((long long)rows + PN2_WAVE - 1) / PN2_WAVE * PN2_WAVE;
    for (long long r = (long long)blockIdx.x * kMetricThreads + threadIdx.x; r < span;
         r += (long long)gridDim.x * kMetricThreads) {
        bool bad = false;
        if (r < rows) {
            const int pd = row_argmax(logits + r * C, C);
            if (pred) pred[r] = pd;
            const long long gt = (long long)labels[r];
            bad = gt < 0 || gt >= C;
            if (confusion && !bad) atomicAdd(&hist[(int)gt * C + pd], 1u);
        }
        const unsigned long long m = __ballot(bad);
        if (lane == 0) my_invalid += (unsigned)__popcll(m);
    }
    if (invalid && lane == 0 && my_invalid) atomicAdd(&s_invalid, my_invalid);
    __syncthreads();

    if (confusion) {
        for (int i = threadIdx.x; i < bins; i += kMetricThreads) {
            const unsigned v = hist[i];
            if (v) atomicAdd(&confusion[i], (unsigned long long)v);
        }
    }
    if (threadIdx.x == 0) {
        if (invalid && s_invalid) atomicAdd(invalid, (unsigned long long)s_invalid);
        // one writer in the whole launch, and launches on a stream run in order: a plain read-modify-write, exact
        if (loss_acc && blockIdx.x == 0) {
            loss_acc[0] += (double)loss[0];
            loss_acc[1] += 1.0;
        }
    }
}

// Confusion counts from two label arrays (ConfusionMatrix.increment_from_list): the same scheme as above without the logits.
// Each lane takes kLabelUnroll pairs a grid sweep apart per iteration, all loads issued before the first use (plain 4- or
// 8-byte loads, coalesced per wave: no alignment demand beyond the element's own).  A pair with either label outside [0, C)
// -- compared at the labels' full width -- is left out of the matrix and counted per lane, summed per wave at the end.
constexpr int kLabelUnroll = 4;
// A workgroup counts at most n / (256 workgroups) + kLabelUnroll * 256 pairs into one uint32 bin (and into its uint32 count
// of dropped pairs) once the grid is full: n <= 2^39 keeps that below 2^31 + 2^10.
constexpr long long kLabelMaxPairs = 1ll << 39;

template <typename LabelT>
__global__ void __launch_bounds__(kMetricThreads)
label_confusion_kernel(long long n, int C, const LabelT* __restrict__ gt, const LabelT* __restrict__ pd,
                       unsigned long long* __restrict__ confusion, unsigned long long* __restrict__ dropped) {
    __shared__ unsigned hist[kMetricMaxClasses * kMetricMaxClasses];
    __shared__ unsigned s_dropped;
    const int bins = C * C;
    for (int i = threadIdx.x; i < bins; i += kMetricThreads) hist[i] = 0u;
    if (threadIdx.x == 0) s_dropped = 0u;
    __syncthreads();

    const unsigned long long uc = (unsigned long long)C;
    const long long sweep = (long long)gridDim.x * kMetricThreads;
    unsigned my_dropped = 0u;
    for (long long r = (long long)blockIdx.x * kMetricThreads + threadIdx.x; r < n; r += sweep * kLabelUnroll) {
        LabelT g[kLabelUnroll], p[kLabelUnroll];
#pragma unroll
        for (int u = 0; u < kLabelUnroll; ++u) {
            const long long i = r + u * sweep;
            g[u] = i < n ? gt[i] : (LabelT)0;
            p[u] = i < n ? pd[i] : (LabelT)0;
        }
#pragma unroll
        for (int u = 0; u < kLabelUnroll; ++u) {
            if (r + u * sweep >= n) break;
            // sign-extended to 64 bits, then unsigned: a negative label and an int64 beyond int32 both compare >= C
            const unsigned long long ug = (unsigned long long)(long long)g[u], up = (unsigned long long)(long long)p[u];
            if (ug < uc && up < uc) atomicAdd(&hist[(int)ug * C + (int)up], 1u);
            else ++my_dropped;
        }
    }
    if (dropped) {
        my_dropped = pn2_wave_all_sum(my_dropped);
        if ((threadIdx.x & (PN2_WAVE - 1)) == 0 && my_dropped) atomicAdd(&s_dropped, my_dropped);
    }
    __syncthreads();

    for (int i = threadIdx.x; i < bins; i += kMetricThreads) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&confusion[i], (unsigned long long)v);
    }
    if (threadIdx.x == 0 && dropped && s_dropped) atomicAdd(dropped, (unsigned long long)s_dropped);
}

}  // namespace

// argmax + confusion-matrix update (+ running loss sum) of one batch; see include/pn2_abi.h.  Every argument check comes
// before the first HIP call.
extern "C" int pn2_confusion_update(int rows, int num_class, const float* logits, const void* labels, int label64, int* pred,
                                    long long* confusion, long long* invalid, const float* loss, double* loss_acc,
                                    void* stream) {
    if (rows <= 0 || num_class <= 0) return PN2_EINVAL;
    if (!pred && !confusion && !invalid && !loss_acc) return PN2_EINVAL;  // nothing to compute
    if ((loss == nullptr) != (loss_acc == nullptr)) return PN2_EINVAL;
    if (num_class > kMetricMaxClasses) return PN2_EUNSUP;
    if (!logits || !labels) return PN2_ENULL;
    long long blocks = ((long long)rows + kMetricThreads - 1) / kMetricThreads;
    if (blocks > kMetricMaxBlocks) blocks = kMetricMaxBlocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* cm = reinterpret_cast<unsigned long long*>(confusion);
    unsigned long long* inv = reinterpret_cast<unsigned long long*>(invalid);
    if (label64)
        confusion_update_kernel<long long><<<(int)blocks, kMetricThreads, 0, st>>>(
            rows, num_class, logits, static_cast<const long long*>(labels), pred, cm, inv, loss, loss_acc);
    else
        confusion_update_kernel<int><<<(int)blocks, kMetricThreads, 0, st>>>(
            rows, num_class, logits, static_cast<const int*>(labels), pred, cm, inv, loss, loss_acc);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}

// confusion counts of n (gt, pd) label pairs; see include/pn2_abi.h.  Every argument check comes before the first HIP call.
extern "C" int pn2_label_confusion(long long n, int num_class, const void* gt, const void* pd, int label64,
                                   long long* confusion, long long* dropped, void* stream) {
    if (n <= 0 || num_class <= 0 || n > kLabelMaxPairs) return PN2_EINVAL;
    if (num_class > kMetricMaxClasses) return PN2_EUNSUP;
    if (!gt || !pd || !confusion) return PN2_ENULL;
    long long blocks = (n + kMetricThreads - 1) / kMetricThreads;
    if (blocks > kMetricMaxBlocks) blocks = kMetricMaxBlocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* cm = reinterpret_cast<unsigned long long*>(confusion);
    unsigned long long* dr = reinterpret_cast<unsigned long long*>(dropped);
    if (label64)
        label_confusion_kernel<long long><<<(int)blocks, kMetricThreads, 0, st>>>(
            n, num_class, static_cast<const long long*>(gt), static_cast<const long long*>(pd), cm, dr);
    else
        label_confusion_kernel<int><<<(int)blocks, kMetricThreads, 0, st>>>(
            n, num_class, static_cast<const int*>(gt), static_cast<const int*>(pd), cm, dr);
    PN2_RETURN_IF_LAUNCH_FAILED();
    return PN2_OK;
}
