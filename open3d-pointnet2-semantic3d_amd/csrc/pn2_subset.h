// pn2_subset.h -- "the N smallest of cnt 64-bit keys, exactly", the random N-subset of pn2_dataset.hip (per sample, over the members
// of a column) and pn2_frame.hip (one cloud).  The N smallest of cnt i.i.d. keys are a uniform random N-subset; which keys they are
// is the device random stream that tests/dataset_stream_ref.py models, so nothing here may change what is chosen.
//
// The method, over three launches of the caller:
//   1 a histogram of the top kBinBits bits of every key (subset_bin) into kBins zeroed counters;
//   2 subset_find_bin: the bin T that holds the N-th smallest key and the count `below` it.  Then per key subset_below_or_push: a key
//     below T is chosen; a key in T joins a candidate list (about cnt / kBins entries, at most kCandCap, in arrival order);
//   3 need = N - below candidates are still to be chosen.  subset_find_cut: the candidate of rank need - 1 in (key, index) order; a
//     tie between keys is broken by the smaller index.  subset_wins then decides every key on its own, and a kernel that emits
//     the chosen in index order takes its prefix from the per-chunk counts of step 2 plus subset_cands_before.
// The caller owns the launches, the layout (histogram, candidate count, candidate keys and indices, by pointer), the index space of
// the keys and its status codes: it must reject nc > kCandCap or need > nc before it calls subset_find_cut.
//
// TT is the thread count of the calling workgroup; every thread must reach subset_find_bin and subset_find_cut (they hold
// barriers).
#pragma once
#include <hip/hip_runtime.h>

constexpr int kBinBits = 12;
constexpr int kBins = 1 << kBinBits;
constexpr int kCandCap = 4096;  // candidates (keys in bin T) of one selection; ~cnt / kBins expected

__device__ __forceinline__ int subset_bin(unsigned long long key) { return (int)(key >> (64 - kBinBits)); }

// bin T: the first bin whose inclusive count reaches n (the histogram must hold at least n keys); below: the keys in the bins
// before it.  Thread t owns bins [t * kBins / TT, (t + 1) * kBins / TT).  sums: TT ints of LDS; s_T, s_below: two shared scalars,
// readable by every thread on return.
template <int TT>
__device__ __forceinline__ void subset_find_bin(const unsigned* __restrict__ hist, int n, int* sums, int* s_T, int* s_below) {
    constexpr int per = kBins / TT;
    const int tid = threadIdx.x;
    int local = 0;
    for (int k = 0; k < per; ++k) local += (int)hist[tid * per + k];
    sums[tid] = local;
    __syncthreads();
    int before = 0;  // exclusive scan of the per-thread sums (small: TT values through LDS)
    for (int t = 0; t < tid; ++t) before += sums[t];
    if (before < n && before + local >= n) {
        int acc = before;
        for (int k = 0; k < per; ++k) {
            const int v = (int)hist[tid * per + k];
            if (acc + v >= n) { *s_T = tid * per + k; *s_below = acc; break; }
            acc += v;
        }
    }
    __syncthreads();
}

// step 2 for the key k of index i: true = below bin T, chosen for certain; a key in T is pushed as a candidate.  A push beyond
// kCandCap is counted and dropped: the caller sees *ncand > kCandCap in step 3
__device__ __forceinline__ bool subset_below_or_push(unsigned long long k, int i, int T, unsigned* ncand,
                                                     unsigned long long* __restrict__ cand_key, int* __restrict__ cand_idx) {
    const int bin = subset_bin(k);
    if (bin < T) return true;
    if (bin == T) {
        const unsigned slot = atomicAdd(ncand, 1u);
        if (slot < (unsigned)kCandCap) { cand_key[slot] = k; cand_idx[slot] = i; }
    }
    return false;
}

// the cut: the candidate of rank need - 1 in (key, index) order, so that exactly `need` candidates are at or under it.
// 1 <= need <= nc <= kCandCap (below < n by the choice of T, so need = n - below >= 1).  cut_key, cut_idx: two shared scalars, readable by every thread on return
template <int TT>
__device__ __forceinline__ void subset_find_cut(const unsigned long long* __restrict__ ck, const int* __restrict__ ci, int nc,
                                                int need, unsigned long long* cut_key, int* cut_idx) {
    for (int a = threadIdx.x; a < nc; a += TT) {
        const unsigned long long ka = ck[a];
        const int ia = ci[a];
        int rank = 0;
        for (int b = 0; b < nc; ++b) {
            const unsigned long long kb = ck[b];
            rank += (kb < ka) || (kb == ka && ci[b] < ia);
        }
        if (rank == need - 1) { *cut_key = ka; *cut_idx = ia; }
    }
    __syncthreads();
}

__device__ __forceinline__ bool subset_under_cut(unsigned long long k, int i, unsigned long long cutk, int cuti) {
    return k < cutk || (k == cutk && i <= cuti);
}

// is the key k of index i among the N smallest?
__device__ __forceinline__ bool subset_wins(unsigned long long k, int i, int T, unsigned long long cutk, int cuti) {
    const int bin = subset_bin(k);
    return bin < T || (bin == T && subset_under_cut(k, i, cutk, cuti));
}

// this thread's share of the count of winning candidates whose index is below `start` (to be summed over the workgroup)
template <int TT>
__device__ __forceinline__ int subset_cands_before(const unsigned long long* __restrict__ ck, const int* __restrict__ ci, int nc,
                                                   int start, unsigned long long cutk, int cuti) {
    int part = 0;
    for (int a = threadIdx.x; a < nc; a += TT) {
        const unsigned long long ka = ck[a];
        const int ia = ci[a];
        part += ia < start && subset_under_cut(ka, ia, cutk, cuti);
    }
    return part;
}
