// pn2_sort.h -- "sort (key, row index) pairs with the library's radix sort", the host half, in one copy: pn2_store.hip,
// pn2_scene.hip (voxels), pn2_tile.hip, pn2_cluster.hip, pn2_neighbors.hip, pn2_icp.hip, pn2_grid_knn.h and pn2_fps_bucket.hip.  The key kernels of the callers
// write vals_in[i] = i themselves.  The sort is stable: equal keys keep ascending row index.
#pragma once
#include <hipcub/hipcub.hpp>

#include "pn2_common.h"
#include "pn2_wg.h"  // WsCarver

template <typename K>  // unsigned, unsigned long long
struct IndexSort {
    K *keys_in, *keys_out;
    int *vals_in, *vals_out;
    void* tmp;  // the library's temporary storage
    size_t tmp_bytes;

    // keys_in, keys_out and vals_in of n pairs; the sorted row indices land in `out`, an array of the caller's own
    void carve_into(WsCarver& c, size_t n, int* out) {
        keys_in = c.take<K>(n);
        keys_out = c.take<K>(n);
        vals_in = c.take<int>(n);
        vals_out = out;
    }
    // all four arrays
    void carve(WsCarver& c, size_t n) {
        carve_into(c, n, nullptr);
        vals_out = c.take<int>(n);
    }

    // what the library wants for a sort of `count` pairs on key bits [begin_bit, end_bit)
    static hipError_t tmp_size(int count, int begin_bit, int end_bit, size_t* bytes) {
        *bytes = 0;
        return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const K*)nullptr, (K*)nullptr, (const int*)nullptr,
                                                  (int*)nullptr, count, begin_bit, end_bit);
    }
    // The LAST step of a carve: the temporary storage.  Two stages, stated once: everything carved so far is known without asking
    // the library, so a workspace too small for it (c.limit) is refused BEFORE the library is asked for its share -- a bad call
    // is refused without a device -- and the whole is checked again behind it.  PN2_OK, PN2_EINVAL or the size query's hipError_t;
    // the piece is carved in every case, so c.used is the total even for a caller that measures and ignores the answer.
    int carve_tmp(WsCarver& c, int count, int begin_bit, int end_bit) {
        if (!c.fits()) return PN2_EINVAL;
        const hipError_t e = tmp_size(count, begin_bit, end_bit, &tmp_bytes);
        tmp = c.take<unsigned char>(tmp_bytes);
        if (e != hipSuccess) return (int)e;
        return c.fits() ? PN2_OK : PN2_EINVAL;
    }

    // rows [at, at + count) of the four arrays, key bits [begin_bit, end_bit), queued on `st`
    hipError_t run(int count, int begin_bit, int end_bit, hipStream_t st, size_t at = 0) const {
        size_t bytes = tmp_bytes;
        return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in + at, keys_out + at, vals_in + at, vals_out + at, count,
                                                  begin_bit, end_bit, st);
    }
};
