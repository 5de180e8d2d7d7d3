// The variant of a SET of window hashes (include/vdf.h: vdf_window_variants_*): which row of the set row `row` of the derived
// set comes from.  ONE rule for the kernel (dct_hash.hip: window_variants_kernel) and its host twin (api.cpp), replayed under the sanitizers by
// tests/cpp/window_variant_main.cpp.  Host and device: plain C++, no HIP.
//   first[n_videos + 1], non-decreasing: video v owns rows first[v] ... first[v + 1] (N = their number; 0 is legal)
//   row = first[v] + j  ->  first[v] + j without bit 2 of the variant, first[v] + N - 1 - j with it (the windows of the reversed video come in
//   reversed order; hash_variant.h turns each around in itself)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VDF_WINDOW_VARIANT_HD __host__ __device__
#else
#define VDF_WINDOW_VARIANT_HD
#endif

namespace vdf {

// row in [first[0], first[n_videos]), n_videos >= 1.  The owner is the last v with first[v] <= row: videos of 0 windows share their first row with
// the video behind them and own nothing, so the search steps over them.
VDF_WINDOW_VARIANT_HD inline uint32_t window_variant_source(const uint32_t *first, uint32_t n_videos, uint32_t row, uint32_t variant)
{
    if (!(variant & 4u)) return row;
    uint32_t lo = 0, hi = n_videos;  // first[lo] <= row < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= row) lo = mid;
        else hi = mid;
    }
    return first[lo] + (first[lo + 1] - 1u - row);
}

}  // namespace vdf
