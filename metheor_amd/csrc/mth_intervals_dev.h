// mth_intervals_dev.h -- the searches over a slice of sorted intervals (mth_regions_host.h) that the per-interval passes share
// (mth_intervals.hip, mth_mhl_regions.hip, mth_pdr_regions.hip).
#pragma once
#include "mth_common.h"

namespace mth {

// first index in [lo, hi) whose value is > v
__device__ __forceinline__ int32_t iv_upper(const int32_t *__restrict__ a, int32_t lo, int32_t hi, int32_t v) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The same for a value the whole wave shares, called where every lane of the wave is active (block-uniform code): 64 probes a round,
// so a slice of 10^5 intervals takes three dependent loads instead of seventeen.  The work items are small (a tile's rows, a run of
// reads) and these searches are what each of them waits for.
__device__ __forceinline__ int32_t iv_upper_wave(const int32_t *__restrict__ a, int32_t lo, int32_t hi, int32_t v, int lane) {
    while (hi - lo > 64) {
        const int32_t step = (hi - lo + 63) >> 6;
        const long long last = (long long)hi - 1;
        const int32_t idx = (int32_t)min((long long)lo + (long long)(lane + 1) * step - 1, last);   // ascending over the lanes; lane 63 probes hi - 1
        const int k = __popcll(__ballot(a[idx] <= v));                        // a is sorted: the probes <= v are the first k
        if (k == 64) return hi;
        hi = (int32_t)min((long long)lo + (long long)(k + 1) * step - 1, last);   // the first probe > v: the answer is at or before it
        if (k) lo = lo + k * step;                                            // the last probe <= v (never the clamped one): the answer is behind it
    }
    const int32_t idx = lo + lane;
    return lo + __popcll(__ballot(idx < hi && a[idx] <= v));
}

}  // namespace mth
