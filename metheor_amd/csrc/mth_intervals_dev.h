// mth_intervals_dev.h -- the device frame the per-interval passes share (mth_intervals.hip, mth_mhl_regions.hip, mth_pdr_regions.hip, mth_quartet_regions.hip):
// the searches over a slice of sorted intervals (IvTab, mth_regions_host.h), and for the two read x interval passes the common
// arguments, the owned-read test, the work item's span, a lane's walk over its candidate entries and the LDS rows.
//
// Every helper here that uses a ballot, a shuffle or a barrier (iv_upper_wave, iv_candidates, rg_span) is called from block-uniform
// code only: every lane of every wave of the workgroup reaches it, with the same arguments where they are shared.  Nothing cross-lane
// goes inside a lane's walk (iv_walk's fn).
#pragma once
#include "mth_common.h"
#include "mth_regions_host.h"

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

// The entries [w_min, w_hi) of slice s that a work item can touch at all (block-uniform): those that start at or before key_hi, the
// largest position an interval must start by, from the first whose running maximum of the ends passes key_lo, the smallest position
// an interval must end beyond -- the running maximum ascends, so below w_min no entry reaches key_lo and no walk gets there.  False:
// every entry starts beyond the work item, or every one that starts in time ends before it.
__device__ __forceinline__ bool iv_candidates(const IvTab &t, uint32_t s, int32_t key_lo, int32_t key_hi, int lane, int32_t &w_min, int32_t &w_hi) {
    const int32_t lo = t.s_beg[s], hi = t.s_end[s];
    w_hi = iv_upper_wave(t.e_start, lo, hi, key_hi, lane);
    if (w_hi == lo) return false;
    w_min = iv_upper_wave(t.e_maxend, lo, w_hi, key_lo, lane);
    return w_min != w_hi;
}

// One lane's walk: from the last candidate with start <= last back while the running maximum says that an end beyond first is still
// ahead; fn(j, ib, ie) for every entry j = [ib, ie) on the way with ie > first (ib <= last holds for all of them).
template <class Fn>
__device__ __forceinline__ void iv_walk(const IvTab &t, int32_t w_min, int32_t w_hi, int32_t first, int32_t last, Fn &&fn) {
    for (int32_t j = iv_upper(t.e_start, w_min, w_hi, last) - 1; j >= w_min && t.e_maxend[j] > first; --j) {
        const int32_t ie = t.e_end[j];
        if (ie > first) fn(j, t.e_start[j], ie);
    }
}

// ---- the read x interval passes (k_mhl_regions, k_pdr_regions, k_quartet_regions) ------------------------------------------------------------------------
// A batch's reads are sorted by start: a work item is RG_B consecutive reads, one per lane, and its workgroup sums what they add to
// the candidate entries of a slice in LDS rows of ROW 32-bit words before it adds every non-zero word to memory once.
constexpr int RG_B = 256;                       // threads of a workgroup = reads of a work item

struct RgReadArgs {
    const int32_t *read_start;                     // the batch (device-resident)
    const uint8_t *read_mapq;
    const uint32_t *cpg_off, *cpg_pos;
    IvTab tab;
    DevState *st;
    uint32_t n_reads, n_cpgs, min_cpgs, sl0, sl1;  // [sl0, sl1): the slices of the batch's domain
    int32_t region_beg, region_end;
    uint8_t min_qual;
};

// read r is the pass's: in the batch, OWNED (region_beg <= read_start < region_end: halo reads belong to a neighbour), of enough
// mapq, and with at least max(min_cpgs, 1) calls [k0, k1) inside the batch's
__device__ __forceinline__ bool rg_owned_read(const RgReadArgs &a, uint32_t r, uint32_t &k0, uint32_t &k1) {
    if (r >= a.n_reads) return false;
    const int32_t rs = a.read_start[r];
    if (rs < a.region_beg || rs >= a.region_end || a.read_mapq[r] < a.min_qual) return false;
    k0 = a.cpg_off[r]; k1 = a.cpg_off[r + 1];
    return k1 > k0 && k1 <= a.n_cpgs && k1 - k0 >= max(a.min_cpgs, 1u);
}

// The work item's span (block-uniform, two barriers): wmin / wmax come in as the lane's first and last call (INT32_MAX / -1 where it
// has no eligible read) and leave as the smallest and the largest over the workgroup.  The first barrier also ends the previous
// work item's reads of s_red and of the LDS rows.  What else a pass reduces rides through the same barriers: put(wave) runs in each
// wave's lane 0 between them, get(w) for every wave w behind them.
template <class Put, class Get>
__device__ __forceinline__ void rg_span(int32_t (&s_red)[2][RG_B / 64], int32_t &wmin, int32_t &wmax, int lane, int wave, Put &&put, Get &&get) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { wmin = min(wmin, __shfl_xor(wmin, o, 64)); wmax = max(wmax, __shfl_xor(wmax, o, 64)); }
    __syncthreads();
    if (lane == 0) { s_red[0][wave] = wmin; s_red[1][wave] = wmax; put(wave); }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RG_B / 64; ++w) { wmin = min(wmin, s_red[0][w]); wmax = max(wmax, s_red[1][w]); get(w); }
}

// the LDS rows of acc_n candidate entries: cleared, and added to the intervals' rows in memory, one atomic per word the workgroup's
// reads filled (the caller's barriers stand between the two and the lanes' adds)
template <int ROW>
__device__ __forceinline__ void iv_rows_zero(uint32_t *s_rows, int32_t acc_n, int tid) {
    for (int32_t i = tid; i < acc_n * ROW; i += RG_B) s_rows[i] = 0u;
}
template <int ROW>
__device__ __forceinline__ void iv_rows_flush(const uint32_t *s_rows, const IvTab &t, int32_t w_min, int32_t acc_n, unsigned long long *rows, int tid) {
    for (int32_t i = tid; i < acc_n * ROW; i += RG_B) {
        // (widened at the load: with a 32-bit v the MHL pass's loop came out waiting for the previous add before every LDS read, 3 % of the pass)
        const unsigned long long v = s_rows[i];
        if (v) atomicAdd(&rows[(unsigned long long)t.e_out[w_min + i / ROW] * ROW + (uint32_t)(i % ROW)], v);
    }
}

}  // namespace mth
