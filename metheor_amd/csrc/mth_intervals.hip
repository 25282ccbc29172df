// mth_intervals.hip -- LPMD per interval (`metheor lpmd --intervals BED`): the pairs table of mth_pairs.hip (lpmd.rs:70-87,
// add_pair_concordance) reduced by interval on the device.
//
// The reference restricts LPMD to a set of positions with `-c`: BismarkRead::filter_isin (readutil.rs:87-94) drops the calls whose
// abspos is not in the set, and compute_pairwise_cpg_concordance_discordance (readutil.rs:166-224) pairs the calls that are left by
// their relpos distance -- a pure function of the two calls.  For the set "every position of [beg, end) on a contig" the counters
// are therefore the pairs-table rows (cpg1, cpg2) of that contig with beg <= cpg1 and cpg2 < end, summed.
//
// Device: the table is not one sorted array (per-tile runs with gaps; the global path's rows unsorted behind each batch; virtual
// coordinates under contig groups), so the reduction runs over the ROWS and needs no order of them.  The intervals are sorted once
// on the host, per domain (a batch's tid: a contig or a contig group, whose intervals are shifted by their contig's voff and cut at
// its end) and per length class (lengths within a factor 4), with a running maximum of the ends.  One workgroup takes one tile's
// rows (or 2048 rows of the global path): per class it finds the intervals that start at or before the rows' largest cpg1 -- none,
// or none that reaches the rows' smallest cpg2, ends the class there -- stages the starts its rows can land on in LDS, and every row
// finds its last interval with start <= cpg1 by binary search and walks back while the running maximum says an end > cpg2 is still
// ahead.  A class keeps the walk short: an interval k steps back starts at least k / depth interval lengths earlier, and the class's
// longest is at most 4x its shortest, so a row passes at most ~4x the intervals that hold it, whatever other lengths the BED mixes in
// (a chromosome-long interval sits in a class of its own and costs one step).  A row adds its counters to its intervals in LDS --
// the workgroup's rows can only touch the intervals from the first whose running maximum passes their smallest cpg2 on -- and the
// workgroup then adds each interval it touched to memory once: a 1 Mbp interval takes two 64-bit atomics per tile, not per row.
// Rows that can touch more than IV_ACC intervals of a class (windows nested thousands deep) add to memory directly: slower, never
// a capacity error.
// The sorted intervals and their packed table (mth_regions_host.h), a batch's domain (mth_regions_table.h) and the searches for the
// candidates of a class (mth_intervals_dev.h) are the frame this pass shares with the two read x interval passes.
#include "mth_regions_table.h"

namespace mth {

constexpr int IV_B = 256;              // threads of a workgroup
constexpr int IV_LDS = 2048;           // interval starts a workgroup stages (8 KiB); a wider window is searched in memory
constexpr int IV_ACC = 1024;           // intervals a workgroup sums in LDS (16 KiB); rows that can touch more add straight to memory
constexpr uint32_t IV_CHUNK = 2048;    // rows of the global path per work item (a tile's LDS table holds as many)

struct IvArgs {
    const unsigned long long *key;                 // rows of the pairs table: cpg1 << 32 | cpg2
    const uint2 *cnt;                              //                          concordant, discordant
    const unsigned long long *tile_row0;           // work items [0, n_tiles): a tile's rows
    const uint32_t *tile_rows;
    const unsigned long long *b_tile_end;          // per batch: tiles of all batches up to and including it
    const uint32_t *b_slice;                       // per batch: its domain's slices [b_slice[2b], b_slice[2b + 1])
    const unsigned long long *c_row0;              // work items [n_tiles, n_tiles + n_chunks): rows of the global path
    const uint32_t *c_n, *c_batch;
    IvTab tab;                                     // the sorted intervals of the batches' domains
    unsigned long long *acc;                       // per interval: concordant, discordant
    unsigned long long n_tiles;
    uint32_t n_chunks, n_batches;
};

__global__ __launch_bounds__(IV_B) void k_pairs_intervals(const IvArgs a) {
    __shared__ int32_t s_start[IV_LDS];
    __shared__ unsigned long long s_acc[2 * IV_ACC];
    __shared__ int32_t s_red[3][IV_B / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long n_items = a.n_tiles + a.n_chunks;
    for (unsigned long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        unsigned long long r0;
        uint32_t n, b;
        if (it < a.n_tiles) {
            n = a.tile_rows[it];
            if (!n) continue;
            r0 = a.tile_row0[it];
            uint32_t lo = 0, hi = a.n_batches;                  // the tile's batch: the first whose tile_end lies beyond it
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.b_tile_end[mid] > it) hi = mid; else lo = mid + 1;
            }
            b = lo;
        } else {
            const unsigned long long k = it - a.n_tiles;
            r0 = a.c_row0[k]; n = a.c_n[k]; b = a.c_batch[k];
        }
        const uint32_t sl0 = a.b_slice[2 * b], sl1 = a.b_slice[2 * b + 1];
        if (sl0 == sl1) continue;                               // no interval on the batch's contig(s)
        // the rows' smallest and largest cpg1 and smallest cpg2: what of a slice they can touch
        int32_t mn1 = INT32_MAX, mx1 = -1, mn2 = INT32_MAX;
        for (uint32_t i = tid; i < n; i += IV_B) {
            const unsigned long long k = a.key[r0 + i];
            const int32_t p1 = (int32_t)(k >> 32), p2 = (int32_t)(k & 0x7fffffffull);
            mn1 = min(mn1, p1); mx1 = max(mx1, p1); mn2 = min(mn2, p2);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn1 = min(mn1, __shfl_xor(mn1, o, 64)); mx1 = max(mx1, __shfl_xor(mx1, o, 64)); mn2 = min(mn2, __shfl_xor(mn2, o, 64));
        }
        __syncthreads();                                        // the previous item's readers of s_red and s_start are done
        if (lane == 0) { s_red[0][wave] = mn1; s_red[1][wave] = mx1; s_red[2][wave] = mn2; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < IV_B / 64; ++w) { mn1 = min(mn1, s_red[0][w]); mx1 = max(mx1, s_red[1][w]); mn2 = min(mn2, s_red[2][w]); }
        for (uint32_t s = sl0; s < sl1; ++s) {                  // everything up to the row loop is block-uniform
            int32_t w_min, w_hi;                                // start <= the rows' largest cpg1, and an end > their smallest cpg2 at or after w_min
            if (!iv_candidates(a.tab, s, mn2, mx1, lane, w_min, w_hi)) continue;
            const int32_t w_lo = iv_upper_wave(a.tab.e_start, a.tab.s_beg[s], w_hi, mn1, lane);
            const int32_t w_n = w_hi - w_lo, acc_n = w_hi - w_min;
            const bool in_lds = w_n <= IV_LDS, acc_lds = acc_n <= IV_ACC;
            __syncthreads();                                    // the previous slice's searches and its flush are done
            if (in_lds)
                for (int32_t i = tid; i < w_n; i += IV_B) s_start[i] = a.tab.e_start[w_lo + i];
            if (acc_lds)
                for (int32_t i = tid; i < 2 * acc_n; i += IV_B) s_acc[i] = 0ull;
            __syncthreads();
            for (uint32_t i = (uint32_t)tid; i < n; i += IV_B) {
                const unsigned long long k = a.key[r0 + i];
                const int32_t p1 = (int32_t)(k >> 32), p2 = (int32_t)(k & 0x7fffffffull);
                const uint2 c = a.cnt[r0 + i];
                // the last interval of the slice with start <= cpg1 (every one before the window starts at or before the rows' smallest
                // cpg1), then back while the running maximum says that an end beyond cpg2 is still ahead
                int32_t j = (in_lds ? w_lo + iv_upper(s_start, 0, w_n, p1) : iv_upper(a.tab.e_start, w_lo, w_hi, p1)) - 1;
                for (; j >= w_min && a.tab.e_maxend[j] > p2; --j) {
                    if (a.tab.e_end[j] <= p2) continue;                     // start <= cpg1 and cpg2 < end: the row is the interval's
                    if (acc_lds) {
                        if (c.x) atomicAdd(&s_acc[2 * (j - w_min)], (unsigned long long)c.x);
                        if (c.y) atomicAdd(&s_acc[2 * (j - w_min) + 1], (unsigned long long)c.y);
                    } else {
                        const unsigned long long t = a.tab.e_out[j];
                        if (c.x) atomicAdd(&a.acc[2ull * t], (unsigned long long)c.x);
                        if (c.y) atomicAdd(&a.acc[2ull * t + 1], (unsigned long long)c.y);
                    }
                }
            }
            if (!acc_lds) continue;
            __syncthreads();
            for (int32_t i = tid; i < acc_n; i += IV_B) {       // one pair of global atomics per interval the workgroup's rows touched
                const unsigned long long nc = s_acc[2 * i], nd = s_acc[2 * i + 1];
                if (!(nc | nd)) continue;
                const unsigned long long t = a.tab.e_out[w_min + i];
                if (nc) atomicAdd(&a.acc[2ull * t], nc);
                if (nd) atomicAdd(&a.acc[2ull * t + 1], nd);
            }
        }
    }
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_lpmd_intervals_fetch(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end,
                             int64_t *n_concordant, int64_t *n_discordant) {
    if (!ctx) return MTH_ERR_INVALID;
    if (n && (!tid || !beg || !end || !n_concordant || !n_discordant)) return fail(ctx, MTH_ERR_INVALID, "intervals: an array is missing");
    if (n >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "intervals: 2^31 or more intervals in one call");
    if (const char *bad = iv_check_intervals(n, tid, beg, end)) return iv_fail(ctx, MTH_ERR_INVALID, "intervals:", bad);
    MTH_ENTER(ctx);                                       // settles the queued batches of the table: its metas are exact from here
    if (n == 0) return sync_and_check(ctx);
    const TileRowTable &t = ctx->pairs;
    hipStream_t s = ctx->stream;

    // ---- the intervals per domain and length class, sorted by start (mth_regions_host.h) ----
    IvDomains dm(n, tid, beg, end);

    // ---- the work items: every tile of the table, and the global path's rows of every batch in chunks ----
    const size_t nb = t.meta.size();
    std::vector<unsigned long long> b_tile_end(nb), c_row0;
    std::vector<uint32_t> b_slice(2 * nb), c_n, c_batch;
    uint64_t rows_end = 0;
    for (size_t b = 0; b < nb; ++b) {
        const TileBatch &mb = t.meta[b];
        if (mb.tid < 0 && (mb.tid > -2 || (size_t)(-2 - (int64_t)mb.tid) >= ctx->groups.size()))
            return fail(ctx, MTH_ERR_STATE, "intervals: a batch of the pairs table carries the handle of a contig group that is not defined (any more)");
        std::pair<uint32_t, uint32_t> sl;
        bool added;
        const int rc = iv_slices_for(ctx, dm, "intervals:", mb.tid, sl, &added);
        if (rc) return rc;
        b_tile_end[b] = mb.tile_end; b_slice[2 * b] = sl.first; b_slice[2 * b + 1] = sl.second;
        rows_end += mb.rows;
        if (sl.first != sl.second)
            for (uint64_t r = mb.heavy0; r < rows_end; r += IV_CHUNK) {
                c_row0.push_back(r); c_n.push_back((uint32_t)std::min<uint64_t>(IV_CHUNK, rows_end - r)); c_batch.push_back((uint32_t)b);
            }
    }
    if (c_row0.size() >= (1ull << 32) || nb >= (1ull << 32)) return fail(ctx, MTH_ERR_CAPACITY, "intervals: too many work items");
    const uint64_t n_tiles = t.tiles(), n_items = n_tiles + c_row0.size();

    MTH_HIP(ctx, ctx->iv_acc.reserve((size_t)n * 16, s));
    MTH_HIP(ctx, hipMemsetAsync(ctx->iv_acc.p, 0, (size_t)n * 16, s));
    std::vector<uint32_t> tab;                            // everything the kernel reads besides the table, as one upload (8-byte words first)
    if (dm.entries() && n_items && t.rows) {
        auto place = [&](const void *src, size_t words) {
            const size_t at = tab.size();
            tab.resize(at + words);
            if (words) memcpy(tab.data() + at, src, words * 4);
            return at;
        };
        const size_t o_bte = place(b_tile_end.data(), nb * 2), o_cr0 = place(c_row0.data(), c_row0.size() * 2);
        const size_t o_bsl = place(b_slice.data(), b_slice.size()), o_cn = place(c_n.data(), c_n.size()), o_cb = place(c_batch.data(), c_batch.size());
        const IvTabOffsets o_tab = dm.pack(tab);
        MTH_HIP(ctx, ctx->iv_tab.reserve(tab.size() * 4, s));
        MTH_HIP(ctx, hipMemcpyAsync(ctx->iv_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
        const uint32_t *base = ctx->iv_tab.as<uint32_t>();
        IvArgs a;
        a.key = ctx->p_out_key.as<unsigned long long>(); a.cnt = ctx->p_out_cnt.as<uint2>();
        a.tile_row0 = t.tile_row0.as<unsigned long long>(); a.tile_rows = t.tile_rows.as<uint32_t>();
        a.b_tile_end = reinterpret_cast<const unsigned long long *>(base + o_bte); a.c_row0 = reinterpret_cast<const unsigned long long *>(base + o_cr0);
        a.b_slice = base + o_bsl; a.c_n = base + o_cn; a.c_batch = base + o_cb;
        a.tab = o_tab.at(base);
        a.acc = ctx->iv_acc.as<unsigned long long>();
        a.n_tiles = n_tiles; a.n_chunks = (uint32_t)c_row0.size(); a.n_batches = (uint32_t)nb;
        LaunchTimer lt(ctx, K_PAIRS_INTERVALS);
        hipLaunchKernelGGL(k_pairs_intervals, dim3((uint32_t)std::min<uint64_t>(n_items, regions_grid_knob(4096u))), dim3(IV_B), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> acc((size_t)n * 2);
    MTH_HIP(ctx, hipMemcpyAsync(acc.data(), ctx->iv_acc.p, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    const int rc = sync_and_check(ctx);                   // the call's one synchronisation (tab and acc are locals)
    if (rc) return rc;
    for (uint64_t i = 0; i < n; ++i) { n_concordant[i] = (int64_t)acc[2 * i]; n_discordant[i] = (int64_t)acc[2 * i + 1]; }
    return MTH_OK;
}

}  // extern "C"
