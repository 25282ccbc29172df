// mth_pdr_regions.hip -- PDR per interval (`metheor pdr-regions`, `all --pdr-intervals`): the proportion of discordant reads of a
// REGION (Landau et al. 2014), for every interval of a BED file in one pass over the reads.
//
// Definition, in the reference's own terms.  For an interval [start, end) on contig c take each record once:
//   1. BismarkRead (readutil.rs:24-53); keep the calls with start <= abspos < end on c (and in the -c set): filter_isin
//      (readutil.rs:87-94) with the set "every position of the interval".  A call at position -1 lies in no interval.
//   2. n = calls kept; the read contributes if mapq >= min_qual and n >= max(min_cpgs, 1) (pdr.rs:147-157, after the filter).
//   3. a contributing read is methylated (every kept call is Z), unmethylated (none is) or discordant (anything else):
//      get_concordance_state() (readutil.rs:134-145) of the kept calls, the concordant ones told apart.
//   4. the value is n_discordant / (n_concordant + n_discordant) in f32 (pdr.rs:47-49), NaN below max(min_depth, 1) contributing reads.
// No flush: every read counts once, so the counts are the same for any record order and any sharding.
//
// Device: a read x interval pass in the frame of mth_intervals_dev.h, as k_mhl_regions is (mth_mhl_regions.hip) -- 256 consecutive
// reads of a batch sorted by start per work item, one per lane; the OWNED ones that pass mapq and hold enough calls are eligible
// (rg_owned_read); per length class of the batch's domain the candidate entries [w_min, w_hi) the work item's reads can touch
// (iv_candidates), a lane's walk over them (iv_walk), LDS rows (iv_rows_zero / iv_rows_flush) -- and three things that pass does not do:
//   * Every eligible lane walks its calls ONCE before any interval is looked at (pr_summary): smallest and largest position, class
//     of the read as a whole.  An interval that holds the read whole takes that class; only a partial overlap walks the calls again,
//     once, counting n and the methylated among them together (pr_entry_class, mth_pdr_regions_dev.h).
//   * SPAN ROUTE.  The workgroup counts its eligible reads per class once per work item (ballot + popcount, block-uniform).  A
//     candidate entry that holds the work item's whole span (e_start <= wmin && wmax < e_end) holds every eligible read whole: the
//     three counts ARE its reads' contribution.  Threads stride over the candidates and add the non-zero counts to the interval's
//     row in memory, at most three atomics per (work item, entry), issued by four neighbouring lanes in one instruction; the lanes'
//     walks skip an entry for which that block-uniform predicate holds.  A class all of whose candidates hold the span has no
//     per-read work at all; a class whose ONLY candidate holds it (a chromosome-long interval) is not even added to per work item:
//     the workgroup keeps the pending sum while its work items meet the same entry and adds it once.
//   * LDS ROWS of four 32-bit words (methylated, unmethylated, discordant, spare) for the rest: up to PDR_REGIONS_LDS_CAP = 1024
//     candidates of a class per work item (16 KiB), flushed as k_mhl_regions flushes, one 64-bit atomic per non-zero word.  A class
//     with more candidates under one workgroup adds to memory directly (DIRECT ROUTE): slower, never wrong.
// No cross-lane operation happens inside a lane's walk.  Memory: four 64-bit words per interval, no overflow list, no second run.
// Nothing here waits for the device: mth_pdr_regions_accumulate queues the kernel and returns; data errors (the word of position -1
// in a batch) surface at the next counts / fetch.  The interval table (a RegionsTable, mth_regions_table.h) is replaced only when a
// batch brings a new domain, and its upload drains the stream first -- a synchronisation per new contig (group), none per batch.
#include "mth_regions_table.h"
#include "mth_pdr_regions_dev.h"

namespace mth {

constexpr int PR_ACC = PDR_REGIONS_LDS_CAP;     // entries of a class a workgroup sums in LDS (16 KiB)
constexpr int PR_PEND = IvDomains::NCLS;        // slices of a domain (one per length class) a workgroup keeps a pending sum for

struct PrArgs {
    RgReadArgs rd;
    unsigned long long *rows;                      // per interval: PR_ROW words
    int32_t acc_cap;                               // 0 .. PR_ACC
    uint8_t span, pend;                            // pend: the domain has at most PR_PEND slices
};

__global__ __launch_bounds__(RG_B) void k_pdr_regions(const PrArgs a) {
    __shared__ uint32_t s_rows[PR_ACC * PR_ROW];
    __shared__ int32_t s_red[2][RG_B / 64];
    __shared__ uint32_t s_cnt[3][RG_B / 64];
    // per slice the entry that was its ONLY candidate and held the whole span, and what is still to be added to it: word c is
    // thread c's alone (each keeps its own copy of the entry), so no barrier orders them
    __shared__ int32_t s_pj[PR_PEND][4];
    __shared__ uint32_t s_pv[PR_PEND][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RgReadArgs &ra = a.rd; const IvTab &tab = a.rd.tab;
    auto pend_flush = [&](const int k) {
        const int32_t j = s_pj[k][tid];
        const uint32_t v = s_pv[k][tid];
        if (j >= 0 && v) atomicAdd(&a.rows[(unsigned long long)tab.e_out[j] * PR_ROW + (uint32_t)tid], (unsigned long long)v);
        s_pv[k][tid] = 0u;
    };
    if (tid < 3)
        for (int k = 0; k < PR_PEND; ++k) { s_pj[k][tid] = -1; s_pv[k][tid] = 0u; }
    const uint32_t n_chunks = (ra.n_reads + RG_B - 1) / RG_B;
    const uint32_t need = max(ra.min_cpgs, 1u);
    for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        bool elig = false;
        PrRead rd;
        rd.k0 = rd.k1 = 0; rd.first = INT32_MAX; rd.last = -1; rd.cls = PR_NONE;
        uint32_t k0, k1;
        if (rg_owned_read(ra, ch * RG_B + (uint32_t)tid, k0, k1)) {
            elig = pr_summary(ra.cpg_pos, k0, k1, rd);
            if (!elig) { atomicOr(&ra.st->err, (uint32_t)ERRB_RANGE); rd.first = INT32_MAX; rd.last = -1; rd.cls = PR_NONE; }
        }
        // the reads' smallest first and largest last call, and how many of them are of each class: all block-uniform from here on
        int32_t wmin = rd.first, wmax = rd.last;
        const uint32_t c0 = (uint32_t)__popcll(__ballot(rd.cls == PR_METH)), c1 = (uint32_t)__popcll(__ballot(rd.cls == PR_UNMETH)),
                       c2 = (uint32_t)__popcll(__ballot(rd.cls == PR_DISC));
        uint32_t cnt[3] = {0u, 0u, 0u};
        rg_span(s_red, wmin, wmax, lane, wave,                  // (its first barrier: the previous item's readers of s_cnt are done, too)
                [&](const int w) { s_cnt[0][w] = c0; s_cnt[1][w] = c1; s_cnt[2][w] = c2; },
                [&](const int w) { cnt[0] += s_cnt[0][w]; cnt[1] += s_cnt[1][w]; cnt[2] += s_cnt[2][w]; });
        if (wmax < 0) continue;                                 // no eligible read
        for (uint32_t s = ra.sl0; s < ra.sl1; ++s) {
            int32_t w_min, w_hi;
            if (!iv_candidates(tab, s, wmin, wmax, lane, w_min, w_hi)) continue;
            const int32_t acc_n = w_hi - w_min;
            // span route: an entry that holds the whole span lies in [w_min, w_hi) (its start <= wmin <= wmax, its end > wmax >= wmin)
            bool rest = false;                                  // one of this thread's candidates is left to the lanes
            if (a.span) {
                // A class whose one candidate holds the span (a chromosome-long interval) would take an add from every work item on
                // the same 32 bytes, and atomics on one line are served one request after the other: the workgroup keeps the sum
                // while its work items meet the same entry and adds it once (at the kernel's end, or when the entry changes)
                if (a.pend && acc_n == 1 && pr_holds_span(tab.e_start[w_min], tab.e_end[w_min], wmin, wmax)) {
                    if (tid < 3) {
                        const int k = (int)(s - ra.sl0);
                        if (s_pj[k][tid] != w_min) { pend_flush(k); s_pj[k][tid] = w_min; }
                        s_pv[k][tid] += tid == 0 ? cnt[0] : (tid == 1 ? cnt[1] : cnt[2]);
                    }
                    continue;
                }
                // four lanes per candidate, one per word: the three adds of an entry leave in one instruction and reach its line as
                // one request
                const int c = tid & 3;
                const uint32_t mine = c == 0 ? cnt[0] : (c == 1 ? cnt[1] : (c == 2 ? cnt[2] : 0u));
                for (int32_t j = w_min + (tid >> 2); j < w_hi; j += RG_B / 4) {
                    if (!pr_holds_span(tab.e_start[j], tab.e_end[j], wmin, wmax)) { rest = true; continue; }
                    if (mine) atomicAdd(&a.rows[(unsigned long long)tab.e_out[j] * PR_ROW + (uint32_t)c], (unsigned long long)mine);
                }
            } else rest = true;
            // (also: the previous slice's flush is done)
            if (!__syncthreads_or(rest ? 1 : 0)) continue;      // every candidate held the span: no per-read work
            const bool use_lds = acc_n <= a.acc_cap;
            if (use_lds) {
                iv_rows_zero<PR_ROW>(s_rows, acc_n, tid);
                __syncthreads();
            }
            if (elig)
                iv_walk(tab, w_min, w_hi, rd.first, rd.last, [&](const int32_t j, const int32_t ib, const int32_t ie) {
                    if (a.span && pr_holds_span(ib, ie, wmin, wmax)) return;                 // counted by the span route
                    const uint32_t cls = pr_entry_class(ra.cpg_pos, rd, ib, ie, need);
                    if (cls == PR_NONE) return;
                    if (use_lds) atomicAdd(&s_rows[(j - w_min) * PR_ROW + (int32_t)cls], 1u);
                    else atomicAdd(&a.rows[(unsigned long long)tab.e_out[j] * PR_ROW + cls], 1ull);
                });
            if (!use_lds) continue;
            __syncthreads();
            iv_rows_flush<PR_ROW>(s_rows, tab, w_min, acc_n, a.rows, tid);
        }
    }
    if (tid < 3)
        for (int k = 0; k < PR_PEND; ++k) pend_flush(k);
}

// what a context keeps between mth_pdr_regions_begin and the fetches
struct PdrRegions {
    bool on = false;
    RegionsTable iv;                                       // the declared intervals and their table
    DevBuf rows;
    int acc_cap = PR_ACC;                                  // the three knobs (mth_knobs.h), read when the context first declares intervals
    bool span = true;
    uint32_t grid_max = 8192;                              // workgroups of a launch at most (MTH_REGIONS_GRID)
};

void pdr_regions_release(mth_ctx *ctx) {
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr) return;
    pr->iv.release(); pr->rows.release();
    delete pr;
    ctx->pdr_regions = nullptr;
}

// forget the sums, keep the intervals (mth_reset, mth_pdr_regions_begin)
int pdr_regions_clear(mth_ctx *ctx) {
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr || !pr->on) return MTH_OK;
    const size_t n = pr->iv.size();
    if (n) MTH_HIP(ctx, hipMemsetAsync(pr->rows.p, 0, n * PR_ROW * 8, ctx->stream));
    return MTH_OK;
}

// the rows of the sums so far into host words (4 per interval); the stream is drained and the data errors of the batches surface here
static int pr_download(mth_ctx *ctx, PdrRegions &pr, std::vector<unsigned long long> &rows) {
    const int rc = sync_and_check(ctx);
    if (rc) return rc;
    const size_t n = pr.iv.size();
    rows.resize(n * PR_ROW);
    if (n) MTH_HIP(ctx, hipMemcpy(rows.data(), pr.rows.p, n * PR_ROW * 8, hipMemcpyDeviceToHost));
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_pdr_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    if (!ctx) return MTH_ERR_INVALID;
    const int bad = regions_check(ctx, "pdr regions:", n, tid, beg, end);
    if (bad) return bad;
    MTH_ENTER(ctx);
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing of an earlier set is in flight when its buffers are reused
    if (!ctx->pdr_regions) {
        ctx->pdr_regions = new PdrRegions;
        ctx->pdr_regions->acc_cap = pdr_regions_lds_cap_knob();
        ctx->pdr_regions->span = pdr_regions_span_knob();
        ctx->pdr_regions->grid_max = regions_grid_knob(8192u);
    }
    PdrRegions &pr = *ctx->pdr_regions;
    pr.iv.declare(n, tid, beg, end);
    MTH_HIP(ctx, pr.rows.reserve(std::max<size_t>((size_t)n, 1) * PR_ROW * 8, ctx->stream));
    pr.on = true;
    return pdr_regions_clear(ctx);
}

int mth_pdr_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_mhl_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    PdrRegions *prp = ctx->pdr_regions;
    if (!prp || !prp->on) return fail(ctx, MTH_ERR_STATE, "pdr regions: mth_pdr_regions_begin has not declared the intervals");
    PdrRegions &pr = *prp;
    mth_batch_t d;
    int rc = stage_batch(ctx, *batch, d);
    if (rc) return rc;
    std::pair<uint32_t, uint32_t> sl;
    if ((rc = pr.iv.slices_for(ctx, "pdr regions:", d.tid, &sl))) return rc;
    if (sl.first == sl.second || d.n_reads == 0 || d.n_cpgs == 0) return MTH_OK;      // no interval on the batch's contig(s), or no call
    if ((rc = pr.iv.upload(ctx))) return rc;
    PrArgs a;
    a.rd = rg_read_args(ctx, d, *params, pr.iv.dev, sl);
    a.rows = pr.rows.as<unsigned long long>(); a.acc_cap = pr.acc_cap;
    a.span = pr.span ? 1 : 0; a.pend = sl.second - sl.first <= (uint32_t)PR_PEND ? 1 : 0;
    const uint32_t grid = std::min<uint32_t>((d.n_reads + RG_B - 1) / RG_B, pr.grid_max);
    {
        LaunchTimer lt(ctx, K_PDR_REGIONS);
        hipLaunchKernelGGL(k_pdr_regions, dim3(grid), dim3(RG_B), 0, ctx->stream, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    return MTH_OK;                                        // queued: the batch's arrays stay as they are until the next call that waits
}

int mth_pdr_regions_counts(mth_ctx_t *ctx, uint64_t *methylated, uint64_t *unmethylated, uint64_t *discordant) {
    if (!ctx) return MTH_ERR_INVALID;
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr || !pr->on) return fail(ctx, MTH_ERR_STATE, "pdr regions: mth_pdr_regions_begin has not declared the intervals");
    std::vector<unsigned long long> rows;
    const int rc = pr_download(ctx, *pr, rows);
    if (rc) return rc;
    for (size_t i = 0; i < pr->iv.size(); ++i) {
        if (methylated) methylated[i] = rows[i * PR_ROW + PR_METH];
        if (unmethylated) unmethylated[i] = rows[i * PR_ROW + PR_UNMETH];
        if (discordant) discordant[i] = rows[i * PR_ROW + PR_DISC];
    }
    return MTH_OK;
}

float mth_pdr_regions_finalise(uint64_t n_concordant, uint64_t n_discordant, uint32_t min_depth) {
    return pdr_regions_finalise(n_concordant, n_discordant, min_depth);
}

int mth_pdr_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *pdr, uint64_t *n_concordant, uint64_t *n_discordant, uint64_t *n_methylated) {
    if (!ctx) return MTH_ERR_INVALID;
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr || !pr->on) return fail(ctx, MTH_ERR_STATE, "pdr regions: mth_pdr_regions_begin has not declared the intervals");
    std::vector<unsigned long long> rows;
    const int rc = pr_download(ctx, *pr, rows);
    if (rc) return rc;
    for (size_t i = 0; i < pr->iv.size(); ++i) {
        const uint64_t m = rows[i * PR_ROW + PR_METH], conc = m + rows[i * PR_ROW + PR_UNMETH], disc = rows[i * PR_ROW + PR_DISC];
        if (pdr) pdr[i] = pdr_regions_finalise(conc, disc, min_depth);
        if (n_concordant) n_concordant[i] = conc;
        if (n_discordant) n_discordant[i] = disc;
        if (n_methylated) n_methylated[i] = m;
    }
    return MTH_OK;
}

}  // extern "C"
