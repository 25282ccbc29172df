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
// Device: a read x interval pass with the work decomposition of k_mhl_regions (mth_mhl_regions.hip) -- 256 consecutive reads of a
// batch sorted by start per work item, one per lane; the OWNED ones that pass mapq and hold enough calls are eligible; per length
// class of the batch's domain two wave-wide searches find the candidate entries [w_min, w_hi) the work item's reads can touch -- and
// three things that pass does not do:
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
// in a batch) surface at the next counts / fetch.  The interval table is replaced only when a batch brings a new domain, and that
// upload drains the stream first -- a synchronisation per new contig (group), none per batch.
#include <algorithm>
#include <memory>

#include "mth_ctx.h"
#include "mth_intervals_dev.h"
#include "mth_pdr_regions_dev.h"
#include "mth_regions_host.h"

namespace mth {

constexpr int PR_B = 256;                       // threads of a workgroup = reads of a work item
constexpr int PR_ACC = PDR_REGIONS_LDS_CAP;     // entries of a class a workgroup sums in LDS (16 KiB)
constexpr int PR_PEND = IvDomains::NCLS;        // slices of a domain (one per length class) a workgroup keeps a pending sum for

struct PrArgs {
    const int32_t *read_start;
    const uint8_t *read_mapq;
    const uint32_t *cpg_off, *cpg_pos;
    const int32_t *s_beg, *s_end;                  // per slice (one domain, one length class): its entries
    const int32_t *e_start, *e_end, *e_maxend;     // per entry, sorted by start within the slice; maxend: running maximum of e_end
    const uint32_t *e_out;                         // the interval (caller's index) the entry adds to
    unsigned long long *rows;                      // per interval: PR_ROW words
    DevState *st;
    uint32_t n_reads, n_cpgs, min_cpgs, sl0, sl1;
    int32_t region_beg, region_end, acc_cap;       // acc_cap: 0 .. PR_ACC
    uint8_t min_qual, span, pend;                  // pend: the domain has at most PR_PEND slices
};

__global__ __launch_bounds__(PR_B) void k_pdr_regions(const PrArgs a) {
    __shared__ uint32_t s_rows[PR_ACC * PR_ROW];
    __shared__ int32_t s_red[2][PR_B / 64];
    __shared__ uint32_t s_cnt[3][PR_B / 64];
    // per slice the entry that was its ONLY candidate and held the whole span, and what is still to be added to it: word c is
    // thread c's alone (each keeps its own copy of the entry), so no barrier orders them
    __shared__ int32_t s_pj[PR_PEND][4];
    __shared__ uint32_t s_pv[PR_PEND][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto pend_flush = [&](const int k) {
        const int32_t j = s_pj[k][tid];
        const uint32_t v = s_pv[k][tid];
        if (j >= 0 && v) atomicAdd(&a.rows[(unsigned long long)a.e_out[j] * PR_ROW + (uint32_t)tid], (unsigned long long)v);
        s_pv[k][tid] = 0u;
    };
    if (tid < 3)
        for (int k = 0; k < PR_PEND; ++k) { s_pj[k][tid] = -1; s_pv[k][tid] = 0u; }
    const uint32_t n_chunks = (a.n_reads + PR_B - 1) / PR_B;
    const uint32_t need = max(a.min_cpgs, 1u);
    for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const uint32_t r = ch * PR_B + (uint32_t)tid;
        bool elig = false;
        PrRead rd;
        rd.k0 = rd.k1 = 0; rd.first = INT32_MAX; rd.last = -1; rd.cls = PR_NONE;
        if (r < a.n_reads) {
            const int32_t rs = a.read_start[r];
            if (rs >= a.region_beg && rs < a.region_end && a.read_mapq[r] >= a.min_qual) {
                const uint32_t k0 = a.cpg_off[r], k1 = a.cpg_off[r + 1];
                if (k1 > k0 && k1 <= a.n_cpgs && k1 - k0 >= need) {
                    elig = pr_summary(a.cpg_pos, k0, k1, rd);
                    if (!elig) { atomicOr(&a.st->err, (uint32_t)ERRB_RANGE); rd.first = INT32_MAX; rd.last = -1; rd.cls = PR_NONE; }
                }
            }
        }
        // the reads' smallest first and largest last call, and how many of them are of each class: all block-uniform from here on
        int32_t wmin = rd.first, wmax = rd.last;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { wmin = min(wmin, __shfl_xor(wmin, o, 64)); wmax = max(wmax, __shfl_xor(wmax, o, 64)); }
        const uint32_t c0 = (uint32_t)__popcll(__ballot(rd.cls == PR_METH)), c1 = (uint32_t)__popcll(__ballot(rd.cls == PR_UNMETH)),
                       c2 = (uint32_t)__popcll(__ballot(rd.cls == PR_DISC));
        __syncthreads();                                        // the previous item's readers of s_red, s_cnt and s_rows are done
        if (lane == 0) { s_red[0][wave] = wmin; s_red[1][wave] = wmax; s_cnt[0][wave] = c0; s_cnt[1][wave] = c1; s_cnt[2][wave] = c2; }
        __syncthreads();
        uint32_t cnt[3] = {0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < PR_B / 64; ++w) {
            wmin = min(wmin, s_red[0][w]); wmax = max(wmax, s_red[1][w]);
            cnt[0] += s_cnt[0][w]; cnt[1] += s_cnt[1][w]; cnt[2] += s_cnt[2][w];
        }
        if (wmax < 0) continue;                                 // no eligible read
        for (uint32_t s = a.sl0; s < a.sl1; ++s) {
            const int32_t lo = a.s_beg[s], hi = a.s_end[s];
            const int32_t w_hi = iv_upper_wave(a.e_start, lo, hi, wmax, lane);
            if (w_hi == lo) continue;                           // every interval starts beyond the reads
            // the running maximum ascends: below w_min no interval reaches the reads' smallest first call, and no walk gets there
            const int32_t w_min = iv_upper_wave(a.e_maxend, lo, w_hi, wmin, lane);
            if (w_min == w_hi) continue;                        // every interval that starts in time ends before the reads
            const int32_t acc_n = w_hi - w_min;
            // span route: an entry that holds the whole span lies in [w_min, w_hi) (its start <= wmin <= wmax, its end > wmax >= wmin)
            bool rest = false;                                  // one of this thread's candidates is left to the lanes
            if (a.span) {
                // A class whose one candidate holds the span (a chromosome-long interval) would take an add from every work item on
                // the same 32 bytes, and atomics on one line are served one request after the other: the workgroup keeps the sum
                // while its work items meet the same entry and adds it once (at the kernel's end, or when the entry changes)
                if (a.pend && acc_n == 1 && pr_holds_span(a.e_start[w_min], a.e_end[w_min], wmin, wmax)) {
                    if (tid < 3) {
                        const int k = (int)(s - a.sl0);
                        if (s_pj[k][tid] != w_min) { pend_flush(k); s_pj[k][tid] = w_min; }
                        s_pv[k][tid] += tid == 0 ? cnt[0] : (tid == 1 ? cnt[1] : cnt[2]);
                    }
                    continue;
                }
                // four lanes per candidate, one per word: the three adds of an entry leave in one instruction and reach its line as
                // one request
                const int c = tid & 3;
                const uint32_t mine = c == 0 ? cnt[0] : (c == 1 ? cnt[1] : (c == 2 ? cnt[2] : 0u));
                for (int32_t j = w_min + (tid >> 2); j < w_hi; j += PR_B / 4) {
                    if (!pr_holds_span(a.e_start[j], a.e_end[j], wmin, wmax)) { rest = true; continue; }
                    if (mine) atomicAdd(&a.rows[(unsigned long long)a.e_out[j] * PR_ROW + (uint32_t)c], (unsigned long long)mine);
                }
            } else rest = true;
            // (also: the previous slice's flush is done)
            if (!__syncthreads_or(rest ? 1 : 0)) continue;      // every candidate held the span: no per-read work
            const bool use_lds = acc_n <= a.acc_cap;
            if (use_lds) {
                for (int32_t i = tid; i < acc_n * PR_ROW; i += PR_B) s_rows[i] = 0u;
                __syncthreads();
            }
            if (elig) {
                // the last entry with start <= the read's last call, then back while an end beyond its first call is still ahead
                for (int32_t j = iv_upper(a.e_start, w_min, w_hi, rd.last) - 1; j >= w_min && a.e_maxend[j] > rd.first; --j) {
                    const int32_t ie = a.e_end[j];
                    if (ie <= rd.first) continue;
                    const int32_t ib = a.e_start[j];
                    if (a.span && pr_holds_span(ib, ie, wmin, wmax)) continue;               // counted by the span route
                    const uint32_t cls = pr_entry_class(a.cpg_pos, rd, ib, ie, need);
                    if (cls == PR_NONE) continue;
                    if (use_lds) atomicAdd(&s_rows[(j - w_min) * PR_ROW + (int32_t)cls], 1u);
                    else atomicAdd(&a.rows[(unsigned long long)a.e_out[j] * PR_ROW + cls], 1ull);
                }
            }
            if (!use_lds) continue;
            __syncthreads();
            for (int32_t i = tid; i < acc_n * PR_ROW; i += PR_B) {      // one atomic per word the workgroup's reads filled
                const uint32_t v = s_rows[i];
                if (v) atomicAdd(&a.rows[(unsigned long long)a.e_out[w_min + i / PR_ROW] * PR_ROW + (uint32_t)(i % PR_ROW)], (unsigned long long)v);
            }
        }
    }
    if (tid < 3)
        for (int k = 0; k < PR_PEND; ++k) pend_flush(k);
}

// what a context keeps between mth_pdr_regions_begin and the fetches
struct PdrRegions {
    bool on = false;
    std::vector<int32_t> tid, beg, end;
    std::unique_ptr<IvDomains> dm;
    bool tab_dirty = true;                                 // a domain was added since the table went up
    size_t o_sb = 0, o_se = 0, o_es = 0, o_ee = 0, o_em = 0, o_eo = 0;      // the table's parts (32-bit words)
    DevBuf tab, rows;
    int acc_cap = PR_ACC;                                  // the two knobs (mth_knobs.h), read when the context first declares intervals
    bool span = true;
};

void pdr_regions_release(mth_ctx *ctx) {
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr) return;
    pr->tab.release(); pr->rows.release();
    delete pr;
    ctx->pdr_regions = nullptr;
}

// forget the sums, keep the intervals (mth_reset, mth_pdr_regions_begin)
int pdr_regions_clear(mth_ctx *ctx) {
    PdrRegions *pr = ctx->pdr_regions;
    if (!pr || !pr->on) return MTH_OK;
    const size_t n = pr->tid.size();
    if (n) MTH_HIP(ctx, hipMemsetAsync(pr->rows.p, 0, n * PR_ROW * 8, ctx->stream));
    return MTH_OK;
}

static int pr_upload_table(mth_ctx *ctx, PdrRegions &pr) {
    const IvDomains &dm = *pr.dm;
    std::vector<uint32_t> tab;
    auto place = [&](const void *src, size_t words) {
        const size_t at = tab.size();
        tab.resize(at + words);
        if (words) memcpy(tab.data() + at, src, words * 4);
        return at;
    };
    pr.o_sb = place(dm.s_beg.data(), dm.s_beg.size()); pr.o_se = place(dm.s_end.data(), dm.s_end.size());
    pr.o_es = place(dm.e_start.data(), dm.e_start.size()); pr.o_ee = place(dm.e_end.data(), dm.e_end.size());
    pr.o_em = place(dm.e_maxend.data(), dm.e_maxend.size()); pr.o_eo = place(dm.e_out.data(), dm.e_out.size());
    // the kernels of earlier batches read the table that is replaced here, and no accumulate waits for them: drain the stream first.
    // Once per new domain (a contig or contig group the intervals had not met), not once per batch; `tab` may go after the copy
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MTH_HIP(ctx, pr.tab.reserve(std::max<size_t>(tab.size(), 1) * 4, ctx->stream));
    if (!tab.empty()) MTH_HIP(ctx, hipMemcpy(pr.tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    pr.tab_dirty = false;
    return MTH_OK;
}

// the rows of the sums so far into host words (4 per interval); the stream is drained and the data errors of the batches surface here
static int pr_download(mth_ctx *ctx, PdrRegions &pr, std::vector<unsigned long long> &rows) {
    const int rc = sync_and_check(ctx);
    if (rc) return rc;
    const size_t n = pr.tid.size();
    rows.resize(n * PR_ROW);
    if (n) MTH_HIP(ctx, hipMemcpy(rows.data(), pr.rows.p, n * PR_ROW * 8, hipMemcpyDeviceToHost));
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_pdr_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    if (!ctx) return MTH_ERR_INVALID;
    if (n && (!tid || !beg || !end)) return fail(ctx, MTH_ERR_INVALID, "pdr regions: an array is missing");
    if (n >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "pdr regions: 2^31 or more intervals");
    for (uint64_t i = 0; i < n; ++i)
        if (tid[i] < 0 || beg[i] < 0 || end[i] < beg[i]) return fail(ctx, MTH_ERR_INVALID, "pdr regions: want tid >= 0 and 0 <= beg <= end");
    MTH_ENTER(ctx);
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing of an earlier set is in flight when its buffers are reused
    if (!ctx->pdr_regions) {
        ctx->pdr_regions = new PdrRegions;
        ctx->pdr_regions->acc_cap = pdr_regions_lds_cap_knob();
        ctx->pdr_regions->span = pdr_regions_span_knob();
    }
    PdrRegions &pr = *ctx->pdr_regions;
    pr.tid.assign(tid, tid + n); pr.beg.assign(beg, beg + n); pr.end.assign(end, end + n);
    pr.dm.reset(new IvDomains(n, pr.tid.data(), pr.beg.data(), pr.end.data()));
    pr.tab_dirty = true;
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
    if (!pr.dm->has(d.tid)) {
        if (d.tid >= 0) pr.dm->add_domain(d.tid);
        else {
            if (d.tid > -2) return fail(ctx, MTH_ERR_INVALID, "pdr regions: batch.tid");
            const mth_ctx::ContigGroup &g = ctx->groups[(size_t)(-2 - (int64_t)d.tid)];      // (stage_batch has checked the handle)
            pr.dm->add_domain(d.tid, g.tids.size(), g.tids.data(), g.voff.data());
        }
        if (pr.dm->entries() >= (size_t)INT32_MAX) return fail(ctx, MTH_ERR_CAPACITY, "pdr regions: 2^31 or more interval entries");
        pr.tab_dirty = true;
    }
    const auto sl = pr.dm->dom_slices[d.tid];
    if (sl.first == sl.second || d.n_reads == 0 || d.n_cpgs == 0) return MTH_OK;      // no interval on the batch's contig(s), or no call
    if (pr.tab_dirty && (rc = pr_upload_table(ctx, pr))) return rc;
    const uint32_t *tab = pr.tab.as<uint32_t>();
    PrArgs a;
    a.read_start = d.read_start; a.read_mapq = d.read_mapq; a.cpg_off = d.cpg_off; a.cpg_pos = d.cpg_pos;
    a.s_beg = reinterpret_cast<const int32_t *>(tab + pr.o_sb); a.s_end = reinterpret_cast<const int32_t *>(tab + pr.o_se);
    a.e_start = reinterpret_cast<const int32_t *>(tab + pr.o_es); a.e_end = reinterpret_cast<const int32_t *>(tab + pr.o_ee);
    a.e_maxend = reinterpret_cast<const int32_t *>(tab + pr.o_em); a.e_out = tab + pr.o_eo;
    a.rows = pr.rows.as<unsigned long long>(); a.st = ctx->d_state;
    a.n_reads = d.n_reads; a.n_cpgs = d.n_cpgs; a.min_cpgs = params->min_cpgs; a.sl0 = sl.first; a.sl1 = sl.second;
    a.region_beg = d.region_beg; a.region_end = d.region_end; a.acc_cap = pr.acc_cap;
    a.min_qual = params->min_qual; a.span = pr.span ? 1 : 0; a.pend = sl.second - sl.first <= (uint32_t)PR_PEND ? 1 : 0;
    const uint32_t grid = std::min<uint32_t>((d.n_reads + PR_B - 1) / PR_B, 8192u);
    {
        LaunchTimer lt(ctx, K_PDR_REGIONS);
        hipLaunchKernelGGL(k_pdr_regions, dim3(grid), dim3(PR_B), 0, ctx->stream, a);
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
    for (size_t i = 0; i < pr->tid.size(); ++i) {
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
    for (size_t i = 0; i < pr->tid.size(); ++i) {
        const uint64_t m = rows[i * PR_ROW + PR_METH], conc = m + rows[i * PR_ROW + PR_UNMETH], disc = rows[i * PR_ROW + PR_DISC];
        if (pdr) pdr[i] = pdr_regions_finalise(conc, disc, min_depth);
        if (n_concordant) n_concordant[i] = conc;
        if (n_discordant) n_discordant[i] = disc;
        if (n_methylated) n_methylated[i] = m;
    }
    return MTH_OK;
}

}  // extern "C"
