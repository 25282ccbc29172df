// mth_quartet_regions.hip -- ME and PM per interval (`metheor me-regions`, `pm-regions`, `all --me-intervals / --pm-intervals`): the
// methylation entropy (Xie et al. 2011) and the epipolymorphism (Landan et al. 2012) of a REGION, for every interval of a BED file in
// one pass over the reads.  Both values come from the same sixteen counters, so one pass serves both.
//
// Definition, in the reference's own terms.  For an interval [start, end) on contig c take each record once:
//   1. BismarkRead (readutil.rs:24-53); keep the calls with start <= abspos < end on c (and in the -c set): filter_isin
//      (readutil.rs:87-94) with the set "every position of the interval".  The kept calls stay in the read's call order.  A call at
//      position -1 lies in no interval.
//   2. the read contributes if mapq >= min_qual (me.rs:115) and at least 4 calls are kept (readutil.rs:101).
//   3. a contributing read adds get_cpg_quartets_and_patterns() (readutil.rs:97-132) of the kept calls: one pattern
//      8*m1 + 4*m2 + 2*m3 + m4 per window of four consecutive kept calls, n - 3 patterns for n kept calls -- all into ONE 16-bin
//      histogram for the interval (me.rs:121-125 with every quartet mapped to the same QuartetStat).
//   4. n_patterns = the sum of the 16 bins (the pooled stat's get_read_depth()), n_reads = the contributing reads.
//   5. ME = compute_me (me.rs:42-55), PM = compute_pm (pm.rs:42-51) of the histogram; each NaN when n_patterns < max(min_depth, 1)
//      (me.rs:82 applied to the pooled stat).  The counts are reported either way.
// No flush: every read counts once, so the counts are the same for any record order and any sharding.
//
// Device: a read x interval pass in the frame of mth_intervals_dev.h, as k_pdr_regions is (mth_pdr_regions.hip) -- 256 consecutive
// reads of a batch sorted by start per work item, one per lane; the OWNED ones that pass mapq and hold at least 4 calls are eligible
// (rg_owned_read); per length class of the batch's domain the candidate entries [w_min, w_hi) the work item's reads can touch
// (iv_candidates), a lane's walk over them (iv_walk), LDS rows (iv_rows_zero / iv_rows_flush).  What this pass has of its own:
//   * ROWS of seventeen words, sixteen bins and the reads: 32-bit in LDS (QUARTET_REGIONS_LDS_CAP = 240 candidates of a class per
//     work item, 15.9 KiB), 64-bit in memory (136 bytes per interval, no overflow list, no limit per read).  A class with more
//     candidates under one workgroup adds to memory directly (DIRECT ROUTE): slower, never wrong.
//   * Every eligible lane walks its calls ONCE before any interval is looked at (qr_summary, mth_quartet_regions_dev.h): smallest and
//     largest position by min / max, and for a read of at most 18 calls its own pattern histogram in sixteen 4-bit fields of one
//     64-bit register.  An interval that holds such a read whole takes one add per non-zero field and one for the reads word -- a
//     concordant read costs two atomics, not n - 2.  A partial overlap, or a longer read, makes one pass over the calls with a rolling
//     4-bit pattern register (qr_entry).
//   * CARRIED ROW.  A class with a single candidate (a chromosome-long interval) would be flushed by every work item to the same 136
//     bytes, and atomics on one line are served one request after the other.  Its row stays in LDS while the
//     workgroup's successive work items meet the same entry and is added to memory when the entry changes and at the kernel's end
//     -- or before the calls of the work items it has taken could reach 2^31: a work item lifts a word by less than its calls.
//   * A work item whose reads hold 2^23 calls or more adds to memory directly, so no 32-bit LDS word can overflow.
// No cross-lane operation happens inside a lane's walk.  Nothing here waits for the device: mth_quartet_regions_accumulate queues the
// kernel and returns; data errors (the word of position -1 in a batch) surface at the next counts / fetch.  The interval table (a
// RegionsTable, mth_regions_table.h) is replaced only when a batch brings a new domain, and its upload drains the stream first.
#include "mth_regions_table.h"
#include "mth_quartet_regions_dev.h"

namespace mth {

constexpr int QR_ACC = QUARTET_REGIONS_LDS_CAP;    // entries of a class a workgroup sums in LDS
constexpr int QR_CARRY = IvDomains::NCLS;          // slices of a domain (one per length class) a workgroup carries a row for

struct QrArgs {
    RgReadArgs rd;
    unsigned long long *rows;                      // per interval: QR_ROW words
    int32_t acc_cap;                               // 0 .. QR_ACC
    uint8_t summary, carry;                        // carry: the knob is on and the domain has at most QR_CARRY slices
};

__global__ __launch_bounds__(RG_B) void k_quartet_regions(const QrArgs a) {
    __shared__ uint32_t s_rows[QR_ACC * QR_ROW];
    __shared__ uint32_t s_carry[QR_CARRY * QR_ROW];        // per slice: the row of its single candidate, not yet in memory
    __shared__ int32_t s_cj[QR_CARRY];                     // ... that candidate (-1: none yet)
    __shared__ uint32_t s_cn[QR_CARRY];                    // ... and the calls of the work items the row has taken
    __shared__ int32_t s_red[2][RG_B / 64];
    __shared__ uint32_t s_calls[RG_B / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RgReadArgs &ra = a.rd; const IvTab &tab = a.rd.tab;
    // thread w < QR_ROW adds word w of slice k's carried row to its interval and clears it (the caller's barriers stand around it)
    auto carry_flush = [&](const int k, const int32_t j) {
        if (tid >= QR_ROW) return;
        const unsigned long long v = s_carry[k * QR_ROW + tid];
        if (j >= 0 && v) atomicAdd(&a.rows[(unsigned long long)tab.e_out[j] * QR_ROW + (uint32_t)tid], v);
        s_carry[k * QR_ROW + tid] = 0u;
    };
    for (int i = tid; i < QR_CARRY * QR_ROW; i += RG_B) s_carry[i] = 0u;
    if (tid < QR_CARRY) { s_cj[tid] = -1; s_cn[tid] = 0u; }
    __syncthreads();
    const uint32_t n_chunks = (ra.n_reads + RG_B - 1) / RG_B;
    for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        bool elig = false;
        QrRead rd;
        rd.k0 = rd.k1 = 0; rd.first = INT32_MAX; rd.last = -1; rd.packed = 0ull; rd.packed_ok = false;
        uint32_t k0, k1, calls = 0u;
        if (rg_owned_read(ra, ch * RG_B + (uint32_t)tid, k0, k1)) {
            elig = qr_summary(ra.cpg_pos, k0, k1, rd);
            if (elig) calls = qr_lane_calls(k0, k1);
            else { atomicOr(&ra.st->err, (uint32_t)ERRB_RANGE); rd.first = INT32_MAX; rd.last = -1; }
        }
        // the reads' smallest first and largest last call, and the calls they hold together: all block-uniform from here on
        int32_t wmin = rd.first, wmax = rd.last;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) calls += __shfl_xor(calls, o, 64);
        uint32_t item_calls = 0u;
        rg_span(s_red, wmin, wmax, lane, wave,                  // (its first barrier: the previous item's readers of s_calls are done, too)
                [&](const int w) { s_calls[w] = calls; }, [&](const int w) { item_calls += s_calls[w]; });
        if (wmax < 0) continue;                                 // no eligible read
        const bool small = item_calls < QR_LANE_CALLS_MAX;      // no lane was clamped: the sum is the true one, and no LDS word can gain 2^23
        for (uint32_t s = ra.sl0; s < ra.sl1; ++s) {
            int32_t w_min, w_hi;
            if (!iv_candidates(tab, s, wmin, wmax, lane, w_min, w_hi)) continue;
            const int32_t acc_n = w_hi - w_min;
            const bool use_lds = small && acc_n <= a.acc_cap;
            const bool carried = use_lds && a.carry && acc_n == 1;
            uint32_t *base = s_rows;                            // the LDS rows of the candidates [w_min, w_hi)
            if (carried) {
                const int k = (int)(s - ra.sl0);
                const int32_t cur = s_cj[k];
                const uint32_t cn = s_cn[k];
                __syncthreads();                                // every thread has read the two before thread 0 replaces them
                const bool flush = cur != w_min || cn + item_calls >= QR_CARRY_CALLS_MAX;      // (cn < 2^31, item_calls < 2^23)
                if (flush) carry_flush(k, cur);                 // (the adds to the row were a work item ago: rg_span's barriers)
                if (tid == 0) { s_cj[k] = w_min; s_cn[k] = (flush ? 0u : cn) + item_calls; }
                if (flush) __syncthreads();                     // the row is clear before the lanes add to it
                base = s_carry + k * QR_ROW;
            } else if (use_lds) {
                // (the previous slice's flush read word i in the thread that clears it here)
                iv_rows_zero<QR_ROW>(s_rows, acc_n, tid);
                __syncthreads();
            }
            if (elig)
                iv_walk(tab, w_min, w_hi, rd.first, rd.last, [&](const int32_t j, const int32_t ib, const int32_t ie) {
                    if (use_lds) {
                        uint32_t *row = base + (j - w_min) * QR_ROW;
                        qr_entry(ra.cpg_pos, rd, ib, ie, a.summary != 0, [&](const uint32_t w, const uint32_t v) { atomicAdd(&row[w], v); });
                    } else {
                        unsigned long long *row = a.rows + (unsigned long long)tab.e_out[j] * QR_ROW;
                        qr_entry(ra.cpg_pos, rd, ib, ie, a.summary != 0, [&](const uint32_t w, const uint32_t v) { atomicAdd(&row[w], (unsigned long long)v); });
                    }
                });
            if (!use_lds || carried) continue;
            __syncthreads();
            iv_rows_flush<QR_ROW>(s_rows, tab, w_min, acc_n, a.rows, tid);
        }
    }
    __syncthreads();
    for (int k = 0; k < QR_CARRY; ++k) carry_flush(k, s_cj[k]);
}

// what a context keeps between mth_quartet_regions_begin and the fetches
struct QuartetRegions {
    bool on = false;
    RegionsTable iv;                                       // the declared intervals and their table
    DevBuf rows;
    int acc_cap = QR_ACC;                                  // the four knobs (mth_knobs.h), read when the context first declares intervals
    bool summary = true, carry = true;
    uint32_t grid_max = 8192;                              // workgroups of a launch at most (MTH_REGIONS_GRID)
};

void quartet_regions_release(mth_ctx *ctx) {
    QuartetRegions *qr = ctx->quartet_regions;
    if (!qr) return;
    qr->iv.release(); qr->rows.release();
    delete qr;
    ctx->quartet_regions = nullptr;
}

// forget the sums, keep the intervals (mth_reset, mth_quartet_regions_begin)
int quartet_regions_clear(mth_ctx *ctx) {
    QuartetRegions *qr = ctx->quartet_regions;
    if (!qr || !qr->on) return MTH_OK;
    const size_t n = qr->iv.size();
    if (n) MTH_HIP(ctx, hipMemsetAsync(qr->rows.p, 0, n * QR_ROW * 8, ctx->stream));
    return MTH_OK;
}

// the rows of the sums so far into host words (17 per interval); the stream is drained and the data errors of the batches surface here
static int qr_download(mth_ctx *ctx, QuartetRegions &qr, std::vector<unsigned long long> &rows) {
    const int rc = sync_and_check(ctx);
    if (rc) return rc;
    const size_t n = qr.iv.size();
    rows.resize(n * QR_ROW);
    if (n) MTH_HIP(ctx, hipMemcpy(rows.data(), qr.rows.p, n * QR_ROW * 8, hipMemcpyDeviceToHost));
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_quartet_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    if (!ctx) return MTH_ERR_INVALID;
    const int bad = regions_check(ctx, "quartet regions:", n, tid, beg, end);
    if (bad) return bad;
    MTH_ENTER(ctx);
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing of an earlier set is in flight when its buffers are reused
    if (!ctx->quartet_regions) {
        ctx->quartet_regions = new QuartetRegions;
        ctx->quartet_regions->acc_cap = quartet_regions_lds_cap_knob();
        ctx->quartet_regions->summary = quartet_regions_summary_knob();
        ctx->quartet_regions->carry = quartet_regions_carry_knob();
        ctx->quartet_regions->grid_max = regions_grid_knob(8192u);
    }
    QuartetRegions &qr = *ctx->quartet_regions;
    qr.iv.declare(n, tid, beg, end);
    MTH_HIP(ctx, qr.rows.reserve(std::max<size_t>((size_t)n, 1) * QR_ROW * 8, ctx->stream));
    qr.on = true;
    return quartet_regions_clear(ctx);
}

int mth_quartet_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_quartet_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    QuartetRegions *qrp = ctx->quartet_regions;
    if (!qrp || !qrp->on) return fail(ctx, MTH_ERR_STATE, "quartet regions: mth_quartet_regions_begin has not declared the intervals");
    QuartetRegions &qr = *qrp;
    mth_batch_t d;
    int rc = stage_batch(ctx, *batch, d);
    if (rc) return rc;
    std::pair<uint32_t, uint32_t> sl;
    if ((rc = qr.iv.slices_for(ctx, "quartet regions:", d.tid, &sl))) return rc;
    if (sl.first == sl.second || d.n_reads == 0 || d.n_cpgs == 0) return MTH_OK;      // no interval on the batch's contig(s), or no call
    if ((rc = qr.iv.upload(ctx))) return rc;
    mth_mhl_params_t rp;
    rp.min_depth = 0; rp.min_cpgs = QR_NEED; rp.min_qual = params->min_qual;         // a read below four calls holds no window (readutil.rs:101)
    QrArgs a;
    a.rd = rg_read_args(ctx, d, rp, qr.iv.dev, sl);
    a.rows = qr.rows.as<unsigned long long>(); a.acc_cap = qr.acc_cap;
    a.summary = qr.summary ? 1 : 0; a.carry = qr.carry && sl.second - sl.first <= (uint32_t)QR_CARRY ? 1 : 0;
    const uint32_t grid = std::min<uint32_t>((d.n_reads + RG_B - 1) / RG_B, qr.grid_max);
    {
        LaunchTimer lt(ctx, K_QUARTET_REGIONS);
        hipLaunchKernelGGL(k_quartet_regions, dim3(grid), dim3(RG_B), 0, ctx->stream, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    return MTH_OK;                                        // queued: the batch's arrays stay as they are until the next call that waits
}

int mth_quartet_regions_counts(mth_ctx_t *ctx, uint64_t *bins, uint64_t *reads) {
    if (!ctx) return MTH_ERR_INVALID;
    QuartetRegions *qr = ctx->quartet_regions;
    if (!qr || !qr->on) return fail(ctx, MTH_ERR_STATE, "quartet regions: mth_quartet_regions_begin has not declared the intervals");
    std::vector<unsigned long long> rows;
    const int rc = qr_download(ctx, *qr, rows);
    if (rc) return rc;
    for (size_t i = 0; i < qr->iv.size(); ++i) {
        if (bins)
            for (int k = 0; k < QR_BINS; ++k) bins[i * QR_BINS + k] = rows[i * QR_ROW + k];
        if (reads) reads[i] = rows[i * QR_ROW + QR_READS];
    }
    return MTH_OK;
}

void mth_quartet_regions_finalise(const uint64_t *bins, uint32_t min_depth, float *me, float *pm, uint64_t *n_patterns) {
    quartet_regions_finalise(bins, min_depth, me, pm, n_patterns);
}

int mth_quartet_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *me, float *pm, uint64_t *n_patterns, uint64_t *n_reads) {
    if (!ctx) return MTH_ERR_INVALID;
    QuartetRegions *qr = ctx->quartet_regions;
    if (!qr || !qr->on) return fail(ctx, MTH_ERR_STATE, "quartet regions: mth_quartet_regions_begin has not declared the intervals");
    std::vector<unsigned long long> rows;
    const int rc = qr_download(ctx, *qr, rows);
    if (rc) return rc;
    for (size_t i = 0; i < qr->iv.size(); ++i) {
        uint64_t bins[QR_BINS];
        for (int k = 0; k < QR_BINS; ++k) bins[k] = rows[i * QR_ROW + k];
        quartet_regions_finalise(bins, min_depth, me ? me + i : nullptr, pm ? pm + i : nullptr, n_patterns ? n_patterns + i : nullptr);
        if (n_reads) n_reads[i] = rows[i * QR_ROW + QR_READS];
    }
    return MTH_OK;
}

}  // extern "C"
