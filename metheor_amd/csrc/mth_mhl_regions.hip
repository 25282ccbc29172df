// mth_mhl_regions.hip -- MHL per interval (`metheor mhl-regions`, `all --mhl-intervals`): methylation haplotype load of a REGION, as
// Guo et al. (2017) define it and the reference's README describes it, for every interval of a BED file in one pass over the reads.
//
// Definition, in the reference's own terms.  For an interval [start, end) on contig c take each record once:
//   1. BismarkRead (readutil.rs:24-53); keep the calls with start <= abspos < end on c (and in the -c set): filter_isin
//      (readutil.rs:87-94) with the set "every position of the interval".  A call at position -1 lies in no interval.
//   2. n = calls kept; the read contributes if mapq >= min_qual and n >= max(min_cpgs, 1) (mhl.rs:176-183, after the filter).
//   3. a contributing read adds n to the interval's num_cpgs and its get_stretch_info() (readutil.rs:147-164) to the interval's
//      stretch_info (mhl.rs:75-80, 36-41): one AssociatedReads per interval instead of one per CpG.
//   4. the value is compute_mhl() (mhl.rs:43-73) of it; fewer than max(min_depth, 1) contributing reads: NaN.
// No flush, no re-open: every read counts once, so the value is the same for any record order and any sharding.
//
// Two histograms per interval carry everything: R[r], maximal methylated runs of length r among the kept calls, and C[n], contributing
// reads with n kept calls (stretch_info[l] = sum_{r >= l} R[r] (r - l + 1), the denominator of l = sum_{n >= l} C[n] (n - l + 1)).  The
// device counts integers; mhl_regions_finalise (mth_regions_host.h) turns them into the f32.
//
// Device: a read x interval pass.  A batch's reads are sorted by start, so a workgroup takes 256 consecutive reads, one per lane; the
// OWNED ones (region_beg <= read_start < region_end: halo reads belong to a neighbour) that pass mapq and hold enough calls are
// eligible.  Per length class of the batch's domain (mth_regions_host.h) the workgroup finds, with wave-wide searches, the entries its
// reads can touch at all: those that start at or before the reads' largest last call and come at or after the first entry whose
// running maximum of the ends passes their smallest first call.  Up to MR_ACC such entries get a C / R row of MHL_REGIONS_BINS lengths in
// LDS; a read finds its last entry with start <= its last call by binary search, walks back while the running maximum is beyond its
// first call, and for every entry that ends beyond its first call walks its calls with the predicate of step 1 -- once to count n
// (not at all when the interval holds the read whole), once more for the runs if n passes.  The adds go to the LDS rows and the
// workgroup adds every non-zero bin to memory once: a chromosome-long interval among tiling windows is a class of its own, one LDS
// row, and costs some thirty 64-bit atomics per workgroup instead of four per read.  Classes that put more than MR_ACC entries under
// one workgroup (windows nested dozens deep, or reads of many kbp over short windows) add to memory directly: slower, never wrong.
// Lengths above MHL_REGIONS_BINS (nanopore reads over a CpG island) take the overflow route: an append-only list of (interval, length,
// kind) behind an atomic cursor, merged by the host.  An entry that does not fit is counted, not written: the batch is then run again
// with a list of the counted size, in a form that only appends, so nothing is added twice and nothing is dropped.
// No cross-lane operation happens inside a lane's walk: the searches and reductions that use the whole wave sit in block-uniform code.
// The frame -- owned-read test, span, candidate searches, the walk, the LDS rows' zeroing and flush -- is mth_intervals_dev.h's, shared
// with k_pdr_regions; the declared intervals and their table on the device are a RegionsTable (mth_regions_table.h).
#include "mth_regions_table.h"

namespace mth {

constexpr int MR_ACC = 32;                      // entries of a class a workgroup sums in LDS (16 KiB)
constexpr int MR_BINS = MHL_REGIONS_BINS;       // lengths of a dense row
constexpr int MR_ROW = 2 * MR_BINS;             // a row: C[1 .. BINS], then R[1 .. BINS]
constexpr uint32_t MR_MAX_CPGS = 16384;         // kept calls of a read (the limit MHL has: mth_sites.hip)

struct MrArgs {
    RgReadArgs rd;
    unsigned long long *dense;                     // per interval: a row
    uint2 *list;                                   // overflow entries: interval, length | kind << 31 (0: a read of that many kept calls, 1: a run)
    unsigned long long *state;                     // [0] the list's cursor
    unsigned long long list_cap;
    uint8_t list_only;
};

__global__ __launch_bounds__(RG_B) void k_mhl_regions(const MrArgs a) {
    __shared__ uint32_t s_rows[MR_ACC * MR_ROW];
    __shared__ int32_t s_red[2][RG_B / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RgReadArgs &rd = a.rd;
    const uint32_t n_chunks = (rd.n_reads + RG_B - 1) / RG_B;
    const uint32_t need = max(rd.min_cpgs, 1u);
    for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        bool elig = false;
        uint32_t k0 = 0, k1 = 0;
        int32_t first = INT32_MAX, last = -1;
        if (rg_owned_read(rd, ch * RG_B + (uint32_t)tid, k0, k1)) {
            const uint32_t w0 = rd.cpg_pos[k0] & 0x7fffffffu, w1 = rd.cpg_pos[k1 - 1] & 0x7fffffffu;
            // the word of position -1: no batch may carry it (include/metheor_hip.h, mth_batch_t.cpg_pos)
            if (w0 == 0x7fffffffu || w1 == 0x7fffffffu) atomicOr(&rd.st->err, (uint32_t)ERRB_RANGE);
            else { first = (int32_t)min(w0, w1); last = (int32_t)max(w0, w1); elig = true; }
        }
        // the reads' smallest first and largest last call: what of a slice the workgroup can touch
        int32_t wmin = first, wmax = last;
        rg_span(s_red, wmin, wmax, lane, wave, [](int) {}, [](int) {});
        if (wmax < 0) continue;                                 // no eligible read (block-uniform, as everything up to the lanes' walks)
        for (uint32_t s = rd.sl0; s < rd.sl1; ++s) {
            int32_t w_min, w_hi;
            if (!iv_candidates(rd.tab, s, wmin, wmax, lane, w_min, w_hi)) continue;
            const int32_t acc_n = w_hi - w_min;
            const bool use_lds = !a.list_only && acc_n <= MR_ACC;
            __syncthreads();                                    // the previous slice's flush is done
            if (use_lds) iv_rows_zero<MR_ROW>(s_rows, acc_n, tid);
            __syncthreads();
            if (elig)
                iv_walk(rd.tab, w_min, w_hi, first, last, [&](const int32_t j, const int32_t ib, const int32_t ie) {
                    uint32_t n = 0;
                    if (ib <= first && last < ie) n = k1 - k0;                                   // the interval holds the read whole
                    else
                        for (uint32_t k = k0; k < k1; ++k) {
                            const int32_t p = (int32_t)(rd.cpg_pos[k] & 0x7fffffffu);
                            n += (p >= ib && p < ie) ? 1u : 0u;
                        }
                    if (n < need) return;
                    if (n > MR_MAX_CPGS) { atomicOr(&rd.st->err, (uint32_t)ERRB_CAPACITY); return; }
                    const uint32_t out = rd.tab.e_out[j];
                    auto add = [&](const uint32_t kind, const uint32_t len) {
                        if (len <= (uint32_t)MR_BINS) {
                            if (a.list_only) return;
                            const uint32_t slot = kind * MR_BINS + len - 1;
                            if (use_lds) atomicAdd(&s_rows[(j - w_min) * MR_ROW + (int32_t)slot], 1u);
                            else atomicAdd(&a.dense[(unsigned long long)out * MR_ROW + slot], 1ull);
                        } else {
                            const unsigned long long at = atomicAdd(&a.state[0], 1ull);
                            if (at < a.list_cap) a.list[at] = make_uint2(out, len | (kind << 31));
                        }
                    };
                    add(0u, n);
                    uint32_t run = 0;                                                            // get_stretch_info, readutil.rs:147-164
                    for (uint32_t k = k0; k < k1; ++k) {
                        const uint32_t w = rd.cpg_pos[k];
                        const int32_t p = (int32_t)(w & 0x7fffffffu);
                        if (p < ib || p >= ie) continue;                                         // filter_isin: not a call of this read here
                        if (w >> 31) ++run;
                        else if (run) { add(1u, run); run = 0; }
                    }
                    if (run) add(1u, run);
                });
            if (!use_lds) continue;
            __syncthreads();
            iv_rows_flush<MR_ROW>(s_rows, rd.tab, w_min, acc_n, a.dense, tid);
        }
    }
}

// what a context keeps between mth_mhl_regions_begin and the fetches
struct MhlRegions {
    bool on = false;
    RegionsTable iv;                                       // the declared intervals and their table
    DevBuf dense, list, state;
    uint64_t list_cap = 0, list_used = 0;
    uint64_t stats[4] = {0, 0, 0, 0};                      // overflow entries, batches run again, batches, reads of the batches
    // the sparse rows (interval, length, runs, reads) as of the latest counts / fetch; valid until the next accumulate
    bool rows_valid = false;
    std::vector<uint32_t> r_iv, r_len;
    std::vector<uint64_t> r_runs, r_reads;
};

void mhl_regions_release(mth_ctx *ctx) {
    MhlRegions *mr = ctx->mhl_regions;
    if (!mr) return;
    mr->iv.release();
    for (DevBuf *b : {&mr->dense, &mr->list, &mr->state}) b->release();
    delete mr;
    ctx->mhl_regions = nullptr;
}

// forget the sums, keep the intervals (mth_reset, mth_mhl_regions_begin)
int mhl_regions_clear(mth_ctx *ctx) {
    MhlRegions *mr = ctx->mhl_regions;
    if (!mr || !mr->on) return MTH_OK;
    const size_t n = mr->iv.size();
    if (n) MTH_HIP(ctx, hipMemsetAsync(mr->dense.p, 0, n * MR_ROW * 8, ctx->stream));
    MTH_HIP(ctx, hipMemsetAsync(mr->state.p, 0, 16, ctx->stream));
    mr->list_used = 0;
    for (uint64_t &k : mr->stats) k = 0;
    mr->rows_valid = false;
    return MTH_OK;
}

// the sparse rows of the sums so far, sorted by (interval, length): the dense rows' non-zero bins and the overflow list merged
static int mr_build_rows(mth_ctx *ctx, MhlRegions &mr) {
    const int rc = sync_and_check(ctx);
    if (rc) return rc;
    if (mr.rows_valid) return MTH_OK;
    mr.r_iv.clear(); mr.r_len.clear(); mr.r_runs.clear(); mr.r_reads.clear();
    struct Ov { uint32_t iv, len; uint64_t runs, reads; };
    std::vector<Ov> ov;
    if (mr.list_used) {
        std::vector<uint2> ent((size_t)mr.list_used);
        MTH_HIP(ctx, hipMemcpy(ent.data(), mr.list.p, ent.size() * sizeof(uint2), hipMemcpyDeviceToHost));
        std::sort(ent.begin(), ent.end(), [](const uint2 &x, const uint2 &y) {
            const uint32_t lx = x.y & 0x7fffffffu, ly = y.y & 0x7fffffffu;
            return x.x != y.x ? x.x < y.x : lx < ly;
        });
        for (const uint2 &e : ent) {
            const uint32_t len = e.y & 0x7fffffffu;
            if (ov.empty() || ov.back().iv != e.x || ov.back().len != len) ov.push_back(Ov{e.x, len, 0, 0});
            if (e.y >> 31) ov.back().runs += 1; else ov.back().reads += 1;
        }
    }
    const size_t n = mr.iv.size();
    constexpr size_t STEP = 65536;                         // intervals per download (64 MiB)
    std::vector<unsigned long long> rows;
    size_t o = 0;
    for (size_t i0 = 0; i0 < n; i0 += STEP) {
        const size_t k = std::min(STEP, n - i0);
        rows.resize(k * MR_ROW);
        MTH_HIP(ctx, hipMemcpy(rows.data(), mr.dense.as<unsigned long long>() + i0 * MR_ROW, k * MR_ROW * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < k; ++i) {
            const unsigned long long *row = rows.data() + i * MR_ROW;
            for (int l = 0; l < MR_BINS; ++l)
                if (row[l] | row[MR_BINS + l]) {
                    mr.r_iv.push_back((uint32_t)(i0 + i)); mr.r_len.push_back((uint32_t)l + 1);
                    mr.r_reads.push_back(row[l]); mr.r_runs.push_back(row[MR_BINS + l]);
                }
            for (; o < ov.size() && ov[o].iv == (uint32_t)(i0 + i); ++o) {
                mr.r_iv.push_back(ov[o].iv); mr.r_len.push_back(ov[o].len);
                mr.r_reads.push_back(ov[o].reads); mr.r_runs.push_back(ov[o].runs);
            }
        }
    }
    mr.rows_valid = true;
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_mhl_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    if (!ctx) return MTH_ERR_INVALID;
    const int bad = regions_check(ctx, "mhl regions:", n, tid, beg, end);
    if (bad) return bad;
    MTH_ENTER(ctx);
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing of an earlier set is in flight when its buffers are reused
    if (!ctx->mhl_regions) ctx->mhl_regions = new MhlRegions;
    MhlRegions &mr = *ctx->mhl_regions;
    mr.iv.declare(n, tid, beg, end);
    MTH_HIP(ctx, mr.dense.reserve(std::max<size_t>((size_t)n, 1) * MR_ROW * 8, ctx->stream));
    MTH_HIP(ctx, mr.state.reserve(16, ctx->stream));
    mr.on = true;
    return mhl_regions_clear(ctx);
}

int mth_mhl_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_mhl_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    MhlRegions *mrp = ctx->mhl_regions;
    if (!mrp || !mrp->on) return fail(ctx, MTH_ERR_STATE, "mhl regions: mth_mhl_regions_begin has not declared the intervals");
    MhlRegions &mr = *mrp;
    mth_batch_t d;
    int rc = stage_batch(ctx, *batch, d);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    std::pair<uint32_t, uint32_t> sl;
    if ((rc = mr.iv.slices_for(ctx, "mhl regions:", d.tid, &sl))) return rc;
    mr.rows_valid = false;
    mr.stats[2] += 1; mr.stats[3] += d.n_reads;
    if (sl.first == sl.second || d.n_reads == 0 || d.n_cpgs == 0) return sync_and_check(ctx);     // no interval on the batch's contig(s), or no call
    if ((rc = mr.iv.upload(ctx))) return rc;
    if (!mr.list_cap) {
        const uint64_t cap = mhl_regions_list_knob();
        MTH_HIP(ctx, mr.list.reserve(cap * sizeof(uint2), s));
        mr.list_cap = cap;
    }
    MrArgs a;
    a.rd = rg_read_args(ctx, d, *params, mr.iv.dev, sl);
    a.dense = mr.dense.as<unsigned long long>(); a.list = mr.list.as<uint2>(); a.state = mr.state.as<unsigned long long>();
    a.list_cap = mr.list_cap; a.list_only = 0;
    const uint32_t grid = std::min<uint32_t>((d.n_reads + RG_B - 1) / RG_B, regions_grid_knob(8192u));      // (both runs of the batch)
    {
        LaunchTimer lt(ctx, K_MHL_REGIONS);
        hipLaunchKernelGGL(k_mhl_regions, dim3(grid), dim3(RG_B), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    if ((rc = sync_and_check(ctx))) return rc;            // the batch's data errors are this call's return value
    unsigned long long cursor = 0;
    MTH_HIP(ctx, hipMemcpy(&cursor, mr.state.p, 8, hipMemcpyDeviceToHost));
    if (cursor > mr.list_cap) {
        // the list was too short: the entries beyond it were counted, not written.  Again with the counted size, appending only --
        // the dense rows have the batch's adds already -- from where the list stood before the batch
        const uint64_t ncap = cursor + cursor / 4;
        MTH_HIP(ctx, mr.list.reserve(ncap * sizeof(uint2), s, true, mr.list_used * sizeof(uint2)));
        mr.list_cap = ncap;
        const unsigned long long back = mr.list_used;
        MTH_HIP(ctx, hipMemcpy(mr.state.p, &back, 8, hipMemcpyHostToDevice));
        a.list = mr.list.as<uint2>(); a.list_cap = mr.list_cap; a.list_only = 1;
        {
            LaunchTimer lt(ctx, K_MHL_REGIONS);
            hipLaunchKernelGGL(k_mhl_regions, dim3(grid), dim3(RG_B), 0, s, a);
        }
        MTH_HIP(ctx, hipGetLastError());
        if ((rc = sync_and_check(ctx))) return rc;
        unsigned long long again = 0;
        MTH_HIP(ctx, hipMemcpy(&again, mr.state.p, 8, hipMemcpyDeviceToHost));
        if (again != cursor) return fail(ctx, MTH_ERR_STATE, "mhl regions: the second run of a batch counted another number of overflow entries");
        mr.stats[1] += 1;
    }
    mr.stats[0] += cursor - mr.list_used;
    mr.list_used = cursor;
    return MTH_OK;
}

int mth_mhl_regions_counts(mth_ctx_t *ctx, uint64_t *n_rows, uint32_t *interval, uint32_t *length, uint64_t *runs, uint64_t *reads) {
    if (!ctx) return MTH_ERR_INVALID;
    MhlRegions *mr = ctx->mhl_regions;
    if (!mr || !mr->on) return fail(ctx, MTH_ERR_STATE, "mhl regions: mth_mhl_regions_begin has not declared the intervals");
    const int rc = mr_build_rows(ctx, *mr);
    if (rc) return rc;
    const size_t k = mr->r_iv.size();
    if (n_rows) *n_rows = k;
    if (interval && k) memcpy(interval, mr->r_iv.data(), k * 4);
    if (length && k) memcpy(length, mr->r_len.data(), k * 4);
    if (runs && k) memcpy(runs, mr->r_runs.data(), k * 8);
    if (reads && k) memcpy(reads, mr->r_reads.data(), k * 8);
    return MTH_OK;
}

float mth_mhl_regions_finalise(uint64_t k, const uint32_t *length, const uint64_t *runs, const uint64_t *reads, uint32_t min_depth,
                               uint64_t *n_reads, uint32_t *max_cpgs) {
    return mhl_regions_finalise((size_t)k, length, runs, reads, min_depth, n_reads, max_cpgs);
}

int mth_mhl_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *mhl, uint64_t *n_reads, uint32_t *max_cpgs) {
    if (!ctx) return MTH_ERR_INVALID;
    MhlRegions *mr = ctx->mhl_regions;
    if (!mr || !mr->on) return fail(ctx, MTH_ERR_STATE, "mhl regions: mth_mhl_regions_begin has not declared the intervals");
    const int rc = mr_build_rows(ctx, *mr);
    if (rc) return rc;
    const size_t n = mr->iv.size(), k = mr->r_iv.size();
    size_t o = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t o0 = o;
        while (o < k && mr->r_iv[o] == (uint32_t)i) ++o;
        uint64_t nr = 0;
        uint32_t mx = 0;
        const float v = mhl_regions_finalise(o - o0, mr->r_len.data() + o0, mr->r_runs.data() + o0, mr->r_reads.data() + o0, min_depth, &nr, &mx);
        if (mhl) mhl[i] = v;
        if (n_reads) n_reads[i] = nr;
        if (max_cpgs) max_cpgs[i] = mx;
    }
    return MTH_OK;
}

int mth_mhl_regions_stats(mth_ctx_t *ctx, uint64_t out[4]) {
    if (!ctx || !out) return MTH_ERR_INVALID;
    const MhlRegions *mr = ctx->mhl_regions;
    for (int k = 0; k < 4; ++k) out[k] = mr ? mr->stats[k] : 0;
    return MTH_OK;
}

}  // extern "C"
