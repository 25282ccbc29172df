// mth_tile_rows.hip -- the tile-row table protocol: the host side that the tile-kernel measures share (ME / PM: mth_quartet.hip,
// LPMD pairs: mth_pairs.hip, and the quartet side of the fused pass: mth_multi.hip).
//
// A measure's tile kernel claims output rows tile by tile from a counter on the device (state word [1]) and leaves per tile where
// its rows went (tile_row0 / tile_rows); tiles its LDS table cannot hold are flagged for the measure's global path ([5]), rows
// claimed beyond the output are counted ([6]).  The output is sized from the rows per CpG call the batches so far gave -- there is
// no counting pre-pass -- and a batch that did not fit is redone once at the exact size, which the kernel reports.  What differs
// between the measures is a TileMeasure (mth_ctx.h); the state it works on is the measure's TileRowTable in the context.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mth_ctx.h"

namespace mth {

constexpr int TILE_STATE_WORDS = 8;
constexpr int TILE_QUEUE_MAX = 4096;    // queued batches between two resolves (their snapshots: 256 KB)

// (re)start of a batch: back to the row count before it, no tile flagged, nothing beyond the output
__global__ void k_tile_rows_rewind(unsigned long long *w, unsigned long long rows_before) { w[1] = rows_before; w[5] = 0; w[6] = 0; }

// a queued batch's state words as its tile kernel left them ([1] rows so far, [5] tiles for the global path and [6] tiles that did not
// fit, both since the run of queued batches began): read back by tile_rows_resolve, not by the call that queued the batch
__global__ void k_tile_rows_snap(const unsigned long long *__restrict__ w, unsigned long long *__restrict__ snap) {
    if (threadIdx.x < TILE_STATE_WORDS) snap[threadIdx.x] = w[threadIdx.x];
}

// a measure's knob MTH_<MEASURE>_<suffix>
static const char *knob(const TileRowTable &t, const char *suffix) { return tile_rows_knob(t.env, suffix); }

int tile_rows_open(mth_ctx *ctx, TileRowTable &t, uint64_t ntiles) {
    hipStream_t s = ctx->stream;
    if (!t.state.p) {
        MTH_HIP(ctx, t.state.reserve(TILE_STATE_WORDS * sizeof(unsigned long long), s));
        MTH_HIP(ctx, hipMemsetAsync(t.state.p, 0, TILE_STATE_WORDS * sizeof(unsigned long long), s));
    }
    const uint64_t tiles_before = t.tiles();
    MTH_HIP(ctx, t.tflag.reserve((size_t)ntiles * 4, s));
    MTH_HIP(ctx, t.tile_row0.reserve((tiles_before + ntiles) * 8, s, true, tiles_before * 8));
    MTH_HIP(ctx, t.tile_rows.reserve((tiles_before + ntiles) * 4, s, true, tiles_before * 4));
    return MTH_OK;
}

hipError_t tile_rows_grow(mth_ctx *ctx, TileRowTable &t, uint64_t cap, uint64_t used) {
    const hipError_t e = t.measure->grow_rows(ctx, cap, used);
    if (e == hipSuccess) t.cap = cap;
    return e;
}

int tile_rows_rewind(mth_ctx *ctx, TileRowTable &t, uint64_t rows_before) {
    hipLaunchKernelGGL(k_tile_rows_rewind, dim3(1), dim3(1), 0, ctx->stream, t.words(), (unsigned long long)rows_before);
    MTH_HIP(ctx, hipGetLastError());
    return MTH_OK;
}

void tile_rows_commit(TileRowTable &t, TileBatch meta, uint64_t total, uint64_t n_cpgs) {
    meta.rows = total - t.rows;
    t.rows = total;
    if (n_cpgs) { t.rows_per_cpg = std::max(t.rows_per_cpg * 0.5, (double)meta.rows / (double)n_cpgs); t.learned = true; }
    t.meta.push_back(meta);
}

// One batch.  queued = false: the call ends knowing the batch's rows (one host sync; redone with the exact size if the rows did not fit,
// the global path for tiles the LDS table could not hold).  queued = true (device-resident batches after the first of a job): tile
// kernel and a snapshot of the state words only -- whether everything fitted is looked at by tile_rows_resolve, at the next call that
// needs the rows, and anything else than "all fitted, no tile for the global path" replays the batches from the first such one on
// through the synchronous form (their arrays are still there: include/metheor_hip.h, device-resident batches stay untouched until
// the next synchronising call).
static int tile_rows_batch(mth_ctx *ctx, TileRowTable &t, const mth_batch_t &d, const TileParams &params, int32_t batch_tid, bool queued) {
    int rc = MTH_OK;
    hipStream_t s = ctx->stream;
    const TileMeasure &m = *t.measure;
    const int64_t region_len = (int64_t)d.region_end - d.region_beg;
    const int tile_shift = m.tile_shift(d, params);
    const int tile_w = 1 << tile_shift;
    const uint32_t ntiles = (d.n_reads && region_len > 0) ? (uint32_t)((region_len + tile_w - 1) / tile_w) : 0u;
    const uint64_t tiles_before = t.tiles();
    // queued: the exact count is on the device only; rows_est bounds it from above (every queued batch so far within its estimate --
    // if one was not, the resolve replays from there and none of this batch's rows survive anyway)
    const uint64_t rows_before = queued && !t.pending.empty() ? t.rows_est : t.rows;
    TileBatch meta{batch_tid, 0, rows_before, tiles_before + ntiles};
    if ((rc = tile_rows_open(ctx, t, ntiles))) return rc;
    if (!ntiles && queued && !t.pending.empty()) queued = false, rc = tile_rows_resolve(ctx, t);       // (rare: an empty batch inside a run)
    if (rc) return rc;
    if (!ntiles) { meta.heavy0 = t.rows; t.meta.push_back(meta); return MTH_OK; }
    int32_t idx_base = 0;
    uint32_t nt = 0;
    rc = build_read_index(ctx, d, tile_w, idx_base, nt);
    if (rc) return rc;
    // output size: rows per CpG call of the batches so far (first batch: a guess); the kernel reports the exact need
    uint64_t want = rows_before + (uint64_t)((double)d.n_cpgs * t.rows_per_cpg * 1.25) + 4096;
    if (const char *e = knob(t, "ROWS_MIN")) want = rows_before + strtoull(e, nullptr, 10);   // tests: force the redo
    unsigned long long *st = ctx->h_words;     // pinned: the read-back does not go through a staging copy
    for (int attempt = 0;; ++attempt) {
        if (want > t.cap) MTH_HIP(ctx, tile_rows_grow(ctx, t, want + (queued ? want / 4 : 0), std::min<uint64_t>(rows_before, t.cap)));
        // a run of queued batches continues from the device's own row count; its first batch (and every synchronous one) starts from
        // the host's, which is exact then
        if ((!queued || t.pending.empty()) && (rc = tile_rows_rewind(ctx, t, rows_before))) return rc;
        // a queued batch must stay within its ESTIMATE, not just within the buffer: the next queued batch takes the estimate as the
        // rows in use and keeps only that many when it grows the buffer (rows between the estimate and the device's count were once
        // lost without a flag); beyond the estimate the batch is unfit and tile_rows_resolve replays it
        m.launch_tiles(ctx, d, params, tile_shift, ntiles, idx_base, tiles_before, queued ? std::min<uint64_t>(t.cap, want) : t.cap);
        if (queued) {
            MTH_HIP(ctx, t.snap.reserve((size_t)TILE_QUEUE_MAX * TILE_STATE_WORDS * sizeof(unsigned long long), s));
            hipLaunchKernelGGL(k_tile_rows_snap, dim3(1), dim3(64), 0, s, (const unsigned long long *)t.words(),
                               t.snap.as<unsigned long long>() + t.pending.size() * TILE_STATE_WORDS);
            MTH_HIP(ctx, hipGetLastError());
            t.pending.push_back(TileRowTable::Queued{d, params, batch_tid, d.n_cpgs});
            t.rows_est = want;
            t.meta.push_back(meta);                     // rows / heavy0: tile_rows_resolve
            return MTH_OK;
        }
        MTH_HIP(ctx, hipMemcpyAsync(st, t.words(), TILE_STATE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipStreamSynchronize(s));            // one sync per batch: rows, flagged tiles, fit
        if (!st[6]) break;
        if (attempt) return fail(ctx, MTH_ERR_STATE, (std::string(t.what) + ": rows did not fit an exactly sized output").c_str());
        want = st[1];                                     // every tile claimed its range: this is the exact size
    }
    uint64_t total = st[1];
    meta.heavy0 = total;
    if (st[5] && (rc = m.global_path(ctx, d, params, tile_shift, total))) return rc;
    MTH_HIP(ctx, hipGetLastError());
    tile_rows_commit(t, meta, total, d.n_cpgs);
    return MTH_OK;
}

// The queued batches' rows: one read-back of their snapshots.  All fitted and no tile was left to the global path: the metas get
// their row counts.  Otherwise the batches from the first one that says so are replayed synchronously, in order.
int tile_rows_resolve(mth_ctx *ctx, TileRowTable &t) {
    if (t.pending.empty()) return MTH_OK;
    // (a replay below rebuilds its batch's read index in the context's own buffer: whatever prepared batch the latest entry point
    // worked on is not this one's)
    ctx->cur_prep = nullptr; ctx->cur_idx = nullptr;
    MTH_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<TileRowTable::Queued> pend;
    pend.swap(t.pending);
    const size_t n = pend.size(), base = t.meta.size() - n;
    std::vector<unsigned long long> snap(n * TILE_STATE_WORDS);
    MTH_HIP(ctx, hipMemcpyAsync(snap.data(), t.snap.p, snap.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t good = 0;
    uint64_t rows = 0, cpgs = 0;
    for (; good < n; ++good) {
        const unsigned long long *w = snap.data() + good * TILE_STATE_WORDS;
        if (w[5] || w[6]) break;
        TileBatch &m = t.meta[base + good];
        m.rows = w[1] - t.rows;
        m.heavy0 = w[1];
        rows += m.rows; cpgs += pend[good].n_cpgs;
        t.rows = w[1];
    }
    if (cpgs) t.rows_per_cpg = std::max(t.rows_per_cpg * 0.5, (double)rows / (double)cpgs);
    if (knob(t, "DEBUG")) fprintf(stderr, "[%s] queued batches %zu, replayed %zu\n", t.name, n, n - good);     // tests
    if (good == n) return MTH_OK;
    t.meta.resize(base + good);
    for (size_t k = good; k < n; ++k) {
        const int rc = tile_rows_batch(ctx, t, pend[k].d, pend[k].params, pend[k].tid, false);
        if (rc) return rc;
    }
    return MTH_OK;
}

// A measure's accumulate entry point.  Queued (no host sync in the call): a device-resident batch once a batch of this context has
// taught the output sizing, unless the launches are being timed.  MTH_*_QUEUE=0 switches it off (A/B).  Every other entry point
// settles the queue (mth::enter).
int tile_rows_accumulate(mth_ctx *ctx, TileRowTable &t, const mth_batch_t &batch, const TileParams &params) {
    if (t.queue_off < 0) {
        const char *e = knob(t, "QUEUE");
        t.queue_off = e && atoi(e) == 0;
    }
    const bool queued = (batch.mem == MTH_MEM_DEVICE || batch.mem == MTH_MEM_PREPARED) && t.learned && !ctx->timing && !t.queue_off &&
                        t.pending.size() < (size_t)TILE_QUEUE_MAX;
    mth_batch_t d;
    ctx->tile_queue_hold = queued;
    int rc = stage_batch(ctx, batch, d);
    ctx->tile_queue_hold = false;
    if (rc) return rc;
    if (!queued && (rc = tile_rows_resolve(ctx, t))) return rc;
    return tile_rows_batch(ctx, t, d, params, batch.tid, queued);
}

}  // namespace mth
