// mth_multi.hip -- mth_multi_accumulate: every requested measure over ONE batch (the entry point of `metheor all`), and the host side
// of the fused PDR + LPMD + ME / PM tile pass it runs on sparse batches (the kernel, k_multi_tile, is the wide form's body with the
// quartet side switched on: mth_pdr_wide.hip).
//
// Each measure's own entry point replaces one compute_helper pass of the reference over the file (pdr.rs:119, lpmd.rs:154, me.rs:90,
// pm.rs:85, mhl.rs:135, fdrp.rs:176, qfdrp.rs:188).  mth_multi_accumulate prepares the batch once (one device copy, one read index)
// and runs the requested measures over it.  PDR + LPMD (k_pdr_lpmd_wide, mth_pdr_wide.hip) and ME / PM (k_quartet_tile,
// mth_quartet.hip) have the same shape -- phase 1 reads cpg_off / start / mapq of every candidate read of a tile and queues the reads
// with work, phase 2 walks the queue with every lane live, rows are bucket-sorted out of an LDS table whose size does not grow with the
// tile -- so where launch_pdr_lpmd takes the wide form, k_multi_tile (the same body as k_pdr_lpmd_wide) does both from ONE walk:
//   queue      a read enters if LPMD (>= 2 calls, lpmd mapq), PDR (>= min_cpgs calls, pdr mapq) or ME / PM (>= 4 calls, quartet mapq)
//              has work for it; each measure keeps its own filters in phase 2
//   phase 2    a queued read's calls are loaded once (two 16-byte loads) and feed the PDR site table, the LPMD sums and the quartet
//              table (512 slots, sixteen 16-bit bins each)
//   outputs    the PDR side exactly as k_pdr_lpmd_wide writes it (scratch slices, tile_cnt, bucket sums: k_gather, mth_pdr_fetch, site
//              discovery unchanged); the quartet side as k_quartet_tile writes it (per-tile tile_row0 / tile_rows, the batch's meta:
//              mth_quartet_fetch unchanged)
//   hand back  a tile with more than 65 535 candidate reads (16-bit bins), more distinct quartets than slots, or a wide quartet (two
//              consecutive CpGs >= 2048 bp apart) is flagged; the host then redoes the batch's ME / PM side through
//              mth_quartet_accumulate, whose global path gives those rows.  A stretch with more PDR sites than slots is redone in halves
//              (PDR + LPMD only: the quartet table is complete after the tile's first stretch, which is the whole tile).
// Where launch_pdr_lpmd takes the dense per-position kernel (dense batches), MTH_MULTI_AUTO runs the two existing passes; MTH_MULTI_FUSED
// takes the fused pass on any batch (16384-bp slices on a dense one).  Synchronous per batch.
#include <cstdlib>

#include "mth_ctx.h"
#include "mth_quartet_dev.h"
#include "mth_tile_dev.h"

namespace mth {

// PDR and / or LPMD plus ME / PM of one (prepared) batch through the fused pass where launch_pdr_lpmd takes its wide form (or
// everywhere: force).  *fused: the pass ran (else the quartet side went through mth_quartet_accumulate as in the split form).
static int fused_batch(mth_ctx *ctx, const mth_batch_t &pb, const mth_multi_params_t &mp, bool force, bool *fused) {
    *fused = false;
    MTH_ENTER(ctx);                                         // queued ME / PM batches settled: the table's row count is exact
    hipStream_t s = ctx->stream;
    TileRowTable &t = ctx->quartets;
    const uint64_t rows_before = t.rows, tiles_before = t.tiles();
    const int64_t region_len = (int64_t)pb.region_end - pb.region_beg;
    // a wide-form tile is at least 8192 positions (half a 16384-bp slice); at most one quartet row per CpG call of the batch
    const uint32_t max_tiles = (uint32_t)std::max<int64_t>(region_len, 0) / 8192u + 2u;
    int rc = tile_rows_open(ctx, t, max_tiles);
    if (rc) return rc;
    if (rows_before + pb.n_cpgs + 1024 > t.cap) MTH_HIP(ctx, tile_rows_grow(ctx, t, rows_before + pb.n_cpgs + 1024, rows_before));
    if ((rc = tile_rows_rewind(ctx, t, rows_before))) return rc;
    unsigned long long *qs = t.words();
    FusedQuartet fq;
    fq.force = force ? 1 : 0;
    fq.force_heavy = multi_force_handback_knob() ? 1 : 0;       // tests: every tile handed back
    fq.min_qual = mp.quartet.min_qual;
    fq.qs = qs; fq.row_cap = t.cap; fq.max_tiles = max_tiles;
    fq.tile_flag = t.tflag.as<uint32_t>();
    fq.tile_row0 = t.tile_row0.as<unsigned long long>() + tiles_before;
    fq.tile_rows = t.tile_rows.as<uint32_t>() + tiles_before;
    fq.out_pos = ctx->q_pos.as<int32_t>(); fq.out_cnt = ctx->q_cnt.as<uint32_t>(); fq.out_me = ctx->q_me.as<float>();
    fq.out_pm = ctx->q_pm.as<float>(); fq.out_depth = ctx->q_depth.as<uint32_t>();
    fq.taken = false; fq.ntiles = 0;
    mth_pdr_lpmd_params_t p = mp.pdr_lpmd;
    p.want_pdr = (mp.want & MTH_MULTI_PDR) ? 1 : 0;
    p.want_lpmd = (mp.want & MTH_MULTI_LPMD) ? 1 : 0;
    ctx->fuse_q = &fq;
    rc = mth_pdr_lpmd_accumulate(ctx, &pb, &p);
    ctx->fuse_q = nullptr;
    if (rc) return rc;
    if (!fq.taken) return mth_quartet_accumulate(ctx, &pb, &mp.quartet);     // (the dense form ran, or a PDR-only exact pass)
    *fused = true;
    unsigned long long *st = ctx->h_words;
    MTH_HIP(ctx, hipMemcpyAsync(st, qs, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    ctx->multi_stats[2] += fq.ntiles;
    if (st[5] || st[6]) {
        // hand back: the batch's ME / PM side again through the single entry point (its rows restart at rows_before; no meta was kept)
        ctx->multi_stats[3] += st[6] ? fq.ntiles : st[5];
        return mth_quartet_accumulate(ctx, &pb, &mp.quartet);
    }
    tile_rows_commit(t, TileBatch{pb.tid, 0, st[1], tiles_before + fq.ntiles}, st[1], pb.n_cpgs);
    ctx->q_epoch += 1;
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_multi_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_multi_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    const uint32_t all = MTH_MULTI_PDR | MTH_MULTI_LPMD | MTH_MULTI_QUARTET | MTH_MULTI_MHL | MTH_MULTI_FDRP | MTH_MULTI_PAIRS;
    const uint32_t want = params->want;
    if (want == 0 || (want & ~all)) return fail(ctx, MTH_ERR_INVALID, "mth_multi_params_t.want: no measure, or an unknown bit");
    if (params->form != MTH_MULTI_AUTO && params->form != MTH_MULTI_FUSED && params->form != MTH_MULTI_SPLIT)
        return fail(ctx, MTH_ERR_INVALID, "mth_multi_params_t.form");
    mth_batch_t pb = *batch;
    const bool own = batch->mem != MTH_MEM_PREPARED;
    if (own) {
        const int rc = mth_batch_prepare(ctx, batch, &pb);
        if (rc) return rc;
    }
    int rc = MTH_OK;
    bool fused = false;
    // the fused pass needs both of its consumers: PDR and / or LPMD, and ME / PM
    if (params->form != MTH_MULTI_SPLIT && (want & MTH_MULTI_QUARTET) && (want & (MTH_MULTI_PDR | MTH_MULTI_LPMD))) {
        rc = fused_batch(ctx, pb, *params, params->form == MTH_MULTI_FUSED, &fused);
    } else {
        if (want & (MTH_MULTI_PDR | MTH_MULTI_LPMD)) {
            mth_pdr_lpmd_params_t p = params->pdr_lpmd;
            p.want_pdr = (want & MTH_MULTI_PDR) ? 1 : 0;
            p.want_lpmd = (want & MTH_MULTI_LPMD) ? 1 : 0;
            rc = mth_pdr_lpmd_accumulate(ctx, &pb, &p);
        }
        if (!rc && (want & MTH_MULTI_QUARTET)) rc = mth_quartet_accumulate(ctx, &pb, &params->quartet);
    }
    if (!rc && (want & MTH_MULTI_MHL)) rc = mth_mhl_accumulate(ctx, &pb, &params->mhl);
    if (!rc && (want & MTH_MULTI_FDRP)) rc = mth_fdrp_accumulate(ctx, &pb, &params->fdrp);
    if (!rc && (want & MTH_MULTI_PAIRS)) rc = mth_lpmd_pairs_accumulate(ctx, &pb, &params->pairs);
    // synchronous per batch: queued ME / PM and pairs batches are settled and the batch's data errors reported here, so that the
    // prepared batch can go (its index and, for a host batch, its device copies) and the caller may reuse its arrays
    if (!rc) rc = mth_ctx_sync(ctx);
    if (own) {
        const int rr = mth_batch_release(ctx, &pb);
        if (!rc) rc = rr;
    }
    if (!rc) ctx->multi_stats[fused ? 0 : 1] += 1;
    return rc;
}

int mth_multi_stats(mth_ctx_t *ctx, uint64_t out[4]) {
    if (!ctx || !out) return MTH_ERR_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = ctx->multi_stats[k];
    return MTH_OK;
}

}  // extern "C"
