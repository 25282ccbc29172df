// mth_ctx.h -- host-side context of the engine (private).
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "mth_common.h"
#include "mth_knobs.h"

namespace mth {

// grow-only device buffer
struct DevBuf {
    void  *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes, hipStream_t s, bool keep = false, size_t keep_bytes = 0);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct TimedLaunch {
    int kernel;
    hipEvent_t beg, end;
};

struct BatchMeta {
    int32_t tid;
};

// One lane of the PDR + LPMD batch pipeline (mth_pdr_lpmd.hip, "Pipelined batches"): a stream of its own, the per-batch work
// buffers (lane 0 borrows the context's own idx / tile_cnt / tile_bucket / scratch, lane 1 has a second set) and a small
// device block for what belongs to the batch in flight on the lane rather than to the job: error bits, safe_hi, the row base.
struct PdrLane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;          // recorded behind the lane's latest k_gather
    DevBuf idx, tile_cnt, tile_bucket, scratch;      // lane 1 only
    DevState *st = nullptr;
    bool used = false;                  // has work that ctx->stream has not been made to wait for
};

}  // namespace mth

struct mth_ctx;
namespace mth { struct FusedQuartet; struct MhlRegions; struct PdrRegions; struct QuartetRegions; }

namespace mth {
// ---- the tile-row table of a tile-kernel measure (ME / PM, LPMD pairs; driver: mth_tile_rows.hip) ----
// a batch: heavy0 = first row of the global path's rows, tile_end = tiles of all batches up to and including it
struct TileBatch { int32_t tid; uint64_t rows, heavy0, tile_end; };
union TileParams { mth_quartet_params_t quartet; mth_lpmd_pairs_params_t pairs; };
// what a measure brings to the driver; everything else of a batch is tile_rows_batch
struct TileMeasure {
    int (*tile_shift)(const mth_batch_t &d, const TileParams &p);                 // log2 of the batch's tile width, 13 .. 16
    hipError_t (*grow_rows)(mth_ctx *ctx, uint64_t cap, uint64_t used);           // the row columns to cap rows, keeping the first `used`
    // the tile kernel over the batch's ntiles tiles (per-tile arrays from tiles_before on; row_cap: rows it may write)
    void (*launch_tiles)(mth_ctx *ctx, const mth_batch_t &d, const TileParams &p, int tile_shift, uint32_t ntiles, int32_t idx_base,
                         uint64_t tiles_before, uint64_t row_cap);
    // the global path for the tiles flagged in tflag; total: rows in use before it -> after it
    int (*global_path)(mth_ctx *ctx, const mth_batch_t &d, const TileParams &p, int tile_shift, uint64_t &total);
};
const TileMeasure *quartet_measure();     // mth_quartet.hip
const TileMeasure *pairs_measure();       // mth_pairs.hip
struct TileRowTable {
    const char *name, *what, *env;         // "[name] ..." debug line, "what: ..." error text, prefix of the MTH_*_ knobs
    double rows_per_cpg;                   // output sizing of the next batch
    const TileMeasure *measure;
    // eight state words: [0] updates (counting pass of the global path) [1] total rows [2] first row of the global path's rows
    // [3] its overflow flag [5] tiles left to the global path [6] tiles whose rows did not fit the output ([7]: the measure's own)
    DevBuf state, snap;                    // snap: the state words as each queued batch's tile kernel left them
    DevBuf tflag, tile_row0, tile_rows;    // per tile: 1 = left to the global path (latest batch only); first row and length (all batches)
    std::vector<TileBatch> meta;
    uint64_t cap = 0, rows = 0;            // row capacity, rows in use (exact as of the last synchronous batch / tile_rows_resolve)
    uint64_t rows_est = 0;                 // upper bound of the rows in use while batches are queued
    bool learned = false;                  // a synchronous batch has set rows_per_cpg
    int queue_off = -1;                    // MTH_*_QUEUE=0 (read once)
    // batches queued without a host sync: their device-side batch (its arrays stay untouched until the resolve)
    struct Queued { mth_batch_t d; TileParams params; int32_t tid; uint64_t n_cpgs; };
    std::vector<Queued> pending;
    unsigned long long *words() const { return state.as<unsigned long long>(); }
    uint64_t tiles() const { return meta.empty() ? 0 : meta.back().tile_end; }
};
int tile_rows_accumulate(mth_ctx *ctx, TileRowTable &t, const mth_batch_t &batch, const TileParams &params);
int tile_rows_resolve(mth_ctx *ctx, TileRowTable &t);
// the pieces the fused pass (mth_multi.hip) drives itself: state words and per-tile arrays for ntiles more tiles, the row columns,
// the (re)start of a batch at rows_before, and a finished batch into the table
int tile_rows_open(mth_ctx *ctx, TileRowTable &t, uint64_t ntiles);
hipError_t tile_rows_grow(mth_ctx *ctx, TileRowTable &t, uint64_t cap, uint64_t used);
int tile_rows_rewind(mth_ctx *ctx, TileRowTable &t, uint64_t rows_before);
void tile_rows_commit(TileRowTable &t, TileBatch meta, uint64_t total, uint64_t n_cpgs);

// a prepared batch (include/metheor_hip.h, "prepared batches"): the device-resident batch, the buffers it owns when it was made
// from a host batch, its fine read index, and a device block with what k_build_index found (error bits, safe_hi)
struct Prepared {
    static constexpr uint64_t MAGIC = 0x6d74685f70726570ull;
    uint64_t magic = MAGIC;
    mth_ctx *owner = nullptr;
    mth_batch_t dev{};
    DevBuf own[7];
    DevBuf idx;
    int32_t idx_base = 0;
    uint32_t nq = 0;
    DevState *st = nullptr;
};

// the .bai index under construction (mth_bai.hip): device tables, the run rows appended window by window, and the host copies
// mth_bai_finish hands out
struct BaiBuild {
    bool on = false;                       // between mth_bai_begin and mth_bai_finish: mth_tag_records_bam indexes its windows
    int err = 0;                           // the first error a window raised (kept until the next mth_bai_begin)
    std::string err_msg;
    int32_t n_refs = 0;
    uint64_t file_off = 0;                 // file offset of the next block mth_tag_records_bam makes
    uint64_t n_records = 0, n_rows = 0, row_cap = 0;
    int par = 0;                           // generation of the device state's "record before" words the next window reads
    DevBuf state, lin, tab, meta, n_intv;  // tab: n_refs + 1 linear-table offsets, then n_refs reference lengths
    DevBuf key, vb, ve, flag, rank, cut;   // per record of the window in flight; cut: an explicit call's cuts + block offsets
    DevBuf r_key, r_vb, r_ve;              // run rows, file order
    DevBuf skey, idx, perm, tmp, cb, ce, bin_key, bin_start, bin_cnt, ref_nbin;     // mth_bai_finish
    std::vector<uint64_t> h_lin_off, h_cb, h_ce, h_bin_key, h_lin, h_meta;
    std::vector<uint32_t> h_bin_cnt, h_bin_id, h_ref_nbin, h_n_intv;
    std::vector<int32_t> h_bin_ref;
};
}  // namespace mth

struct mth_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;
    // the prepared batches this context owns (mth_batch_prepare): a handle is valid iff it is in here -- never dereferenced to find out;
    // mth_ctx_destroy frees what the caller did not release
    std::unordered_set<mth::Prepared *> prepared;
    mth::Prepared *cur_prep = nullptr;   // the batch of the entry point in progress is a prepared one (set by stage_batch, every call)
    const uint32_t *cur_idx = nullptr;   // the fine read index the call's kernels use: the prepared batch's, or ctx->idx after a build
    uint32_t notes = 0;                 // mth_notes(): non-fatal findings so far (MTH_NOTE_*)

    mth::DevState *d_state = nullptr;   // device
    mth::DevState *h_state = nullptr;   // pinned host mirror
    unsigned long long *h_words = nullptr;   // 16 pinned words: per-batch read-backs of the tile-kernel measures

    // staging for MTH_MEM_HOST batches
    mth::DevBuf st_start, st_end, st_mapq, st_fwd, st_off, st_pos, st_rel;
    // per-batch work buffers
    mth::DevBuf idx, tile_cnt, tile_bucket, scratch, batch_cnt;
    // PDR + LPMD batch pipeline: consecutive device-resident batches alternate between two lanes so that batch k+1's index build
    // and the head of its tile kernel run beside batch k's tail and gather; only the gathers form a chain (each waits for the one
    // before it: row bases, batch counts and the LPMD totals live in DevState).  Any other entry point joins the lanes back into
    // ctx->stream first (mth::enter).
    mth::PdrLane lane[2];
    hipEvent_t pipe_in = nullptr;       // recorded on ctx->stream at each pipelined call: the lane waits for the caller's producers
    int pipe_mode = -1;                 // -1: not decided (MTH_PIPELINE env), 0: off, 1: on
    int pipe_next = 0;                  // lane of the next pipelined batch
    int pipe_tail = -1;                 // lane that holds the latest gather (-1: none since the last join)
    bool pipe_active = false;           // lanes hold work ctx->stream has not been ordered behind
    unsigned pdr_streak = 0;            // consecutive eligible mth_pdr_lpmd_accumulate calls (mth_reset does not break the run)
    bool reset_pending = false;         // mth_reset inside a pipelined run: folded into the next batch's gather
    // device-side BAM record decode (mth_decode.hip): staged input, decoded SoA, scan scratch, one batch's 32-bit offsets
    mth::DevBuf dec_raw, dec_recoff, dec_tid, dec_start, dec_end, dec_mapq, dec_fwd, dec_n, dec_off, dec_pos, dec_rel, dec_blk, dec_off32, dec_runs, dec_xm, dec_filter;
    bool dec_filter_on = false;
    uint32_t dec_xm_min_mapq = 0;       // records without XM:Z are an error from this mapq up (0: always)
    uint64_t dec_filter_n = 0;
    uint64_t dec_reads = 0, dec_cpgs = 0;
    uint32_t dec_contig_flags = 0;      // flags of the latest mth_decoded_contigs over the decoded stream (bit0 / bit1: records a batch cannot hold)
    // device-side BGZF inflate + per-block record walk (mth_inflate.hip)
    mth::DevBuf inf_file, inf_tab, inf_raw, inf_cnt, inf_base, inf_recoff, crc_mat;
    // mth_bgzf_stage: the NEXT chunk's file bytes, copied on a side stream while the current chunk is being inflated
    mth::DevBuf inf_file2;
    hipStream_t copy_stream = nullptr;
    hipEvent_t staged_ev = nullptr;
    hipStream_t piece_stream = nullptr;  // an in-line chunk's file bytes travel here in pieces, each piece's blocks inflate as it lands
    std::vector<hipEvent_t> piece_ev;
    const void *staged_src = nullptr;
    uint64_t staged_bytes = 0;
    const void *next_src = nullptr;      // announced by mth_bgzf_stage, copied by a helper thread the next inflate call starts
    uint64_t next_bytes = 0;
    std::thread stage_thread;
    int stage_rc = 0;
    mth_load_stats_t load_stats = {0, 0, 0, 0, 0, 0};    // mth_load_stats: which way the load calls went since the last mth_reset
    // mth_bgzf_decode_straddle: per-block entry / exit / count of the record chain (two generations, a round reads one and writes
    // the other), and the bytes of the record the previous call's stream ended in (they come first in the next call's stream)
    mth::DevBuf inf_links, inf_carry;
    uint64_t carry_bytes = 0;
    // mth_bgzf_straddle_scan: the run's inflated bytes (inf_raw), block table (inf_tab) and links (inf_links) stay for
    // mth_bgzf_straddle_rescan until the next call that inflates (or mth_reset)
    bool scan_valid = false;
    uint64_t scan_n_run = 0, scan_total = 0;
    uint64_t *scan_uoff = nullptr;
    uint32_t *scan_isize = nullptr;
    int scan_cur = 0;
    // `tag` (mth_tag.hip): the genome (contigs back to back), per-contig offsets + header lengths, per-record work arrays,
    // and the host copies mth_tag_records hands out
    mth::DevBuf tag_genome, tag_goff, tag_ncol, tag_coloff, tag_xmlen, tag_cols, tag_xm;
    int32_t tag_n_refs = -1;
    std::vector<uint64_t> tag_h_goff;        // host copy of the n_refs + 1 contig offsets (mth_tag_genome_fetch)
    // mth_tag_set_genome_fasta (mth_fasta.hip): the genome being packed -- it becomes tag_genome only when the whole file has
    // passed verification -- and the segment table + error word of the window in flight
    mth::DevBuf fa_genome, fa_tab;
    // mth_decode_set_genome: the decode derives its calls from tag_genome (mth_decode_genome.hip) instead of XM:Z
    bool dec_genome = false, dec_genome_paired = false;
    // mth_decode_set_modtags: the decode takes its calls from MM:Z / ML:B:C (mth_decode_mm.hip)
    bool dec_modtags = false;
    uint32_t dec_mm_threshold = 128;
    unsigned long long tag_cols_total = 0;   // column scratch of the decode call in progress (count pass -> fill pass)
    std::vector<uint64_t> tag_h_off;
    std::vector<uint32_t> tag_h_len;
    std::vector<uint8_t> tag_h_xm;
    // `tag -O bam` (mth_tag.hip: the tagged record stream; mth_deflate.hip: its BGZF blocks): per-record tagged sizes and output
    // offsets, the stream, and the deflate step's block table, token scratch, per-block slots and the compacted blocks
    mth::DevBuf tag_sz, tag_ooff, tag_stream;
    std::vector<uint32_t> tag_h_sz;
    std::vector<uint64_t> tag_h_cut;
    mth::DevBuf def_src, def_tab, def_tok, def_slot, def_boff, def_out;
    std::vector<uint8_t> def_h_out;
    std::vector<uint64_t> def_h_boff;
    mth::BaiBuild bai;
    // contig groups (include/metheor_hip.h, "contig groups"): handle -2 - k is groups[k]
    struct ContigGroup { std::vector<int32_t> tids; std::vector<int64_t> voff; mth::DevBuf d_tab; };   // d_tab: n voff (int32) then n tids
    std::vector<ContigGroup> groups;
    bool dec_grouped = false;                // mth_decoded_group has shifted the decoded stream's positions
    // results (PDR columns)
    mth::DevBuf out_pos, out_pdr, out_nc, out_nd;
    uint64_t out_cap = 0;        // rows
    uint64_t out_bound = 0;      // host-known upper bound of rows in use
    std::vector<mth::BatchMeta> batches;
    size_t batch_cnt_cap = 0;

    // ME / PM (mth_quartet.hip): hash table of the batch in flight + appended result rows
    mth::TileRowTable quartets{"quartet", "quartets", "MTH_QUARTET", 0.15, mth::quartet_measure()};
    mth::DevBuf q_keys, q_hist, q_blk, q_batch_rows, q_wpos, q_wpat, q_wk0, q_wk1;
    mth::DevBuf q_pos, q_cnt, q_me, q_pm, q_depth;
    bool tile_queue_hold = false;          // set by the accumulate call that is queueing a batch: enter() leaves the queues alone
    // the row order worked out by a count-only mth_quartet_fetch, kept for the fetch that follows it (same min_depth,
    // nothing accumulated in between: q_epoch)
    uint64_t q_epoch = 0, q_order_epoch = ~0ull;
    uint32_t q_order_min_depth = 0;
    std::vector<uint64_t> q_order;
    std::vector<int32_t> q_order_tid;

    // site-walk measures (mth_sites.hip): discovery sink, per-candidate work arrays, MHL result rows
    mth::DevState *d_state2 = nullptr;
    mth::DevBuf s_pos, s_pdr, s_nc, s_nd, s_batch_cnt;
    mth::DevBuf w_val, w_cov, w_aux, w_flags, w_blk, w_huge;
    mth::DevBuf m_state, m_pos, m_val, m_cov, m_batch_rows;
    uint64_t m_cap = 0, m_rows_bound = 0;
    std::vector<mth::BatchMeta> m_batches;

    // FDRP / qFDRP result rows (mth_fdrp.hip)
    mth::DevBuf f_state, f_pos, f_val, f_qval, f_n, f_batch_rows, f_rows, f_pairtab, f_redo, f_terms, f_soff, f_snz, f_sdisc, f_quot;
    uint64_t f_cap = 0, f_rows_bound = 0;
    std::vector<mth::BatchMeta> f_batches;

    // the flush-based measures of a stream that is not coordinate-sorted (mth_fileorder.hip): work arrays, result rows
    mth::DevBuf fo_sel, fo_flag, fo_tmp, fo_out;
    uint64_t fo_rows = 0;

    // LPMD per-pair table (mth_pairs.hip)
    mth::TileRowTable pairs{"pairs", "pairs", "MTH_PAIRS", 0.1, mth::pairs_measure()};
    mth::DevBuf p_keys, p_cnt, p_out_key, p_out_cnt, p_batch_rows;
    // LPMD per interval (mth_intervals.hip): the sorted intervals + work items of the call in flight, the per-interval sums
    mth::DevBuf iv_tab, iv_acc;
    // MHL per interval (mth_mhl_regions.hip): the declared intervals, their sorted slices, the histograms (nullptr until the first begin)
    mth::MhlRegions *mhl_regions = nullptr;
    // PDR per interval (mth_pdr_regions.hip): the declared intervals, their sorted slices, three counters each (nullptr until the first begin)
    mth::PdrRegions *pdr_regions = nullptr;
    // ME / PM per interval (mth_quartet_regions.hip): the declared intervals, their sorted slices, sixteen bins and the reads each (nullptr until the first begin)
    mth::QuartetRegions *quartet_regions = nullptr;

    // multi-GPU exchange step (mth_rccl.hip): communicator of the one-process-per-GPU form; lpmd_reduced = DevState.lpmd
    // already holds the all-reduced totals (cleared by the next batch that adds to them)
    void *rccl_comm = nullptr;
    int rccl_rank = 0, rccl_world = 1;
    bool lpmd_reduced = false;
    // the rank form reduces out of place on a side stream: ring of 4-counter slots, red_slot = slot of the latest reduce
    // (-1: the totals are in DevState.lpmd itself)
    static constexpr int RED_RING = 4;
    hipStream_t red_stream = nullptr;
    long long *red_buf = nullptr;
    hipEvent_t red_ready[RED_RING] = {}, red_done[RED_RING] = {};
    uint64_t red_head = 0;
    int red_slot = -1;

    // mth_multi_accumulate (mth_multi.hip): batches fused / split, tiles fused / handed back since the last mth_reset
    uint64_t multi_stats[4] = {0, 0, 0, 0};
    // set by mth_multi_accumulate around its PDR + LPMD call: the wide form of that pass then runs as the fused tile pass (nullptr always else)
    mth::FusedQuartet *fuse_q = nullptr;

    bool timing = false;
    std::vector<mth::TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
};

namespace mth {

int  fail(mth_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess);
// first thing every entry point does: make the context's device current for the calling thread (it may be new) and order
// ctx->stream behind whatever the PDR + LPMD pipeline lanes still hold
int  enter(mth_ctx *ctx);
// rows of grouped batches back to (tid, position): tid[i] <= -2 is a group handle, pos_a[i * stride .. + cols) and pos_b[i] (optional)
// its virtual positions (mth_api.hip)
int  ungroup_rows(mth_ctx *ctx, uint64_t n, int32_t *tid, int32_t *pos_a, int stride, int cols, int32_t *pos_b);
bool has_group_batch(const mth_ctx *ctx, int which);      // any grouped batch among the accumulated ones of measure `which` (0 pdr 1 mhl 2 fdrp 3 quartet 4 pairs)
// device table of a group handle (n voff as int32, then n tids), nullptr / 0 for a plain tid
const int32_t *group_table(const mth_ctx *ctx, int32_t tid, uint32_t *n);
int  pipe_join(mth_ctx *ctx);
// the context's prepared batch behind a caller's handle, nullptr if it is not one of them (released, another context's, made up)
Prepared *prepared_lookup(const mth_ctx *ctx, const void *handle);
void prepared_free(mth_ctx *ctx, Prepared *pr);           // buffers + the object itself; the registry entry goes with it
#define MTH_ENTER(ctx)                                                  \
    do {                                                                \
        const int rc__ = mth::enter(ctx);                               \
        if (rc__) return rc__;                                          \
    } while (0)
#define MTH_HIP(ctx, call)                                              \
    do {                                                                \
        hipError_t e__ = (call);                                        \
        if (e__ != hipSuccess) return mth::fail(ctx, MTH_ERR_HIP, #call, e__); \
    } while (0)

// time-bracketed kernel launch helper
struct LaunchTimer {
    mth_ctx *ctx;
    int kernel;
    hipEvent_t beg = nullptr, end = nullptr;
    LaunchTimer(mth_ctx *c, int k);
    ~LaunchTimer();
};

void rccl_release(mth_ctx *ctx);    // mth_rccl.hip: destroy the context's communicator, if any
int sync_and_check(mth_ctx *ctx);   // stream sync + read DevState + map error bits
// validate a caller batch and make it device-resident (MTH_MEM_HOST arrays go through the staging buffers)
int stage_batch(mth_ctx *ctx, const mth_batch_t &b, mth_batch_t &dev, bool join = true);
// mth_decode.hip: 64-bit exclusive scan of a u32 array (synchronises), and the record decode over device-resident input
int scan_u32_to_u64(mth_ctx *ctx, const uint32_t *n, uint32_t count, unsigned long long base, unsigned long long *off,
                    unsigned long long *total_host);
int decode_core(mth_ctx *ctx, const uint8_t *d_raw, const uint64_t *d_off, uint64_t n_rec, int append, mth_decoded_t *out);
// mth_tag.hip: the tail of the two genome entry points -- the genome's bytes are in ctx->tag_genome, contig t at off[t]: the
// offsets and header lengths go up, the stream is drained and the genome is the context's from there on
int genome_commit(mth_ctx *ctx, int32_t n_refs, const std::vector<uint64_t> &off, const int64_t *ref_len);
// mth_tag.hip: the XM strings of n device-resident records into ctx->tag_xm (offsets tag_coloff, lengths tag_xmlen); *total = bytes
int tag_core(mth_ctx *ctx, const uint8_t *d_raw, const uint64_t *d_off, uint32_t n, int is_paired_end, unsigned long long *total);
// mth_inflate.hip: CRC-32 of device-resident blocks (k_crc32) into d_out
int crc32_blocks(mth_ctx *ctx, const uint8_t *raw, const uint64_t *d_uoff, const uint32_t *d_isize, uint32_t n_blocks, uint32_t *d_out);
// mth_deflate.hip: n_blocks BGZF blocks of the device-resident bytes d_src cut at h_cut (n_blocks + 1 ascending offsets, blocks of
// at most 0xff00 bytes) into ctx->def_h_out, block b at ctx->def_h_boff[b]; synchronises
int deflate_core(mth_ctx *ctx, const uint8_t *d_src, const uint64_t *h_cut, uint64_t n_blocks);
// mth_bai.hip: one window of the index under construction -- n records of the device-resident stream d_raw at d_off, cut at the
// device-resident stream offsets d_cut (n_blocks + 1), block b at file offset coff_base + d_coff[b]; synchronises.  bai_release:
// the index's device buffers (mth_ctx_destroy)
int bai_window(mth_ctx *ctx, const uint8_t *d_raw, const unsigned long long *d_off, uint32_t n, const unsigned long long *d_cut,
               const unsigned long long *d_coff, unsigned long long coff_base, uint32_t n_blocks);
void bai_release(mth_ctx *ctx);
// mth_mhl_regions.hip: the per-interval MHL state's buffers (mth_ctx_destroy); its sums cleared, the intervals kept (mth_reset)
void mhl_regions_release(mth_ctx *ctx);
int mhl_regions_clear(mth_ctx *ctx);
// mth_pdr_regions.hip: the same two for the per-interval PDR state
void pdr_regions_release(mth_ctx *ctx);
int pdr_regions_clear(mth_ctx *ctx);
// mth_quartet_regions.hip: ... and for the per-interval ME / PM state
void quartet_regions_release(mth_ctx *ctx);
int quartet_regions_clear(mth_ctx *ctx);
struct DecArgs;
// mth_decode_genome.hip: the two passes of the decode with the calls derived from the genome (k_decode_genome); `a` as decode_core
// fills it for k_decode<false>.  count: ncpg / tid / start / end / mapq / fwd; fill: cpg_pos / cpg_rel at a.cpg_off
int decode_genome_count(mth_ctx *ctx, const DecArgs &a);
int decode_genome_fill(mth_ctx *ctx, const DecArgs &a);
// mth_decode_mm.hip: a pass of the decode with the calls taken from MM:Z / ML:B:C (k_decode_mm), and the staged form's first half:
// X(record, T) of every record into ctx->tag_xm (offsets tag_coloff, lengths tag_xmlen), named in a.xm_base / xm_off / xm_lens
int decode_mm_pass(mth_ctx *ctx, const DecArgs &a, bool fill);
int decode_mm_stage(mth_ctx *ctx, DecArgs &a);
// implemented in mth_sites.hip: PDR with exact flush / re-open semantics (spans > 150 bp)
int launch_pdr_exact(mth_ctx *ctx, const mth_batch_t &dev_batch, const mth_pdr_lpmd_params_t &p);
// site discovery (tile pipeline into the private sink): positions called by >= 1 read with
// mapq >= min_qual and n_cpgs >= max(min_cpgs,1); bound = host-known upper bound of the site count
int discover_sites(mth_ctx *ctx, const mth_batch_t &dev_batch, uint32_t min_cpgs, uint8_t min_qual, uint64_t &bound,
                   uint32_t min_cov = 0);

// implemented in mth_pdr_lpmd.hip.  sink == nullptr: rows go to the ctx's PDR result columns.
struct TileSink {
    DevState *st;          // counters (n_sites / cur_base / n_batches / lpmd) of this sink
    int32_t *pos;
    float *pdr;
    uint32_t *nc, *nd;
    uint32_t *batch_cnt;
};
int build_read_index(mth_ctx *ctx, const mth_batch_t &dev_batch, int tile_w, int32_t &idx_base, uint32_t &ntiles);
// the fine index of a batch into a caller-owned buffer; errors (unsorted) and safe_hi land in *st (mth_batch_prepare)
int build_fine_index(mth_ctx *ctx, const mth_batch_t &dev_batch, int32_t idx_base, uint32_t nq, uint32_t *idx, DevState *st);
// the index the kernels of the call in progress look reads up in (after build_read_index / launch_pdr_lpmd)
inline const uint32_t *idx_ptr(const mth_ctx *ctx) { return ctx->cur_idx ? ctx->cur_idx : ctx->idx.as<uint32_t>(); }
// extent of the fine index of a batch: origin and entries, for any tile width up to 65536
inline void fine_index_extent(const mth_batch_t &b, int32_t &idx_base, uint32_t &nq) {
    const IndexGeom g = index_geometry(batch_shape(b), 65536u);
    idx_base = g.idx_base; nq = g.nq;
}
// MHL as one tile pass (mth_mhl_tile.hip): candidate-site arrays filled with finished rows and the sites left to the exact walk
int launch_mhl_tile(mth_ctx *ctx, const mth_batch_t &dev_batch, const mth_mhl_params_t &p, const MhlKnobs &kn, uint64_t &bound);
// FDRP + qFDRP at WGBS depth as one tile pass (mth_fdrp_wtile.hip): candidate-site arrays filled with finished rows and the sites left
// to k_fdrp_walk (listed in redo_list / *redo_cnt)
int launch_fdrp_wtile(mth_ctx *ctx, const mth_batch_t &dev_batch, const mth_fdrp_params_t &p, const uint16_t *pair_tab, uint32_t *redo_list, uint32_t *redo_cnt);
int launch_pdr_lpmd(mth_ctx *ctx, const mth_batch_t &dev_batch, const mth_pdr_lpmd_params_t &p,
                    const TileSink *sink = nullptr, bool pipelined = false);

// How a fetch opens: the rows of a table live in [0, rows) with gaps (the unused tails of the tile kernels' chunks).  Per batch,
// row(meta, device row, from the global path) sees its tiles' rows in tile order -- sorted, each tile sorts in LDS -- and then the
// rows [heavy0, batch end) of the global path, in table order; batch_end(batch number) follows.
template <class Row, class End>
int tile_rows_walk(mth_ctx *ctx, const TileRowTable &t, Row &&row, End &&batch_end) {
    const uint64_t n_tiles = t.tiles();
    std::vector<unsigned long long> trow0(n_tiles);
    std::vector<uint32_t> trows(n_tiles);
    if (n_tiles) {
        MTH_HIP(ctx, hipMemcpy(trow0.data(), t.tile_row0.p, n_tiles * 8, hipMemcpyDeviceToHost));
        MTH_HIP(ctx, hipMemcpy(trows.data(), t.tile_rows.p, n_tiles * 4, hipMemcpyDeviceToHost));
    }
    uint64_t rows_end = 0, tile = 0;
    for (size_t b = 0; b < t.meta.size(); ++b) {
        const TileBatch &mb = t.meta[b];
        rows_end += mb.rows;
        for (; tile < mb.tile_end; ++tile)
            for (uint32_t j = 0; j < trows[tile]; ++j) row(mb, (uint64_t)trow0[tile] + j, false);
        for (uint64_t i = mb.heavy0; i < rows_end; ++i) row(mb, i, true);
        batch_end(b);
    }
    return MTH_OK;
}

}  // namespace mth
