/*
 * metheor_hip.h -- C ABI of the MI355X (gfx950) methylation-heterogeneity engine.
 *
 * This is the drop-in boundary for the per-read CpG-pattern hot path of dohlee/metheor
 * (v0.1.9).  The reference has no FFI of its own: the seam is cut inside each measure's
 * `compute_helper()` AFTER `BismarkRead::new` (host: BAM iteration + XM decode) and BEFORE the
 * hash-map accumulation.  A host (Rust via `extern "C"`, C++, ctypes) decodes records into the
 * flat SoA batch below and calls one `mth_*_accumulate` per batch; the per-measure result
 * getters return exactly what the corresponding `compute_helper()` returns.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every entry point returns an
 * `int` status (MTH_OK == 0, negative on error, never throws); one `mth_ctx_t` per GPU; a ctx
 * is not thread-safe; work is enqueued on the ctx's HIP stream and the getters synchronise.
 * There is NO CPU fallback: without a gfx950 device `mth_ctx_create` fails.
 *
 * Reference interfaces replaced (paths under the reference repo):
 *   src/pdr.rs:119-125    pdr::compute_helper(input,min_depth,min_cpgs,min_qual,cpg_set)
 *                         -> BTreeMap<CpGPosition,(f32,u32,u32)>      => mth_pdr_lpmd_accumulate + mth_pdr_fetch
 *   src/lpmd.rs:154-160   lpmd::compute_helper(input,min_distance,max_distance,min_qual,cpg_set)
 *                         -> LPMDResult                               => mth_pdr_lpmd_accumulate + mth_lpmd_global (+ mth_lpmd_pairs_accumulate/_fetch)
 *   src/mhl.rs:135-141    mhl::compute_helper(...) -> BTreeMap<CpGPosition,f32>        => mth_mhl_accumulate + mth_mhl_fetch (built)
 *   src/me.rs:90-94       me::compute_helper(input,min_qual,cpg_set) -> HashMap<Quartet,QuartetStat>
 *   src/pm.rs:85-89       pm::compute_helper(...)                                      => mth_quartet_accumulate + mth_quartet_fetch (built)
 *   src/fdrp.rs:176-183   fdrp::compute_helper(input,min_qual,min_depth,max_depth,min_overlap,cpg_set)
 *   src/qfdrp.rs:188-195  qfdrp::compute_helper(...) -> BTreeMap<CpGPosition,f32>      => mth_fdrp_accumulate + mth_fdrp_fetch (built)
 *   src/readutil.rs:15-21 BismarkRead {start_pos,end_pos,cpgs:Vec<CpG{relpos,abspos,methylated}>}
 *                                                                                      => mth_batch_t (SoA)
 */
#ifndef METHEOR_HIP_H
#define METHEOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTH_ABI_VERSION 1

typedef struct mth_ctx mth_ctx_t;

enum {
    MTH_OK = 0,
    MTH_ERR_INVALID = -1,   /* bad argument */
    MTH_ERR_HIP = -2,       /* a HIP runtime call failed (mth_last_error has the text) */
    MTH_ERR_NO_DEVICE = -3, /* no gfx950 device: there is no CPU fallback */
    MTH_ERR_UNSORTED = -4,  /* reads of a batch are not sorted by start */
    MTH_ERR_SPAN = -5,      /* a read spans more than batch.max_span */
    MTH_ERR_REOPEN = -6,    /* reserved (was: flush re-open semantics not implemented; they are now) */
    MTH_ERR_RANGE = -7,     /* a CpG of an owned site lies outside what the batch declared: a batch carries the word of position -1 */
    MTH_ERR_CAPACITY = -8,  /* an on-chip capacity was exceeded */
    MTH_ERR_STATE = -9,     /* call order violated */
    MTH_ERR_FORMAT = -10,   /* device decode: corrupt BGZF block, malformed BAM record, or a record without XM:Z */
    MTH_ERR_UNALIGNED = -11,/* mth_bgzf_decode: a record straddles two BGZF blocks (mth_bgzf_decode_straddle takes such a file; it returns this when
                               its rounds do not settle or the carry is too large: decode via the host walk instead) */
    MTH_ERR_RCCL = -12      /* librccl could not be loaded, or an RCCL call failed (mth_last_error has the text) */
};
/* Several data errors pending at one synchronising call: one is reported, in the order UNSORTED, RANGE, SPAN, CAPACITY, FORMAT, UNALIGNED.
 * RANGE comes before SPAN: the word of position -1 in a batch also reads as a call 2^31 positions past its read to some tile kernels.  A
 * file-order run over a stream that holds both a contig-less record with calls and a span violation therefore reports RANGE. */

enum { MTH_MEM_HOST = 0, MTH_MEM_DEVICE = 1, MTH_MEM_PREPARED = 2 /* only in batches made by mth_batch_prepare */ };

/*
 * One batch = the reads of ONE contig that can touch the genomic region [region_beg, region_end),
 * sorted by `read_start` (coordinate-sorted BAM order).  Sites inside the region and reads whose
 * start lies inside it are OWNED by the batch; reads starting outside are halo (they contribute
 * to owned sites only).  A whole contig is region [0, contig_length).
 *
 * Per read  (readutil.rs:15-21; pdr.rs:150 mapq):
 *   read_start/read_end  first / last reference position covered (readutil.rs:25-33), -1 if none
 *   read_mapq            Record::mapq()
 *   read_fwd             1 iff flags in {0,99,147} (readutil.rs:332) -- informational; cpg_pos
 *                        already has the strand rule applied
 *   cpg_off[n_reads+1]   CSR offsets into the per-call arrays
 * Per CpG call (readutil.rs:247-251), in query order:
 *   cpg_pos              abspos (31 bits) | methylated << 31
 *                        Position -1 -- a record at position 0 whose flag is outside {0,99,147} calling on its first aligned base reports
 *                        abspos - 1 (readutil.rs:338), and the reference keeps -1 as an ordinary i32 key, first of its contig -- has no
 *                        word of its own in 31 bits.  The decoders write it as 0x7fffffff (no contig has a position 2^31 - 1).  A BATCH
 *                        must not carry that word: such a contig goes in as a contig group (below), shifted by a voff >= 1, where the
 *                        call lies at voff - 1 and every fetch returns it as position -1, first row of its contig.  mth_decoded_group /
 *                        _each do that for a decoded stream.  A batch that does carry the word is refused with MTH_ERR_RANGE (found by
 *                        the read index build -- by a small launch of its own in the run form MTH_TILE_RUNS=1, which builds no index --, on a
 *                        read that starts at 0, as its first call; a host batch before anything is copied).  mth_fileorder_run takes the word as it
 *                        is and orders it before position 0.
 *   cpg_rel              relpos = query offset of the call (u8; use cpg_rel16 when reads > 255 bp)
 */
typedef struct {
    int32_t  tid;
    int32_t  region_beg, region_end;
    int32_t  max_span;   /* >= max(read_end - read_start + 1) over the batch */
    uint32_t n_reads;
    uint32_t n_cpgs;
    int32_t  mem;        /* MTH_MEM_HOST or MTH_MEM_DEVICE: where ALL the arrays below live */
    const int32_t  *read_start;
    const int32_t  *read_end;
    const uint8_t  *read_mapq;
    const uint8_t  *read_fwd;
    const uint32_t *cpg_off;
    const uint32_t *cpg_pos;
    const uint8_t  *cpg_rel;    /* exactly one of cpg_rel / cpg_rel16 is non-NULL */
    const uint16_t *cpg_rel16;
} mth_batch_t;

/* pdr.rs:82-89 + lpmd.rs:125-133 arguments (clap defaults: lib.rs:36-46, 206-214) */
typedef struct {
    uint32_t pdr_min_depth;  /* -d 10 */
    uint32_t pdr_min_cpgs;   /* -p 4  */
    uint8_t  pdr_min_qual;   /* -q 10 */
    uint8_t  lpmd_min_qual;  /* -q 10 */
    uint8_t  want_pdr, want_lpmd;
    int32_t  lpmd_min_distance; /* -m 2  */
    int32_t  lpmd_max_distance; /* -M 16 */
} mth_pdr_lpmd_params_t;

/* ---- prepared batches: one read index per batch, shared by the measures ----------------------------------
 * Every measure's entry point builds the linear read index of its batch ("first read starting at or after q x 32 bp", plus the
 * sortedness check) before its kernels can find a tile's or a site's candidate reads -- once per call: PDR + LPMD, ME / PM, MHL,
 * FDRP / qFDRP and the pairs table over the same batch build it five times (each replaces one pass of the reference's
 * compute_helper over the file: pdr.rs:119, me.rs:90, mhl.rs:135, fdrp.rs:176, lpmd.rs:154).  mth_batch_prepare makes the batch
 * device-resident ONCE (a host batch is copied into buffers the prepared batch owns; a device batch is borrowed) and builds the index
 * ONCE; `*prepared` is then a batch (mem = MTH_MEM_PREPARED, its arrays are the device arrays, read_fwd carries the handle) that
 * every mth_*_accumulate entry point takes in place of the original and gives the same rows for.  Contract: the arrays of the batch
 * given to mth_batch_prepare (device batches) stay untouched until mth_batch_release; release only after a synchronising call has
 * returned for every measure that used it.  An unsorted batch is reported by the first synchronising call after a measure used it. */
int  mth_batch_prepare(mth_ctx_t *ctx, const mth_batch_t *batch, mth_batch_t *prepared);
int  mth_batch_release(mth_ctx_t *ctx, mth_batch_t *prepared);

/* ---- context ------------------------------------------------------------------------- */
int  mth_abi_version(void);
int  mth_ctx_create(int device_id, mth_ctx_t **out);
void mth_ctx_destroy(mth_ctx_t *ctx);
/* enqueue on a caller-owned hipStream_t (e.g. torch's current stream); NULL = ctx's own stream */
int  mth_ctx_set_stream(mth_ctx_t *ctx, void *hip_stream);
int  mth_ctx_sync(mth_ctx_t *ctx);
const char *mth_strerror(int status);
const char *mth_last_error(const mth_ctx_t *ctx);
/* Non-fatal findings of the device-side record decode so far (sticky; as of the latest synchronising call).
 * MTH_NOTE_CIGAR_PAD: a record's CIGAR holds a P (padding) operation.  readutil.rs:28,326 take the read's positions from
 * rust-htslib's reference_positions_full(), whose aligned-pairs iterator is believed to panic on Cigar::Pad (the crate is not part
 * of the reference tree and cannot be checked here); this engine treats P as "no query base, no reference base". */
#define MTH_NOTE_CIGAR_PAD 1u
/* MTH_NOTE_MODTAG_SKIPPED: under mth_decode_set_modtags, a record contributed no call because its MM / ML cannot be placed on
 * SEQ: no SEQ, a hard clip in the CIGAR, or an MN field that differs from l_seq. */
#define MTH_NOTE_MODTAG_SKIPPED 2u
uint32_t mth_notes(const mth_ctx_t *ctx);
/* forget all accumulated results (a new input file) */
int  mth_reset(mth_ctx_t *ctx);

/* ---- PDR + LPMD, fused single pass (pdr.rs:119-212, lpmd.rs:154-202) --------------------
 * Asynchronous: kernels are enqueued on the ctx stream; data errors (UNSORTED/SPAN/REOPEN/
 * RANGE) are detected on the device and reported by the next synchronising call below.
 * Pipelining (round 4): from the second of a run of consecutive calls with device-resident batches on (mth_reset does not break a
 * run), the engine runs the batches on two internal streams, ordered behind the work already enqueued on the ctx stream at the time
 * of the call; the ctx stream is ordered behind them again by every other entry point of this header (getters, mth_ctx_sync, the
 * other measures, mth_ctx_set_stream, mth_ctx_destroy).  Consequence for a caller that enqueues its OWN work on the stream it gave
 * to mth_ctx_set_stream: the arrays of a device-resident batch must not be overwritten or freed in stream order right behind the
 * call -- only after the next entry point that joins (as they always had to outlive the asynchronous kernels).  MTH_PIPELINE=0 in
 * the environment keeps everything on the ctx stream. */
int  mth_pdr_lpmd_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch,
                             const mth_pdr_lpmd_params_t *params);
/* number of emitted sites so far (synchronises) */
int  mth_pdr_count(mth_ctx_t *ctx, uint64_t *n_sites);
/* copy out the BTreeMap<CpGPosition,(f32,u32,u32)> rows, sorted by (tid,pos) given batches were
 * submitted in that order; any pointer may be NULL; buffers hold >= mth_pdr_count entries */
int  mth_pdr_fetch(mth_ctx_t *ctx, int32_t *tid, int32_t *pos, float *pdr,
                   uint32_t *n_concordant, uint32_t *n_discordant);
/* page-locked host memory for the *_fetch destinations: device-to-host copies into it run at the link's rate (pageable
 * destinations work too, through the runtime's bounce buffers -- ~4x slower on a 700 k-row table).  Freed by
 * mth_result_buffer_free or with the context's process. */
int  mth_result_buffer_alloc(mth_ctx_t *ctx, size_t bytes, void **out);
int  mth_result_buffer_free(mth_ctx_t *ctx, void *p);
/* device pointers of the same columns (valid until the next accumulate/reset) */
int  mth_pdr_device_view(mth_ctx_t *ctx, uint64_t *n_sites, const int32_t **pos,
                         const float **pdr, const uint32_t **n_concordant,
                         const uint32_t **n_discordant);
/* LPMDResult: out[4] = {n_concordant, n_discordant, n_read, n_valid_read} (exact, int64);
 * *lpmd = compute_lpmd() with the reference's wrapping i32 counters (lpmd.rs:11-12,51-55) */
int  mth_lpmd_global(mth_ctx_t *ctx, int64_t out[4], float *lpmd);
/* lpmd.rs:176-179: records that never enter a batch (no contig, no aligned base) still count in n_read, and in n_valid_read when
 * their mapq passes; the caller that left them out of its batches adds their counts here (queued on the context's stream).
 * lpmd.rs:181 builds a BismarkRead for every record whose mapq passes, placed or not: a passing record without XM:Z is the
 * reference's panic -- both decoders refuse such a record before it can be counted here (mth_decode_set_xm_min_mapq) */
int  mth_lpmd_add_unbatched(mth_ctx_t *ctx, uint64_t n_read, uint64_t n_valid_read);
/* multi-GPU: enqueue (on the ctx stream) a copy of the 4 exact int64 counters into a DEVICE buffer
 * the caller owns, ready for an RCCL all-reduce(sum) over ranks; no host synchronisation */
int  mth_lpmd_export_device(mth_ctx_t *ctx, int64_t *dst_device4);
/* compute_lpmd() (lpmd.rs:51-55, wrapping-i32 semantics) from summed integer counters, e.g. the
 * all-reduced ones */
float mth_lpmd_from_counts(int64_t n_concordant, int64_t n_discordant);

/* ---- multi-GPU: the path's one exchange step ------------------------------------------------
 * A sharded run gives every GPU a genomic region; per-site / per-quartet / per-pair rows are owned by region and
 * never exchanged.  Only LPMDResult's four counters (lpmd.rs:11-12: n_concordant, n_discordant, n_read,
 * n_valid_read, accumulated per read at lpmd.rs:176-200 and divided at lpmd.rs:51-55) are genome-wide: they are
 * summed with ONE RCCL all-reduce (ncclInt64 x 4, ncclSum) over xGMI, ordered after the work already enqueued on each
 * context's stream; afterwards mth_lpmd_global() of EVERY context returns the node-wide LPMDResult.  Call it once,
 * after the last mth_pdr_lpmd_accumulate (a second call without new batches is MTH_ERR_STATE: it would add the
 * totals again).  librccl.so.1 is loaded on first use; a single-GPU run never touches it. */
int  mth_device_count(int *n_devices);
/* one process, one context per GPU: collective over ctxs[0..n) called from ONE host thread.  Contexts that share a
 * device are summed on that device and RCCL runs between the distinct devices. */
int  mth_allreduce_lpmd(mth_ctx_t **ctxs, int n);
/* one process per GPU: rank 0 makes the id, the host ships its 128 bytes to every rank (MPI_Bcast,
 * torch.distributed.broadcast, a file), every rank joins, every rank calls the reduce. */
#define MTH_RCCL_ID_BYTES 128
int  mth_rccl_unique_id(void *id128);
int  mth_rccl_init_rank(mth_ctx_t *ctx, const void *id128, int rank, int world);
/* asynchronous: the counters are snapshotted on the context's stream and reduced on a side stream (the context's
 * stream does not wait for the collective; mth_lpmd_global does) */
int  mth_allreduce_lpmd_rank(mth_ctx_t *ctx);

/* ---- LPMD per-pair table (`lpmd --pairs`; lpmd.rs:70-122) -------------------------------------
 * Separate pass over the same batches (the global counters above do not need it). */
typedef struct {
    int32_t min_distance;  /* -m 2  */
    int32_t max_distance;  /* -M 16 */
    uint8_t min_qual;      /* -q 10 */
} mth_lpmd_pairs_params_t;
int  mth_lpmd_pairs_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_lpmd_pairs_params_t *params);
/* rows of print_pair_statistics, sorted by ((tid,cpg1),(tid,cpg2)); lpmd = n_d as f32/(n_c as f32+n_d as f32)
 * (lpmd.rs:111); *n_rows always set, arrays may be NULL */
int  mth_lpmd_pairs_fetch(mth_ctx_t *ctx, uint64_t *n_rows, int32_t *tid, int32_t *pos1, int32_t *pos2, float *lpmd,
                          uint32_t *n_concordant, uint32_t *n_discordant);
/* ---- LPMD per interval (`lpmd --intervals`; lpmd.rs:70-87, readutil.rs:87-94) ------------------------
 * The pairs table accumulated so far, reduced on the device by interval: for each of the n intervals [beg[i], end[i]) on contig
 * tid[i] (host arrays; 0-based, half-open, 0 <= beg <= end; any order, overlap, nesting and duplicates), the exact sums of
 * n_concordant and n_discordant (add_pair_concordance, lpmd.rs:70-87) over the rows with that contig, beg <= cpg1 and cpg2 < end.
 * That is what `lpmd -c` counts for the set "every position of the interval": BismarkRead::filter_isin (readutil.rs:87-94) keeps
 * the calls inside, and a pair of kept calls is a pair of the table.  mth_lpmd_from_counts of the two sums is the interval's LPMD.
 * A call at position -1 lies in no interval; a contig without batches gives zeros.  Rows of contig groups are compared in the
 * group's coordinates (the interval is shifted by its contig's voff).  Queued on the context's stream, one synchronisation at the
 * end; the table is not changed: a second call gives the same sums and mth_lpmd_pairs_fetch is unaffected.  With several contexts
 * (a pair is owned by the context whose region holds cpg1) the caller adds the contexts' sums. */
int  mth_lpmd_intervals_fetch(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end,
                              int64_t *n_concordant, int64_t *n_discordant);

/* ---- contig groups: many contigs in one batch -------------------------------------------------------------------------------------
 * A batch is a coordinate interval of ONE contig (mth_batch_t.tid).  A job over many contigs -- 24 for a human genome, thousands with
 * alt / decoy contigs -- pays every pass's fixed costs (index build, kernel boundaries, a half-filled last wave of workgroups) once
 * per contig.  A GROUP lays several contigs out in one virtual coordinate space: contig k's positions are shifted by voff[k], the gaps
 * between contigs are wider than anything a measure looks across (a read's span, PDR's 150-bp flush margin, FDRP's 201-bp window), and
 * the group is accumulated as ONE batch whose `tid` is the group's handle (<= -2).  No measure looks at a tid: the reference's
 * per-contig behaviour -- a record on a later contig flushes every earlier site (is_before(), readutil.rs:304-310) -- is what a larger
 * virtual position does too.  Every fetch maps a grouped batch's rows back: (handle, virtual position) -> (tids[k], position - voff[k])
 * with k the last contig whose voff is <= the (first) position of the row + 1 (a contig's call at position -1 lies at voff - 1 and comes
 * back as -1); row order stays the (tid, pos) order when tids ascend.
 * The reservoir draw of FDRP / qFDRP (keyed by tid and position) is made on the mapped-back site.
 * voff: ascending, voff[0] >= 0, voff[k + 1] >= voff[k] + contig k's extent + max_span + 152 + 202 (checked only for order), all
 * virtual positions below 2^31 - 1.  mth_group_clear forgets all groups (results fetched afterwards would keep their handles).
 * mth_pdr_device_view hands out the virtual positions unmapped. */
int  mth_group_define(mth_ctx_t *ctx, uint32_t n_contigs, const int32_t *tids, const int64_t *voff, int32_t *handle);
int  mth_group_clear(mth_ctx_t *ctx);

/* ---- ME / PM: per-quartet 16-bin epiallele histograms (me.rs:90-132, pm.rs:85-128) ------------
 * One accumulate serves both measures (they share the histogram).  Windows whose consecutive CpGs are >= 2048 bp
 * apart (reference skips, long reads) are aggregated under a 128-bit key on a side path; the calls of a read must be in
 * ascending position order (MTH_ERR_SPAN otherwise).
 * Device-resident batches after a context's first are QUEUED: the call returns without a host sync, and the next call on the
 * context that is not another mth_quartet_accumulate of a device-resident batch (mth_ctx_sync, any fetch, any other accumulate,
 * decode or mth_decoded_batch) reads back whether every queued batch fitted the output it was given -- one that did not, or that
 * has tiles for the global-table path, is replayed there together with the batches behind it.  As for every device-resident
 * batch, the arrays must stay untouched until then.  MTH_QUARTET_QUEUE=0 restores one sync per batch.  mth_lpmd_pairs_accumulate
 * queues the same way (MTH_PAIRS_QUEUE=0). */
typedef struct {
    uint8_t min_qual;   /* -q 10 (lib.rs:66-68, 90-92) */
} mth_quartet_params_t;
int  mth_quartet_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_quartet_params_t *params);
/* HashMap<Quartet,QuartetStat> rows with read depth >= min_depth (the write-time filter of me.rs:82 /
 * pm.rs:77; pass 0 for compute_helper's full map).  *n_rows is always set; the arrays may be NULL
 * (count only) or hold >= *n_rows entries: pos4[n*4] = pos1..pos4, counts16[n*16] = pattern
 * histogram (pattern = 8*m1+4*m2+2*m3+m4), me = compute_me() (me.rs:42-55), pm = compute_pm()
 * (pm.rs:42-51).  Rows come sorted by (batch, pos1..pos4) -- deterministic; the reference's order is HashMap-random.  Like the other measures, batches must be coordinate-sorted (MTH_ERR_UNSORTED) and no CpG call
 * of a read may lie outside [start - 1, start - 1 + max_span] (MTH_ERR_SPAN). */
int  mth_quartet_fetch(mth_ctx_t *ctx, uint32_t min_depth, uint64_t *n_rows, int32_t *tid, int32_t *pos4,
                       uint32_t *counts16, float *me, float *pm);

/* ---- MHL: methylation haplotype load per site (mhl.rs:135-208, 43-73) -------------------------
 * Exact stream semantics of the reference, including its flush / re-open of sites:
 * flush on strict '<' by any read with >= 1 CpG, before the mapq / min_cpgs filters.  Reads with
 * more than 16384 CpGs covering a site are refused (MTH_ERR_CAPACITY); reads with 513..16384 take a walk whose
 * histograms live in 256 MB of HBM scratch.  MTH_ERR_SPAN (a call outside [start - 1, start - 1 + max_span]) is
 * raised for the reads the pass evaluates: every contributing read, and -- on batches of <= 1.8 calls a read, where
 * the flush rule is looked at per finished row -- the reads around a row; otherwise every read's first call. */
typedef struct {
    uint32_t min_depth;  /* -d 10 */
    uint32_t min_cpgs;   /* -p 4  */
    uint8_t  min_qual;   /* -q 10 */
} mth_mhl_params_t;
int  mth_mhl_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_mhl_params_t *params);
/* BTreeMap<CpGPosition,f32> rows sorted by (tid,pos); *n_rows always set, arrays may be NULL;
 * coverage = number of reads of the segment the value comes from */
int  mth_mhl_fetch(mth_ctx_t *ctx, uint64_t *n_rows, int32_t *tid, int32_t *pos, float *mhl, uint32_t *coverage);

/* ---- MHL per interval (`mhl-regions`; mhl.rs:43-73, 176-183, readutil.rs:87-94, 147-164) -------------------------------
 * MHL of a REGION: one value per interval [beg, end) of contig tid, from every read taken once.  Per record: BismarkRead
 * (readutil.rs:24-53); the calls with beg <= abspos < end are kept -- filter_isin (readutil.rs:87-94) with the set "every position
 * of the interval", a call at position -1 lies in no interval --; with n calls kept the read contributes if mapq >= min_qual and
 * n >= max(min_cpgs, 1) (mhl.rs:176-183, applied after the filter as the reference applies them); a contributing read adds n to the
 * interval's num_cpgs and its get_stretch_info() (readutil.rs:147-164) to the interval's stretch_info (mhl.rs:75-80, 36-41: one
 * AssociatedReads per interval instead of one per CpG); the value is compute_mhl() (mhl.rs:43-73) of it, NaN below
 * max(min_depth, 1) contributing reads.  No flush and no re-open: the value does not depend on the record order or on how the
 * reads are split over batches and contexts.
 * Two histograms per interval carry it: runs[r], maximal methylated runs of length r, and reads[n], contributing reads with n
 * kept calls.  The device counts them as integers; the finaliser derives stretch_info[l] = sum_{r >= l} runs[r] (r - l + 1) and the
 * denominator of l = sum_{n >= l} reads[n] (n - l + 1) as exact 64-bit integers, converts each to f32 ONCE and then follows
 * compute_mhl's arithmetic (terms in ascending l, running f32 l_sum, no contraction).  The reference adds its denominator in f32
 * read by read: the same bits whenever the interval's sum of n is below 2^24; beyond that the reference's value depends on the
 * record order and this definition takes over.
 *   begin       declares the n intervals (host arrays, copied; 0-based, half-open, 0 <= beg <= end; any order, overlap, nesting
 *               and duplicates; fewer than 2^31) and clears the sums.  mth_reset clears the sums and keeps the intervals.
 *   accumulate  one batch (host, device-resident or prepared; a contig or a contig group, whose intervals are shifted by their
 *               contig's voff).  Only the reads the batch OWNS count (region_beg <= read_start < region_end): with several
 *               batches or contexts over one contig every read is owned once.  min_depth is not used here.  Synchronous: data
 *               errors are the return value; a read with more than 16384 kept calls in an interval is MTH_ERR_CAPACITY, a batch
 *               that carries the word of position -1 MTH_ERR_RANGE.  The calls of a read lie between its first and its last one.
 *   counts      the histograms as sparse rows sorted by (interval, length): *n_rows always set, arrays may be NULL.  Several
 *               contexts (shards): add their rows and finalise once.
 *   finalise    host only, no context: the value of ONE interval from its k rows of ascending length; *n_reads = contributing
 *               reads, *max_cpgs = the largest n among them (0 when there are none); either may be NULL.
 *   fetch       finalise of every declared interval, in the caller's order; arrays of n, any may be NULL.
 *   stats       out[4] = overflow-list entries so far (lengths above the dense rows' 64), batches run a second time because
 *               the list was too short, batches, reads of those batches. */
int  mth_mhl_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end);
int  mth_mhl_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_mhl_params_t *params);
int  mth_mhl_regions_counts(mth_ctx_t *ctx, uint64_t *n_rows, uint32_t *interval, uint32_t *length, uint64_t *runs, uint64_t *reads);
float mth_mhl_regions_finalise(uint64_t k, const uint32_t *length, const uint64_t *runs, const uint64_t *reads, uint32_t min_depth,
                               uint64_t *n_reads, uint32_t *max_cpgs);
int  mth_mhl_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *mhl, uint64_t *n_reads, uint32_t *max_cpgs);
int  mth_mhl_regions_stats(mth_ctx_t *ctx, uint64_t out[4]);

/* ---- PDR per interval (`pdr-regions`; pdr.rs:47-49, 147-157, readutil.rs:87-94, 134-145) -------------------------------
 * The proportion of discordant reads of a REGION: one value per interval [beg, end) of contig tid, from every read taken once.
 * Per record: BismarkRead (readutil.rs:24-53); the calls with beg <= abspos < end are kept -- filter_isin (readutil.rs:87-94)
 * with the set "every position of the interval", a call at position -1 lies in no interval --; with n calls kept the read
 * contributes if mapq >= min_qual and n >= max(min_cpgs, 1) (pdr.rs:147-157, applied after the filter as the reference applies
 * them); a contributing read is methylated (every kept call is Z), unmethylated (none is) or discordant (anything else):
 * get_concordance_state() (readutil.rs:134-145) of the kept calls.  n_concordant = methylated + unmethylated; the value is
 * n_discordant as f32 / (n_concordant as f32 + n_discordant as f32) (pdr.rs:47-49), NaN below max(min_depth, 1) contributing
 * reads.  No flush: the counts do not depend on the record order or on how the reads are split over batches and contexts.
 * The counters are 64-bit integers, each converted to f32 once: the reference's bits whenever the counts fit its u32.
 *   begin       declares the n intervals (host arrays, copied; 0-based, half-open, 0 <= beg <= end; any order, overlap, nesting
 *               and duplicates; fewer than 2^31) and clears the sums.  mth_reset clears the sums and keeps the intervals.
 *   accumulate  one batch (host, device-resident or prepared; a contig or a contig group, whose intervals are shifted by their
 *               contig's voff).  Only the reads the batch OWNS count (region_beg <= read_start < region_end): with several
 *               batches or contexts over one contig every read is owned once.  params: min_cpgs and min_qual; min_depth is not
 *               used here.  NOT synchronous: the pass is queued on the context's stream and the call returns; a device-resident
 *               batch's arrays stay untouched until the next counts / fetch (or any call that waits for the stream).  Data
 *               errors -- a batch that carries the word of position -1: MTH_ERR_RANGE -- are the return value of that call.
 *   counts      per interval, in the caller's order: contributing reads that are methylated, unmethylated, discordant (pdr.rs:185-
 *               193's two counters, the concordant one split).  Dense arrays of n; any may be NULL.  Several contexts (shards):
 *               add their arrays and finalise once.
 *   finalise    host only, no context: pdr.rs:47-49 of ONE interval's counters, NaN when n_concordant + n_discordant is below
 *               max(min_depth, 1).
 *   fetch       finalise of every declared interval, in the caller's order; n_methylated: the methylated among the concordant
 *               reads.  Arrays of n, any may be NULL.  Another min_depth needs no new pass. */
int  mth_pdr_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end);
int  mth_pdr_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_mhl_params_t *params);
int  mth_pdr_regions_counts(mth_ctx_t *ctx, uint64_t *methylated, uint64_t *unmethylated, uint64_t *discordant);
float mth_pdr_regions_finalise(uint64_t n_concordant, uint64_t n_discordant, uint32_t min_depth);
int  mth_pdr_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *pdr, uint64_t *n_concordant, uint64_t *n_discordant, uint64_t *n_methylated);

/* ---- ME and PM per interval (`me-regions`, `pm-regions`; me.rs:42-55, 82, 115-125, pm.rs:42-51, readutil.rs:87-132) ----------------
 * The methylation entropy and the epipolymorphism of a REGION: one value each per interval [beg, end) of contig tid, from every read
 * taken once.  Per record: BismarkRead (readutil.rs:24-53); the calls with beg <= abspos < end are kept, in the read's call order --
 * filter_isin (readutil.rs:87-94) with the set "every position of the interval", a call at position -1 lies in no interval --; the
 * read contributes if mapq >= min_qual (me.rs:115) and at least 4 calls are kept (readutil.rs:101); a contributing read adds
 * get_cpg_quartets_and_patterns() (readutil.rs:97-132) of the kept calls, one pattern 8*m1 + 4*m2 + 2*m3 + m4 per window of four
 * consecutive kept calls (n - 3 patterns for n kept calls), all into ONE 16-bin histogram for the interval (me.rs:121-125 with
 * every quartet mapped to the same QuartetStat).  n_patterns = the sum of the bins (the pooled stat's get_read_depth()), n_reads =
 * the contributing reads.  ME = compute_me (me.rs:42-55), PM = compute_pm (pm.rs:42-51) of the histogram, each NaN when
 * n_patterns < max(min_depth, 1) (me.rs:82 applied to the pooled stat); the counts are reported either way.  No flush: the counts
 * do not depend on the record order or on how the reads are split over batches and contexts.  The counters are 64-bit integers;
 * each counter and the total are converted to f32 once: the reference's bits whenever they fit its u32.
 *   begin       declares the n intervals (host arrays, copied; 0-based, half-open, 0 <= beg <= end; any order, overlap, nesting
 *               and duplicates; fewer than 2^31) and clears the sums.  mth_reset clears the sums and keeps the intervals.
 *   accumulate  one batch (host, device-resident or prepared; a contig or a contig group, whose intervals are shifted by their
 *               contig's voff).  Only the reads the batch OWNS count (region_beg <= read_start < region_end).  The calls of a
 *               read may come in any order of position: the windows follow the call order (me.rs:120).  NOT synchronous: the pass
 *               is queued on the context's stream and the call returns; a device-resident batch's arrays stay untouched until the
 *               next counts / fetch (or any call that waits for the stream).  Data errors -- a batch that carries the word of
 *               position -1: MTH_ERR_RANGE -- are the return value of that call.
 *   counts      per interval, in the caller's order: bins[i * 16 + p] = windows of pattern p (me.rs:38-40), reads[i] = contributing
 *               reads.  Either may be NULL.  Several contexts (shards): add their arrays and finalise once.
 *   finalise    host only, no context: me.rs:42-55 and pm.rs:42-51 of ONE interval's sixteen bins, in the reference's operation
 *               order (bins ascending, me *= -0.25 last, pm -= p * p for every bin), NaN below max(min_depth, 1) patterns;
 *               *n_patterns = the sum of the bins.  Any output may be NULL.
 *   fetch       finalise of every declared interval, in the caller's order.  Arrays of n, any may be NULL.  Another min_depth
 *               needs no new pass. */
int  mth_quartet_regions_begin(mth_ctx_t *ctx, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end);
int  mth_quartet_regions_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_quartet_params_t *params);
int  mth_quartet_regions_counts(mth_ctx_t *ctx, uint64_t *bins, uint64_t *reads);
void mth_quartet_regions_finalise(const uint64_t *bins, uint32_t min_depth, float *me, float *pm, uint64_t *n_patterns);
int  mth_quartet_regions_fetch(mth_ctx_t *ctx, uint32_t min_depth, float *me, float *pm, uint64_t *n_patterns, uint64_t *n_reads);

/* ---- FDRP and qFDRP (fdrp.rs:176-246, qfdrp.rs:188-258): both from one pass ---------------------
 * Exact stream semantics (strict '<' flush by reads passing mapq with >= 1 CpG, +-201-bp window
 * drop, fill to max_depth in file order).  Beyond max_depth the reference replaces stored reads at
 * random from an OS-seeded RNG (fdrp.rs:90) -- not reproducible; here the draw is the counter-based
 * hash of (seed, tid, pos, n-th read) shared with the test oracle.  max_depth up to 16384: sites that hold more than 64 reads at
 * once are redone by a second pass with 256 slots in LDS, those beyond 256 by a third with max_depth rows per wave in HBM
 * scratch; max_depth above 16384 is refused with MTH_ERR_CAPACITY (never a truncated result).
 * The reference's own panic on this path (fdrp.rs:70-72, window index -1: a reverse-strand read of 203..403 reference bases that
 * passes min_qual, calls a CpG at its start - 1 and another one at start + 201) is reproduced as MTH_ERR_FORMAT at the next
 * synchronising call, on sorted and unsorted input alike (k_fdrp_guard; batches whose max_span is below 203 skip the pass). */
typedef struct {
    uint64_t min_depth;    /* -d 10 */
    uint64_t seed;         /* reservoir draws; any value */
    uint32_t max_depth;    /* -D 40 */
    int32_t  min_overlap;  /* -l 35 */
    uint8_t  min_qual;     /* -q 10 */
} mth_fdrp_params_t;
int  mth_fdrp_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_fdrp_params_t *params);
/* BTreeMap<CpGPosition,f32> rows of BOTH measures, sorted by (tid,pos); n_reads = num_sampled_read of
 * the segment the values come from; *n_rows always set, arrays may be NULL */
int  mth_fdrp_fetch(mth_ctx_t *ctx, uint64_t *n_rows, int32_t *tid, int32_t *pos, float *fdrp, float *qfdrp,
                    uint32_t *n_reads);

/* ---- several measures over one batch (`metheor all`) ------------------------------------------------------------------------------
 * One call accumulates ONE batch (plain, device-resident or prepared) into the result store of every measure `want` names; the
 * getters above return the results, bit-identical to calling the single entry points on the same batch (rows, row order where it is
 * defined, the LPMD counters).  A batch that is not prepared is prepared inside the call and released before it returns, so the read
 * index is built once for all the measures.  Synchronous: the call returns after a synchronising step, and data errors of the batch
 * (MTH_ERR_UNSORTED, MTH_ERR_SPAN, ...) are its return value.
 * pdr_lpmd.want_pdr / want_lpmd are ignored: taken from `want`.  `form`: with ME / PM and PDR and / or LPMD requested, MTH_MULTI_AUTO
 * runs them as ONE fused tile pass where the PDR + LPMD pass would take its wide (sparse-batch) form and as the two existing passes on
 * dense batches; MTH_MULTI_FUSED takes the fused pass on every batch; MTH_MULTI_SPLIT always the existing passes.  A fused tile the
 * pass cannot hold (more distinct quartets than its table, > 65 535 candidate reads, CpGs >= 2048 bp apart) is handed back: the batch's
 * ME / PM side is redone by mth_quartet_accumulate.  MHL, FDRP / qFDRP and the pairs table always run their own passes.
 * mth_multi_stats: out[0] batches run in the fused form, out[1] batches run in the split form, out[2] tiles of the fused pass,
 * out[3] of those handed back (their batch's ME / PM side redone) -- since the context's creation or its last mth_reset.
 * The test knob MTH_MULTI_FORCE_HANDBACK (environment) hands back every fused tile. */
#define MTH_MULTI_PDR     1u
#define MTH_MULTI_LPMD    2u
#define MTH_MULTI_QUARTET 4u    /* ME and PM: one histogram */
#define MTH_MULTI_MHL     8u
#define MTH_MULTI_FDRP    16u   /* FDRP and qFDRP: one pass */
#define MTH_MULTI_PAIRS   32u   /* the LPMD per-pair table */
enum { MTH_MULTI_AUTO = 0, MTH_MULTI_FUSED = 1, MTH_MULTI_SPLIT = 2 };
typedef struct {
    uint32_t want;                     /* MTH_MULTI_* bits, at least one */
    mth_pdr_lpmd_params_t   pdr_lpmd;
    mth_quartet_params_t    quartet;
    mth_mhl_params_t        mhl;
    mth_fdrp_params_t       fdrp;
    mth_lpmd_pairs_params_t pairs;
    int32_t form;                      /* MTH_MULTI_AUTO / _FUSED / _SPLIT */
} mth_multi_params_t;
int  mth_multi_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_multi_params_t *params);
int  mth_multi_stats(mth_ctx_t *ctx, uint64_t out[4]);

/* ---- BAM record + XM decode on the device (the step before the hot path) ----------
 * Replaces, per record, BismarkRead::new (readutil.rs:24-53: start/end = first/last aligned reference
 * position) and get_cpgs (readutil.rs:323-345: XM z/Z at aligned query offsets, abspos for flags in
 * {0,99,147} else abspos-1; insertions / soft clips skipped), i.e. what bamutil.rs:4-11's record
 * iterator feeds every measure.  Input is the INFLATED BAM record stream (BGZF-decompressed bytes after
 * the header) and the byte offset of each record (rec_off[i] points at record i's block_size field,
 * rec_off[n_rec] = end of the last record); the walk over block_size fields stays on the host.  `mem`
 * says where raw and rec_off live; append != 0 adds the records after those of the previous calls (a file
 * streamed window by window), append == 0 starts over.  The decoded SoA stays in HBM, owned by the context:
 * the arrays of mth_batch_t for ALL records so far, in file order (64-bit offsets, 16-bit relpos).  A record without XM:Z or a malformed record -> MTH_ERR_FORMAT (the reference panics,
 * readutil.rs:46).  The --cpg-set filter (filter_isin, readutil.rs:87-95) is applied when set, see below. */
typedef struct {
    uint64_t n_reads, n_cpgs;
    const int32_t  *tid, *start, *end;   /* device pointers */
    const uint8_t  *mapq, *fwd;
    const uint64_t *cpg_off;             /* n_reads + 1 */
    const uint32_t *cpg_pos;             /* abspos | methylated << 31 */
    const uint16_t *cpg_rel;
} mth_decoded_t;
int  mth_decode_records(mth_ctx_t *ctx, const void *raw, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec,
                        int mem, int append, mth_decoded_t *out);
/* --cpg-set (get_target_cpgs / filter_isin, readutil.rs:347-374, 87-95): keep only the calls whose (tid, pos) is in the set;
 * relpos of the kept calls is unchanged.  keys_sorted = strictly ascending (uint64)tid << 32 | pos, host memory.
 * enabled != 0 with n_keys == 0 is the empty set (every call dropped, as HashSet::contains on an empty set);
 * enabled == 0 removes the filter.  Applies to the following mth_decode_records / mth_bgzf_decode calls. */
int  mth_decode_set_cpg_filter(mth_ctx_t *ctx, const uint64_t *keys_sorted, uint64_t n_keys, int enabled);
/* lpmd applies its mapq filter BEFORE BismarkRead::new (lpmd.rs:176-181): a record without XM:Z that the filter skips never
 * panics there.  Records without XM:Z whose mapq is below min_mapq are decoded with zero calls instead of raising
 * MTH_ERR_FORMAT (default 0: every such record is an error, as in the other six measures).  Applies to the following
 * mth_decode_records / mth_bgzf_decode calls. */
int  mth_decode_set_xm_min_mapq(mth_ctx_t *ctx, uint32_t min_mapq);
/* the inflate step alone: inflated bytes of the given blocks, concatenated, copied to dst_host (may be NULL); *n_out = size.
 * The 4 bytes after each payload (the gzip trailer's CRC32) must lie inside the file bytes given: they are verified. */
int  mth_bgzf_inflate(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                      const uint32_t *isize, uint64_t n_blocks, void *dst_host, uint64_t *n_out);
/* The mirror image, the compression step alone: src[0, n_bytes) (mem says where it lives) cut at cut_off (HOST memory, n_blocks + 1
 * ascending offsets from 0 to n_bytes, at most 0xff00 bytes apart) becomes n_blocks BGZF blocks, each deflated on its own by
 * k_deflate (RFC 1951 dynamic Huffman, or fixed or stored where that is smaller: a payload is never above its input + 5 bytes)
 * and framed with the BC subfield, CRC32 and ISIZE.  The output is a function of the bytes and the cuts alone.  *out_bytes =
 * the blocks back to back, *out_n bytes, block b at (*out_block_off)[b] (n_blocks + 1 entries; may be NULL): host memory owned
 * by the context, valid until its next deflate or tag call.  n_blocks == 0 returns nothing; the EOF block is the caller's. */
int  mth_bgzf_deflate(mth_ctx_t *ctx, const void *src, uint64_t n_bytes, int mem, const uint64_t *cut_off, uint64_t n_blocks,
                      const uint8_t **out_bytes, uint64_t *out_n, const uint64_t **out_block_off);
/* The whole step on the device: BGZF inflate (one wave per block, RFC 1951 stored / fixed / dynamic blocks, checked
 * against ISIZE), record boundaries (one thread per block; htslib-family writers never let a record straddle a BGZF
 * block, which is verified -- MTH_ERR_UNALIGNED otherwise, nothing is appended then), record + XM decode as above.
 * `file` = n_bytes of the BAM file in HOST memory covering the blocks; per block: coff = offset of its DEFLATE payload
 * inside `file`, csize = payload bytes, isize = inflated bytes (blocks with isize 0 omitted); first_byte = offset in
 * the inflated stream of these blocks where the records start (the header's uncompressed size for the first call,
 * 0 afterwards).  Replaces bamutil.rs:4-11 (htslib's reader) + readutil.rs:24-53, 323-345 for a coordinate-sorted
 * Bismark BAM.  Every inflated block is checked against its ISIZE and its CRC32 (as htslib does); a mismatch is
 * MTH_ERR_FORMAT. */
int  mth_bgzf_decode(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                     const uint32_t *isize, uint64_t n_blocks, uint64_t first_byte, int append, mth_decoded_t *out);
/* The same step for a BAM whose records STRADDLE BGZF blocks (htsjdk / Picard / GATK, sambamba, biobambam and most writers
 * that are not htslib cut blocks at a byte count): mth_bgzf_decode refuses such a file, this entry point decodes it.  The
 * record offsets come from speculation and exact verification: every block guesses its first record start (the first offset whose
 * 36 header bytes look like a record and whose block_size leads to another such offset or exactly to the end of the call's
 * stream -- one whose block_size leads PAST the stream is not taken, so the record a call ends inside is nobody's guess; the
 * block that holds first_byte starts there) and is walked from its guess; the result stands when block 0 enters at first_byte and every block enters where its
 * predecessor's walk left (a block whose entry lies at or past its own end passes it on).  A block that disagrees takes its
 * predecessor's exit and is walked again when every block before it is final, or when the predecessor itself agrees with ITS
 * predecessor -- one round per launch, at most MTH_STRADDLE_MAX_ROUNDS rounds (a record that covers k blocks costs about k),
 * MTH_ERR_UNALIGNED beyond (the caller takes the host walk, as after mth_bgzf_decode; nothing is appended).  The offsets are
 * those of the serial chain whatever the guesses were.
 * The arguments are mth_bgzf_decode's; flags: MTH_STRADDLE_APPEND = its `append`.  The stream of a call may end inside a record:
 *   neither _LAST nor _DROP_TAIL  the bytes from the start of the first unfinished record on are kept on the device (the carry) and
 *                                 come first in the stream of the next _APPEND call, which passes first_byte = 0; a carry above
 *                                 MTH_STRADDLE_MAX_CARRY bytes is MTH_ERR_UNALIGNED
 *   MTH_STRADDLE_LAST             the stream ends with this call: an unfinished record is MTH_ERR_FORMAT
 *   MTH_STRADDLE_DROP_TAIL        the stream ends with this call and an unfinished last record is dropped (a --region load: the
 *                                 last block the index names may end inside a record that starts past the region)
 * A call without _APPEND, and mth_reset, drop the carry.  info (may be NULL): rounds = repair rounds run, repaired_blocks = blocks
 * walked again in them, carry_bytes = the carry this call leaves.  mth_timing_get: k_straddle_guess / _walk / _repair. */
#define MTH_STRADDLE_APPEND     1u
#define MTH_STRADDLE_LAST       2u
#define MTH_STRADDLE_DROP_TAIL  4u
#define MTH_STRADDLE_MAX_ROUNDS 64
#define MTH_STRADDLE_MAX_CARRY  (256ull << 20)
typedef struct {
    uint32_t rounds, repaired_blocks;
    uint64_t carry_bytes;
} mth_straddle_info_t;
int  mth_bgzf_decode_straddle(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                              const uint32_t *isize, uint64_t n_blocks, uint64_t first_byte, unsigned flags, mth_decoded_t *out,
                              mth_straddle_info_t *info);
/* The record chain of a RUN of blocks of such a file, without decoding anything: what a shard of a multi-GPU run needs to know
 * about its part of the file before any block has a verified entry.  The scheme of mth_bgzf_decode_straddle one level up: every
 * run is scanned from a guessed entry, in parallel, and the caller then verifies the guesses against the serial chain (run 0
 * enters at the header's end, run r where run r - 1 leaves; a run whose assumed entry differs is scanned again from the true one),
 * so nothing of the guess rule enters the result.
 * Arguments as mth_bgzf_decode_straddle's (file bytes, coff / csize / isize of n_blocks blocks), of which the first n_run are the
 * run and the rest look-ahead: the caller passes blocks after the run until the stream reaches at least MTH_STRADDLE_LOOKAHEAD
 * bytes past the run's end, or the file ends -- a block_size field or the 12 key bytes of a record that lie across a block's end
 * can then be read, and a record that ends beyond the stream leaves at p + 4 + block_size, a value (not "cannot go on").
 * entry: offset in the run's stream where the chain enters (it may lie past any number of the run's blocks: a record that started
 * before the run covers them), or MTH_STRADDLE_ENTRY_GUESS: the run's first block guesses like every other block and the rounds
 * settle relative to that guess; where a block finds no guess, or leaves at or past the END of the block behind it, the chain
 * breaks and a new one starts at that block's own guess (no block has a certain entry yet, so an exit is believed only as far as
 * the next block: a wrong guess whose block_size leads megabytes on must not overwrite good guesses one block per round).
 * rows (host memory, n_run of them), per block of the run: start = offset inside the block of the first record that STARTS there
 * (MTH_STRADDLE_NO_START: a record covers the whole block), ref_id / pos = that record's refID and pos as stored, exit = bytes
 * past the block's end where the chain leaves it (MTH_STRADDLE_EXIT_BAD: it cannot go on from this block -- no entry, block_size
 * < 32 or unreadable; under a guessed entry that says nothing about the file).  run: the entry that was used
 * (MTH_STRADDLE_ENTRY_GUESS: the first block found no guess, or the chain breaks inside the run -- scan it again) and the run's exit relative to the first byte after the run.
 * info as above (carry_bytes 0); the round bound and MTH_ERR_UNALIGNED as above.
 * A second pass: the inflated bytes, the block table and the links of the latest scan stay in the context until its next call
 * that inflates (or mth_reset), so mth_bgzf_straddle_rescan(ctx, entry, ...) -- the same run from the true entry -- costs repair
 * rounds from block 0 only, no copy and no inflate: guesses that are 4 bytes short are common on look-alike data
 * (profiles/straddle_walk.md), rescans are not rare.  MTH_ERR_INVALID when the context holds no scan. */
#define MTH_STRADDLE_ENTRY_GUESS (~0ull)
#define MTH_STRADDLE_NO_START    0xffffffffu
#define MTH_STRADDLE_EXIT_BAD    (~0ull)
#define MTH_STRADDLE_LOOKAHEAD   36
typedef struct {
    uint32_t start;
    int32_t  ref_id, pos;
    uint32_t pad_;
    uint64_t exit;
} mth_straddle_row_t;
typedef struct {
    uint64_t entry, exit;
} mth_straddle_run_t;
int  mth_bgzf_straddle_scan(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                            const uint32_t *isize, uint64_t n_blocks, uint64_t n_run, uint64_t entry, mth_straddle_row_t *rows,
                            mth_straddle_run_t *run, mth_straddle_info_t *info);
int  mth_bgzf_straddle_rescan(mth_ctx_t *ctx, uint64_t entry, mth_straddle_row_t *rows, mth_straddle_run_t *run,
                              mth_straddle_info_t *info);
/* Overlap of the NEXT chunk's host-to-device copy with the current chunk's kernels: announces file[0, n_bytes) (host memory
 * that stays valid) as the chunk after the one the next mth_bgzf_decode / mth_bgzf_inflate call is given.  That call starts a
 * helper thread which copies the announced bytes into a second staging buffer on a side stream while its own kernels run;
 * the following call, given the SAME pointer and size, uses them instead of copying.  n_bytes = 0 withdraws the announcement. */
int  mth_bgzf_stage(mth_ctx_t *ctx, const void *file, uint64_t n_bytes);
/* size the decoded arrays for n_reads / n_cpgs in total (what is decoded so far is kept): spares the appending calls their
 * reallocations when the caller can estimate the file's totals */
int  mth_decode_reserve(mth_ctx_t *ctx, uint64_t n_reads, uint64_t n_cpgs);
/* Which way the load calls went, since the context's creation or its last mth_reset (read-only, host counters): calls of the inflate
 * step (mth_bgzf_inflate / mth_bgzf_decode / mth_bgzf_decode_straddle / mth_bgzf_straddle_scan) that took the buffer announced by
 * mth_bgzf_stage, that copied their bytes in line with one copy, that copied them in pieces (METHEOR_COPY_PIECE_MB), the k_inflate
 * launches of the pieced calls, announcements whose bytes were copied but not taken (the following call came with another pointer
 * or size), and growths of the eight decoded arrays (one per array and growth, the first allocation included) by the decode itself
 * and by mth_decode_reserve. */
typedef struct {
    uint64_t staged_calls, inline_calls, pieced_calls, pieced_launches, stage_misses, decode_reallocs;
} mth_load_stats_t;
int  mth_load_stats(mth_ctx_t *ctx, mth_load_stats_t *out);
/* copy the decoded arrays to the host (any pointer may be NULL) */
int  mth_decoded_fetch(mth_ctx_t *ctx, int32_t *tid, int32_t *start, int32_t *end, uint8_t *mapq, uint8_t *fwd,
                       uint64_t *cpg_off, uint32_t *cpg_pos, uint16_t *cpg_rel);
/* the decoded stream as runs of equal tid, in file order (a coordinate-sorted file has one run per contig): up to `cap`
 * runs are returned, *n_runs is the true number; *flags bit0 = some read has no aligned base (start < 0), bit1 = some
 * record has no contig (tid < 0) -- such records cannot enter a batch as they are --, bit2 = some read starts before its
 * predecessor on the same contig (the input is not coordinate-sorted) */
int  mth_decoded_contigs(mth_ctx_t *ctx, uint32_t cap, int32_t *tids, uint64_t *read_beg, uint64_t *read_end,
                         uint32_t *n_runs, uint32_t *flags);
/* Contig groups for the decoded stream (see "contig groups" above): the runs of mth_decoded_contigs (n_contigs of them, tids strictly
 * ascending, consecutive read ranges) are packed greedily into groups of at most 2^31 - 2^22 virtual positions; the reads' and calls'
 * positions of every group with more than one contig are shifted IN PLACE on the device (mth_decoded_fetch then returns the shifted
 * values) and the groups are registered.  Returns per group g < *n_groups: the contigs [first_contig[g], first_contig[g + 1]) and
 * batch_tid[g] = the group's handle, or the contig's own tid for a group of one; the caller batches a group with
 * mth_decoded_batch(ctx, read_beg[first_contig[g]], read_end[first_contig[g + 1] - 1], batch_tid[g], 0, -1, &b).
 * When some contig holds a call at position -1 (the word 0x7fffffff, see mth_batch_t), every group starts at virtual position
 * MTH_GROUP_MINUS_ONE_BASE instead of 0 and a group of one contig is registered (and shifted) like any other: no batch carries the word.
 * *n_groups = 0: nothing was changed (tids not ascending, a read without an aligned base, a previous grouping in place, or nothing to
 * merge and no call at -1).
 * mth_decoded_group_each: the same with ONE contig per group -- only the contigs that hold a call at -1 are shifted (by
 * MTH_GROUP_MINUS_ONE_BASE: batch_tid[g] is a handle, and a region of such a contig is given in shifted positions, from BASE - 1 to own
 * the site at -1); the others come back under their own tid, untouched.  For callers that batch per contig or per region. */
#define MTH_GROUP_MINUS_ONE_BASE 4096
int  mth_decoded_group(mth_ctx_t *ctx, uint32_t n_contigs, const int32_t *tids, const uint64_t *read_beg, const uint64_t *read_end,
                       uint32_t *n_groups, uint32_t *first_contig /* [n_contigs + 1] */, int32_t *batch_tid /* [n_contigs] */);
int  mth_decoded_group_each(mth_ctx_t *ctx, uint32_t n_contigs, const int32_t *tids, const uint64_t *read_beg, const uint64_t *read_end,
                            uint32_t *n_groups, uint32_t *first_contig /* [n_contigs + 1] */, int32_t *batch_tid /* [n_contigs] */);
/* re-order the decoded stream by (tid, start), stably, on the device -- for the measures whose result does not depend on the
 * record order (lpmd.rs:175-200, me.rs:106-125, pm.rs:101-121): an input that is not coordinate-sorted or not grouped by contig
 * can then be batched like a sorted one.  Every record must have a contig and an aligned base (flags bit0 / bit1 clear). */
int  mth_decoded_sort(mth_ctx_t *ctx);

/* ---- PDR, MHL, FDRP and qFDRP of a decoded stream that is NOT coordinate-sorted (mth_fileorder.hip) ----------------------------
 * The reference iterates the records in file order and never checks it (pdr.rs:139, mhl.rs:155, fdrp.rs:197, qfdrp.rs:209); these
 * four measures finalise a site when a later record's first CpG lies beyond it (pdr.rs:160-177 margin 150, passing records;
 * mhl.rs:162-173 any record with a CpG; fdrp.rs:212-223 passing records) and a site that is called again starts over, the last
 * segment with enough reads winning.  On a sorted file the per-contig batches compute that; for any other order this call replays
 * the stream itself, over the WHOLE decoded stream (mth_decode_records / mth_bgzf_decode, --cpg-set filter included) in the order
 * it was decoded: rows sorted by (tid, pos) as the reference's BTreeMap gives them.
 *   MTH_FO_PDR  v0 = pdr, c0 = n_concordant, c1 = n_discordant        (min_depth, min_cpgs, min_qual)
 *   MTH_FO_MHL  v0 = mhl, c0 = coverage                                (min_depth, min_cpgs, min_qual)
 *   MTH_FO_FDRP v0 = fdrp, v1 = qfdrp, c0 = stored reads               (min_depth, min_qual, max_depth <= 16384, min_overlap, seed)
 * Synchronous.  MTH_ERR_CAPACITY beyond 2^31 records / calls, MHL reads with > 1024 CpGs, --max-depth > 16384 (as on the sorted
 * path; up to 256 stored reads a site's slots live in LDS, beyond that in a per-wave row of HBM scratch). */
enum { MTH_FO_PDR = 0, MTH_FO_MHL = 1, MTH_FO_FDRP = 2 };
typedef struct {
    int32_t  measure;
    uint32_t min_depth, min_cpgs, max_depth;
    int32_t  min_overlap;
    uint8_t  min_qual;
    uint64_t seed;
} mth_fileorder_params_t;
int  mth_fileorder_run(mth_ctx_t *ctx, const mth_fileorder_params_t *params);
int  mth_fileorder_fetch(mth_ctx_t *ctx, uint64_t *n_rows, int32_t *tid, int32_t *pos, float *v0, float *v1, uint32_t *c0, uint32_t *c1);
/* reads [read_beg, read_end) of the decoded stream -- ONE contig's reads (or a region slice of them), or one contig GROUP's after
 * mth_decoded_group (tid = the group's handle, region_beg 0, region_end -1) -- as a
 * device-resident batch for the accumulate calls: 32-bit offsets rebased on the device, max_span reduced on
 * the device.  region_end < 0 = up to the last position these reads cover (reduced on the device too): what a
 * whole-contig batch should pass -- the reference emits every site it sees, also past the header's LN.
 * Valid until the next mth_decoded_batch / mth_decode_records call. */
int  mth_decoded_batch(mth_ctx_t *ctx, uint64_t read_beg, uint64_t read_end, int32_t tid, int32_t region_beg,
                       int32_t region_end, mth_batch_t *batch);

/* ---- `metheor tag`: the Bismark XM string of every record from the read's bases and the genome ----------
 * Replaces src/tag.rs:130-384 determine_xm_tag_string (per record) and the genome side of run(), tag.rs:419-431.
 * mth_tag_set_genome: n_refs contigs in header (tid) order; ref_len[t] = the header's LN (tag.rs:60-72), seq[t] / seq_len[t] =
 * the bases the FASTA gave for positions [0, seq_len[t]) (any case; HOST memory; copied).  A contig the FASTA lacks is the
 * caller's error to raise (tag.rs:427 expect).
 * mth_tag_records: a window of BAM records as mth_decode_records takes it (raw bytes + n_rec + 1 offsets); is_paired_end =
 * bamutil.rs:27-37 (flag 0x1 of the file's first record).  On return record i's string is xm[xm_off[i] .. xm_off[i] + xm_len[i])
 * (host memory owned by the context, valid until the next call).  MTH_ERR_FORMAT where the reference panics. */
typedef struct {
    uint64_t        n_records;
    const uint64_t *xm_off;     /* n_records + 1 slot starts */
    const uint32_t *xm_len;
    const char     *xm;
} mth_tag_out_t;
int  mth_tag_set_genome(mth_ctx_t *ctx, int32_t n_refs, const int64_t *ref_len, const uint8_t *const *seq, const int64_t *seq_len);
int  mth_tag_records(mth_ctx_t *ctx, const void *raw, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                     int is_paired_end, mth_tag_out_t *out);
/* `tag --output-format bam`: mth_tag_records' arguments and errors (MTH_ERR_FORMAT where the reference panics; nothing is
 * returned then), but what comes back is the window's TAGGED records as BGZF blocks, made on the device: every input record with
 * XM:Z:<string> appended as its last optional field (its bytes, 'X' 'M' 'Z', the string, NUL; block_size raised by the string's
 * length + 4 -- a zero-length string still gets the field), cut into blocks by htslib's rule (at most 0xff00 bytes per block, a
 * record that does not fit starts a new block, a record longer than a block starts one and fills consecutive blocks, the window's
 * last block is closed short) and deflated as mth_bgzf_deflate does.  The strings stay on the device; only the records' sizes come
 * back for the cuts.  bytes / block_off: host memory owned by the context, valid until its next deflate or tag call; block b is
 * bytes[block_off[b] .. block_off[b + 1]).  stream_bytes = size of the tagged record stream.  No EOF block is added. */
typedef struct {
    uint64_t        n_records, n_blocks, stream_bytes, n_bytes;
    const uint8_t  *bytes;
    const uint64_t *block_off;  /* n_blocks + 1 */
} mth_tag_bam_out_t;
int  mth_tag_records_bam(mth_ctx_t *ctx, const void *raw, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                         int is_paired_end, mth_tag_bam_out_t *out);
/* ---- the BAM index (.bai, SAM spec 5.2) of a record stream, built on the device (mth_bai.hip) -------------------------------
 * What is indexed, for every record with refID >= 0 in file order: beg = pos, end = pos + max(1, reference length of the CIGAR:
 * M D N = X), bin = reg2bin(beg, end), and the virtual offsets (file offset of the BGZF block << 16 | offset inside it) of its first
 * byte and of the byte after its last -- a record that ends exactly at a block's end keeps that block, as bgzf_tell does; a record
 * longer than a block begins in its first block.  Chunks: a run of consecutive records of one (refID, bin) is one chunk, across
 * calls too.  Linear index: per 16-kbp window the smallest first-byte offset of the records that touch it; a window nothing touches
 * takes the entry before it, leading ones are 0.  Per reference with records the four words of samtools' metadata pseudo-bin 37450.
 *   mth_bai_begin        starts an index (any earlier one is dropped): ref_len[t] = the header's LN (the linear table is sized from
 *                        it), file_off = file offset of the next block mth_tag_records_bam will make.  From here to mth_bai_finish
 *                        every successful mth_tag_records_bam call also indexes its window from the buffers it has on the device and
 *                        advances the offset by the window's compressed bytes.
 *   mth_bai_add_records  the same step with everything given: records as mth_decode_records takes them (mem says where raw / rec_off
 *                        live), n_blocks + 1 ascending cut offsets into the stream and every block's file offset, both in HOST memory
 *                        (cut_off[0] = 0, the records must end at or before cut_off[n_blocks]).  n_rec = 0 with an empty block
 *                        (cut_off = {0, 0}): that block follows the stream -- the EOF block; the record that ended where the blocks
 *                        so far end is given its offset as its end, which is what bgzf_tell reports there.
 *   mth_bai_finish       the tables (host memory owned by the context, valid until the next mth_bai_* call) and the end of indexing.
 * Refused, with the record's ordinal (counted from 0 over all calls) in mth_last_error; the lowest one is reported, by the call
 * that met it, by every later mth_bai_add_records and by mth_bai_finish, which then returns no tables -- a new mth_bai_begin
 * starts afresh: MTH_ERR_UNSORTED for a stream that is not coordinate-sorted (refID descending, pos descending inside a
 * reference, a placed record after one with refID < 0; equal positions are fine); MTH_ERR_RANGE for a record that ends beyond
 * 2^29 (the format's limit: a .csi would be needed), lies at pos < 0 or ends beyond its reference's length, or names refID >=
 * n_refs; MTH_ERR_FORMAT for a malformed record.  mth_tag_records_bam itself does not fail on these: the BAM stays complete. */
typedef struct {
    int32_t         n_refs;
    uint64_t        n_records;     /* records seen, with and without a reference */
    uint64_t        n_chunks;
    const uint64_t *chunk_beg, *chunk_end;   /* sorted by (refID, bin), file order inside a bin */
    uint64_t        n_bins;        /* bins that hold chunks, over all references, ascending (refID, bin) */
    const int32_t  *bin_ref;
    const uint32_t *bin_id, *bin_n_chunks;
    const uint32_t *ref_n_bins;    /* n_refs */
    const uint32_t *ref_n_intv;    /* n_refs: highest window touched + 1 */
    const uint64_t *lin_off;       /* n_refs + 1: reference t's entries are lin[lin_off[t] .. lin_off[t] + ref_n_intv[t]) */
    const uint64_t *lin;
    const uint64_t *meta;          /* 4 per reference with records: first offset, last end, records with flag 0x4 clear / set */
    uint64_t        n_no_coor;     /* records with refID < 0 */
} mth_bai_out_t;
int  mth_bai_begin(mth_ctx_t *ctx, int32_t n_refs, const int64_t *ref_len, uint64_t file_off);
int  mth_bai_add_records(mth_ctx_t *ctx, const void *raw, const uint64_t *rec_off, uint64_t n_rec, int mem, const uint64_t *cut_off,
                         const uint64_t *block_coff, uint64_t n_blocks);
int  mth_bai_finish(mth_ctx_t *ctx, mth_bai_out_t *out);
/* mth_tag_set_genome with the FASTA read on the device: the same genome (bytes, offsets, header lengths) straight from the
 * file's text, plain or bgzip-compressed -- what faidx_fetch_seq(name, 0, LN) returns for every contig, with no host pass over
 * the bases.
 *   file / n_bytes  the FASTA file in HOST memory (a read-only mapping will do)
 *   blocks          NULL for plain text; for a BGZF file its block table as mth_bgzf_inflate takes it (payload offset / payload
 *                   bytes / inflated bytes per block, blocks with isize 0 left out; the 8 trailer bytes of every block inside
 *                   the file bytes)
 *   rows[t]         per header contig, tid order: src_off = offset of base 0 in the UNCOMPRESSED stream (.fai column 3), n_bases =
 *                   bases to take = min(LN + 1, .fai length), line_bases / line_width = .fai columns 4 and 5; name (may be NULL)
 *                   only serves the messages
 * The stream is taken in windows (a byte range of a plain file; a run of whole BGZF blocks, inflated and CRC-checked as
 * mth_bgzf_inflate does) of METHEOR_FASTA_CHUNK bytes (default 256 MiB; at least one block), the next window's bytes travelling
 * while k_fasta_pack gathers the current one: base i of a contig is the byte at src_off + (i / line_bases) * line_width +
 * i % line_bases.  That equals what faidx keeps (the isgraph bytes from src_off on) exactly when every gathered byte is isgraph
 * and every byte skipped between two gathered bases is not, and the kernel verifies just that for every byte of every contig's
 * source span.  MTH_ERR_FORMAT: a contig's span leaves the stream ("FASTA shorter than its index says", found before anything is
 * launched), the text does not have the layout the rows state (the message names the contig), or a BGZF block fails its inflate,
 * ISIZE or CRC32.  A call that fails leaves the context's genome as it was. */
typedef struct {
    const uint64_t *coff;
    const uint32_t *csize, *isize;
    uint64_t        n_blocks;
} mth_fasta_blocks_t;
typedef struct {
    uint64_t    src_off;
    int64_t     n_bases, line_bases, line_width;
    const char *name;
} mth_fasta_row_t;
int  mth_tag_set_genome_fasta(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const mth_fasta_blocks_t *blocks, int32_t n_refs,
                              const int64_t *ref_len, const mth_fasta_row_t *rows);
/* n bases of contig tid from base beg on, as the device genome holds them, to dst_host (MTH_ERR_INVALID past the bases the
 * genome holds of the contig; MTH_ERR_STATE without a genome) */
int  mth_tag_genome_fetch(mth_ctx_t *ctx, int32_t tid, int64_t beg, int64_t n, void *dst_host);
/* derive the calls from the genome of mth_tag_set_genome instead of the records' XM:Z (what `metheor tag` followed by
 * the measure computes): applies to the following mth_decode_records / mth_bgzf_decode calls.  is_paired_end =
 * bamutil.rs:27-37.  enabled != 0 before mth_tag_set_genome: MTH_ERR_STATE.
 * The result is the composition of tag.rs:130-384 and readutil.rs:323-345, quirks included (tag.rs walks M, I and D only, the
 * decode reads letter q for the aligned base at query offset q).  An XM:Z field the records carry is not
 * looked at and a record is never "without XM" in this mode (mth_decode_set_xm_min_mapq has no effect); a record on which
 * determine_xm_tag_string panics is MTH_ERR_FORMAT ("tag: ..."), whatever its mapq.  The kernel is k_decode_genome
 * (mth_decode_genome.hip); METHEOR_GENOME_STAGED=1 in the environment selects the second form, k_tag_xm into HBM and k_decode
 * reading the strings from there. */
int  mth_decode_set_genome(mth_ctx_t *ctx, int enabled, int is_paired_end);
/* Take the calls from the SAM base-modification tags MM:Z / ML:B:C (with MN:i) instead of the records' XM:Z: applies to the
 * following mth_decode_records / mth_bgzf_decode / mth_bgzf_decode_straddle calls.  threshold (an ML value, 0..=255; above:
 * MTH_ERR_INVALID): a listed base with ML >= threshold is methylated.  Enabling it while mth_decode_set_genome is on, or the
 * reverse, is MTH_ERR_STATE.
 * The rule, an equivalence: a record decodes as the same record with (1) its flag replaced by flag & 0x10 -- the position rule
 * of readutil.rs:332 then depends on the strand alone: a forward record's call lies at the aligned position of its query
 * offset, a reverse record's one below, so both strands of a CpG land on the top-strand C, and read_fwd = !(flag & 0x10) --,
 * (2) its XM:Z fields removed and (3) XM:Z:X appended, where X has l_seq characters, all '.' except:
 *   - the chosen group is the first group of MM:Z (grammar: (base strand codes mode? (',' digits)* ';')*, base one of ACGTUN,
 *     strand + or -, codes [a-z]+ or [0-9]+, mode . or ?, digits 1 to 9 of them) with base C, strand + and the letter m among
 *     its codes; a group of k letter codes (a numeric code: k = 1) and n numbers owns n * k entries of ML, interleaved in code
 *     order per position, the groups' entries in the groups' order;
 *   - the fundamental bases are the Cs of the ORIGINAL read 5'->3' (SEQ for a forward record; the reverse complement of SEQ for
 *     a reverse one, so query offset q = l_seq - 1 - j and an original C is a stored G); the first number d0 selects fundamental
 *     base d0, each next number d the base d + 1 further on; the i-th listed base has probability ML[base of the group + i * k
 *     + index of m], 255 when the record has no ML field;
 *   - only a fundamental base in read CpG context (the original read's next base is G) gets a character: 'Z' listed with
 *     probability >= threshold, 'z' listed below it or unlisted under mode '.' / no mode, '.' unlisted under mode '?'.
 * Records that contribute nothing (all dots, MTH_NOTE_MODTAG_SKIPPED): l_seq = 0, an H operation in the CIGAR, an integer MN
 * field that differs from l_seq -- checked before MM / ML are looked at.  A record without an MM field of type Z has all dots
 * (its ML is not looked at); a record is never "without XM" in this mode and XM:Z fields are ignored.  The first MM:Z, the
 * first ML and the first MN count; the spellings Mm / Ml count as absent.
 * MTH_ERR_FORMAT ("modtags: ..."), whatever the record's mapq: aux fields that cannot be walked; with an MM:Z field, an ML field
 * that is not B:C, MM outside the grammar, an ML count that differs from the sum of n * k over all groups, a list of the chosen
 * group that selects a fundamental base the read does not have.  MTH_ERR_CAPACITY: l_seq > 65535 (cpg_rel is 16 bits).
 * The kernels are k_mm_xm, which writes X into HBM, and k_decode reading it from there (mth_decode_mm.hip: the staged form,
 * the default, measured the faster one); METHEOR_MM_STAGED=0 in the environment selects the direct form, k_decode_mm, which
 * takes the calls in the decode's own two passes without any string.  There is no host form. */
int  mth_decode_set_modtags(mth_ctx_t *ctx, int enabled, uint32_t threshold);

/* ---- measurement hooks (bench.py's roofline leg) -------------------------------------- */
/* when enabled, every kernel launch is bracketed by hipEvents on the launch stream */
int  mth_timing_enable(mth_ctx_t *ctx, int on);
int  mth_timing_reset(mth_ctx_t *ctx);
/* synchronises; name is one of mth_timing_kernel_name(i); avg over recorded launches */
int  mth_timing_get(mth_ctx_t *ctx, const char *kernel, double *avg_ms, uint64_t *launches);
int  mth_timing_num_kernels(void);
const char *mth_timing_kernel_name(int i);

#ifdef __cplusplus
}
#endif
#endif
