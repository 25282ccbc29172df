// mth_tag.hip -- the `tag` subcommand's per-record function on the device.
//
// Replaces src/tag.rs:130-384 `determine_xm_tag_string`: the Bismark XM string of an alignment from the read's
// bases and the reference genome.  The reference builds, per record, two gapped strings (read / reference columns
// over the CIGAR's M, I and D runs -- nothing else is walked, tag.rs:185-237 -- with two flank columns on each side),
// reverse-complements them for reads from the G->A strand, and classifies every column whose reference base is C by
// the next two read-aligned reference bases (CG / CHG / CHH / unknown), skipping columns a deletion removed.
//
// Here: the genome is resident in HBM (all contigs concatenated, uploaded once); one thread per record, two kernels
// (columns per record -> 64-bit scan -> columns + letters).  The gapped columns of a record live in a scratch slice
// the thread writes and reads back itself (a column's letter looks at up to two later -- for the reverse complement,
// earlier -- read-aligned columns, further away behind deletions).  The letter of a column does not depend on the
// order the columns are visited in, so both strands are emitted in ascending column order, which is what the
// reference's final `rev()` (tag.rs:386-389) produces.  Where the reference panics (a base the complement table does
// not hold, tag.rs:24; an alignment outside the contig, tag.rs:158-170; no second context base, tag.rs:297; an
// unplaced record, tag.rs:155) the batch fails with MTH_ERR_FORMAT.
// Not the hot path: byte-walking threads (HBM/L2-latency bound like k_decode); no MFMA.
#include "mth_bgzf_cuts.h"
#include "mth_ctx.h"
#include "mth_tag_dev.h"

namespace mth {

__global__ __launch_bounds__(256) void k_tag_count(const TagArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const TagRec r = tg_parse(a, i);
    uint64_t n = 4;
    if (!r.bad) {
        for (uint32_t k = 0; k < r.n_cigar; ++k) {
            const uint32_t c = tg_u32(r.cigar + 4 * k), op = c & 15u;
            if (op <= 2u) n += c >> 4;                           // M, I, D (tag.rs:188-235)
        }
    }
    if (r.bad || n >= (1ull << 31)) { atomicOr(a.err, (uint32_t)ERRB_FORMAT); n = 4; }
    a.ncol[i] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void k_tag_xm(const TagArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    a.xm_len[i] = 0;
    const TagRec r = tg_parse(a, i);
    if (r.bad) return;                                           // reported by the count pass
    uint8_t *R = a.cols + a.col_off[i], *G = R + a.total;
    const int64_t nx = tg_xm_record(a, r, a.ncol[i], R, G, a.xm + a.col_off[i]);
    if (nx < 0) { atomicOr(a.err, (uint32_t)ERRB_TAGPANIC); return; }
    a.xm_len[i] = (uint32_t)nx;
}

// the XM strings of n device-resident records into ctx->tag_xm: record i's letters start at tag_coloff[i], tag_xmlen[i] of them.
// k_tag_xm is left in flight: its findings surface at the caller's next synchronisation.
int tag_core(mth_ctx *ctx, const uint8_t *d_raw, const uint64_t *d_off, uint32_t n, int is_paired_end, unsigned long long *total_out) {
    hipStream_t s = ctx->stream;
    const uint32_t nb = (n + 255) / 256;
    MTH_HIP(ctx, ctx->tag_ncol.reserve((size_t)n * 4 + 16, s));
    MTH_HIP(ctx, ctx->tag_coloff.reserve(((size_t)n + 1) * 8 + 16, s));
    MTH_HIP(ctx, ctx->tag_xmlen.reserve((size_t)n * 4 + 16, s));
    TagArgs a{};
    a.raw = d_raw; a.off = d_off; a.n_rec = n;
    a.genome = ctx->tag_genome.as<uint8_t>(); a.g_off = ctx->tag_goff.as<uint64_t>();
    a.g_ln = reinterpret_cast<const int64_t *>(ctx->tag_goff.as<uint64_t>() + ctx->tag_n_refs + 1);
    a.n_refs = ctx->tag_n_refs; a.paired = is_paired_end ? 1 : 0;
    a.ncol = ctx->tag_ncol.as<uint32_t>(); a.xm_len = ctx->tag_xmlen.as<uint32_t>(); a.err = &ctx->d_state->err;
    hipLaunchKernelGGL(k_tag_count, dim3(nb), dim3(256), 0, s, a);
    unsigned long long total = 0;
    int rc = scan_u32_to_u64(ctx, a.ncol, n, 0ull, ctx->tag_coloff.as<unsigned long long>(), &total);   // synchronises
    if (rc) return rc;
    MTH_HIP(ctx, ctx->tag_cols.reserve((size_t)total * 2 + 16, s));
    MTH_HIP(ctx, ctx->tag_xm.reserve((size_t)total + 16, s));
    a.col_off = ctx->tag_coloff.as<unsigned long long>(); a.cols = ctx->tag_cols.as<uint8_t>(); a.total = total;
    a.xm = ctx->tag_xm.as<uint8_t>();
    hipLaunchKernelGGL(k_tag_xm, dim3(nb), dim3(256), 0, s, a);
    MTH_HIP(ctx, hipGetLastError());
    *total_out = total;
    return MTH_OK;
}

// ---- `tag -O bam`: the tagged record stream in HBM -------------------------------------------------------------------------
// Record i of the output is the input record with XM:Z appended as its last optional field: its bytes, 'X' 'M' 'Z', the string,
// a NUL, and block_size raised by xm_len + 4.  k_tag_sizes: bytes per output record (-> 64-bit scan -> where each one starts);
// k_tag_assemble: one wave per record copies the record and its string to that place.  The strings never leave the device.
struct TagBamArgs {
    const uint8_t *raw;
    const uint64_t *off;              // n_rec + 1
    uint32_t n_rec;
    const uint8_t *xm;                // record i's letters at xm_off[i], xm_len[i] of them
    const unsigned long long *xm_off;
    const uint32_t *xm_len;
    uint32_t *sz;                     // sizes pass out: rec_len + 4 + xm_len
    const unsigned long long *out_off;   // assemble in: exclusive scan of sz
    uint8_t *out;
    uint32_t *err;
};

__global__ __launch_bounds__(256) void k_tag_sizes(const TagBamArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const uint64_t n = a.off[i + 1] - a.off[i] + 4ull + a.xm_len[i];
    if (n >= (1ull << 31)) { atomicOr(a.err, (uint32_t)ERRB_FORMAT); a.sz[i] = 0; return; }
    a.sz[i] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void k_tag_assemble(const TagBamArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= a.n_rec) return;
    const uint64_t o0 = a.off[i];
    const uint64_t n = a.off[i + 1] - o0;                       // >= 36: k_tag_count refuses shorter records
    const uint32_t nx = a.xm_len[i];
    if (a.sz[i] != n + 4 + nx) return;                           // (a record k_tag_sizes refused)
    const uint8_t *src = a.raw + o0;
    uint8_t *dst = a.out + a.out_off[i];
    const uint32_t bs = tg_u32(src) + nx + 4u;                   // block_size of the tagged record
    for (uint64_t k = lane; k < n; k += 64) dst[k] = k < 4 ? (uint8_t)(bs >> (8 * k)) : src[k];
    const uint8_t *x = a.xm + a.xm_off[i];
    uint8_t *t = dst + n;
    if (lane < 3) t[lane] = (uint8_t)"XMZ"[lane];
    for (uint32_t k = lane; k < nx; k += 64) t[3 + k] = x[k];
    if (lane == 0) t[3 + nx] = 0;
}

int genome_commit(mth_ctx *ctx, int32_t n_refs, const std::vector<uint64_t> &off, const int64_t *ref_len) {
    hipStream_t s = ctx->stream;
    MTH_HIP(ctx, ctx->tag_goff.reserve(((size_t)n_refs + 1) * 8 + (size_t)n_refs * 8 + 16, s));
    MTH_HIP(ctx, hipMemcpyAsync(ctx->tag_goff.p, off.data(), ((size_t)n_refs + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_refs) MTH_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(ctx->tag_goff.p) + ((size_t)n_refs + 1) * 8, ref_len, (size_t)n_refs * 8, hipMemcpyHostToDevice, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));                      // the caller's buffers may go away
    ctx->tag_h_goff = off;
    ctx->tag_n_refs = n_refs;
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_tag_set_genome(mth_ctx_t *ctx, int32_t n_refs, const int64_t *ref_len, const uint8_t *const *seq, const int64_t *seq_len) {
    if (!ctx || n_refs < 0 || (n_refs && (!ref_len || !seq || !seq_len))) return MTH_ERR_INVALID;
    MTH_ENTER(ctx);
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> off((size_t)n_refs + 1, 0);
    for (int32_t t = 0; t < n_refs; ++t) {
        if (seq_len[t] < 0 || (seq_len[t] && !seq[t])) return MTH_ERR_INVALID;
        off[t + 1] = off[t] + (uint64_t)seq_len[t];
    }
    MTH_HIP(ctx, ctx->tag_genome.reserve((size_t)off[n_refs] + 16, s));
    for (int32_t t = 0; t < n_refs; ++t)
        if (seq_len[t]) MTH_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(ctx->tag_genome.p) + off[t], seq[t], (size_t)seq_len[t], hipMemcpyHostToDevice, s));
    return genome_commit(ctx, n_refs, off, ref_len);
}

int mth_tag_genome_fetch(mth_ctx_t *ctx, int32_t tid, int64_t beg, int64_t n, void *dst_host) {
    if (!ctx || beg < 0 || n < 0 || (n && !dst_host)) return MTH_ERR_INVALID;
    if (ctx->tag_n_refs < 0) return fail(ctx, MTH_ERR_STATE, "mth_tag_set_genome has not been called");
    if (tid < 0 || tid >= ctx->tag_n_refs) return fail(ctx, MTH_ERR_INVALID, "mth_tag_genome_fetch: no such contig");
    const uint64_t o0 = ctx->tag_h_goff[(size_t)tid], o1 = ctx->tag_h_goff[(size_t)tid + 1];
    if ((uint64_t)beg > o1 - o0 || (uint64_t)n > o1 - o0 - (uint64_t)beg) return fail(ctx, MTH_ERR_INVALID, "mth_tag_genome_fetch: the slice leaves the bases the genome holds of this contig");
    MTH_ENTER(ctx);
    MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) MTH_HIP(ctx, hipMemcpy(dst_host, ctx->tag_genome.as<uint8_t>() + o0 + (uint64_t)beg, (size_t)n, hipMemcpyDeviceToHost));
    return MTH_OK;
}

int mth_tag_records(mth_ctx_t *ctx, const void *raw, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                    int is_paired_end, mth_tag_out_t *out) {
    if (!ctx || !out || (n_rec && (!raw || !rec_off))) return MTH_ERR_INVALID;
    if (n_rec >= (1ull << 32) - 16) return fail(ctx, MTH_ERR_CAPACITY, "more than 2^32 records in one tag call: split the stream");
    if (ctx->tag_n_refs < 0) return fail(ctx, MTH_ERR_STATE, "mth_tag_set_genome has not been called");
    MTH_ENTER(ctx);
    hipStream_t s = ctx->stream;
    *out = mth_tag_out_t{};
    ctx->tag_h_off.assign(1, 0);
    ctx->tag_h_len.clear(); ctx->tag_h_xm.clear();
    out->xm_off = ctx->tag_h_off.data();
    if (n_rec == 0) return MTH_OK;
    const uint8_t *d_raw = (const uint8_t *)raw;
    const uint64_t *d_off = rec_off;
    if (mem == MTH_MEM_HOST) {
        MTH_HIP(ctx, ctx->dec_raw.reserve(n_bytes + 16, s));
        MTH_HIP(ctx, ctx->dec_recoff.reserve((n_rec + 1) * 8, s));
        if (n_bytes) MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_raw.p, raw, n_bytes, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_recoff.p, rec_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, s));
        d_raw = ctx->dec_raw.as<uint8_t>(); d_off = ctx->dec_recoff.as<uint64_t>();
    } else if (mem != MTH_MEM_DEVICE) {
        return fail(ctx, MTH_ERR_INVALID, "mem");
    }
    const uint32_t n = (uint32_t)n_rec;
    unsigned long long total = 0;
    int rc = tag_core(ctx, d_raw, d_off, n, is_paired_end, &total);
    if (rc) return rc;
    if ((rc = sync_and_check(ctx))) return rc;
    // results to the host: slot offsets, lengths, letters
    ctx->tag_h_off.resize((size_t)n + 1);
    ctx->tag_h_len.resize(n);
    ctx->tag_h_xm.resize((size_t)total);
    MTH_HIP(ctx, hipMemcpy(ctx->tag_h_off.data(), ctx->tag_coloff.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    MTH_HIP(ctx, hipMemcpy(ctx->tag_h_len.data(), ctx->tag_xmlen.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (total) MTH_HIP(ctx, hipMemcpy(ctx->tag_h_xm.data(), ctx->tag_xm.p, (size_t)total, hipMemcpyDeviceToHost));
    out->n_records = n_rec; out->xm_off = ctx->tag_h_off.data(); out->xm_len = ctx->tag_h_len.data();
    out->xm = reinterpret_cast<const char *>(ctx->tag_h_xm.data());
    return MTH_OK;
}

int mth_tag_records_bam(mth_ctx_t *ctx, const void *raw, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                        int is_paired_end, mth_tag_bam_out_t *out) {
    if (!ctx || !out || (n_rec && (!raw || !rec_off))) return MTH_ERR_INVALID;
    if (n_rec >= (1ull << 32) - 16) return fail(ctx, MTH_ERR_CAPACITY, "more than 2^32 records in one tag call: split the stream");
    if (ctx->tag_n_refs < 0) return fail(ctx, MTH_ERR_STATE, "mth_tag_set_genome has not been called");
    MTH_ENTER(ctx);
    hipStream_t s = ctx->stream;
    *out = mth_tag_bam_out_t{};
    ctx->def_h_out.clear();
    ctx->def_h_boff.assign(1, 0);
    out->block_off = ctx->def_h_boff.data();
    if (n_rec == 0) return MTH_OK;
    const uint8_t *d_raw = (const uint8_t *)raw;
    const uint64_t *d_off = rec_off;
    if (mem == MTH_MEM_HOST) {
        MTH_HIP(ctx, ctx->dec_raw.reserve(n_bytes + 16, s));
        MTH_HIP(ctx, ctx->dec_recoff.reserve((n_rec + 1) * 8, s));
        if (n_bytes) MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_raw.p, raw, n_bytes, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_recoff.p, rec_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, s));
        d_raw = ctx->dec_raw.as<uint8_t>(); d_off = ctx->dec_recoff.as<uint64_t>();
    } else if (mem != MTH_MEM_DEVICE) {
        return fail(ctx, MTH_ERR_INVALID, "mem");
    }
    const uint32_t n = (uint32_t)n_rec;
    unsigned long long xm_total = 0;
    int rc = tag_core(ctx, d_raw, d_off, n, is_paired_end, &xm_total);
    if (rc) return rc;
    MTH_HIP(ctx, ctx->tag_sz.reserve((size_t)n * 4 + 16, s));
    MTH_HIP(ctx, ctx->tag_ooff.reserve(((size_t)n + 1) * 8 + 16, s));
    TagBamArgs a{};
    a.raw = d_raw; a.off = d_off; a.n_rec = n; a.xm = ctx->tag_xm.as<uint8_t>(); a.xm_off = ctx->tag_coloff.as<unsigned long long>();
    a.xm_len = ctx->tag_xmlen.as<uint32_t>(); a.sz = ctx->tag_sz.as<uint32_t>(); a.err = &ctx->d_state->err;
    hipLaunchKernelGGL(k_tag_sizes, dim3((n + 255) / 256), dim3(256), 0, s, a);
    unsigned long long total = 0;
    if ((rc = scan_u32_to_u64(ctx, a.sz, n, 0ull, ctx->tag_ooff.as<unsigned long long>(), &total))) return rc;   // synchronises
    if ((rc = sync_and_check(ctx))) return rc;                   // a record the reference panics on: nothing is returned
    MTH_HIP(ctx, ctx->tag_stream.reserve((size_t)total + 16, s));
    a.out_off = ctx->tag_ooff.as<unsigned long long>(); a.out = ctx->tag_stream.as<uint8_t>();
    {
        LaunchTimer lt(ctx, K_TAG_ASSEMBLE);
        hipLaunchKernelGGL(k_tag_assemble, dim3((n + 3) / 4), dim3(256), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    // the block cuts need the records' sizes: 4 bytes per record come back, the strings do not
    ctx->tag_h_sz.resize(n);
    MTH_HIP(ctx, hipMemcpyAsync(ctx->tag_h_sz.data(), ctx->tag_sz.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    bgzf_record_cuts(ctx->tag_h_sz.data(), n, ctx->tag_h_cut);
    const uint64_t nb = ctx->tag_h_cut.size() - 1;
    if ((rc = deflate_core(ctx, ctx->tag_stream.as<uint8_t>(), ctx->tag_h_cut.data(), nb))) return rc;
    if (ctx->bai.on) {
        // mth_bai_begin: the window goes into the index from what is on the device -- the stream, its record offsets, the cuts at
        // the head of the deflate table and the blocks' offsets.  What the index refuses (unsorted input, a record a .bai cannot
        // address) does not fail the window: mth_bai_finish reports it
        rc = bai_window(ctx, ctx->tag_stream.as<uint8_t>(), ctx->tag_ooff.as<unsigned long long>(), n, ctx->def_tab.as<unsigned long long>(),
                        ctx->def_boff.as<unsigned long long>(), ctx->bai.file_off, (uint32_t)nb);
        if (rc == MTH_ERR_HIP) return rc;
        ctx->bai.file_off += ctx->def_h_out.size();
    }
    out->n_records = n_rec; out->n_blocks = nb; out->stream_bytes = total;
    out->bytes = ctx->def_h_out.data(); out->n_bytes = ctx->def_h_out.size(); out->block_off = ctx->def_h_boff.data();
    return MTH_OK;
}

}  // extern "C"
