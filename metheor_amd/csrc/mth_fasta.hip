// mth_fasta.hip -- the --genome FASTA read on the device: FASTA text in HBM -> the packed genome the decode kernels read.
//
// Replaces the host side of tag.rs:412-431 (faidx::Reader::from_path + fetch_seq(name, 0, LN) per @SQ contig): htslib seeks to the
// .fai offset of the contig and keeps the isgraph bytes until it has the bases asked for.  Here the file's bytes go to the device as
// they are -- plain text, or BGZF blocks through the inflate of mth_inflate.hip -- and base i of a contig is GATHERED from where the
// .fai row says it lies: src_off + (i / line_bases) * line_width + i % line_bases.  That is faidx's result exactly when every
// gathered byte is isgraph (0x21..0x7e) and every byte skipped between two gathered bases is not; k_fasta_pack checks both for every
// byte of every contig's source span (up to its last wanted base), each byte once, and a violation fails the call: nothing is
// taken on trust from the index.
//
// The stream is taken in WINDOWS (a byte range of a plain file, a run of whole BGZF blocks), the next window's file bytes travelling
// on the side stream (mth_bgzf_stage's helper thread) while the current one is inflated and packed; neither the file nor the inflated
// stream is ever resident as a whole.  The host cuts every contig's source span at the window borders into SEGMENTS; a launch takes
// one window's segments, a workgroup one TILE of a segment: 4 KiB of source, 16-byte aligned in the window buffer.
//   1. the tile's bytes into LDS, one aligned 16-B load per lane; the lane classifies its own 16 bytes against the line layout
//      (one modulo per lane, then a running column) -- the verification;
//   2. the bases whose source lies in the tile are a contiguous run of the genome; a lane assembles one 16-B aligned chunk of it
//      from LDS (one division per lane and chunk, then a running column that hops over the line end) and stores it whole.  The
//      run's first and last chunk are shared with the neighbouring tile, segment or contig and are written byte by byte by each
//      side: a wide store there would race with the neighbour.
// All stream, layout and genome offsets are 64-bit; what is 32-bit is relative to a tile.  Memory-bound streaming (reads the text
// once, writes the genome once); no MFMA.
#include "mth_ctx.h"
#include "mth_inflate.h"

namespace mth {

constexpr uint32_t FA_TILE = 4096;           // source bytes per workgroup: 256 lanes x 16 B
constexpr uint32_t FA_NO_TID = 0xffffffffu;

struct FaSeg {
    uint64_t win_off;      // the segment's first byte in the window buffer
    uint64_t lay_off;      // the same byte's offset from the contig's base 0: its place in the line layout
    uint64_t n;            // bytes
    uint64_t dst;          // the contig's base 0 in the genome
    uint64_t lb, lw;       // line_bases, line_width
    uint64_t tile0;        // the segment's first tile in the launch
    uint32_t tid, pad_;
};
struct FaArgs {
    const uint8_t *win;    // the window's bytes, 16-byte aligned
    uint64_t win_readable; // bytes of it that may be loaded (the window rounded up to 16: the buffers are padded)
    const FaSeg *seg;
    uint32_t n_seg;
    uint8_t *genome;
    uint64_t genome_bytes;
    uint32_t *bad_tid;     // the error word: lowest tid with a byte that does not fit its layout
};

// the first base whose place in the layout is at or behind d
__device__ __forceinline__ uint64_t fa_base_at(uint64_t d, uint64_t lb, uint64_t lw) {
    const uint64_t line = d / lw, r = d - line * lw;
    return r < lb ? line * lb + r : (line + 1) * lb;
}

__global__ __launch_bounds__(256) void k_fasta_pack(const FaArgs a) {
    __shared__ uint4 s_v[FA_TILE / 16];
    const uint8_t *const s_b = reinterpret_cast<const uint8_t *>(s_v);
    const uint32_t lane = threadIdx.x;
    uint32_t si = 0, sj = a.n_seg;                        // the last segment that starts at or before this tile
    while (sj - si > 1) {
        const uint32_t m = (si + sj) >> 1;
        if (a.seg[m].tile0 <= blockIdx.x) si = m; else sj = m;
    }
    const FaSeg sg = a.seg[si];
    const uint64_t t0 = (sg.win_off & ~15ull) + (blockIdx.x - sg.tile0) * FA_TILE;      // the tile in the window buffer
    const uint64_t lo = t0 > sg.win_off ? t0 : sg.win_off;
    const uint64_t hi = t0 + FA_TILE < sg.win_off + sg.n ? t0 + FA_TILE : sg.win_off + sg.n;    // the tile's bytes of the segment: [lo, hi)
    if (lo >= hi) return;                                 // (uniform; the host counts no such tile)
    const uint64_t dlo = sg.lay_off + (lo - sg.win_off), dhi = dlo + (hi - lo);        // the same in the layout
    // ---- 1. load and verify ----
    const uint64_t off = t0 + 16ull * lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (off + 16 <= a.win_readable) v = *reinterpret_cast<const uint4 *>(a.win + off);
    s_v[lane] = v;
    const uint64_t p0 = off > lo ? off : lo, p1 = off + 16 < hi ? off + 16 : hi;
    if (p0 < p1) {
        // the column of byte p0 in its line: dlo's column (uniform) plus less than a tile
        const uint64_t x = dlo % sg.lw + (p0 - lo);
        uint64_t r = sg.lw > 8192 ? (x >= sg.lw ? x - sg.lw : x) : (uint64_t)((uint32_t)x % (uint32_t)sg.lw);
        const uint32_t j0 = (uint32_t)(p0 - off), j1 = (uint32_t)(p1 - off);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        bool bad = false;
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
            if (j >= j0 && j < j1) {
                const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                const bool graph = c - 0x21u < 0x5eu;                 // isgraph: 0x21 .. 0x7e
                bad |= graph != (r < sg.lb);
                if (++r == sg.lw) r = 0;
            }
        }
        if (bad) atomicMin(a.bad_tid, sg.tid);
    }
    __syncthreads();
    // ---- 2. the bases whose source lies in [lo, hi): one 16-B chunk of the genome per lane ----
    const uint64_t b0 = fa_base_at(dlo, sg.lb, sg.lw), b1 = fa_base_at(dhi, sg.lb, sg.lw);
    if (b0 >= b1) return;
    const uint64_t line0 = b0 / sg.lb, r0 = b0 - line0 * sg.lb;
    const uint64_t s0 = line0 * sg.lw + r0 - dlo + (lo - t0);           // base b0's byte in the tile
    const uint64_t g0 = sg.dst + b0, g1 = sg.dst + b1, c0 = g0 >> 4;
    const uint32_t n_chunks = (uint32_t)(((g1 + 15) >> 4) - c0);        // <= FA_TILE / 16 + 1
    for (uint32_t ci = lane; ci < n_chunks; ci += 256) {
        const uint64_t ga = (c0 + ci) << 4;
        const uint64_t glo = ga > g0 ? ga : g0, ghi = ga + 16 < g1 ? ga + 16 : g1;
        // line and column of the chunk's first base, from the start of b0's line: x < lb + FA_TILE + 16
        const uint64_t x = r0 + (glo - g0);
        uint64_t lines, r;
        if (sg.lb > 8192) { lines = x >= sg.lb ? 1u : 0u; r = x - (lines ? sg.lb : 0u); }
        else { const uint32_t q = (uint32_t)x / (uint32_t)sg.lb; lines = q; r = (uint32_t)x - q * (uint32_t)sg.lb; }
        uint64_t idx = s0 + lines * sg.lw + r - r0;                     // its byte in the tile
        const uint32_t n = (uint32_t)(ghi - glo), sh = (uint32_t)(glo - ga);
        uint64_t wlo = 0, whi = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint64_t c = idx < FA_TILE ? s_b[idx] : 0u;          // (always inside: the base's source lies in the tile)
            const uint32_t q = sh + j;
            if (q < 8) wlo |= c << (8 * q); else whi |= c << (8 * (q - 8));
            ++idx;
            if (++r == sg.lb) { r = 0; idx += sg.lw - sg.lb; }
        }
        if (n == 16) {
            if (ga + 16 <= a.genome_bytes)
                *reinterpret_cast<uint4 *>(a.genome + ga) = make_uint4((uint32_t)wlo, (uint32_t)(wlo >> 32), (uint32_t)whi, (uint32_t)(whi >> 32));
        } else {
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t q = sh + j;
                if (glo + j < a.genome_bytes) a.genome[glo + j] = (uint8_t)(q < 8 ? wlo >> (8 * q) : whi >> (8 * (q - 8)));
            }
        }
    }
}

namespace {

struct FaWin { uint64_t u0, u1, f0, fn, b0, b1; size_t seg0, seg1; uint64_t tiles; };

// nothing of the caller's file may be in use when the call returns: the helper thread's copy included
void fa_drain(mth_ctx *ctx) {
    ctx->next_src = nullptr; ctx->next_bytes = 0;
    if (ctx->stage_thread.joinable()) ctx->stage_thread.join();
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    ctx->staged_src = nullptr;
}

}  // namespace

}  // namespace mth

using namespace mth;

extern "C" int mth_tag_set_genome_fasta(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const mth_fasta_blocks_t *blocks, int32_t n_refs,
                                        const int64_t *ref_len, const mth_fasta_row_t *rows) {
    if (!ctx || n_refs < 0 || (n_refs && (!ref_len || !rows)) || (n_bytes && !file)) return MTH_ERR_INVALID;
    const size_t nb = blocks ? (size_t)blocks->n_blocks : 0;
    if (blocks && nb && (!blocks->coff || !blocks->csize || !blocks->isize)) return MTH_ERR_INVALID;
    // the stream: the file itself, or the blocks' inflated bytes back to back
    std::vector<uint64_t> ustart(nb + 1, 0);
    for (size_t i = 0; i < nb; ++i) {
        const uint64_t c = blocks->coff[i], end = c + (uint64_t)blocks->csize[i] + 8;      // payload, CRC32, ISIZE
        if (c > n_bytes || end > n_bytes || blocks->isize[i] > 65536u || (i && c < blocks->coff[i - 1] + blocks->csize[i - 1] + 8))
            return fail(ctx, MTH_ERR_INVALID, "BGZF block table does not fit the file bytes");
        ustart[i + 1] = ustart[i] + blocks->isize[i];
    }
    const uint64_t stream = blocks ? ustart[nb] : n_bytes;
    // bounds first: every contig's source span inside the stream, before anything is launched
    std::vector<uint64_t> off((size_t)n_refs + 1, 0), span_hi((size_t)n_refs, 0);
    uint64_t need_lo = ~0ull, need_hi = 0;
    for (int32_t t = 0; t < n_refs; ++t) {
        const mth_fasta_row_t &r = rows[t];
        if (r.n_bases < 0 || (r.n_bases && (r.line_bases <= 0 || r.line_width < r.line_bases))) return fail(ctx, MTH_ERR_INVALID, "mth_tag_set_genome_fasta: a row with a negative length or an impossible line layout");
        off[(size_t)t + 1] = off[(size_t)t] + (uint64_t)r.n_bases;
        if (!r.n_bases) continue;
        const uint64_t last = (uint64_t)r.n_bases - 1;
        const unsigned __int128 e = (unsigned __int128)r.src_off + (unsigned __int128)(last / (uint64_t)r.line_bases) * (uint64_t)r.line_width + last % (uint64_t)r.line_bases + 1;
        if (e > (unsigned __int128)stream) return fail(ctx, MTH_ERR_FORMAT, "FASTA shorter than its index says");
        span_hi[(size_t)t] = (uint64_t)e;
        need_lo = std::min(need_lo, r.src_off); need_hi = std::max(need_hi, (uint64_t)e);
    }
    MTH_ENTER(ctx);
    hipStream_t s = ctx->stream;
    const uint64_t total = off[(size_t)n_refs];
    MTH_HIP(ctx, ctx->fa_genome.reserve((size_t)total + 16, s));
    // the windows: METHEOR_FASTA_CHUNK bytes of the file each (a test knob: windows that end inside lines and contigs), whole blocks
    uint64_t budget = 256ull << 20;
    if (const char *e = getenv("METHEOR_FASTA_CHUNK")) { const long long k = atoll(e); if (k >= 1) budget = (uint64_t)k; }
    budget = std::min<uint64_t>(budget, 2ull << 30);
    std::vector<FaWin> wins;
    if (need_lo < need_hi) {
        if (blocks) {
            for (size_t b0 = 0; b0 < nb;) {
                size_t b1 = b0;
                while (b1 < nb && (b1 == b0 || blocks->coff[b1] + blocks->csize[b1] + 8 - blocks->coff[b0] <= budget)) ++b1;
                wins.push_back(FaWin{ustart[b0], ustart[b1], blocks->coff[b0], blocks->coff[b1 - 1] + blocks->csize[b1 - 1] + 8 - blocks->coff[b0], b0, b1, 0, 0, 0});
                b0 = b1;
            }
        } else {
            for (uint64_t u = need_lo; u < need_hi; u += budget) wins.push_back(FaWin{u, std::min(need_hi, u + budget), u, std::min(need_hi, u + budget) - u, 0, 0, 0, 0, 0});
        }
    }
    // the segments: every contig's span cut at the window borders (contigs in tid order inside a window)
    std::vector<FaSeg> segs;
    {
        std::vector<FaWin> kept;
        for (FaWin w : wins) {
            w.seg0 = segs.size();
            for (int32_t t = 0; t < n_refs; ++t) {
                const mth_fasta_row_t &r = rows[t];
                if (!r.n_bases) continue;
                const uint64_t lo = std::max(r.src_off, w.u0), hi = std::min(span_hi[(size_t)t], w.u1);
                if (lo >= hi) continue;
                FaSeg g{};
                g.win_off = lo - w.u0; g.lay_off = lo - r.src_off; g.n = hi - lo; g.dst = off[(size_t)t];
                g.lb = (uint64_t)r.line_bases; g.lw = (uint64_t)r.line_width; g.tile0 = w.tiles; g.tid = (uint32_t)t;
                w.tiles += (g.win_off + g.n - (g.win_off & ~15ull) + FA_TILE - 1) / FA_TILE;
                segs.push_back(g);
            }
            w.seg1 = segs.size();
            if (w.seg1 > w.seg0) kept.push_back(w);          // a window no wanted contig touches is never copied
        }
        wins.swap(kept);
    }
    for (const FaWin &w : wins) if (w.tiles >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "a FASTA window of more than 2^31 tiles");
    MTH_HIP(ctx, ctx->fa_tab.reserve(64 + segs.size() * sizeof(FaSeg) + 16, s));
    uint32_t *const d_bad = ctx->fa_tab.as<uint32_t>();
    FaSeg *const d_seg = reinterpret_cast<FaSeg *>(ctx->fa_tab.as<uint8_t>() + 64);
    MTH_HIP(ctx, hipMemsetAsync(d_bad, 0xff, 4, s));
    if (!segs.empty()) MTH_HIP(ctx, hipMemcpyAsync(d_seg, segs.data(), segs.size() * sizeof(FaSeg), hipMemcpyHostToDevice, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    const uint8_t *const fb = static_cast<const uint8_t *>(file);
    std::vector<uint64_t> rel;
    int rc = MTH_OK;
    uint32_t bad_tid = FA_NO_TID;
    auto step = [&](size_t wi) -> int {
        const FaWin &w = wins[wi];
        if (wi + 1 < wins.size()) { ctx->next_src = fb + wins[wi + 1].f0; ctx->next_bytes = wins[wi + 1].fn; }     // (mth_bgzf_stage)
        FaArgs a{};
        if (blocks) {
            rel.resize(w.b1 - w.b0);
            for (size_t k = w.b0; k < w.b1; ++k) rel[k - w.b0] = blocks->coff[k] - w.f0;
            uint64_t tot = 0, *d_uoff = nullptr;
            uint32_t *d_isize = nullptr;
            const int r = inflate_blocks(ctx, fb + w.f0, w.fn, rel.data(), blocks->csize + w.b0, blocks->isize + w.b0, w.b1 - w.b0, tot, d_uoff, d_isize);
            if (r) return r;
            a.win = ctx->inf_raw.as<uint8_t>(); a.win_readable = (tot + 15) & ~15ull;           // (inf_raw is reserved with 64 bytes to spare)
        } else {
            bool staged = false;
            int r = stage_take(ctx, fb + w.f0, w.fn, staged);
            if (r) return r;
            if (!staged) MTH_HIP(ctx, hipMemcpyAsync(ctx->inf_file.p, fb + w.f0, (size_t)w.fn, hipMemcpyHostToDevice, s));
            if ((r = stage_start_next(ctx))) return r;
            a.win = ctx->inf_file.as<uint8_t>(); a.win_readable = (w.fn + 15) & ~15ull;         // (inf_file carries INF_FILE_PAD)
        }
        a.seg = d_seg + w.seg0; a.n_seg = (uint32_t)(w.seg1 - w.seg0);
        a.genome = ctx->fa_genome.as<uint8_t>(); a.genome_bytes = total; a.bad_tid = d_bad;
        {
            LaunchTimer lt(ctx, K_FASTA_PACK);
            hipLaunchKernelGGL(k_fasta_pack, dim3((uint32_t)w.tiles), dim3(256), 0, s, a);
        }
        MTH_HIP(ctx, hipGetLastError());
        // the window is done before its buffers are the next copy's: inflate / CRC findings and the error word, per window
        const int r = sync_and_check(ctx);
        if (r) return r;
        MTH_HIP(ctx, hipMemcpy(&bad_tid, d_bad, 4, hipMemcpyDeviceToHost));
        return MTH_OK;
    };
    for (size_t wi = 0; wi < wins.size() && rc == MTH_OK && bad_tid == FA_NO_TID; ++wi) rc = step(wi);
    fa_drain(ctx);
    if (rc != MTH_OK) {
        const std::string why = ctx->last_error;
        (void)hipMemsetAsync(&ctx->d_state->err, 0, 4, s);      // reported: the context stays usable, its genome untouched
        (void)hipStreamSynchronize(s);
        ctx->fa_genome.release();
        return fail(ctx, rc, why.c_str());
    }
    if (bad_tid != FA_NO_TID) {
        ctx->fa_genome.release();
        const char *nm = bad_tid < (uint32_t)n_refs ? rows[bad_tid].name : nullptr;
        const std::string msg = "the FASTA text does not have the line layout its index states (a blank inside a line, lines of other lengths, or an index of another file): " +
                                (nm ? std::string(nm) : "contig #" + std::to_string(bad_tid));
        return fail(ctx, MTH_ERR_FORMAT, msg.c_str());
    }
    // the whole file has passed: the packed genome becomes the context's, and the tail is mth_tag_set_genome's
    std::swap(ctx->tag_genome, ctx->fa_genome);
    ctx->fa_genome.release();
    return genome_commit(ctx, n_refs, off, ref_len);
}
