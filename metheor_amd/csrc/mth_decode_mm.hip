// mth_decode_mm.hip -- the record decode of mth_decode.hip with the CpG calls taken from the SAM base-modification tags
// MM:Z / ML:B:C (/ MN:i) instead of an XM:Z field (mth_decode_set_modtags; `--mm-tags` on the measure commands).
//
// The contract is an equivalence (include/metheor_hip.h): the decoded SoA of a record equals that of
// the same record with its flag reduced to flag & 0x10 and an XM:Z field holding X(record, T) -- the per-record routine is
// mth_modtags_dev.h.  Two forms:
//   direct (METHEOR_MM_STAGED=0)   k_decode_mm<FILL>: one thread per record, count -> scan -> fill as k_decode; the CIGAR walk
//                          steps the MmWalk cursor over every query base (I and S too: the list counts all the read's Cs)
//                          and makes a call where an M / = / X base has a z / Z.  No X string ever exists, but the tags are
//                          parsed and walked twice (count and fill).
//   staged (default)       k_mm_count: l_seq per record -> scan -> k_mm_xm: X of every record into HBM, laid out as
//                          tag_core's strings; k_decode (DecArgs.strand_fwd = 1) reads them from there.  The tags are parsed
//                          once; measured 1.4 x (150 bp) and 1.6 x (5 kbp) faster than the direct form (profiles/modtags.md).
// Roofline: the regime of k_decode -- divergent lanes, each streaming its own record through the L2 / texture path; per 150-bp
// record ~75 B of SEQ, its MM string and ML bytes twice (count and fill), 14 B + 6 B per call out; the ALU work is one short
// iteration per base.  A 5 kbp record is ~2.5 KB of SEQ and a few hundred list numbers walked by ONE lane: the wave waits for
// its longest record (DESIGN.md section 10 keeps a wave-per-record kernel as a lead).  No LDS, no MFMA.
#include "mth_ctx.h"
#include "mth_decode_dev.h"
#include "mth_modtags_dev.h"

namespace mth {

struct MmRec {
    const uint8_t *p;         // the record past block_size
    uint32_t len, l_seq, n_cigar, flag, o_cigar, o_seq, o_aux;
    int32_t tid, pos;
    uint8_t mapq;
    bool bad, longer;
};

__device__ __forceinline__ MmRec mm_record(const DecArgs &a, uint32_t i) {
    MmRec r{};
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    r.p = a.raw + o0 + 4;
    r.len = (uint32_t)(o1 - o0 - 4);
    r.bad = o1 < o0 + 4 + 32 || ld_u32(a.raw + o0) != r.len;
    r.tid = -1;
    if (r.bad) return r;
    r.tid = (int32_t)ld_u32(r.p);
    r.pos = (int32_t)ld_u32(r.p + 4);
    const uint32_t l_read_name = r.p[8];
    r.mapq = r.p[9];
    r.n_cigar = ld_u16(r.p + 12); r.flag = ld_u16(r.p + 14); r.l_seq = ld_u32(r.p + 16);
    const uint64_t o_cigar = 32ull + l_read_name, o_seq = o_cigar + 4ull * r.n_cigar;
    const uint64_t o_aux = o_seq + ((uint64_t)r.l_seq + 1) / 2 + r.l_seq;
    if (o_aux > r.len) { r.bad = true; return r; }
    r.o_cigar = (uint32_t)o_cigar; r.o_seq = (uint32_t)o_seq; r.o_aux = (uint32_t)o_aux;
    r.longer = r.l_seq > 65535u;
    return r;
}

// the findings of mm_prepare as error bits / notes (count pass, or k_mm_xm)
__device__ __forceinline__ void mm_report(const DecArgs &a, const MmPlan &P) {
    if (P.status == MM_ERROR) atomicOr(a.err, (uint32_t)ERRB_MODTAG);
    if (P.status == MM_NOTHING) atomicOr(a.notes, 2u);                   // MTH_NOTE_MODTAG_SKIPPED
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_decode_mm(const DecArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const MmRec r = mm_record(a, i);
    uint32_t n = 0;
    int32_t first = -1, last = -1;
    uint8_t fwd = 0;
    if (r.bad) {
        if (!FILL) atomicOr(a.err, (uint32_t)ERRB_FORMAT);
    } else {
        const bool forward = !(r.flag & 16u);
        fwd = forward ? 1 : 0;
        MmPlan P;
        P.status = MM_DOTS;
        if (r.longer) { if (!FILL) atomicOr(a.err, (uint32_t)ERRB_MODLONG); }
        else {
            mm_prepare(r.p, r.len, r.o_cigar, r.n_cigar, r.o_seq, r.l_seq, r.o_aux, !forward, P);
            if (!FILL) mm_report(a, P);
        }
        const bool walk = P.status == MM_CALLS;
        MmWalk W;
        if (walk) W.init(P, r.p + r.o_seq, r.l_seq, !forward, a.mm_threshold);
        unsigned long long w = FILL ? a.cpg_off[i] : 0ull;
        int64_t ref = r.pos;
        uint64_t q = 0;
        const uint8_t *cg = r.p + r.o_cigar;
        for (uint32_t c = 0; c < r.n_cigar; ++c) {
            const uint32_t cw = ld_u32(cg + 4 * c), op = cw & 15u, ln = cw >> 4;
            if (op == 0 || op == 7 || op == 8) {                              // M = X: query and reference advance
                if (ln) { if (first < 0) first = (int32_t)ref; last = (int32_t)(ref + ln - 1); }
                if (walk) {
                    const uint64_t qe = q + ln < r.l_seq ? q + ln : r.l_seq;    // (SEQ shorter than the query: nothing beyond it)
                    for (uint64_t qq = q; qq < qe; ++qq) {
                        const uint32_t ch = W.step((uint32_t)qq);
                        if (!ch) continue;
                        const int64_t rr = ref + (int64_t)(qq - q);
                        const int32_t ap = forward ? (int32_t)rr : (int32_t)(rr - 1);   // readutil.rs:332 on the strand alone
                        if (a.filt && !in_cpg_set(a.filt, a.n_filt, ((unsigned long long)(uint32_t)r.tid << 32) | (uint32_t)ap)) continue;
                        if (FILL) {
                            a.cpg_pos[w] = ((uint32_t)ap & 0x7fffffffu) | (ch == 2u ? 0x80000000u : 0u);
                            a.cpg_rel[w] = (uint16_t)qq;
                            ++w;
                        }
                        ++n;
                    }
                }
                q += ln; ref += ln;
            } else if (op == 1 || op == 4) {                                  // I, S: query only -- their Cs count in the list
                if (walk) {
                    const uint64_t qe = q + ln < r.l_seq ? q + ln : r.l_seq;
                    for (uint64_t qq = q; qq < qe; ++qq) W.step((uint32_t)qq);
                }
                q += ln;
            } else if (op == 2 || op == 3) {                                  // D, N: reference only
                ref += ln;
            } else if (op == 6 && !FILL) {
                atomicOr(a.notes, 1u);                                        // P: noted as k_decode notes it
            }
        }
    }
    if (!FILL) {
        a.ncpg[i] = n;
        a.tid[i] = r.tid; a.start[i] = first; a.end[i] = last; a.mapq[i] = r.mapq; a.fwd[i] = fwd;
    }
}

// ---- the staged form: X(record, T) as bytes in HBM -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mm_count(const DecArgs a, uint32_t *__restrict__ xm_len) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const MmRec r = mm_record(a, i);
    if (!r.bad && r.longer) atomicOr(a.err, (uint32_t)ERRB_MODLONG);
    xm_len[i] = (r.bad || r.longer) ? 0u : r.l_seq;                           // (a malformed record: k_decode reports it)
}

__global__ __launch_bounds__(256) void k_mm_xm(const DecArgs a, const unsigned long long *__restrict__ xm_off, const uint32_t *__restrict__ xm_len,
                                               uint8_t *__restrict__ xm) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const MmRec r = mm_record(a, i);
    if (r.bad || r.longer) return;
    const bool reverse = r.flag & 16u;
    MmPlan P;
    mm_prepare(r.p, r.len, r.o_cigar, r.n_cigar, r.o_seq, r.l_seq, r.o_aux, reverse, P);
    mm_report(a, P);
    uint8_t *out = xm + xm_off[i];
    if (P.status != MM_CALLS) {
        for (uint32_t q = 0; q < r.l_seq; ++q) out[q] = '.';
        return;
    }
    MmWalk W;
    W.init(P, r.p + r.o_seq, r.l_seq, reverse, a.mm_threshold);
    for (uint32_t q = 0; q < r.l_seq; ++q) {
        const uint32_t ch = W.step(q);
        out[q] = ch == 2u ? 'Z' : (ch == 1u ? 'z' : '.');
    }
}

int decode_mm_pass(mth_ctx *ctx, const DecArgs &a, bool fill) {
    LaunchTimer lt(ctx, K_DECODE_MM);
    const dim3 grid((a.n_rec + 255) / 256);
    if (fill) hipLaunchKernelGGL((k_decode_mm<true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_decode_mm<false>), grid, dim3(256), 0, ctx->stream, a);
    return MTH_OK;
}

int decode_mm_stage(mth_ctx *ctx, DecArgs &a) {
    hipStream_t s = ctx->stream;
    const uint32_t n = a.n_rec, nb = (n + 255) / 256;
    MTH_HIP(ctx, ctx->tag_coloff.reserve(((size_t)n + 1) * 8 + 16, s));
    MTH_HIP(ctx, ctx->tag_xmlen.reserve((size_t)n * 4 + 16, s));
    {
        LaunchTimer lt(ctx, K_MM_XM);
        hipLaunchKernelGGL(k_mm_count, dim3(nb), dim3(256), 0, s, a, ctx->tag_xmlen.as<uint32_t>());
    }
    unsigned long long total = 0;
    const int rc = scan_u32_to_u64(ctx, ctx->tag_xmlen.as<uint32_t>(), n, 0ull, ctx->tag_coloff.as<unsigned long long>(), &total);   // synchronises
    if (rc) return rc;
    MTH_HIP(ctx, ctx->tag_xm.reserve((size_t)total + 16, s));
    {
        LaunchTimer lt(ctx, K_MM_XM);
        hipLaunchKernelGGL(k_mm_xm, dim3(nb), dim3(256), 0, s, a, ctx->tag_coloff.as<unsigned long long>(), ctx->tag_xmlen.as<uint32_t>(),
                           ctx->tag_xm.as<uint8_t>());
    }
    MTH_HIP(ctx, hipGetLastError());
    a.xm_base = ctx->tag_xm.as<uint8_t>(); a.xm_off = ctx->tag_coloff.as<unsigned long long>(); a.xm_lens = ctx->tag_xmlen.as<uint32_t>();
    return MTH_OK;
}

}  // namespace mth
