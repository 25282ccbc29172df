// mth_decode_genome.hip -- the record decode of mth_decode.hip with the CpG calls derived from the reference genome instead
// of an XM:Z field (mth_decode_set_genome; `--genome` on the measure commands).
//
// Computes, per record, what `metheor tag` followed by the decode computes: determine_xm_tag_string (tag.rs:130-384) gives a
// letter per M / I base, get_cpgs (readutil.rs:323-345) zips that string with the query offsets of the aligned bases and keeps
// the z / Z.  The composition keeps the reference's quirks: tag.rs:186-237 walks M, I and D only, so behind a soft clip, an
// `=` / X run or an N skip the letter the decode reads at query offset q was computed for SEQ[q] against genome[pos + q] --
// not for the base that is aligned there.  Nothing here "fixes" that: the result has to equal the two-step run's.
//
// Only z / Z reach the decode, and for a PLAIN record -- every CIGAR operation M, S or H, SEQ at least as long as the M runs
// together (m bases) -- they need no columns at all: column t is SEQ[t] against genome[pos + t], t < m, without a gap, so
// the deletion branch of tag.rs:268-270 cannot be taken (the only '-' read columns are the flanks, and the two indices that
// could see them are the ones its condition excludes).  A letter is then Z / z exactly when
//   read not reverse-complemented: genome[p] = C, genome[p + 1] = G, SEQ[t] = C (Z) or T (z)
//   reverse-complemented:          genome[p] = G, genome[p - 1] = C, SEQ[t] = G (Z) or A (z)
// with p = pos + t, the genome upper-cased and N outside the bases the contig has (tag.rs:155-172).  Both cases are the
// dinucleotide CG at P = p (resp. p - 1): the span is searched for it sixteen genome bytes a load, SEQ nibbles are touched at
// hits only.  What tag.rs does besides and a plain record still has to carry:
//   * the range checks of tag.rs:155-170 (unplaced, outside the contig or the bases the FASTA gave): the reference panics;
//   * on a reverse-complemented read EVERY character of the two strings goes through the complement table (tag.rs:19-25)
//     and one outside it is a panic although no letter depends on it: '=' in SEQ, a stray character in the FASTA;
//   * a reference C whose context is none of tag.rs:334-372's -- an IUPAC code or a stray character after it, no N beside --
//     gets NO letter: the string is one short and every later letter is read one query offset early.  So a record whose
//     reference span [start - 2, end + 2) holds anything but A C G T N (either case) is not treated as plain: it takes the
//     column walk, which also settles whether that character is a panic.
// Every other record (I, D, N, =, X, P, SEQ shorter than its CIGAR) takes the exact column walk of mth_tag_dev.h into
// per-record scratch sized by the count pass (zero for plain records: a file of plain records allocates none), and the
// decode then reads the letters from there.
//
// One thread per record, count -> scan -> fill as k_decode.  Roofline: the same regime as k_decode (divergent lanes, each
// streaming its own record: L2 / texture path round trips, not ALUs); per 150-bp record ~60 B of record core + CIGAR, the
// ~152 B genome span (coordinate-sorted neighbours overlap: L2 hits) and a SEQ nibble per hit in, 14 B + 6 B per call out.
// No LDS, no MFMA.
#include "mth_ctx.h"
#include "mth_decode_dev.h"
#include "mth_tag_dev.h"

namespace mth {

struct GenArgs {
    DecArgs d;
    TagArgs t;      // raw / off / n_rec as d; genome, contig table, paired flag; ncol (0: a plain record), col_off, cols, xm, xm_len
};

// 0x80 in every byte of v that is zero, exactly (no carry between bytes)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) { return ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu); }

// 0x80 in every byte of x that is none of A C G T N in either case
__device__ __forceinline__ uint32_t not_acgtn(uint32_t x) {
    const uint32_t u = x & 0xdfdfdfdfu;
    return ~(zero_bytes(u ^ 0x41414141u) | zero_bytes(u ^ 0x43434343u) | zero_bytes(u ^ 0x47474747u) | zero_bytes(u ^ 0x54545454u) |
             zero_bytes(u ^ 0x4e4e4e4eu)) & 0x80808080u;
}

enum { GEN_PANIC = 0, GEN_PLAIN = 1, GEN_WALK = 2 };

template <bool FILL>
struct CallSink {
    const DecArgs &a;
    int32_t tid;
    bool forward;
    unsigned long long w;
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(uint32_t q, int64_t r, bool meth) {
        const int32_t ap = forward ? (int32_t)r : (int32_t)(r - 1);        // readutil.rs:332
        if (a.filt && !in_cpg_set(a.filt, a.n_filt, ((unsigned long long)(uint32_t)tid << 32) | (uint32_t)ap)) return;
        if (FILL) {
            a.cpg_pos[w] = ((uint32_t)ap & 0x7fffffffu) | (meth ? 0x80000000u : 0u);
            a.cpg_rel[w] = (uint16_t)q;
            ++w;
        }
        ++n;
    }
};

// get_cpgs over a letter string (what k_decode does with an XM:Z field), for the few records that took the column walk
template <bool FILL>
__device__ __forceinline__ uint32_t gen_walk_letters(const DecArgs &a, const TagRec &r, int32_t tid, bool forward, unsigned long long w,
                                                  const uint8_t *xm, uint32_t xm_len) {
    CallSink<FILL> call{a, tid, forward, w};
    int64_t ref = r.pos;
    uint32_t q = 0;
    for (uint32_t c = 0; c < r.n_cigar; ++c) {
        const uint32_t cw = tg_u32(r.cigar + 4 * c), op = cw & 15u, ln = cw >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const uint32_t qe = min(q + ln, xm_len);                         // (a string shorter than the query: nothing beyond it)
            for (uint32_t qq = q; qq < qe; ++qq) {
                const uint8_t ch = xm[qq];
                if (ch == 'z' || ch == 'Z') call(qq, ref + (qq - q), ch == 'Z');
            }
            q += ln; ref += ln;
        } else if (op == 1 || op == 4) q += ln;
        else if (op == 2 || op == 3) ref += ln;
    }
    return call.n;
}

// the plain-record rule (file header) -> GEN_PLAIN; GEN_PANIC = the reference panics on this record; GEN_WALK (count pass
// only) = its reference span holds a character that can cost a letter, the column walk has to take it
template <bool FILL>
__device__ __forceinline__ int gen_plain(const GenArgs &a, const TagRec &r, uint32_t m, bool forward, unsigned long long w, uint32_t &n_out) {
    const TagArgs &t = a.t;
    n_out = 0;
    if (r.tid < 0 || r.tid >= t.n_refs) return GEN_PANIC;                    // tag.rs:155 tid2size[&tid]
    const int64_t start = r.pos, end = start + (m ? m : 1u);                 // htslib bam_endpos
    const bool is_rev = r.flag & 16u, first = r.flag & 64u, last = r.flag & 128u;
    const bool rc = t.paired ? !((!is_rev && first) || (is_rev && last)) : is_rev;
    const int64_t ln = t.g_ln[r.tid], have = (int64_t)(t.g_off[r.tid + 1] - t.g_off[r.tid]);
    const int64_t cs = start - 2 > 0 ? start - 2 : 0, ce = end + 2 < ln ? end + 2 : ln;
    if (start < 0 || cs > ce || ce > have || end > ln) return GEN_PANIC;     // tag.rs:158-170
    const uint8_t *g = t.genome + t.g_off[r.tid];
    auto gat = [&](int64_t p) -> uint8_t { return (p < 0 || p >= ce) ? (uint8_t)'N' : tg_up(g[p]); };
    if (!FILL) {
        uint32_t odd = 0;                                                    // anything but A C G T N in [cs, ce): not a plain record
        int64_t p = cs;
        for (; p + 4 <= ce; p += 4) odd |= not_acgtn(ld_u32(g + p));
        for (; p < ce; ++p) odd |= not_acgtn(0x41414100u | g[p]);
        if (odd) return GEN_WALK;
    }
    if (!FILL && rc) {
        // tag.rs:246-256: reverse_complement() maps the two flank columns and all m columns of both strings.  The reference
        // bases are A C G T N here, all in the table; '=' (nibble 0) is the one SEQ code without a complement
        uint32_t bad = 0, b = 0;
        for (; 2u * (b + 4u) <= m; b += 4) {
            const uint32_t x = ld_u32(r.seq + b);
            bad |= zero_bytes(x & 0x0f0f0f0fu) | zero_bytes((x >> 4) & 0x0f0f0f0fu);
        }
        for (uint32_t k = 2u * b; k < m; ++k) bad |= ((r.seq[k >> 1] >> ((k & 1u) ? 0 : 4)) & 15u) ? 0u : 1u;
        if (bad) return GEN_PANIC;
    }
    CallSink<FILL> call{a.d, r.tid, forward, w};
    const int64_t shift = rc ? 1 : 0;                                        // t = P + shift - start for the dinucleotide at P
    const uint32_t zcode = rc ? 4u : 2u, ucode = rc ? 1u : 8u;               // "=ACMGRSVTWYHKDBN": G / A on a reverse-complemented read, C / T
    auto hit = [&](int64_t P, uint32_t q, int64_t ref) {
        const uint32_t tt = (uint32_t)(P + shift - start);
        const uint32_t nib = (r.seq[tt >> 1] >> ((tt & 1u) ? 0 : 4)) & 15u;
        if (nib == zcode || nib == ucode) call(tt, ref + (tt - q), nib == zcode);
    };
    // the decode's walk (readutil.rs:323-345): S advances the query only, H nothing; an M run of the query offsets [q, q + ln)
    // reads the letters of the columns with the same numbers, of which there are m
    int64_t ref = r.pos;
    uint32_t q = 0;
    for (uint32_t c = 0; c < r.n_cigar; ++c) {
        const uint32_t cw = tg_u32(r.cigar + 4 * c), op = cw & 15u, len = cw >> 4;
        if (op == 4u) { q += len; continue; }
        if (op != 0u) continue;
        const uint32_t te = min(q + len, m);
        if (q < te) {
            int64_t P = start + q - shift;
            const int64_t P1 = start + te - shift;
            // sixteen genome bytes a load give the fifteen dinucleotides that start in the first fifteen; most windows hold no CG
            for (; P >= 0 && P + 16 <= ce && P + 15 <= P1; P += 15) {
                const u32x4_a1 x4 = *reinterpret_cast<const u32x4_a1 *>(g + P);
                const uint32_t u[4] = {x4.x & 0xdfdfdfdfu, x4.y & 0xdfdfdfdfu, x4.z & 0xdfdfdfdfu, x4.w & 0xdfdfdfdfu};   // c -> C, g -> G; nothing else becomes C / G
                uint32_t zc[4], zg[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { zc[j] = zero_bytes(u[j] ^ 0x43434343u); zg[j] = zero_bytes(u[j] ^ 0x47474747u); }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t h = zc[j] & ((zg[j] >> 8) | (j < 3 ? zg[(j + 1) & 3] << 24 : 0u));
                    while (h) {
                        hit(P + 4 * j + (__builtin_ctz(h) >> 3), q, ref);
                        h &= h - 1u;
                    }
                }
            }
            for (; P < P1; ++P)
                if (gat(P) == 'C' && gat(P + 1) == 'G') hit(P, q, ref);
        }
        q += len; ref += len;
    }
    n_out = call.n;
    return GEN_PLAIN;
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_decode_genome(const GenArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.d.n_rec) return;
    const TagRec r = tg_parse(a.t, i);
    uint32_t n = 0, ncol = 0;
    int32_t tid = -1, first = -1, last = -1;
    uint8_t mapq = 0, fwd = 0;
    if (r.bad) {
        if (!FILL) atomicOr(a.d.err, (uint32_t)ERRB_FORMAT);
    } else {
        tid = r.tid;
        mapq = a.t.raw[a.t.off[i] + 4 + 9];
        const bool forward = r.flag == 0u || r.flag == 99u || r.flag == 147u;   // readutil.rs:332
        fwd = forward ? 1 : 0;
        // start / end as k_decode; the CIGAR's class; the columns tag.rs would build (M, I, D + the four flanks)
        int64_t ref = r.pos;
        uint64_t m = 0, cols = 4;
        bool plain = true;
        for (uint32_t c = 0; c < r.n_cigar; ++c) {
            const uint32_t cw = tg_u32(r.cigar + 4 * c), op = cw & 15u, ln = cw >> 4;
            if (op == 0u || op == 7u || op == 8u) {
                if (ln) { if (first < 0) first = (int32_t)ref; last = (int32_t)(ref + ln - 1); }
                ref += ln;
            } else if (op == 2u || op == 3u) ref += ln;
            if (op == 0u) m += ln;
            if (op <= 2u) cols += ln;
            if (op != 0u && op != 4u && op != 5u) plain = false;
            if (op == 6u && !FILL) atomicOr(a.d.notes, 1u);                     // P: noted as k_decode notes it
        }
        if (cols >= (1ull << 31)) {
            if (!FILL) atomicOr(a.d.err, (uint32_t)ERRB_FORMAT);
        } else if (FILL ? a.t.ncol[i] == 0u : (plain && m <= r.l_seq)) {
            const int how = gen_plain<FILL>(a, r, (uint32_t)m, forward, FILL ? a.d.cpg_off[i] : 0ull, n);
            if (!FILL && how == GEN_PANIC) atomicOr(a.d.err, (uint32_t)ERRB_TAGPANIC);
            if (!FILL && how == GEN_WALK) ncol = (uint32_t)cols;             // as any record that is not plain
        } else if (FILL) {
            n = gen_walk_letters<true>(a.d, r, tid, forward, a.d.cpg_off[i], a.t.xm + a.t.col_off[i], a.t.xm_len[i]);
        } else {
            ncol = (uint32_t)cols;                                           // k_genome_columns counts this record's calls
        }
    }
    if (!FILL) {
        a.t.ncol[i] = ncol;
        a.d.ncpg[i] = n;
        a.d.tid[i] = tid; a.d.start[i] = first; a.d.end[i] = last; a.d.mapq[i] = mapq; a.d.fwd[i] = fwd;
    }
}

// the records the count pass left to the column walk: tag.rs's columns and letters into the record's scratch slice, then the
// number of calls the decode takes from them
__global__ __launch_bounds__(256) void k_genome_columns(const GenArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.d.n_rec) return;
    const uint32_t ncol = a.t.ncol[i];
    if (ncol == 0u) return;
    const TagRec r = tg_parse(a.t, i);
    uint8_t *R = a.t.cols + a.t.col_off[i], *G = R + a.t.total, *xm = a.t.xm + a.t.col_off[i];
    const int64_t nx = tg_xm_record(a.t, r, ncol, R, G, xm);
    if (nx < 0) { a.t.xm_len[i] = 0; atomicOr(a.d.err, (uint32_t)ERRB_TAGPANIC); return; }
    a.t.xm_len[i] = (uint32_t)nx;
    // the thread reads its own letters back
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const bool forward = r.flag == 0u || r.flag == 99u || r.flag == 147u;
    a.d.ncpg[i] = gen_walk_letters<false>(a.d, r, r.tid, forward, 0ull, xm, (uint32_t)nx);
}

static GenArgs gen_args(mth_ctx *ctx, const DecArgs &d) {
    GenArgs a{};
    a.d = d;
    a.t.raw = d.raw; a.t.off = d.off; a.t.n_rec = d.n_rec;
    a.t.genome = ctx->tag_genome.as<uint8_t>(); a.t.g_off = ctx->tag_goff.as<uint64_t>();
    a.t.g_ln = reinterpret_cast<const int64_t *>(ctx->tag_goff.as<uint64_t>() + ctx->tag_n_refs + 1);
    a.t.n_refs = ctx->tag_n_refs; a.t.paired = ctx->dec_genome_paired ? 1 : 0;
    a.t.ncol = ctx->tag_ncol.as<uint32_t>(); a.t.xm_len = ctx->tag_xmlen.as<uint32_t>(); a.t.err = d.err;
    a.t.col_off = ctx->tag_coloff.as<unsigned long long>(); a.t.cols = ctx->tag_cols.as<uint8_t>(); a.t.xm = ctx->tag_xm.as<uint8_t>();
    return a;
}

int decode_genome_count(mth_ctx *ctx, const DecArgs &d) {
    hipStream_t s = ctx->stream;
    const uint32_t n = d.n_rec, nb = (n + 255) / 256;
    MTH_HIP(ctx, ctx->tag_ncol.reserve((size_t)n * 4 + 16, s));
    MTH_HIP(ctx, ctx->tag_coloff.reserve(((size_t)n + 1) * 8 + 16, s));
    MTH_HIP(ctx, ctx->tag_xmlen.reserve((size_t)n * 4 + 16, s));
    GenArgs a = gen_args(ctx, d);
    {
        LaunchTimer lt(ctx, K_DECODE_GENOME);
        hipLaunchKernelGGL((k_decode_genome<false>), dim3(nb), dim3(256), 0, s, a);
    }
    unsigned long long total = 0;
    const int rc = scan_u32_to_u64(ctx, a.t.ncol, n, 0ull, ctx->tag_coloff.as<unsigned long long>(), &total);   // synchronises; surfaces panics
    if (rc) return rc;
    ctx->tag_cols_total = total;
    if (total) {
        MTH_HIP(ctx, ctx->tag_cols.reserve((size_t)total * 2 + 16, s));
        MTH_HIP(ctx, ctx->tag_xm.reserve((size_t)total + 16, s));
        a = gen_args(ctx, d);
        a.t.total = total;
        LaunchTimer lt(ctx, K_DECODE_GENOME);
        hipLaunchKernelGGL(k_genome_columns, dim3(nb), dim3(256), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    return MTH_OK;
}

int decode_genome_fill(mth_ctx *ctx, const DecArgs &d) {
    GenArgs a = gen_args(ctx, d);
    a.t.total = ctx->tag_cols_total;
    LaunchTimer lt(ctx, K_DECODE_GENOME);
    hipLaunchKernelGGL((k_decode_genome<true>), dim3((d.n_rec + 255) / 256), dim3(256), 0, ctx->stream, a);
    return MTH_OK;
}

}  // namespace mth
