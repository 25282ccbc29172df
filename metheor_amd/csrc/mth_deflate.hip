// mth_deflate.hip -- BGZF blocks on the device: the write direction of mth_inflate.hip (`tag -O bam`, mth_bgzf_deflate).
//
// k_deflate: one workgroup of 256 threads (four waves) per BGZF block of at most 0xff00 bytes, RFC 1951:
//   a. LZ77: the block is taken in segments of 256 positions, one per thread.  A position looks its 3-byte hash up in an LDS table
//      of the latest position per hash -- which holds EARLIER segments only -- and also tries distance 1 (runs); the segment's
//      positions are inserted with atomicMax after the barrier.  What a position finds therefore depends on the bytes alone, never
//      on which wave came first: the output is a function of the input.  Match 3..258, distance <= 32768 (a length-3 match further
//      than 4096 away costs more than its literals and is dropped, as zlib does).  Nothing before the block is a dictionary.
//   b. greedy parse: next = i + max(1, len[i]) is a serial chain; one lane walks the segment's 256 lengths in LDS while the other
//      lanes insert the hashes, and lists the chosen positions; the lanes then emit those tokens (32-bit words in HBM scratch) and
//      count their symbols in LDS histograms.
//   c. three forms are costed exactly and the smallest is written: dynamic Huffman (BTYPE 10), fixed (01), stored (00), so a payload
//      never exceeds isize + 5 and BSIZE fits its 16 bits.
//   d. Huffman lengths: rank sort of the used symbols (all lanes), two-queue merge (one lane); a code deeper than the limit (15; 7
//      for the code-length code) is rebuilt from halved frequencies until it fits -- every round is a true Huffman tree, so the
//      code is always complete and never over-subscribed.  At least two symbols per code (zlib does the same).  The code-length
//      sequence is sent plain (symbols 0..15 only).
//   e. packing: bit length per token, prefix sum over the lanes' chunks of the token list, every lane packs its chunk from its bit
//      offset into the zeroed slot of the block, whole 32-bit words at a time with atomicOr (neighbouring chunks share a word).
//   f. framing: the 18-byte gzip header with the BC subfield, CRC32 (k_crc32, mth_inflate.hip) and ISIZE; k_bgzf_compact then
//      moves the blocks' slots to one contiguous buffer at the prefix sum of their sizes.
// The block body is written as phases between barriers (DF_PHASE ... DF_SYNC) over LDS state only, so the same text compiles as
// a host model (MTH_DEFLATE_HOST_MODEL: a phase is a loop over the 256 lanes), which is how the format logic is exercised without
// a device.
#ifndef MTH_DEFLATE_HOST_MODEL
#include "mth_bgzf_cuts.h"
#include "mth_ctx.h"
#define DF_DEV __device__ __forceinline__
#define DF_PHASE for (uint32_t t = threadIdx.x, once_ = 1; once_; once_ = 0)
#define DF_SYNC __syncthreads()
#define DF_SYNC_GLOBAL do { __threadfence(); __syncthreads(); } while (0)
#define DF_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define DF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define DF_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#include <stdint.h>
#define DF_DEV static inline
#define DF_PHASE for (uint32_t t = 0; t < DF_NT; ++t)
#define DF_SYNC do { } while (0)
#define DF_SYNC_GLOBAL do { } while (0)
#define DF_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define DF_ATOMIC_ADD(p, v) (*(p) += (v))
#define DF_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

namespace mth {

constexpr uint32_t DF_NT = 256;                 // threads per block = positions per segment
constexpr uint32_t DF_HASH_BITS = 13;
constexpr uint32_t DF_MAX_IN = 0xff00u;
constexpr uint32_t DF_SLOT = 65536;             // bytes per block slot: 18 + (0xff00 + 5) + 8 fits
constexpr uint32_t DF_NLL = 286, DF_ND = 30, DF_NCL = 19;

struct DfLds {
    uint32_t tab[1u << DF_HASH_BITS];           // hash -> latest position + 1 (0: none), earlier segments only
    uint32_t ll_hist[288], d_hist[32], cl_hist[20];
    uint32_t wfreq[288], nfreq[288];            // code construction: working frequencies, internal nodes' weights
    uint32_t part[DF_NT];                       // packing: bits per lane chunk -> bit offsets
    uint16_t s_len[DF_NT], s_dist[DF_NT], sel[DF_NT];
    uint16_t order[288], lpar[288], ipar[288], idep[288];
    uint16_t ll_code[288], d_code[32], cl_code[20];
    uint8_t ll_len[288], d_len[32], cl_len[20];
    uint32_t cur, ntok, cnt, m, maxlen, form, hdr_bits, hlit, hdist, pay_bytes;
};

DF_DEV uint32_t df_ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
DF_DEV uint32_t df_hash(const uint8_t *p) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return (v * 0x9e3779b1u) >> (32 - DF_HASH_BITS);
}
// common prefix of s[a ..] and s[b ..], at most maxl bytes (a < b; a + maxl and b + maxl stay inside the block)
DF_DEV uint32_t df_match(const uint8_t *s, uint32_t a, uint32_t b, uint32_t maxl) {
    uint32_t k = 0;
    while (k + 4 <= maxl) {
        const uint32_t x = df_ld32(s + a + k) ^ df_ld32(s + b + k);
        if (x) return k + ((uint32_t)__builtin_ctz(x) >> 3);
        k += 4;
    }
    while (k < maxl && s[a + k] == s[b + k]) ++k;
    return k;
}
DF_DEV uint32_t df_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
// length 3..258 -> literal/length symbol, extra bits, extra value
DF_DEV uint32_t df_len_sym(uint32_t len, uint32_t &eb, uint32_t &ev) {
    const uint32_t x = len - 3;
    eb = 0; ev = 0;
    if (x < 8) return 257 + x;
    if (x == 255) return 285;
    const uint32_t e = df_log2(x) - 2;
    eb = e; ev = x & ((1u << e) - 1);
    return 261 + 4 * e + ((x - (1u << (e + 2))) >> e);
}
// distance 1..32768 -> distance symbol, extra bits, extra value
DF_DEV uint32_t df_dist_sym(uint32_t dist, uint32_t &eb, uint32_t &ev) {
    const uint32_t y = dist - 1;
    eb = 0; ev = 0;
    if (y < 4) return y;
    const uint32_t e = df_log2(y) - 1;
    eb = e; ev = y & ((1u << e) - 1);
    return 2 * e + 2 + ((y >> e) & 1u);
}
DF_DEV uint32_t df_ll_extra(uint32_t s) { return (s < 265 || s == 285) ? 0u : (s - 261) >> 2; }
DF_DEV uint32_t df_d_extra(uint32_t s) { return s < 4 ? 0u : (s >> 1) - 1; }
DF_DEV uint32_t df_fixed_len(uint32_t s) { return s < 144 ? 8u : (s < 256 ? 9u : (s < 280 ? 7u : 8u)); }
DF_DEV uint32_t df_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// bit writer into a zeroed slot: whole words leave with atomicOr (the first and the last word of a lane's chunk are shared)
struct DfBits {
    uint32_t *w;
    uint32_t word, nb;
    uint64_t acc;
};
DF_DEV DfBits df_bits_at(uint32_t *w, uint32_t bitpos) { DfBits b; b.w = w; b.word = bitpos >> 5; b.nb = bitpos & 31u; b.acc = 0; return b; }
DF_DEV void df_put(DfBits &b, uint32_t v, uint32_t n) {          // n <= 32, v < 2^n
    b.acc |= (uint64_t)v << b.nb;
    b.nb += n;
    if (b.nb >= 32) {
        if ((uint32_t)b.acc) DF_ATOMIC_OR(b.w + b.word, (uint32_t)b.acc);
        ++b.word; b.acc >>= 32; b.nb -= 32;
    }
}
DF_DEV void df_flush(DfBits &b) {
    if (b.nb && (uint32_t)b.acc) DF_ATOMIC_OR(b.w + b.word, (uint32_t)b.acc);
    b.nb = 0; b.acc = 0;
}

// canonical code of the lengths len[0 .. n) (RFC 1951 3.2.2), stored bit-reversed: the packer writes LSB first.  One lane.
DF_DEV void df_canonical(const uint8_t *len, uint32_t n, uint16_t *code) {
    uint32_t cnt[16], next[16];
    for (uint32_t i = 0; i < 16; ++i) cnt[i] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[len[s]];
    cnt[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (uint32_t b = 1; b < 16; ++b) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
    for (uint32_t s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)df_rev(next[len[s]]++, len[s]) : (uint16_t)0;
}

// code lengths of hist[0 .. n), none above `limit`, into out_len; every lane calls it
DF_DEV void df_build(DfLds &L, const uint32_t *hist, uint32_t n, uint32_t limit, uint8_t *out_len) {
    DF_PHASE { for (uint32_t s = t; s < n; s += DF_NT) { L.wfreq[s] = hist[s]; out_len[s] = 0; } }
    DF_SYNC;
    DF_PHASE {
        if (t == 0) {
            uint32_t m = 0;
            for (uint32_t s = 0; s < n; ++s) m += L.wfreq[s] != 0;
            for (uint32_t s = 0; m < 2 && s < n; ++s) if (!L.wfreq[s]) { L.wfreq[s] = 1; ++m; }      // a decoder wants two codes
            L.m = m;
        }
    }
    DF_SYNC;
    for (;;) {
        DF_PHASE {                                             // rank of a used symbol among the used ones by (weight, symbol)
            for (uint32_t s = t; s < n; s += DF_NT) {
                const uint32_t f = L.wfreq[s];
                if (!f) continue;
                uint32_t r = 0;
                for (uint32_t q = 0; q < n; ++q) { const uint32_t g = L.wfreq[q]; r += g && (g < f || (g == f && q < s)); }
                L.order[r] = (uint16_t)s;
            }
        }
        DF_SYNC;
        DF_PHASE {
            if (t == 0) {
                const uint32_t m = L.m;
                uint32_t li = 0, ii = 0;
                for (uint32_t nn = 0; nn + 1 < m; ++nn) {       // two-queue merge: leaves in rank order, internal nodes in creation order
                    uint32_t w = 0;
                    for (int k = 0; k < 2; ++k) {
                        if (li < m && (ii >= nn || L.wfreq[L.order[li]] <= L.nfreq[ii])) { w += L.wfreq[L.order[li]]; L.lpar[li++] = (uint16_t)nn; }
                        else { w += L.nfreq[ii]; L.ipar[ii++] = (uint16_t)nn; }
                    }
                    L.nfreq[nn] = w;
                }
                L.idep[m - 2] = 0;
                for (uint32_t j = m - 2; j-- > 0;) L.idep[j] = (uint16_t)(L.idep[L.ipar[j]] + 1);
                uint32_t mx = 0;
                for (uint32_t k = 0; k < m; ++k) { const uint32_t d = L.idep[L.lpar[k]] + 1u; mx = d > mx ? d : mx; }
                L.maxlen = mx;
                if (mx <= limit) for (uint32_t k = 0; k < m; ++k) out_len[L.order[k]] = (uint8_t)(L.idep[L.lpar[k]] + 1u);
                else for (uint32_t s = 0; s < n; ++s) L.wfreq[s] = (L.wfreq[s] + 1) >> 1;
            }
        }
        DF_SYNC;
        if (L.maxlen <= limit) break;
    }
    DF_SYNC;
}

// the code-length code's transmission order (RFC 1951 3.2.7)
DF_DEV uint32_t df_cl_order(uint32_t i) {
    const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// One BGZF block: src[0 .. n) -> slot (DF_SLOT bytes, 4-byte aligned), returns nothing; lane 0 leaves the block's size in
// L.pay_bytes + 26.  tok: n words of scratch.  Every lane of the workgroup calls it.
DF_DEV void df_block(DfLds &L, const uint8_t *src, uint32_t n, uint32_t *slot, uint32_t *tok, uint32_t crc) {
    DF_PHASE {
        for (uint32_t i = t; i < (1u << DF_HASH_BITS); i += DF_NT) L.tab[i] = 0;
        for (uint32_t i = t; i < 288; i += DF_NT) L.ll_hist[i] = 0;
        if (t < 32) L.d_hist[t] = 0;
        if (t < 20) L.cl_hist[t] = 0;
        if (t == 0) { L.cur = 0; L.ntok = 0; L.cnt = 0; }
        const uint32_t words = (18 + n + 5 + 8 + 3) / 4 + 1;      // everything any of the three forms writes
        for (uint32_t i = t; i < words; i += DF_NT) slot[i] = 0;
    }
    DF_SYNC_GLOBAL;
    // a + b: matches, greedy parse, tokens, histograms -- segment by segment
    for (uint32_t base = 0; base < n; base += DF_NT) {
        DF_PHASE {
            if (t == 0) L.ntok += L.cnt;                       // (the previous segment's tokens)
            const uint32_t p = base + t;
            uint32_t len = 0, dist = 0;
            if (p + 3 <= n) {
                const uint32_t maxl = n - p < 258 ? n - p : 258;
                const uint32_t c = L.tab[df_hash(src + p)];
                if (c && p - (c - 1) <= 32768) {
                    const uint32_t l = df_match(src, c - 1, p, maxl);
                    if (l >= 3 && !(l == 3 && p - (c - 1) > 4096)) { len = l; dist = p - (c - 1); }
                }
                if (p >= 1 && len < maxl && src[p - 1] == src[p]) {
                    const uint32_t l = df_match(src, p - 1, p, maxl);
                    if (l >= 3 && l >= len) { len = l; dist = 1; }
                }
            }
            L.s_len[t] = (uint16_t)len; L.s_dist[t] = (uint16_t)(dist - (dist != 0));       // stored as distance - 1
        }
        DF_SYNC;
        DF_PHASE {
            const uint32_t p = base + t;
            if (p + 3 <= n) DF_ATOMIC_MAX(&L.tab[df_hash(src + p)], p + 1);
            if (t == 0) {                                      // the chain of the greedy parse through this segment
                uint32_t cur = L.cur, cnt = 0;
                const uint32_t end = base + DF_NT < n ? base + DF_NT : n;
                while (cur < end) {
                    const uint32_t i = cur - base, l = L.s_len[i];
                    L.sel[cnt++] = (uint16_t)i;
                    cur += l ? l : 1;
                }
                L.cur = cur; L.cnt = cnt;
            }
        }
        DF_SYNC;
        DF_PHASE {
            if (t < L.cnt) {
                const uint32_t i = L.sel[t], l = L.s_len[i];
                uint32_t word, eb, ev;
                if (l) {
                    const uint32_t d1 = L.s_dist[i];
                    word = 0x80000000u | (l - 3) | (d1 << 8);
                    DF_ATOMIC_ADD(&L.ll_hist[df_len_sym(l, eb, ev)], 1u);
                    DF_ATOMIC_ADD(&L.d_hist[df_dist_sym(d1 + 1, eb, ev)], 1u);
                } else {
                    word = src[base + i];
                    DF_ATOMIC_ADD(&L.ll_hist[word], 1u);
                }
                tok[L.ntok + t] = word;
            }
        }
        DF_SYNC;
    }
    DF_PHASE { if (t == 0) { L.ntok += L.cnt; L.cnt = 0; L.ll_hist[256] = 1; } }
    DF_SYNC;
    // d: the three codes
    df_build(L, L.ll_hist, DF_NLL, 15, L.ll_len);
    df_build(L, L.d_hist, DF_ND, 15, L.d_len);
    DF_PHASE {
        if (t == 0) {
            uint32_t hlit = DF_NLL, hdist = DF_ND;
            while (hlit > 257 && !L.ll_len[hlit - 1]) --hlit;
            while (hdist > 1 && !L.d_len[hdist - 1]) --hdist;
            L.hlit = hlit; L.hdist = hdist;
            for (uint32_t s = 0; s < hlit; ++s) ++L.cl_hist[L.ll_len[s]];
            for (uint32_t s = 0; s < hdist; ++s) ++L.cl_hist[L.d_len[s]];
        }
    }
    DF_SYNC;
    df_build(L, L.cl_hist, DF_NCL, 7, L.cl_len);
    // c: the three forms' exact sizes
    DF_PHASE {
        if (t == 0) {
            uint32_t dyn = 3 + 14 + 3 * DF_NCL, fix = 3;
            for (uint32_t s = 0; s < L.hlit; ++s) dyn += L.cl_len[L.ll_len[s]];
            for (uint32_t s = 0; s < L.hdist; ++s) dyn += L.cl_len[L.d_len[s]];
            for (uint32_t s = 0; s < DF_NLL; ++s) {
                dyn += L.ll_hist[s] * (L.ll_len[s] + df_ll_extra(s));
                fix += L.ll_hist[s] * (df_fixed_len(s) + df_ll_extra(s));
            }
            for (uint32_t s = 0; s < DF_ND; ++s) {
                dyn += L.d_hist[s] * (L.d_len[s] + df_d_extra(s));
                fix += L.d_hist[s] * (5 + df_d_extra(s));
            }
            const uint32_t dyn_b = (dyn + 7) / 8, fix_b = (fix + 7) / 8, sto_b = n + 5;
            uint32_t form = 2, best = dyn_b;
            if (fix_b <= best) { form = 1; best = fix_b; }
            if (sto_b <= best) { form = 0; best = sto_b; }
            L.form = form; L.pay_bytes = best;
        }
    }
    DF_SYNC;
    if (L.form == 0) {
        DF_PHASE {
            if (t == 0) {
                DfBits b = df_bits_at(slot, 18 * 8);
                df_put(b, 1, 8);                               // BFINAL, BTYPE 00, padding to the byte
                df_put(b, n, 16); df_put(b, ~n & 0xffffu, 16);
                df_flush(b);
            }
            for (uint32_t i = 4 * t; i < n; i += 4 * DF_NT) {
                const uint32_t k = n - i < 4 ? n - i : 4;
                uint32_t v = 0;
                for (uint32_t j = 0; j < k; ++j) v |= (uint32_t)src[i + j] << (8 * j);
                DfBits b = df_bits_at(slot, (18 + 5 + i) * 8);
                df_put(b, v, 8 * k);
                df_flush(b);
            }
        }
    } else {
        DF_PHASE {                                             // the fixed code replaces the built one
            if (L.form == 1) {
                for (uint32_t s = t; s < 288; s += DF_NT) L.ll_len[s] = (uint8_t)df_fixed_len(s);
                if (t < 32) L.d_len[t] = 5;
            }
        }
        DF_SYNC;
        DF_PHASE {
            if (t == 0) {
                df_canonical(L.ll_len, L.form == 1 ? 288u : DF_NLL, L.ll_code);      // (the fixed code has 288 and 32 symbols)
                df_canonical(L.d_len, L.form == 1 ? 32u : DF_ND, L.d_code);
                DfBits b = df_bits_at(slot, 18 * 8);
                uint32_t bits = 3;
                if (L.form == 1) {
                    df_put(b, 3, 3);                           // BFINAL, BTYPE 01
                } else {
                    df_canonical(L.cl_len, DF_NCL, L.cl_code);
                    df_put(b, 5, 3);                           // BFINAL, BTYPE 10
                    df_put(b, L.hlit - 257, 5); df_put(b, L.hdist - 1, 5); df_put(b, DF_NCL - 4, 4);
                    for (uint32_t i = 0; i < DF_NCL; ++i) df_put(b, L.cl_len[df_cl_order(i)], 3);
                    bits += 14 + 3 * DF_NCL;
                    for (uint32_t s = 0; s < L.hlit; ++s) { const uint32_t l = L.ll_len[s]; df_put(b, L.cl_code[l], L.cl_len[l]); bits += L.cl_len[l]; }
                    for (uint32_t s = 0; s < L.hdist; ++s) { const uint32_t l = L.d_len[s]; df_put(b, L.cl_code[l], L.cl_len[l]); bits += L.cl_len[l]; }
                }
                df_flush(b);
                L.hdr_bits = bits;
            }
        }
        DF_SYNC;
        // e: bits per lane chunk, offsets, packing
        const uint32_t chunk = (L.ntok + DF_NT - 1) / DF_NT;
        DF_PHASE {
            uint32_t bits = 0;
            const uint32_t i1 = (t + 1) * chunk < L.ntok ? (t + 1) * chunk : L.ntok;
            for (uint32_t i = t * chunk; i < i1; ++i) {
                const uint32_t w = tok[i];
                uint32_t eb, ev;
                if (w & 0x80000000u) {
                    bits += L.ll_len[df_len_sym((w & 0xffu) + 3, eb, ev)] + eb;
                    bits += L.d_len[df_dist_sym(((w >> 8) & 0x7fffu) + 1, eb, ev)] + eb;
                } else bits += L.ll_len[w];
            }
            L.part[t] = bits;
        }
        DF_SYNC;
        DF_PHASE {
            if (t == 0) {
                uint32_t acc = 18 * 8 + L.hdr_bits;
                for (uint32_t i = 0; i < DF_NT; ++i) { const uint32_t b = L.part[i]; L.part[i] = acc; acc += b; }
                DfBits b = df_bits_at(slot, acc);
                df_put(b, L.ll_code[256], L.ll_len[256]);      // end of block
                df_flush(b);
            }
        }
        DF_SYNC;
        DF_PHASE {
            DfBits b = df_bits_at(slot, L.part[t]);
            const uint32_t i1 = (t + 1) * chunk < L.ntok ? (t + 1) * chunk : L.ntok;
            for (uint32_t i = t * chunk; i < i1; ++i) {
                const uint32_t w = tok[i];
                uint32_t eb, ev;
                if (w & 0x80000000u) {
                    const uint32_t ls = df_len_sym((w & 0xffu) + 3, eb, ev);
                    df_put(b, L.ll_code[ls], L.ll_len[ls]);
                    df_put(b, ev, eb);
                    const uint32_t ds = df_dist_sym(((w >> 8) & 0x7fffu) + 1, eb, ev);
                    df_put(b, L.d_code[ds], L.d_len[ds]);
                    df_put(b, ev, eb);
                } else df_put(b, L.ll_code[w], L.ll_len[w]);
            }
            df_flush(b);
        }
    }
    // f: gzip header with the BC subfield, CRC32 and ISIZE
    DF_PHASE {
        if (t == 0) {
            const uint32_t total = 18 + L.pay_bytes + 8;
            DfBits b = df_bits_at(slot, 0);
            df_put(b, 0x04088b1fu, 32); df_put(b, 0, 32); df_put(b, 0x0006ff00u, 32); df_put(b, 0x00024342u, 32);
            df_put(b, total - 1, 16);
            df_flush(b);
            b = df_bits_at(slot, (18 + L.pay_bytes) * 8);
            df_put(b, crc, 32); df_put(b, n, 32);
            df_flush(b);
        }
    }
    DF_SYNC_GLOBAL;
}

#ifndef MTH_DEFLATE_HOST_MODEL

struct DeflArgs {
    const uint8_t *src;
    const uint64_t *cut;            // n_blocks + 1
    const uint32_t *crc;
    uint32_t n_blocks;
    uint8_t *slot;                  // n_blocks * DF_SLOT
    uint32_t *tok;                  // gridDim.x * DF_MAX_IN words
    uint32_t *bsize;                // out: bytes of each finished block
};

__global__ __launch_bounds__(DF_NT) void k_deflate(const DeflArgs a) {
    __shared__ DfLds L;
    uint32_t *tok = a.tok + (size_t)blockIdx.x * DF_MAX_IN;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint64_t c0 = a.cut[blk];
        const uint32_t n = (uint32_t)(a.cut[blk + 1] - c0);
        df_block(L, a.src + c0, n, reinterpret_cast<uint32_t *>(a.slot + (size_t)blk * DF_SLOT), tok, a.crc[blk]);
        if (threadIdx.x == 0) a.bsize[blk] = 18 + L.pay_bytes + 8;
        __syncthreads();
    }
}

// the finished blocks, back to back: block b's bsize[b] bytes to out + boff[b]
__global__ __launch_bounds__(256) void k_bgzf_compact(const uint8_t *slot, const uint32_t *bsize, const unsigned long long *boff, uint8_t *out) {
    const uint32_t blk = blockIdx.x, n = bsize[blk];
    const uint8_t *s = slot + (size_t)blk * DF_SLOT;
    uint8_t *d = out + boff[blk];
    for (uint32_t i = threadIdx.x; i < n; i += 256) d[i] = s[i];
}

int deflate_core(mth_ctx *ctx, const uint8_t *d_src, const uint64_t *h_cut, uint64_t n_blocks) {
    hipStream_t s = ctx->stream;
    ctx->def_h_out.clear();
    ctx->def_h_boff.assign(1, 0);
    if (n_blocks == 0) return MTH_OK;
    if (n_blocks >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "too many BGZF blocks in one deflate call: split the stream");
    const size_t nb = (size_t)n_blocks;
    // table: cuts (nb + 1) u64 | isize nb u32 | crc nb u32 | bsize nb u32
    std::vector<uint8_t> tab((nb + 1) * 8 + nb * 4);
    memcpy(tab.data(), h_cut, (nb + 1) * 8);
    uint32_t *h_isize = reinterpret_cast<uint32_t *>(tab.data() + (nb + 1) * 8);
    for (size_t b = 0; b < nb; ++b) {
        if (h_cut[b + 1] < h_cut[b] || h_cut[b + 1] - h_cut[b] > DF_MAX_IN) return fail(ctx, MTH_ERR_INVALID, "BGZF cuts: offsets must ascend in steps of at most 0xff00 bytes");
        h_isize[b] = (uint32_t)(h_cut[b + 1] - h_cut[b]);
    }
    MTH_HIP(ctx, ctx->def_tab.reserve((nb + 1) * 8 + nb * 12 + 64, s));
    MTH_HIP(ctx, ctx->def_boff.reserve((nb + 1) * 8 + 64, s));
    MTH_HIP(ctx, ctx->def_slot.reserve(nb * DF_SLOT, s));
    int cus = 256;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && v > 0) cus = v; }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nb, (uint64_t)cus * 4);        // ~38 KB of LDS each: four workgroups per CU
    MTH_HIP(ctx, ctx->def_tok.reserve((size_t)grid * DF_MAX_IN * 4, s));
    MTH_HIP(ctx, hipMemcpyAsync(ctx->def_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    uint8_t *dt = ctx->def_tab.as<uint8_t>();
    const uint64_t *d_cut = reinterpret_cast<const uint64_t *>(dt);
    const uint32_t *d_isize = reinterpret_cast<const uint32_t *>(dt + (nb + 1) * 8);
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(dt + (nb + 1) * 8 + nb * 4);
    uint32_t *d_bsize = reinterpret_cast<uint32_t *>(dt + (nb + 1) * 8 + nb * 8);
    { const int rc = crc32_blocks(ctx, d_src, d_cut, d_isize, (uint32_t)nb, d_crc); if (rc) return rc; }
    DeflArgs a{};
    a.src = d_src; a.cut = d_cut; a.crc = d_crc; a.n_blocks = (uint32_t)nb; a.slot = ctx->def_slot.as<uint8_t>();
    a.tok = ctx->def_tok.as<uint32_t>(); a.bsize = d_bsize;
    {
        LaunchTimer lt(ctx, K_DEFLATE);
        hipLaunchKernelGGL(k_deflate, dim3(grid), dim3(DF_NT), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    unsigned long long total = 0;
    { const int rc = scan_u32_to_u64(ctx, d_bsize, (uint32_t)nb, 0ull, ctx->def_boff.as<unsigned long long>(), &total); if (rc) return rc; }   // synchronises
    MTH_HIP(ctx, ctx->def_out.reserve((size_t)total + 16, s));
    {
        LaunchTimer lt(ctx, K_BGZF_COMPACT);
        hipLaunchKernelGGL(k_bgzf_compact, dim3((uint32_t)nb), dim3(256), 0, s, ctx->def_slot.as<uint8_t>(), d_bsize, ctx->def_boff.as<unsigned long long>(), ctx->def_out.as<uint8_t>());
    }
    MTH_HIP(ctx, hipGetLastError());
    ctx->def_h_out.resize((size_t)total);
    ctx->def_h_boff.resize(nb + 1);
    {
        LaunchTimer lt(ctx, K_BGZF_D2H);                           // (mth_timing_get "bgzf_d2h": the finished blocks' way back)
        MTH_HIP(ctx, hipMemcpyAsync(ctx->def_h_boff.data(), ctx->def_boff.p, nb * 8, hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipMemcpyAsync(ctx->def_h_out.data(), ctx->def_out.p, (size_t)total, hipMemcpyDeviceToHost, s));
    }
    MTH_HIP(ctx, hipStreamSynchronize(s));
    ctx->def_h_boff[nb] = total;
    return MTH_OK;
}

#endif  // !MTH_DEFLATE_HOST_MODEL

}  // namespace mth

#ifndef MTH_DEFLATE_HOST_MODEL
using namespace mth;

extern "C" int mth_bgzf_deflate(mth_ctx_t *ctx, const void *src, uint64_t n_bytes, int mem, const uint64_t *cut_off, uint64_t n_blocks,
                                const uint8_t **out_bytes, uint64_t *out_n, const uint64_t **out_block_off) {
    if (!ctx || !out_bytes || !out_n || (n_blocks && (!cut_off || (n_bytes && !src)))) return MTH_ERR_INVALID;
    if (mem != MTH_MEM_HOST && mem != MTH_MEM_DEVICE) return fail(ctx, MTH_ERR_INVALID, "mem");
    MTH_ENTER(ctx);
    *out_bytes = nullptr; *out_n = 0;
    if (out_block_off) *out_block_off = nullptr;
    if (n_blocks && (cut_off[0] != 0 || cut_off[n_blocks] != n_bytes)) return fail(ctx, MTH_ERR_INVALID, "BGZF cuts: the offsets must run from 0 to n_bytes");
    const uint8_t *d_src = static_cast<const uint8_t *>(src);
    if (mem == MTH_MEM_HOST && n_blocks) {
        hipStream_t s = ctx->stream;
        MTH_HIP(ctx, ctx->def_src.reserve((size_t)n_bytes + 16, s));
        if (n_bytes) MTH_HIP(ctx, hipMemcpyAsync(ctx->def_src.p, src, (size_t)n_bytes, hipMemcpyHostToDevice, s));
        d_src = ctx->def_src.as<uint8_t>();
    }
    const int rc = deflate_core(ctx, d_src, cut_off, n_blocks);
    if (rc) return rc;
    *out_bytes = ctx->def_h_out.data(); *out_n = ctx->def_h_out.size();
    if (out_block_off) *out_block_off = ctx->def_h_boff.data();
    return MTH_OK;
}
#endif
