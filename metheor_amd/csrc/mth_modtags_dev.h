// mth_modtags_dev.h -- methylation calls from the SAM base-modification tags MM:Z / ML:B:C (/ MN:i) of ONE record
// (mth_decode_set_modtags; `--mm-tags` on the measure commands; the rule is stated in include/metheor_hip.h and DESIGN.md 9d).
//
// Three steps, all on the record's own bytes, no allocation and no array sized by the read:
//   mm_prepare   one walk over the aux fields for MM, ML and MN; the records that contribute nothing (no SEQ, an H in the CIGAR,
//                MN != l_seq); the grammar of MM, which picks the first C+...m... group and adds up the ML entries every group
//                owns; the count of the read's fundamental bases (stored C, or stored G on a reverse record) against the list
//   MmWalk       a cursor over SEQ's 4-bit codes, query offset 0 upwards: step(q) is 0 / 1 / 2 for the character '.' / 'z' /
//                'Z' of X(record, T) at q.  A reverse record's list runs from SEQ's END: the walk starts with the unlisted tail
//                (stored Gs - sum of the skips - entries) and reads the list's numbers and ML right to left, so the
//                characters, and with them the calls, still come out in ascending position
// The same text is the device routine (k_decode_mm, k_mm_xm: mth_decode_mm.hip) and, under MTH_MODTAGS_HOST_MODEL, a host
// function a stand-alone program can run under a sanitizer (tests/test_modtags_model.py).
// Every byte is fetched through MmBytes: one (unaligned) 32-bit load per four bytes where the word lies inside the field,
// single bytes at its end -- nothing outside [p, p + n) is touched.  The lanes of a wave parse different records: the loads
// diverge (an L2 / texture-path round trip each) and the loop trip counts differ, which is the cost of one thread per record.
#pragma once
#include <stdint.h>

#ifdef MTH_MODTAGS_HOST_MODEL
#define MM_FN static inline
#define MM_MEM inline
#else
#define MM_FN __device__ __forceinline__
#define MM_MEM __device__ __forceinline__
#endif

namespace mth {

struct MmBytes {
    const uint8_t *p;
    uint32_t n, wi, w;
    MM_MEM void init(const uint8_t *p_, uint32_t n_) { p = p_; n = n_; wi = 0xffffffffu; w = 0; }
    MM_MEM uint32_t at(uint32_t i) {                                   // i < n
        const uint32_t k = i >> 2;
        if (k != wi) {
            wi = k;
            const uint32_t b = k << 2;
            if (b + 4u <= n) __builtin_memcpy(&w, p + b, 4);
            else { w = 0; for (uint32_t j = b; j < n; ++j) w |= (uint32_t)p[j] << (8u * (j - b)); }
        }
        return (w >> (8u * (i & 3u))) & 255u;
    }
};

enum : uint32_t {
    MM_CALLS = 0,     // a chosen group: walk SEQ
    MM_DOTS = 1,      // no MM:Z, or no group qualifies: X is all dots
    MM_NOTHING = 2,   // the record contributes nothing (notes bit 1): X is all dots
    MM_ERROR = 3,     // ERRB_MODTAG
};

struct MmPlan {
    uint32_t status;
    const uint8_t *mm;            // the MM:Z string (without its NUL)
    uint32_t mm_len;
    const uint8_t *ml;            // the ML:B:C entries
    uint32_t ml_n;
    bool have_mm, have_ml, ml_bad;
    // the chosen group
    uint32_t list_beg, list_end;  // its numbers: mm[list_beg, list_end) is (',' digits)*, mm[list_end] is the ';'
    uint32_t n;                   // how many numbers
    uint64_t sum;                 // their sum
    uint32_t k, im;               // letter codes of the group, index of 'm' among them
    uint64_t ml_base;             // ML entries owned by the groups before it
    bool mode_q;                  // mode '?': an unlisted base is no call ('.'); '.' or none: it is unmethylated ('z')
    uint32_t n_fund;              // fundamental bases of the read
};

MM_FN bool mm_digit(uint32_t c) { return c - 48u < 10u; }

// one walk over the aux fields: the first MM of type Z, the first ML, the first integer MN.  false: the fields cannot be walked
MM_FN bool mm_scan_aux(const uint8_t *aux, uint32_t len, MmPlan &P, bool &have_mn, int64_t &mn) {
    MmBytes A;
    A.init(aux, len);
    P.have_mm = P.have_ml = P.ml_bad = false;
    P.mm = P.ml = aux; P.mm_len = P.ml_n = 0;
    have_mn = false; mn = 0;
    uint32_t o = 0;
    while (o < len) {
        if (o + 3u > len) return false;
        const uint32_t t0 = A.at(o), t1 = A.at(o + 1), ty = A.at(o + 2);
        o += 3;
        const bool is_mm = t0 == 'M' && t1 == 'M', is_ml = t0 == 'M' && t1 == 'L', is_mn = t0 == 'M' && t1 == 'N';
        const bool first_ml = is_ml && !P.have_ml;
        if (first_ml) { P.have_ml = true; P.ml_bad = true; }                 // (cleared below when it is B:C)
        uint32_t w = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': w = 1; break;
            case 's': case 'S': w = 2; break;
            case 'i': case 'I': case 'f': w = 4; break;
            case 'Z': case 'H': {
                const uint32_t b = o;
                while (o < len && A.at(o) != 0u) ++o;
                if (o >= len) return false;
                if (is_mm && ty == 'Z' && !P.have_mm) { P.have_mm = true; P.mm = aux + b; P.mm_len = o - b; }
                o += 1;
                continue;
            }
            case 'B': {
                if (o + 5u > len) return false;
                const uint32_t sub = A.at(o);
                const uint64_t cnt = (uint64_t)A.at(o + 1) | ((uint64_t)A.at(o + 2) << 8) | ((uint64_t)A.at(o + 3) << 16) | ((uint64_t)A.at(o + 4) << 24);
                uint64_t bw;
                switch (sub) {
                    case 'c': case 'C': bw = 1; break;
                    case 's': case 'S': bw = 2; break;
                    case 'i': case 'I': case 'f': bw = 4; break;
                    default: return false;
                }
                // 64-bit: a crafted count must not wrap the cursor back into the record (the walk would never leave)
                const uint64_t nx = (uint64_t)o + 5u + cnt * bw;
                if (nx > len) return false;
                if (first_ml && sub == 'C') { P.ml_bad = false; P.ml = aux + o + 5u; P.ml_n = (uint32_t)cnt; }
                o = (uint32_t)nx;
                continue;
            }
            default: return false;
        }
        if (o + w > len) return false;
        if (is_mn && !have_mn && ty != 'A' && ty != 'f') {
            have_mn = true;
            uint64_t v = 0;
            for (uint32_t j = 0; j < w; ++j) v |= (uint64_t)A.at(o + j) << (8u * j);
            if (ty == 'c') mn = (int8_t)v; else if (ty == 's') mn = (int16_t)v; else if (ty == 'i') mn = (int32_t)v; else mn = (int64_t)v;
        }
        o += w;
    }
    return true;
}

// the grammar (base strand codes mode? (',' digits)* ';')* over the whole string; false: violated.  Sets the chosen group's
// fields and *ml_total = the ML entries all groups own; P.status = MM_CALLS or MM_DOTS
MM_FN bool mm_parse(MmPlan &P, uint64_t &ml_total) {
    MmBytes S;
    S.init(P.mm, P.mm_len);
    const uint32_t L = P.mm_len;
    uint32_t o = 0;
    uint64_t run = 0;
    bool chosen = false;
    while (o < L) {
        const uint32_t base = S.at(o);
        if (!(base == 'A' || base == 'C' || base == 'G' || base == 'T' || base == 'U' || base == 'N')) return false;
        if (++o >= L) return false;
        const uint32_t strand = S.at(o);
        if (strand != '+' && strand != '-') return false;
        if (++o >= L) return false;
        uint32_t c = S.at(o), k = 0, im = 0xffffffffu;
        if (c - 97u < 26u) {
            while (o < L && (c = S.at(o)) - 97u < 26u) { if (c == 'm' && im == 0xffffffffu) im = k; ++k; ++o; }
        } else if (mm_digit(c)) {
            while (o < L && mm_digit(c = S.at(o))) ++o;
            k = 1;                                                      // a numeric (ChEBI) code: one entry per position, never chosen
        } else {
            return false;
        }
        if (o >= L) return false;
        bool mode_q = false;
        if (c == '.' || c == '?') { mode_q = c == '?'; if (++o >= L) return false; c = S.at(o); }
        const uint32_t lb = o;
        uint32_t n = 0;
        uint64_t sum = 0;
        while (c == ',') {
            ++o;
            uint32_t nd = 0, v = 0;
            while (o < L && mm_digit(c = S.at(o))) { if (++nd > 9u) return false; v = v * 10u + (c - 48u); ++o; }
            if (nd == 0u || o >= L) return false;
            ++n; sum += v;
        }
        if (c != ';') return false;
        if (!chosen && base == 'C' && strand == '+' && im != 0xffffffffu) {
            chosen = true;
            P.list_beg = lb; P.list_end = o; P.n = n; P.sum = sum; P.k = k; P.im = im; P.ml_base = run; P.mode_q = mode_q;
        }
        run += (uint64_t)n * k;
        ++o;
    }
    ml_total = run;
    P.status = chosen ? MM_CALLS : MM_DOTS;
    return true;
}

MM_FN uint32_t mm_nibble(MmBytes &seq, uint32_t q) { return (seq.at(q >> 1) >> ((q & 1u) ? 0u : 4u)) & 15u; }

// bases of SEQ whose 4-bit code is `code`: eight per word
MM_FN uint32_t mm_count_code(const uint8_t *seq, uint32_t l_seq, uint32_t code) {
    MmBytes B;
    B.init(seq, (l_seq + 1u) >> 1);
    uint32_t q = 0, cnt = 0;
    for (; q + 8u <= l_seq; q += 8u) {
        B.at(q >> 1);                                                   // (loads the word that holds bases q .. q + 7)
        const uint32_t x = B.w ^ (code * 0x11111111u);
        const uint32_t nz = (((x & 0x77777777u) + 0x77777777u) | x) & 0x88888888u;      // bit 3 of every non-zero nibble
        cnt += 8u - (uint32_t)__builtin_popcount(nz);
    }
    for (; q < l_seq; ++q) cnt += mm_nibble(B, q) == code ? 1u : 0u;
    return cnt;
}

// core: the record past its block_size, len bytes, field lengths already checked (o_aux <= len).  Fills P (status first)
MM_FN void mm_prepare(const uint8_t *core, uint32_t len, uint32_t o_cigar, uint32_t n_cigar, uint32_t o_seq, uint32_t l_seq, uint32_t o_aux,
                      bool reverse, MmPlan &P) {
    bool have_mn;
    int64_t mn;
    P.n = 0; P.sum = 0; P.k = 1; P.im = 0; P.ml_base = 0; P.mode_q = false; P.list_beg = P.list_end = 0; P.n_fund = 0;
    if (!mm_scan_aux(core + o_aux, len - o_aux, P, have_mn, mn)) { P.status = MM_ERROR; return; }
    bool hard = false;
    for (uint32_t c = 0; c < n_cigar; ++c) { uint32_t cw; __builtin_memcpy(&cw, core + o_cigar + 4u * c, 4); hard |= (cw & 15u) == 5u; }
    if (l_seq == 0u || hard || (have_mn && mn != (int64_t)l_seq)) { P.status = MM_NOTHING; return; }
    if (!P.have_mm) { P.status = MM_DOTS; return; }
    if (P.have_ml && P.ml_bad) { P.status = MM_ERROR; return; }
    uint64_t ml_total = 0;
    if (!mm_parse(P, ml_total)) { P.status = MM_ERROR; return; }
    if (P.have_ml && (uint64_t)P.ml_n != ml_total) { P.status = MM_ERROR; return; }
    if (P.status != MM_CALLS) return;
    P.n_fund = mm_count_code(core + o_seq, l_seq, reverse ? 4u : 2u);                  // "=ACMGRSVTWYHKDBN": C = 2, G = 4
    if (P.sum + P.n > (uint64_t)P.n_fund) P.status = MM_ERROR;                           // the list selects a base the read does not have
}

struct MmWalk {
    MmBytes seq, lst, ml;
    uint32_t l_seq, T, n, k, im, remaining, skip, cur, fund, nb_prev, nb_cur;
    uint64_t ml_base;
    bool rev, mode_q, have_ml;

    MM_MEM uint32_t next_fwd() {                                         // cur at a ','
        uint32_t v = 0, c;
        ++cur;
        while (mm_digit(c = lst.at(cur))) { v = v * 10u + (c - 48u); ++cur; }      // (ends at ',' or the ';': inside the string)
        return v;
    }
    MM_MEM uint32_t next_bwd() {                                         // cur one past a number's last digit
        uint32_t v = 0, mul = 1, c;
        while (cur > 0u && mm_digit(c = lst.at(cur - 1u))) { v += (c - 48u) * mul; mul *= 10u; --cur; }
        if (cur > 0u) --cur;                                            // its ','
        return v;
    }
    MM_MEM void init(const MmPlan &P, const uint8_t *seq_p, uint32_t l_seq_, bool reverse, uint32_t threshold) {
        seq.init(seq_p, (l_seq_ + 1u) >> 1);
        lst.init(P.mm, P.mm_len);
        ml.init(P.ml, P.ml_n);
        l_seq = l_seq_; T = threshold; n = P.n; k = P.k; im = P.im; ml_base = P.ml_base;
        rev = reverse; mode_q = P.mode_q; have_ml = P.have_ml;
        fund = reverse ? 4u : 2u;
        remaining = n;
        if (rev) { skip = (uint32_t)((uint64_t)P.n_fund - P.sum - n); cur = P.list_end; }
        else { cur = P.list_beg; skip = n ? next_fwd() : 0u; }
        nb_prev = 0xffu;
        nb_cur = l_seq ? mm_nibble(seq, 0) : 0xffu;
    }
    // the character of X at query offset q: 0 '.', 1 'z', 2 'Z'.  To be called for q = 0, 1, 2, ... l_seq - 1 in this order
    MM_MEM uint32_t step(uint32_t q) {
        const uint32_t nb_next = q + 1u < l_seq ? mm_nibble(seq, q + 1u) : 0xffu;
        uint32_t r = 0;
        if (nb_cur == fund) {
            bool listed = false;
            uint32_t prob = 255u;
            if (remaining) {
                if (skip == 0u) {
                    listed = true;
                    const uint32_t idx = rev ? remaining - 1u : n - remaining;
                    if (have_ml) prob = ml.at((uint32_t)(ml_base + (uint64_t)idx * k + im));
                    --remaining;
                    if (rev) skip = next_bwd(); else if (remaining) skip = next_fwd();
                } else {
                    --skip;
                }
            }
            // read CpG context: the next base of the ORIGINAL read is G -- stored, the G after a C, or the C before a reverse record's G
            const bool cpg = rev ? nb_prev == 2u : nb_next == 4u;
            if (cpg) r = listed ? (prob >= T ? 2u : 1u) : (mode_q ? 0u : 1u);
        }
        nb_prev = nb_cur; nb_cur = nb_next;
        return r;
    }
};

}  // namespace mth
