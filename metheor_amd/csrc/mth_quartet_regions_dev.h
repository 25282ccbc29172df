// mth_quartet_regions_dev.h -- what one lane (one read) of the per-interval ME / PM pass does (k_quartet_regions,
// mth_quartet_regions.hip): the summary of a read as a whole with its own pattern histogram packed into one register, the whole /
// partial decision against one interval, the rolling walk over the kept calls and the words a read adds to an interval's row.
//
// The same text is the device routine and, under MTH_QUARTET_REGIONS_HOST_MODEL, a host routine: tests/test_quartet_regions_model.py
// compiles it with a plain C++ compiler and the sanitizers and plays the kernel work item by work item around it.  Nothing here uses
// another lane: reductions and the wave-wide searches belong to the kernel's block-uniform code.
#pragma once
#include <stdint.h>

#ifdef MTH_QUARTET_REGIONS_HOST_MODEL
#define QR_FN static inline
#else
#define QR_FN __device__ __forceinline__
#endif

namespace mth {

// An interval's row: the sixteen bins of its ONE pooled QuartetStat (me.rs:121-125 with every quartet mapped to the same stat;
// bin = 8*m1 + 4*m2 + 2*m3 + m4, readutil.rs:105-129), then the contributing reads.
constexpr int QR_BINS = 16;
constexpr int QR_READS = 16;                    // the word that counts the contributing reads
constexpr int QR_ROW = 17;
constexpr uint32_t QR_NEED = 4;                 // calls a read must keep to hold a window (readutil.rs:101)
constexpr uint32_t QR_PACK_CALLS = 18;          // at most 15 windows: every 4-bit field of the packed histogram holds its count

// a read as a whole: its calls [k0, k1) of cpg_pos, the smallest and the largest called position, and -- when it has at most
// QR_PACK_CALLS calls -- its own pattern histogram as sixteen 4-bit fields (field p: windows of pattern p); packed_ok tells
struct QrRead {
    uint32_t k0, k1;
    int32_t first, last;
    unsigned long long packed;
    bool packed_ok;
};

// One walk over the calls [k0, k1), k1 - k0 >= QR_NEED, in call order (the windows follow the order of the calls, whatever their
// positions do): the positions' extremes by min / max and the packed histogram.  Returns false when a call carries the word of
// position -1 (no batch may: include/metheor_hip.h, mth_batch_t.cpg_pos); the read is then not eligible.
QR_FN bool qr_summary(const uint32_t *cpg_pos, uint32_t k0, uint32_t k1, QrRead &rd) {
    uint32_t lo = 0x7fffffffu, hi = 0u, pat = 0u, n = 0u;
    unsigned long long packed = 0ull;
    const bool fits = k1 - k0 <= QR_PACK_CALLS;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t w = cpg_pos[k], p = w & 0x7fffffffu;
        lo = p < lo ? p : lo;
        hi = p > hi ? p : hi;
        pat = ((pat << 1) | (w >> 31)) & 15u;
        ++n;
        if (fits && n >= QR_NEED) packed += 1ull << (4u * pat);
    }
    rd.k0 = k0; rd.k1 = k1;
    rd.first = (int32_t)lo; rd.last = (int32_t)hi;
    rd.packed = packed; rd.packed_ok = fits;
    return hi != 0x7fffffffu;
}

// The read against the interval [ib, ie): filter_isin (readutil.rs:87-94) with the interval's positions, then
// get_cpg_quartets_and_patterns() (readutil.rs:97-132) of what is kept -- add(word, count) for every word of the interval's row the
// read adds to, nothing when fewer than QR_NEED calls are kept.
//   * The interval holds the read whole and the read has a packed histogram (use_packed: the knob): one add per NON-ZERO field and
//     one for the reads word; no call is looked at.
//   * A partial overlap, or a read of more than QR_PACK_CALLS calls: one pass over the calls with a rolling 4-bit pattern register
//     that advances on kept calls only and emits from the fourth kept call on.  Right for any call order and any length; no array is
//     sized by the read.
template <class Add>
QR_FN void qr_entry(const uint32_t *cpg_pos, const QrRead &rd, int32_t ib, int32_t ie, bool use_packed, Add &&add) {
    if (use_packed && rd.packed_ok && ib <= rd.first && rd.last < ie) {
        unsigned long long left = rd.packed;
        while (left) {
            const uint32_t b = (uint32_t)__builtin_ctzll(left) >> 2;
            add(b, (uint32_t)(left >> (4u * b)) & 15u);
            left &= ~(15ull << (4u * b));
        }
        add((uint32_t)QR_READS, 1u);
        return;
    }
    uint32_t n = 0u, pat = 0u;
    for (uint32_t k = rd.k0; k < rd.k1; ++k) {
        const uint32_t w = cpg_pos[k];
        const int32_t p = (int32_t)(w & 0x7fffffffu);
        if (p < ib || p >= ie) continue;
        pat = ((pat << 1) | (w >> 31)) & 15u;
        if (++n >= QR_NEED) add(pat, 1u);
    }
    if (n >= QR_NEED) add((uint32_t)QR_READS, 1u);
}

// Calls a lane reports to its work item's sum, clamped: 256 lanes of at most 2^23 stay below 2^32, and a sum below 2^23 is the true
// one.  A work item whose sum reaches 2^23 adds to memory directly; a smaller one cannot lift a 32-bit LDS word by 2^23 or more.
constexpr uint32_t QR_LANE_CALLS_MAX = 1u << 23;
QR_FN uint32_t qr_lane_calls(uint32_t k0, uint32_t k1) { return k1 - k0 < QR_LANE_CALLS_MAX ? k1 - k0 : QR_LANE_CALLS_MAX; }
// the carried row of a class with a single candidate is added to memory before it has taken this many calls' worth of adds
constexpr uint32_t QR_CARRY_CALLS_MAX = 1u << 31;

}  // namespace mth
