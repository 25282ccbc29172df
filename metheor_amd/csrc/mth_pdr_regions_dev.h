// mth_pdr_regions_dev.h -- what one lane (one read) of the per-interval PDR pass does (k_pdr_regions, mth_pdr_regions.hip): the
// summary of a read as a whole, the whole / partial decision against one interval, the partial walk and the class.
//
// The same text is the device routine and, under MTH_PDR_REGIONS_HOST_MODEL, a host routine: tests/test_pdr_regions_model.py compiles
// it with a plain C++ compiler and the sanitizers and plays the kernel work item by work item around it.  Nothing here uses another
// lane: ballots, reductions and the wave-wide searches belong to the kernel's block-uniform code.
#pragma once
#include <stdint.h>

#ifdef MTH_PDR_REGIONS_HOST_MODEL
#define PR_FN static inline
#else
#define PR_FN __device__ __forceinline__
#endif

namespace mth {

// the class of a contributing read in an interval, by get_concordance_state() (readutil.rs:134-145) of its kept calls -- and the
// word of an interval's row that counts it; PR_NONE: fewer than max(min_cpgs, 1) calls kept, the read does not contribute
constexpr uint32_t PR_METH = 0, PR_UNMETH = 1, PR_DISC = 2, PR_NONE = 3;
constexpr int PR_ROW = 4;                       // words of a row: methylated, unmethylated, discordant, one spare

// n kept calls (n >= 1), m of them methylated
PR_FN uint32_t pr_class(uint32_t n, uint32_t m) { return m == n ? PR_METH : (m == 0 ? PR_UNMETH : PR_DISC); }

// a read as a whole: its calls [k0, k1) of cpg_pos, the smallest and the largest called position, its class
struct PrRead {
    uint32_t k0, k1;
    int32_t first, last;
    uint32_t cls;
};

// One walk over the calls [k0, k1), k1 > k0: positions' extremes, methylated count, class.  Returns false when a call carries the
// word of position -1 (no batch may: include/metheor_hip.h, mth_batch_t.cpg_pos); the read is then not eligible.
PR_FN bool pr_summary(const uint32_t *cpg_pos, uint32_t k0, uint32_t k1, PrRead &rd) {
    uint32_t lo = 0x7fffffffu, hi = 0u, m = 0u;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t w = cpg_pos[k], p = w & 0x7fffffffu;
        lo = p < lo ? p : lo;
        hi = p > hi ? p : hi;
        m += w >> 31;
    }
    rd.k0 = k0; rd.k1 = k1;
    rd.first = (int32_t)lo; rd.last = (int32_t)hi;
    rd.cls = pr_class(k1 - k0, m);
    return hi != 0x7fffffffu;
}

// The read against the interval [ib, ie): filter_isin (readutil.rs:87-94) with the interval's positions, pdr.rs:147's test on what is
// kept (need = max(min_cpgs, 1); the read as a whole holds at least `need` calls), then the class.  An interval that holds the read
// whole takes the summary's class and no call is looked at; a partial overlap walks the calls once, n and m in the same pass.
PR_FN uint32_t pr_entry_class(const uint32_t *cpg_pos, const PrRead &rd, int32_t ib, int32_t ie, uint32_t need) {
    if (ib <= rd.first && rd.last < ie) return rd.cls;
    uint32_t n = 0, m = 0;
    for (uint32_t k = rd.k0; k < rd.k1; ++k) {
        const uint32_t w = cpg_pos[k];
        const int32_t p = (int32_t)(w & 0x7fffffffu);
        const uint32_t in = (p >= ib && p < ie) ? 1u : 0u;
        n += in;
        m += in & (w >> 31);
    }
    return n >= need ? pr_class(n, m) : PR_NONE;
}

// the span route's predicate: the interval holds every call of every eligible read of the work item (wmin / wmax: their smallest
// first and largest last call) -- block-uniform, so the lanes' walks and the workgroup's strided loop agree on it
PR_FN bool pr_holds_span(int32_t ib, int32_t ie, int32_t wmin, int32_t wmax) { return ib <= wmin && wmax < ie; }

}  // namespace mth
