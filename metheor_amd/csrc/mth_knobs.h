// mth_knobs.h -- the environment switches that pick a kernel form or a width, or force a hand-back: parsed and clamped here, one
// reader per measure, called at the top of the measure's accumulate path.  The only header of the engine that reads the environment
// (the I/O path's, METHEOR_TIMING and the debug / trace switches apart); the knob structs themselves are mth_plan.h's, which stays
// pure.  Test and A/B switches, not an interface: INTEGRATION.md lists them with their lifetimes.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "mth_plan.h"

namespace mth {

// ---- PDR + LPMD: read per call (the tests switch them between cases in one process) ----
inline PdrKnobs pdr_knobs_from_env() {
    PdrKnobs kn;
    if (const char *e = getenv("MTH_PDR_WIDE")) { const int k = atoi(e); kn.wide = k >= 14 && k <= 16 ? k : 0; }
    if (const char *e = getenv("MTH_PDR_WIDE_W")) kn.wide_w = std::max(atoi(e), 0);      // (below 1024: no narrowed width, as any value outside the domain)
    if (const char *e = getenv("MTH_COARSE_INDEX")) kn.coarse_off = atoi(e) == 0;
    if (const char *e = getenv("MTH_TILE_RUNS")) kn.runs = atoi(e) == 1;
    if (const char *e = getenv("MTH_TILE_B")) { const int k = atoi(e); if (k == 128 || k == 256) kn.tile_b = k; }
    return kn;
}
// ... and the three that are read once per process (A/B switches of a whole run)
inline bool tile_no_margin_knob() { static const bool v = getenv("MTH_TILE_NO_MARGIN") != nullptr; return v; }
inline bool gather_per_tile_knob() { static const bool v = getenv("MTH_GATHER") && atoi(getenv("MTH_GATHER")) == 1; return v; }
inline int runs_wgs_per_cu_knob() {      // 0: not set
    static const int v = [] { const char *e = getenv("MTH_RUNS_WGS_PER_CU"); return e && atoi(e) > 0 ? atoi(e) : 0; }();
    return v;
}
// MTH_PIPELINE=0: no pipelined batches (read once per context: mth_pdr_lpmd_accumulate keeps the answer)
inline bool pipeline_knob() { const char *e = getenv("MTH_PIPELINE"); return !(e && atoi(e) == 0); }

// ---- FDRP / qFDRP: read per call ----
inline FdrpKnobs fdrp_knobs_from_env() {
    FdrpKnobs kn;
    if (const char *e = getenv("METHEOR_FDRP_WTILE")) kn.wtile = atoi(e) != 0;
    if (const char *e = getenv("METHEOR_FDRP_WALK4")) { const int k = atoi(e); kn.walk4 = k == 1 ? 16 : (k == 16 || k == 32 ? k : 0); }
    if (const char *e = getenv("METHEOR_FDRP_TILE")) kn.tile = atoi(e) != 0;
    if (const char *e = getenv("METHEOR_FDRP_WIN")) kn.win = atoi(e) == 32 ? 32 : 64;
    kn.wide_rows = getenv("METHEOR_FDRP_TILE_WIDE_ROWS") != nullptr;
    return kn;
}
// (the tile pass's own: read where that pass runs)
inline FdrpWtileKnobs fdrp_wtile_knobs_from_env() {
    FdrpWtileKnobs kn;
    if (const char *e = getenv("METHEOR_FDRP_WTILE_W")) kn.w = std::min(FW_WMAX, std::max(64, atoi(e))) & ~63;   // tests / tuning
    kn.force_sub = getenv("METHEOR_FDRP_WTILE_SUB") != nullptr;
    kn.force_heavy = getenv("METHEOR_FDRP_WTILE_HEAVY") != nullptr;
    return kn;
}

// ---- MHL: read per call ----
inline MhlKnobs mhl_knobs_from_env() {
    MhlKnobs kn;
    kn.walk = getenv("MTH_MHL_WALK") != nullptr;
    if (kn.walk) return kn;              // (the rest are the tile pass's)
    if (const char *e = getenv("MTH_MHL_ROWCHK")) kn.rowchk = atoi(e) != 0;
    if (const char *e = getenv("MTH_MHL_TILE_SHIFT")) kn.tile_shift = std::min(16, std::max(12, atoi(e)));
    kn.force_sub = getenv("MTH_MHL_FORCE_SUB") != nullptr;
    kn.force_hand_on = getenv("MTH_MHL_FORCE_HAND_ON") != nullptr;
    kn.no_wave_walk = getenv("MTH_MHL_NO_WAVE_WALK") != nullptr;
    return kn;
}

// ---- MHL per interval (mth_mhl_regions.hip) ----
// lengths a dense per-interval row holds (kept calls of a read, methylated runs): 64 covers short reads on 1 kbp windows; longer ones
// take the overflow list
constexpr int MHL_REGIONS_BINS = 64;
// MTH_MHL_REGIONS_LIST (tests: force the second run of a batch): the overflow list's first size in entries, at least 1
inline unsigned long long mhl_regions_list_knob() {
    const char *e = getenv("MTH_MHL_REGIONS_LIST");
    const unsigned long long k = e ? strtoull(e, nullptr, 10) : 0;
    return k ? k : (1ull << 16);
}

// ---- PDR per interval (mth_pdr_regions.hip): read once per context, when it first declares intervals ----
// entries of a length class a workgroup sums in LDS rows of four 32-bit words (16 KiB); a class with more candidates adds to memory
constexpr int PDR_REGIONS_LDS_CAP = 1024;
// MTH_PDR_REGIONS_LDS_CAP (tests: the differential forms): that cap, 0 .. PDR_REGIONS_LDS_CAP; 0: every add goes to memory directly
inline int pdr_regions_lds_cap_knob() {
    const char *e = getenv("MTH_PDR_REGIONS_LDS_CAP");
    return e ? std::min(PDR_REGIONS_LDS_CAP, std::max(0, atoi(e))) : PDR_REGIONS_LDS_CAP;
}
// MTH_PDR_REGIONS_SPAN=0 (tests, A/B): no span route -- an interval that holds a workgroup's whole span is counted read by read
inline bool pdr_regions_span_knob() { const char *e = getenv("MTH_PDR_REGIONS_SPAN"); return !(e && atoi(e) == 0); }

// ---- ME / PM per interval (mth_quartet_regions.hip): read once per context, when it first declares intervals ----
// entries of a length class a workgroup sums in LDS rows of seventeen 32-bit words (sixteen bins and the reads: 15.9 KiB); a class with
// more candidates adds to memory
constexpr int QUARTET_REGIONS_LDS_CAP = 240;
// MTH_QUARTET_REGIONS_LDS_CAP (tests: the differential forms): that cap, 0 .. QUARTET_REGIONS_LDS_CAP; 0: every add goes to memory directly
inline int quartet_regions_lds_cap_knob() {
    const char *e = getenv("MTH_QUARTET_REGIONS_LDS_CAP");
    return e ? std::min(QUARTET_REGIONS_LDS_CAP, std::max(0, atoi(e))) : QUARTET_REGIONS_LDS_CAP;
}
// MTH_QUARTET_REGIONS_SUMMARY=0 (tests, A/B): no packed histogram -- a read an interval holds whole walks its calls as any other
inline bool quartet_regions_summary_knob() { const char *e = getenv("MTH_QUARTET_REGIONS_SUMMARY"); return !(e && atoi(e) == 0); }
// MTH_QUARTET_REGIONS_CARRY=0 (tests, A/B): no carried row -- a class with a single candidate is flushed once per work item
inline bool quartet_regions_carry_knob() { const char *e = getenv("MTH_QUARTET_REGIONS_CARRY"); return !(e && atoi(e) == 0); }

// ---- the per-interval passes (k_pairs_intervals, k_mhl_regions, k_pdr_regions, k_quartet_regions): read where the pass reads its others ----
// MTH_REGIONS_GRID (tests: several work items per workgroup on a small input): an upper bound, 1 .. dflt, on the workgroups of a
// launch, so that each comes round its persistent loop again -- with 1, one workgroup takes every work item in order.  Not a tuning
// switch: unset -- or empty, not a number, or below 1 -- a launch has min(work items, dflt) workgroups as ever, and no smaller grid is
// faster.
inline uint32_t regions_grid_knob(const uint32_t dflt) {
    const char *e = getenv("MTH_REGIONS_GRID");
    const long long k = e ? atoll(e) : 0;
    return k >= 1 ? (uint32_t)std::min<long long>(dflt, k) : dflt;
}

// ---- the tile-row measures (ME / PM: MTH_QUARTET_*, LPMD pairs: MTH_PAIRS_*): each read per call, where it is used ----
inline const char *tile_rows_knob(const char *prefix, const char *suffix) {
    char name[48];
    snprintf(name, sizeof name, "%s_%s", prefix, suffix);
    return getenv(name);
}
// MTH_*_TILE_SHIFT as 13 .. 16, -1: not set
inline int tile_shift_knob(const char *prefix) {
    const char *e = tile_rows_knob(prefix, "TILE_SHIFT");
    return e ? std::min(16, std::max(13, atoi(e))) : -1;
}
// MTH_*_FORCE_GLOBAL: every tile is handed to the global path
inline bool force_global_knob(const char *prefix) { return tile_rows_knob(prefix, "FORCE_GLOBAL") != nullptr; }
// MTH_*_SLOTS_MIN (tests: force the global table's retry): the table's first size, a power of two >= the value; 0: not set (or below 16)
inline unsigned long long slots_min_knob(const char *prefix) {
    const char *e = tile_rows_knob(prefix, "SLOTS_MIN");
    const unsigned long long k = e ? strtoull(e, nullptr, 10) : 0;
    if (k < 16) return 0;
    unsigned long long n_slots = 16;
    while (n_slots < k) n_slots <<= 1;
    return n_slots;
}
// MTH_MULTI_FORCE_HANDBACK (tests): every tile of the fused pass handed back
inline bool multi_force_handback_knob() { return getenv("MTH_MULTI_FORCE_HANDBACK") != nullptr; }

}  // namespace mth
