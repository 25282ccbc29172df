// mth_plan.h -- which kernel form, tile width and index a batch gets: pure functions of the batch's shape, the measure's parameters
// and its knobs.  Host only and nothing of HIP: the launch functions (mth_pdr_lpmd.hip, mth_fdrp.hip, mth_fdrp_wtile.hip,
// mth_mhl_tile.hip, mth_quartet.hip, mth_pairs.hip) call these first and then reserve and launch what the plan says;
// tests/test_launch_plan.py compiles this header with a plain C++ compiler and pins the switch points.  The kernel capacities the
// rules are tuned against live here too, beside the rules.  Nothing here allocates or reads the environment (mth_knobs.h does).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/metheor_hip.h"

namespace mth {

// ---- kernel capacities --------------------------------------------------------------------
// A tile is TILE_W consecutive reference positions of one contig; one workgroup owns the sites
// of one tile and keeps their accumulators in LDS.  The read index has one entry per IDX_Q bp.
// (the tile width is a template parameter of the tile kernel: 1024 / 2048 / 4096)
constexpr int IDX_QSHIFT = 5;   // 32-bp quanta (256 until round 2: up to 362 bp of useless candidates per tile / site)
constexpr int IDX_Q = 1 << IDX_QSHIFT;

// pdr.rs:162 -- a site is flushed once a passing read's first CpG lies more than 150 bp past it
constexpr int PDR_FLUSH_MARGIN = 150;

constexpr int TILE_BUCKET_SHIFT = 8;   // 256 tiles per bucket
constexpr int DENSE_TILE_SHIFT = 12;   // the dense kernel's 4096-bp tiles
constexpr int TILE_MARGIN = 256;   // counter margins on either side of a tile for batches with max_span <= 256
#ifndef MTH_TILE_B_DEFAULT
#define MTH_TILE_B_DEFAULT 128     // threads per workgroup of the dense kernel on 8-bit relpos batches (plan_pdr_lpmd)
#endif

constexpr int MT_S = 256;             // MHL tile kernel: LDS slots (one per thread)
constexpr uint32_t MT_HEAVY = 8191;   // candidate reads a sub-range may have with 16-bit bins (a read adds up to 8 to one hm bin)

#ifndef MTH_FW_U
#define MTH_FW_U 2
#endif
constexpr int FW_U = MTH_FW_U;                          // 64-read chunks of a stretch
constexpr int FW_WPT = FW_U > 2 ? 2 : 1;                // bitmap words per lane
constexpr int FW_WMAX = FW_WPT * 2048 - 448;            // the tile + 200 on either side fit the bitmap (1600 / 3648 positions)
constexpr int FW_RCAP = 64 * FW_U;                      // candidate reads of a stretch (more: the stretch is halved)
constexpr int FW_V = FW_U > 2 ? 6 : 4;                  // 64-call chunks of a stretch
constexpr int FW_CCAP = 64 * FW_V;                      // calls of a stretch's candidate reads (more: the stretch is halved)

constexpr int QT_S = 512;             // ME / PM tile kernel: LDS slots (quartets of a tile)
constexpr int PT_S = 2048;            // LPMD pairs tile kernel: LDS slots (pairs of a tile)

constexpr int FD_SLOTS_DEEP = 256;
constexpr uint32_t FD_DEPTH_MAX = 16384;

// ---- a batch's shape ----------------------------------------------------------------------
struct BatchShape {
    uint32_t n_reads, n_cpgs;
    int32_t max_span, region_beg, region_end;
    bool rel8;            // 8-bit relative positions (cpg_rel); 16-bit ones (cpg_rel16) otherwise
    bool start_al16;      // read_start is 16-byte aligned
    int64_t region_len() const { return (int64_t)region_end - region_beg; }
};
inline BatchShape batch_shape(const mth_batch_t &b) {
    return BatchShape{b.n_reads, b.n_cpgs, b.max_span, b.region_beg, b.region_end, b.cpg_rel != nullptr,
                      (reinterpret_cast<uintptr_t>(b.read_start) & 15u) == 0};
}

// ---- the fine read index ------------------------------------------------------------------
// index origin: a whole number of quanta below the region so that halo reads are indexed; entries for ntiles tiles of tile_step
// positions (65536: every tile width -- what a prepared batch's index covers)
struct IndexGeom { int32_t ext, idx_base; uint32_t nq, ntiles; };
inline int32_t index_ext(int32_t max_span) { return ((max_span + 2 + IDX_Q - 1) / IDX_Q) * IDX_Q; }
inline IndexGeom index_geometry(const BatchShape &b, uint32_t tile_step) {
    IndexGeom g;
    g.ntiles = (uint32_t)((b.region_len() + (int64_t)tile_step - 1) / (int64_t)tile_step);
    g.ext = index_ext(b.max_span);
    g.idx_base = b.region_beg - g.ext;
    g.nq = (uint32_t)(((int64_t)g.ntiles * tile_step + g.ext) >> IDX_QSHIFT) + 2;
    return g;
}

// ---- PDR + LPMD (launch_pdr_lpmd) ---------------------------------------------------------
// knobs: -1 = not set
struct PdrKnobs {
    int wide = -1;          // MTH_PDR_WIDE: the slice shift 14 .. 16, 0 (any other value) = the dense form
    int wide_w = -1;        // MTH_PDR_WIDE_W: the value as given (its domain depends on the slice: plan_pdr_lpmd)
    bool coarse_off = false;   // MTH_COARSE_INDEX=0
    bool runs = false;      // MTH_TILE_RUNS=1
    int tile_b = -1;        // MTH_TILE_B: 128 / 256 (anything else: not set)
};
struct PdrPlan {
    int wide_shift;         // 0: the dense form
    int tile_w;             // the dense tile's or the wide slice's positions
    uint32_t tile_w_rt;     // wide form: positions per tile where that is not the slice (0: it is)
    uint32_t tile_step, ntiles;
    int32_t idx_base;
    uint32_t nq;
    bool prepared_fits;     // the prepared batch's fine index serves this call
    bool coarse;
    uint32_t coarse_stride;
    bool runs;
    int tile_b;
    uint32_t nbk, n_bucket_words;
    uint32_t hint_stride;   // run form
};
// prepared_nq = 0: the batch is not a prepared one
inline PdrPlan plan_pdr_lpmd(const BatchShape &b, const mth_pdr_lpmd_params_t &p, const PdrKnobs &kn, bool has_sink, bool fused_force,
                             bool pipelined, int32_t prepared_idx_base, uint32_t prepared_nq) {
    PdrPlan pl{};
    const int64_t region_len = b.region_len();
    // Two forms of the tile kernel.  Dense batches: one LDS counter per position, 4096-bp tiles (8192-bp tiles, 4 workgroups per CU:
    // config 3 0.1655 -> 0.1956 ms, config 2 0.0858 -> 0.1069; profiles/r03_stream_kernel.md).  Sparse batches (WGBS depth: few calls
    // per read and few reads per 4096 bp, so that a tile's fixed chain of round trips is what the kernel waits for): hashed sites,
    // 16384- to 65536-bp tiles (mth_pdr_wide.hip).  MTH_PDR_WIDE=0 / 14 / 15 / 16 overrides the choice (tests, A/B).
    int wide_shift = 0;
    if (b.n_reads && region_len > 0) {
        const double sites_per_bp = (double)b.n_cpgs / (double)b.n_reads / (double)std::max(b.max_span, 1);
        const double reads_per_bp = (double)b.n_reads / (double)region_len;
        // (1024 slots: up to ~0.6 of them for the sites a tile can expect; a denser stretch is redone in halves)
        // A hashed insert (compare-and-swap + adds) costs more than the dense form's one LDS add: the wide form only pays while few
        // calls are inserted.  Expected insertions per read = E[n; n >= min_cpgs] = lambda P(N >= min_cpgs - 1) for Poisson calls per
        // read: 0.22 under the CLI defaults at config-3 density (0.117 against 0.170 ms), 1.37 for FDRP's site discovery (min_cpgs 1:
        // 0.202 against 0.153 ms -- that pass keeps the dense form).
        double ins_per_read = 0.0;
        if (p.want_pdr) {
            const double lam = (double)b.n_cpgs / (double)b.n_reads;
            const int kmin = (int)std::min<uint32_t>(std::max<uint32_t>(p.pdr_min_cpgs, 1u), 64u) - 1;     // P(N >= kmin)
            double term = std::exp(-lam), cdf = 0.0;
            for (int k = 0; k < kmin; ++k) { cdf += term; term *= lam / (double)(k + 1); }
            ins_per_read = lam * std::max(0.0, 1.0 - cdf);
        }
        // Depth: measured on a chr1-sized contig at density 0.0091 -- 16 M reads (10x) dense 0.170 / wide 0.113 ms, 24 M 0.201 / 0.160,
        // 32 M 0.238 / 0.196, 48 M (29x) 0.295 / 0.277, each with a gather of 0.027 / 0.008 on top; 65536-bp tiles only lead at 10x.
        if (sites_per_bp <= 0.012 && reads_per_bp * 4096.0 <= 900.0 && ins_per_read <= 0.6)
        {
            wide_shift = sites_per_bp * 65536.0 <= 0.6 * 1024 && reads_per_bp * 65536.0 <= 4500.0 ? 16 : sites_per_bp * 32768.0 <= 0.6 * 1024 ? 15 : 14;
            // ... and enough tiles to fill the chip twice over (7 workgroups on each of 256 CUs): a short contig takes narrower tiles
            // (config 3's 24 contigs: 2.33 -> 2.20 ms; the same rule made the quartet / pairs kernels slower -- 2.36 -> 2.62, 2.72 -> 2.95 ms --
            // whose persistent workgroups gain more from the wider tile than they lose to a half-filled last round)
            while (wide_shift > 14 && (region_len >> wide_shift) < 2 * 7 * 256) --wide_shift;
        }
    }
    if (kn.wide >= 0) wide_shift = kn.wide;
    if (fused_force && wide_shift == 0) wide_shift = 14;       // MTH_MULTI_FUSED on a dense batch
    const int tile_w = wide_shift ? 1 << wide_shift : 4096;
    // Wide form: the tile need not be as wide as its slice.  A chr1-sized contig is 2.12 rounds of 65536-position tiles over the chip's
    // 1 792 resident workgroups (7 on each of 256 CUs) and ends on a nearly empty third round; tiles of region / (3 x 1 792) positions
    // make three full rounds of smaller tiles.  Only where the last round would be less than half full, and never below
    // half the slice (the chain of round trips per tile is what the wide form exists to pay less often).  MTH_PDR_WIDE_W forces a width.
    uint32_t tile_w_rt = 0;
    if (wide_shift) {
        const double slots = 7.0 * 256.0, rounds = (double)region_len / (double)tile_w / slots;
        const double frac = rounds - std::floor(rounds);
        if (rounds > 1.0 && rounds < 8.0 && frac > 0.02 && frac < 0.5) {
            const uint64_t w = (uint64_t)std::ceil((double)region_len / (std::ceil(rounds) * slots));
            const uint32_t wr = (uint32_t)((w + 63) & ~63ull);
            if (wr >= (uint32_t)tile_w / 2 && wr < (uint32_t)tile_w) tile_w_rt = wr;
        }
        if (kn.wide_w >= 0) { const int k = kn.wide_w; tile_w_rt = (k >= 1024 && k < tile_w) ? (uint32_t)k & ~63u : 0u; }
    }
    pl.wide_shift = wide_shift; pl.tile_w = tile_w; pl.tile_w_rt = tile_w_rt;
    pl.tile_step = tile_w_rt ? tile_w_rt : (uint32_t)tile_w;
    const IndexGeom g = index_geometry(b, pl.tile_step);
    pl.ntiles = g.ntiles; pl.idx_base = g.idx_base; pl.nq = g.nq;
    if (pl.ntiles == 0) return pl;

    // The dense tile kernel's own index: one entry per tile in each of two families (k_build_index<2>).  Site discovery for the walk
    // measures (sink) leaves the fine index behind for them; the wide form looks up arbitrary stretch bounds.  MTH_COARSE_INDEX=0: A/B.
    // a prepared batch brings its fine index: no index kernel in this call (k_batch_begin does what else that kernel did)
    pl.prepared_fits = prepared_nq != 0 && prepared_idx_base == pl.idx_base && pl.nq <= prepared_nq;
    pl.coarse = !has_sink && wide_shift == 0 && !kn.coarse_off && !pl.prepared_fits;
    pl.coarse_stride = (pl.ntiles + 2u + 3u) & ~3u;
    // the run form of the dense kernel (k_pdr_lpmd_runs; persistent workgroups, no index, no atomics): opt-in with MTH_TILE_RUNS=1 --
    // parity-green on every PDR / LPMD case, measured SLOWER than the one-tile-per-workgroup form on config 2 (0.127 against 0.084 ms;
    // profiles/r05_persistent.md).  8-bit relative positions, call offsets that fit a buffer descriptor's 32-bit byte offset.
    pl.runs = wide_shift == 0 && b.rel8 && b.n_cpgs < (1u << 30) && kn.runs;
    // threads per workgroup of the one-tile-per-workgroup form: 128 (two waves, two chunks of reads per trip, nine workgroups on a CU;
    // profiles/tile_two_waves.md) for pipelined batches with 8-bit relative positions, 256 for 16-bit ones (built for 256 only) and for
    // a batch outside a pipelined run -- a job's first batch, MTH_PIPELINE=0, site discovery through a sink: alone on the chip the
    // four-wave kernel is the faster one (75.8 against 82.2 us on config 2); the two-wave form wins where the index build, the gather
    // and the other lane's tile kernel run beside it.  MTH_TILE_B=128 / 256 forces either for 8-bit batches.
    pl.tile_b = pipelined ? MTH_TILE_B_DEFAULT : 256;
    if (kn.tile_b >= 0) pl.tile_b = kn.tile_b;
    if (!b.rel8) pl.tile_b = 256;
    pl.nbk = (pl.ntiles + (1u << TILE_BUCKET_SHIFT) - 1) >> TILE_BUCKET_SHIFT;
    pl.n_bucket_words = pl.nbk * 5u;      // rows, 4 LPMD sums per bucket
    pl.hint_stride = (uint32_t)std::max(1.0, std::ceil((double)b.n_reads / (double)pl.ntiles * (1.0 + (double)b.max_span / (double)tile_w) * 1.3 / 63.0));
    return pl;
}

// ---- FDRP / qFDRP (mth_fdrp_accumulate) ---------------------------------------------------
// knobs: -1 = not set
struct FdrpKnobs {
    int wtile = -1;         // METHEOR_FDRP_WTILE: 0 / 1
    int walk4 = -1;         // METHEOR_FDRP_WALK4: lanes per site 0 / 16 / 32 (1 = 16, anything else 0); set at all: no wtile by itself
    int tile = -1;          // METHEOR_FDRP_TILE: 0 / 1; set at all: no wtile by itself
    int win = -1;           // METHEOR_FDRP_WIN: 32 / 64 (anything but 32 is 64)
    bool wide_rows = false; // METHEOR_FDRP_TILE_WIDE_ROWS
};
struct FdrpPlan {
    bool wtile, dense;
    int walk4, win;         // lanes per site of the four-sites-per-wave kernel (0: not taken), sites per window
    bool tile;              // the read x read form (before the launch function weighs its term list against free memory)
    uint64_t bound;         // wtile: candidate sites the tile pass may find (no discovery pass gives the number)
};
inline FdrpPlan plan_fdrp(const BatchShape &d, const mth_fdrp_params_t &params, const FdrpKnobs &kn) {
    FdrpPlan pl{};
    // WGBS depth (about a dozen candidate reads per site -- reads starting in [c - max_span + 1, c + 1]), sparse calls, spans <= 200 bp:
    // ONE tile pass finds the sites and computes them (k_fdrp_wtile, round 6); the general walk only redoes what it hands back.
    // METHEOR_FDRP_WTILE=0 / 1 forces the choice (A/B, tests).
    // dense CpGs (hotspots, RRBS): 16 call registers per stored read keep the per-call match out of
    // the memory loop; sparse WGBS keeps 8 (half the compares per call)
    const bool dense = d.n_reads && ((double)d.n_cpgs / (double)d.n_reads) > 6.0;
    const double cand = (double)d.n_reads * ((double)d.max_span + 2.0) / std::max<double>(1.0, (double)d.region_end - (double)d.region_beg);
    // (round 6: a dense form of the tile pass -- 64-bit masks, sites up to 64 reads, term lists in HBM -- was built for the depths of config 4:
    // parity-green, 4.2 ms against mth_fdrp.hip's k_fdrp_tile + k_fdrp_chain 3.4 ms: profiles/r06_fdrp_dense.md, tools/experiments/)
    // How deep: a site holds up to 64 readers there, but readers beyond max_depth are the reservoir's (handed back), so the depth must
    // stay 4 sigma below max_depth (CLI default 40: ~22 candidate reads a site).  Measured on a chr1-sized contig at density 0.0091,
    // pass ms, this form against rounds 2-5's choice: 16 M reads (10 x) 0.45 / 0.615, 24 M 0.85 / 1.48, 32 M (20 x) 1.26 / 2.91 (the
    // read x read form), 48 M (29 x) 3.06 / 3.45 (hand-backs 0.7), 64 M (39 x) 10.5 / 4.8.  Sparse calls only (<= 2 a read):
    // config 2 -- 25.6 x, 3 calls a read -- 2.1 / 1.35.
    const bool sparse_calls = d.n_reads && (double)d.n_cpgs / (double)d.n_reads <= 2.0;
    bool wtile = sparse_calls && d.max_span <= 200 && cand <= 24.0 && cand + 4.0 * std::sqrt(cand) <= (double)params.max_depth &&
                 kn.walk4 < 0 && kn.tile < 0;
    if (kn.wtile >= 0) wtile = d.max_span <= 200 && kn.wtile != 0;
    // WGBS depth: when a site has about a dozen reads that can call it (reads starting in [c - max_span + 1, c + 1]), four
    // sites share a wave (k_fdrp_walk4<16>) and the general walk only redoes what that kernel handed back.  Measured on a
    // chr1-sized contig (profiles/r02_fdrp_walk4.md): ~10 such reads per site 0.887 -> 0.568 ms, 12 1.29 -> 0.94, 14.6 1.58 -> 1.39,
    // 17 1.79 -> 1.83 (the switch is at 16), ~19.5 per site 1.95 -> 2.17
    // (16 lanes) / 2.13 (32 lanes) -- deeper sites are bound by their pair rounds and keep the wave-per-site walk.
    // METHEOR_FDRP_WALK4=0 / 16 / 32 (1 = 16) forces the choice (A/B, tests).
    int walk4 = (!wtile && !dense && d.max_span <= 200 && cand <= 16.0) ? 16 : 0;                        // lanes per site
    if (kn.walk4 >= 0) walk4 = d.max_span <= 200 ? kn.walk4 : 0;
    // The read x read form (k_fdrp_tile + k_fdrp_chain) for everything the four-sites-per-wave kernel does not take:
    // METHEOR_FDRP_TILE=0 / 1 forces the choice (A/B, tests).
    bool tile = d.max_span <= 200 && !walk4 && !wtile;
    if (kn.tile >= 0) { tile = d.max_span <= 200 && kn.tile != 0 && !wtile; if (tile) walk4 = 0; }
    if (wtile) walk4 = 0;
    // 32-site windows where 32 sites reach well beyond +- 200 bp (at the batch's site density; METHEOR_FDRP_WIN=64 / 32 forces it)
    const double sites_per_bp = d.n_reads ? (double)d.n_cpgs / (double)d.n_reads / (double)std::max(d.max_span, 1) : 0.0;   // (the site count itself is on the device)
    int win = sites_per_bp * 402.0 <= 12.0 ? 32 : 64;
    if (kn.win >= 0) win = kn.win;
    pl.wtile = wtile; pl.dense = dense; pl.walk4 = walk4; pl.win = win; pl.tile = tile;
    if (wtile) {
        // the candidate-site arrays the tile pass fills itself (no discovery pass)
        const uint64_t region_len = (uint64_t)((int64_t)d.region_end - d.region_beg);
        pl.bound = d.n_cpgs < region_len ? d.n_cpgs : region_len;
    }
    return pl;
}
// bytes of the read x read form's term list for `bound` candidate sites:
// sum over sites of C(n, 2) <= (dcap - 1) / 2 x the sum of n <= (dcap - 1) / 2 x the batch's calls; + the 64-byte rounding
inline uint64_t fdrp_term_budget(const BatchShape &d, const mth_fdrp_params_t &params, uint64_t bound) {
    const uint64_t dcap = std::min<uint64_t>(std::max<uint32_t>(params.max_depth, 1u), 64u);
    return (uint64_t)d.n_cpgs * (dcap - 1) / 2 + 64 * bound + 64;
}

// ---- FDRP / qFDRP as one tile pass (launch_fdrp_wtile) ------------------------------------
struct FdrpWtileKnobs {
    int w = -1;             // METHEOR_FDRP_WTILE_W: a multiple of 64 in [64, FW_WMAX]
    bool force_sub = false, force_heavy = false;     // METHEOR_FDRP_WTILE_SUB, METHEOR_FDRP_WTILE_HEAVY
};
// Tile width: the widest whose candidate reads (start in [P0 - max_span + 1, P1]) fill the stretch's two 64-read chunks without
// spilling over too often (mean + 2 sigma <= 128: an overfull tile is redone in halves), at most FW_WMAX.
// (a batch with reads and a region of at least one position)
inline int plan_fdrp_wtile(const BatchShape &d, const FdrpWtileKnobs &kn) {
    int W;
    {
        const double rpb = (double)d.n_reads / (double)d.region_len();
        const double want = (double)FW_RCAP - 2.0 * std::sqrt((double)FW_RCAP);     // ~105 of 128 reads
        W = (int)(want / std::max(rpb, 1e-9)) - d.max_span;
        // ... and their calls the stretch's call lanes (denser calls: a narrower tile rather than a tile redone in halves)
        const double cpr = (double)d.n_cpgs / (double)d.n_reads, wantc = (double)FW_CCAP - 2.0 * std::sqrt((double)FW_CCAP);
        W = std::min(W, (int)(wantc / std::max(rpb * cpr, 1e-9)) - d.max_span);
        W = std::max(256, std::min(FW_WMAX, W)) & ~63;
    }
    if (kn.w >= 0) W = kn.w;
    return W;
}

// ---- MHL as one tile pass (launch_mhl_tile) -----------------------------------------------
struct MhlKnobs {
    bool walk = false;      // MTH_MHL_WALK: site discovery + the per-site walk (the knobs below are the tile pass's: not read then)
    int rowchk = -1;        // MTH_MHL_ROWCHK: 0 / 1
    int tile_shift = -1;    // MTH_MHL_TILE_SHIFT: 12 .. 16
    bool force_sub = false, force_hand_on = false, no_wave_walk = false;    // MTH_MHL_FORCE_SUB, MTH_MHL_FORCE_HAND_ON, MTH_MHL_NO_WAVE_WALK
};
struct MhlPlan { bool rowchk; int shift; };
// (a batch with reads and a region of at least one position)
inline MhlPlan plan_mhl(const BatchShape &d, const mth_mhl_params_t &p, const MhlKnobs &kn) {
    const int64_t region_len = d.region_len();
    // Tile width: up to 0.65 x 256 slots' worth of sites per tile at the batch's call density (a denser stretch is redone in halves)
    // and few enough candidate reads for the 16-bit bins.  A tile is a chain of ~6 dependent round trips and ~10 barriers whatever it
    // holds, so the widest tile that fits wins: config-3 density 0.319 / 0.220 / 0.144 ms at 4096 / 8192 / 16384 bp, config 2 0.209 /
    // 0.204 at 4096 / 8192 (16384 overflows the slots there: 1.27 ms)
    // (round 6: the one-wave-per-tile form that pays for FDRP was built for MHL too -- parity-green and 30 % slower than this kernel, whose
    // tile is eleven times larger: profiles/r06_mhl_wtile.md, tools/experiments/mth_mhl_wtile.hip)
    int shift = 12;
    // the flush rule per read (position bitmap in the tile kernel) or per finished row (k_mhl_rowcheck): rows are few where calls are
    // sparse -- at <= 2 CpGs a read one read in twenty reaches min_cpgs = 4 -- and there the per-read marks (start, a dependent first-call
    // load, bitmap atomics) were 29 % of the tile kernel for a test only the rows need (chr1-sized contig at config-3 density: 0.170 ->
    // 0.130 ms + 0.009 for the row kernel); config 2 (2.94 CpGs a read, 100 rows a tile) keeps the marks
    bool rowchk = (double)d.n_cpgs <= 1.8 * (double)d.n_reads;       // (density sweep, profiles/r06_mhl_rowcheck.md: even at 2.0)
    if (kn.rowchk >= 0) rowchk = kn.rowchk != 0;                     // tests / tuning
    {
        const double cpr = (double)d.n_cpgs / (double)d.n_reads;
        const double sites_per_bp = cpr / (double)std::max(d.max_span, 1);
        const double reads_per_bp = (double)d.n_reads / (double)region_len;
        while (shift < 14 && sites_per_bp * (double)(2 << shift) <= 0.65 * MT_S &&
               reads_per_bp * (double)((2 << shift) + d.max_span + 2 * IDX_Q) <= 0.75 * MT_HEAVY)
            ++shift;
        // Without the marks a tile's cost is its contributors', and a slot is taken only by a site that a CONTRIBUTOR calls: 32 768-position
        // tiles where those sites fit (config 3: MHL pass 2.21 -> 1.56 ms; 65 536 overflows the slots on a chr1-sized contig: 0.092 ->
        // 0.227 ms) and the region still gives three rounds of tiles.  The share of such sites: a covering read has min_cpgs - 1 other
        // CpGs with probability pc (Poisson at the batch's calls per read); overlapping readers are far from independent -- sqrt(depth)
        // of them counted (measured at 10 x: 0.35 of the sites).  An underestimate costs time only (the stretch is redone in halves).
        if (rowchk && shift == 14) {
            double pc = 1.0, term = std::exp(-cpr);
            for (uint32_t k = 0; k + 1 < p.min_cpgs && k < 64; ++k) { pc -= term; term *= cpr / (double)(k + 1); }
            pc = std::min(1.0, std::max(pc, 0.0));
            const double depth = reads_per_bp * (double)std::max(d.max_span, 1);
            const double share = 1.0 - std::pow(1.0 - pc, std::max(1.0, std::sqrt(depth)));
            if (sites_per_bp * share * 32768.0 <= 0.5 * MT_S && reads_per_bp * (double)(32768 + d.max_span + 2 * IDX_Q) <= 0.75 * MT_HEAVY &&
                region_len >= 3ll * 1536 * 32768)
                shift = 15;
        }
    }
    if (kn.tile_shift >= 0) shift = kn.tile_shift;                   // tests / tuning
    return MhlPlan{rowchk, shift};
}

// ---- ME / PM and LPMD pairs (the tile-row driver, mth_tile_rows.hip) ----------------------
// Tile width: wide tiles pay the per-tile costs (index look-up, LDS clear, barriers, halo reads) less often, but the
// table holds QT_S quartets and a 16-bit bin 65535 candidate reads.  About one quartet starts per CpG site; sites per
// bp ~ calls per read / read length (max_span stands in for the length).  Tiles that overflow anyway take the global path.
// shift_knob: MTH_QUARTET_TILE_SHIFT as 13 .. 16, -1 = not set
inline int quartet_tile_shift(const BatchShape &d, int shift_knob) {
    const int64_t region_len = d.region_len();
    int tile_shift = 13;
    if (d.n_reads && region_len > 0) {
        const double sites_per_bp = (double)d.n_cpgs / (double)d.n_reads / (double)std::max(d.max_span, 1);
        const double reads_per_bp = (double)d.n_reads / (double)region_len;
        // a site starts a quartet only if three more sites follow within a read's span: Poisson tail P(>= 3 | sites_per_bp x span).
        // (Without it config 2 stayed at 8192 bp and config-3 density at 16384: 0.119 against 0.100 ms at 16384 and 0.159 against
        // 0.112 ms at 32768 -- a tile's fixed chain of round trips and barriers is what these kernels wait for.)
        const double lam = sites_per_bp * (double)std::max(d.max_span, 1);
        const double p3 = std::max(0.05, 1.0 - std::exp(-lam) * (1.0 + lam + 0.5 * lam * lam));
        while (tile_shift < 16 && sites_per_bp * p3 * (double)(2 << tile_shift) <= 0.4 * QT_S &&
               reads_per_bp * (double)((2 << tile_shift) + d.max_span + 2 * IDX_Q) <= 30000.0)
            ++tile_shift;
    }
    if (shift_knob >= 0) tile_shift = shift_knob;   // tests / tuning
    return tile_shift;
}
// Tile width (see quartet_tile_shift): distinct pairs per tile ~ sites per tile x sites per pair window
// shift_knob: MTH_PAIRS_TILE_SHIFT as 13 .. 16, -1 = not set
inline int pairs_tile_shift(const BatchShape &d, const mth_lpmd_pairs_params_t &p, int shift_knob) {
    const int64_t region_len = d.region_len();
    int tile_shift = 13;
    if (d.n_reads && region_len > 0) {
        const double sites_per_bp = (double)d.n_cpgs / (double)d.n_reads / (double)std::max(d.max_span, 1);
        const double reads_per_bp = (double)d.n_reads / (double)region_len;
        const double window = std::max(1.0, (double)std::min<int64_t>((int64_t)p.max_distance - std::max(p.min_distance, 0) + 1, d.max_span));
        while (tile_shift < 16 && sites_per_bp * (double)(2 << tile_shift) * std::max(1.0, sites_per_bp * window) <= 0.3 * PT_S &&
               reads_per_bp * (double)((2 << tile_shift) + d.max_span + 2 * IDX_Q) <= 30000.0)
            ++tile_shift;
    }
    if (shift_knob >= 0) tile_shift = shift_knob;   // tests / tuning
    return tile_shift;
}

}  // namespace mth
