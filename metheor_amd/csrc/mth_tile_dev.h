// mth_tile_dev.h -- device helpers shared by the PDR + LPMD kernels (mth_pdr_lpmd.hip: dense tile kernel, mth_pdr_wide.hip: hashed-site form
// and, from the same body, the fused PDR + LPMD + ME / PM kernel).
#pragma once
#include "mth_common.h"
#include "mth_lpmd_bytes.h"

namespace mth {

// ---------------------------------------------------------------------------------------------
// DPP controls (gfx9 family): no LDS traffic, one VALU per step
#define MTH_DPP(v, ctrl, rmask, bctl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rmask), 0xf, (bctl)))
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {   // wave-uniform result
    v += MTH_DPP(v, 0xb1 /*quad_perm [1,0,3,2]*/, 0xf, true);
    v += MTH_DPP(v, 0x4e /*quad_perm [2,3,0,1]*/, 0xf, true);
    v += MTH_DPP(v, 0x141 /*row_half_mirror*/, 0xf, true);
    v += MTH_DPP(v, 0x140 /*row_mirror*/, 0xf, true);          // every lane: sum of its row of 16
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v += MTH_DPP(v, 0x111 /*row_shr:1*/, 0xf, true);
    v += MTH_DPP(v, 0x112 /*row_shr:2*/, 0xf, true);
    v += MTH_DPP(v, 0x114 /*row_shr:4*/, 0xf, true);
    v += MTH_DPP(v, 0x118 /*row_shr:8*/, 0xf, true);
    v += MTH_DPP(v, 0x142 /*row_bcast:15*/, 0xa, false);
    v += MTH_DPP(v, 0x143 /*row_bcast:31*/, 0xc, false);
    return v;
}

// arguments of the PDR + LPMD tile kernels (mth_pdr_lpmd.hip: dense counters, 4096-bp tiles; mth_pdr_wide.hip: hashed sites, wide tiles)
struct TileArgs {
    const int32_t  *read_start;
    const uint8_t  *read_mapq;
    const uint32_t *cpg_off;
    const uint32_t *cpg_pos;
    const void     *cpg_rel;
    const uint32_t *idx;
    const uint32_t *idx2;         // dense kernel only: second family of its tile-granular index (nullptr: idx is the fine index)
    const DevState *st;
    uint32_t *tile_cnt;
    unsigned long long *bucket;   // per 256-tile bucket: [nbk] rows, then [nbk][4] LPMD partial sums
    uint32_t nbk;
    SiteRec  *scratch;     // TILE_W rows per tile
    int32_t region_beg, region_end, idx_base, max_span;
    uint32_t n_reads, n_cpgs;
    uint32_t min_cov;      // max(pdr_min_depth, 1)
    uint32_t min_cpgs;
    int32_t  min_dist, max_dist;
    uint8_t  pdr_min_qual, lpmd_min_qual, want_pdr, want_lpmd;
    uint32_t tile_w_rt;    // wide form only: positions per tile when it is not the slice width 1 << SHIFT (0: it is) -- see plan_pdr_lpmd
#ifdef MTH_TILE_TRACE
    unsigned long long *trace;     // experiment build: 8 ticks per tile (tools/tile_trace.py)
#endif
};

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));

// ---- per-slot liveness without compare + select (profiles/r02_ubench_valu.md: v_cmp, v_cndmask, v_min/max are half rate) ----
// The live call slots of a read are a PREFIX (k < n), so everything that depends on "slot k is dead" is a function of n
// alone.  It lives in two registers, not in LDS: LB(n) = 0x80 in byte k of 64 bits iff k < min(n, 8) (lpmd_live_bytes, mth_lpmd_bytes.h:
// a shift of a constant by the call count).  From it, each where it is used,
//   slot_mask(LB, k)   0xffffffff if k < n else 0 (v_bfe_i32)     -> masks for the span check / dead-word insertion
//   LB >> 8 g          0x80 in byte j iff the pair (j, j + g) is live: the byte form's mask of diagonal g (mth_lpmd_bytes.h)
// (These were 9-row LDS tables, mtab and m8, read at the top of every chunk of 64 reads and once per diagonal: LDS round trips queued
// behind the previous chunk's scatter atomics with nothing of the wave's own to cover them; profiles/tile_loop_lds.md.  The hashed-site
// and fused kernels keep them: SlotTabsMasks below.)
// One table is left in the dense tile and run kernels, for the windows the byte form does not take, and only a launch with such a window builds it (slot_tabs_init):
//   dtab[n][c]   relpos offsets of the packed fields (below) that push every dead slot 0x400 * (k + 1) past the live
//                ones, so that any distance involving a dead slot is >= 0x400 - 255 and all distances stay >= 0
// ---- windowed pair counts on 8-bit relpos ----
// Four pairs per instruction on the bytes as loaded (mth_lpmd_bytes.h) while the window allows it (min <= 128, max <= 127: the
// command line's 2 / 16 and anything near it); two pairs per instruction on 16-bit fields otherwise (lpmd_pairs_fields16 below).
// lpmd_pairs8 picks one per launch: the window comes from the kernel arguments.
// hashed-site form for sparse batches (mth_pdr_wide.hip): shift = log2 of the tile width (14 or 15)
void launch_tile_wide(const TileArgs &a, uint32_t ntiles, int shift, bool rel8, hipStream_t s);

// The fused PDR + LPMD + ME / PM tile pass (k_multi_tile, mth_pdr_wide.hip: the wide form's body with the quartet side on; host side in
// mth_multi.hip): k_pdr_lpmd_wide's outputs plus k_quartet_tile's per-tile quartet rows.
// Filled in by mth_multi_accumulate and handed to launch_pdr_lpmd through ctx->fuse_q; launch_pdr_lpmd sets taken / ntiles when its
// wide form ran as the fused pass.
struct FusedQuartet {
    uint8_t force;                 // MTH_MULTI_FUSED: the wide form even where launch_pdr_lpmd would take the dense one
    uint8_t force_heavy;           // tests: every tile is handed back
    uint8_t min_qual;              // me.rs:115 / pm.rs:110
    unsigned long long *qs;        // the quartet state words: [1] rows claimed so far, [5] tiles handed back, [6] rows beyond row_cap
    unsigned long long row_cap;    // rows the quartet outputs hold
    uint32_t max_tiles;            // tiles the per-tile arrays below hold
    uint32_t *tile_flag;           // per tile of the batch: 1 = handed back
    unsigned long long *tile_row0; // per tile: first row ...
    uint32_t *tile_rows;           // ... and the number of rows
    int32_t *out_pos; uint32_t *out_cnt; float *out_me, *out_pm; uint32_t *out_depth;
    bool taken;                    // out: the fused pass ran
    uint32_t ntiles;               // out: its tiles
};
void launch_tile_fused(const TileArgs &a, const FusedQuartet &q, uint32_t ntiles, int shift, bool rel8, hipStream_t s);

struct SlotTabs {
    uint32_t dtab[9][8];
};
// does this launch count its pairs on 16-bit fields (and read dtab)?  The window as the kernels clamp it for 8-bit relpos; wave-uniform
__device__ __forceinline__ bool slot_tabs_wanted(const TileArgs &a) {
    return a.want_lpmd && !lpmd_bytes_domain(max(a.min_dist, 0), min(a.max_dist, 255));
}
// Before the workgroup's first barrier.  A launch whose window the byte form takes issues nothing here.  (72 threads fill the table in one step.)
__device__ __forceinline__ void slot_tabs_init(SlotTabs &T, const int tid, const bool wanted) {
    if (wanted && tid < 72) {
        const uint32_t nn = (uint32_t)tid >> 3, c = (uint32_t)tid & 7u;
        auto dead = [&](uint32_t k) { return k >= 8u ? 0x2400u : (k >= nn ? 0x400u * (k + 1u) : 0u); };
        const uint32_t lo = c < 4 ? 2u * c : 2u * (c - 4u) + 1u;       // first slot of the packed register Q_c / O_(c-4)
        T.dtab[nn][c] = dead(lo) | (dead(lo + 1u) << 16);
    }
}
// The table form of the same masks, for the hashed-site and fused kernels (mth_pdr_wide.hip, PW_TABLE_MASKS): seven waves a SIMD cover
// an LDS read there, and the dozen vector instructions a read that replace it cost 1.7 % of the hashed-site kernel (profiles/tile_loop_lds.md)
//   mtab[n][k]   0xffffffff if k < n else 0
//   m8[n][g]     LB(n) >> 8 g, the two words of the byte form's mask of diagonal g
struct SlotTabsMasks : SlotTabs {
    uint32_t mtab[9][8];
    LpMask   m8[9][8];
};
// (256 threads: every table in one step, built by every launch)
__device__ __forceinline__ void slot_tabs_init(SlotTabsMasks &T, const int tid) {
    slot_tabs_init(static_cast<SlotTabs &>(T), tid, true);
    if (tid < 144) (&T.m8[0][0].w0)[tid] = lpmd_bytes_mask((uint32_t)tid >> 4, ((uint32_t)tid >> 1) & 7u, (uint32_t)tid & 1u);
    if (tid < 72) T.mtab[(uint32_t)tid >> 3][(uint32_t)tid & 7u] = ((uint32_t)tid & 7u) < ((uint32_t)tid >> 3) ? 0xffffffffu : 0u;
}
// 0xffffffff if slot k is live else 0: the sign extension of bit 8 k + 7 of LB (one v_bfe_i32 where the mask is used)
__device__ __forceinline__ uint32_t slot_mask(const LpMask lb, const int k) {
    return (uint32_t)((int32_t)((k < 4 ? lb.w0 : lb.w1) << (24 - 8 * (k & 3))) >> 31);
}
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }   // v_bfi_b32

// Windowed pair counts, two pairs per instruction: any window up to the 255 an 8-bit relpos can span.
// Slots are packed two per register as 16-bit fields: Q_e = (slot 2e, slot 2e+1), O_e = (slot 2e+1, slot 2e+2), slot 8
// being a dummy that is always dead.  The pairs at call-index gap g are then  later - earlier  with earlier = Q_m and
// later = O_{(g-1)/2+m} (g odd) or Q_{g/2+m} (g even): one 32-bit subtraction gives two distances (no borrows: relpos
// ascends with the slot, dead offsets ascend faster).  With A = D + (0x8000 - min) and B = (0x8000 + max) - D per
// field, bit 15 of A & B says "min <= distance <= max"; the call states sit in bit 15 of a second set of packed words,
// so one xor + and gives "in the window and discordant".  Only full-rate VALU ops (add / sub / and / xor / or / shift).
__device__ __forceinline__ void lpmd_pairs_fields16(const uint32_t (&v)[8], const uint32_t rraw0, const uint32_t rraw1, const uint32_t *drow,
                                                    const uint32_t mind, const uint32_t maxd, uint32_t &lp_c, uint32_t &lp_d) {
    // packed call states (bit 15 of each field; the other bits of the top bytes are ignored by the masks below)
    uint32_t SQ[4], SO[4], Q[4], O[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) SQ[e] = __builtin_amdgcn_perm(v[2 * e + 1], v[2 * e], 0x070c030cu);
#pragma unroll
    for (int e = 0; e < 3; ++e) SO[e] = __builtin_amdgcn_perm(v[2 * e + 2], v[2 * e + 1], 0x070c030cu);
    SO[3] = __builtin_amdgcn_perm(0u, v[7], 0x070c030cu);
    Q[0] = __builtin_amdgcn_perm(0u, rraw0, 0x0c010c00u); Q[1] = __builtin_amdgcn_perm(0u, rraw0, 0x0c030c02u);
    Q[2] = __builtin_amdgcn_perm(0u, rraw1, 0x0c010c00u); Q[3] = __builtin_amdgcn_perm(0u, rraw1, 0x0c030c02u);
    O[0] = __builtin_amdgcn_perm(0u, rraw0, 0x0c020c01u); O[1] = __builtin_amdgcn_perm(rraw1, rraw0, 0x0c040c03u);
    O[2] = __builtin_amdgcn_perm(0u, rraw1, 0x0c020c01u); O[3] = __builtin_amdgcn_perm(0u, rraw1, 0x0c0c0c03u);
    {
        const uint4 da = reinterpret_cast<const uint4 *>(drow)[0], db = reinterpret_cast<const uint4 *>(drow)[1];
        Q[0] += da.x; Q[1] += da.y; Q[2] += da.z; Q[3] += da.w; O[0] += db.x; O[1] += db.y; O[2] += db.z; O[3] += db.w;
    }
    const uint32_t KA = (0x8000u - mind) * 0x10001u, KB = (0x8000u + maxd) * 0x10001u;
    uint32_t accIN = 0, accDD = 0;
#pragma unroll
    for (int g = 1; g < 8; ++g) {
        // The fields of the registers m = 0, 1, .. are the pairs (0, g), (1, 1 + g), .. in order, so two adjacent pairs within max are
        // two neighbouring fields with bit 15 of Bw set: the exit rule of mth_lpmd_bytes.h (a pair on diagonal g + 1 needs two adjacent
        // ones on g), with v_alignbit_b32 bringing the next register's low field beside this one's high field
        uint32_t adjB = 0, prevB = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int li = (g & 1) ? (g - 1) / 2 + m : g / 2 + m;      // index of the later operand in O (g odd) / Q (g even)
            if (li > 3) break;
            const uint32_t later = (g & 1) ? O[li] : Q[li], sl = (g & 1) ? SO[li] : SQ[li];
            const uint32_t D = later - Q[m];
            const uint32_t Bw = KB - D;
            const uint32_t IN = __builtin_amdgcn_bitop3_b32(D + KA, Bw, 0x80008000u, 0x80);   // min <= distance <= max (readutil.rs:184, 196)
            const uint32_t DD = IN & (sl ^ SQ[m]);
            accIN += __builtin_popcount(IN);        // v_bcnt_u32_b32 adds its second operand: one instruction per count
            accDD += __builtin_popcount(DD);
            if (m > 0) adjB |= prevB & __builtin_amdgcn_alignbit(Bw, prevB, 16);
            prevB = Bw;
        }
        adjB |= prevB & (prevB >> 16);
        if (!__any((adjB & 0x80008000u) != 0u)) break;      // no lane has two adjacent pairs within max_distance on this diagonal
    }
    lp_c += accIN - accDD;
    lp_d += accDD;
}

// The pairs among a read's first 8 calls (readutil.rs:166-224): v = its call words (dead slots: any word), rraw0 / rraw1 = its 8
// relpos bytes as loaded (dead slots: any byte), lb = LB(n) of its n calls, lp_ok = its pairs count (false: count nothing), [mind, maxd] =
// the window, 0 <= mind, mind <= maxd <= 255 (the callers have excluded an empty window).  The lanes of a wave that have a read call it
// together: the early exit is a vote among them.
__device__ __forceinline__ void lpmd_pairs8(const uint32_t (&v)[8], const uint32_t rraw0, const uint32_t rraw1, const uint32_t n, const bool lp_ok,
                                            const LpMask lb, const SlotTabs &T, const int32_t mind, const int32_t maxd, uint32_t &lp_c, uint32_t &lp_d) {
    if (lpmd_bytes_domain(mind, maxd))
        lpmd_pairs_bytes(rraw0, rraw1, lpmd_state_bytes(v[0], v[1], v[2], v[3]), lpmd_state_bytes(v[4], v[5], v[6], v[7]), lp_ok ? lb.w0 : 0u,
                         lp_ok ? lb.w1 : 0u, (uint32_t)mind, (uint32_t)maxd, lp_c, lp_d);
    else
        lpmd_pairs_fields16(v, rraw0, rraw1, &T.dtab[lp_ok ? min(n, 8u) : 0u][0], (uint32_t)mind, (uint32_t)maxd, lp_c, lp_d);      // (slot_tabs_wanted: built)
}
// the table form: n_lp = live slots whose pairs count (0: count nothing), the row of either table
__device__ __forceinline__ void lpmd_pairs8(const uint32_t (&v)[8], const uint32_t rraw0, const uint32_t rraw1, const uint32_t n_lp,
                                            const SlotTabsMasks &T, const int32_t mind, const int32_t maxd, uint32_t &lp_c, uint32_t &lp_d) {
    if (lpmd_bytes_domain(mind, maxd))
        lpmd_pairs_bytes(rraw0, rraw1, lpmd_state_bytes(v[0], v[1], v[2], v[3]), lpmd_state_bytes(v[4], v[5], v[6], v[7]), &T.m8[n_lp][0],
                         (uint32_t)mind, (uint32_t)maxd, lp_c, lp_d);
    else
        lpmd_pairs_fields16(v, rraw0, rraw1, &T.dtab[n_lp][0], (uint32_t)mind, (uint32_t)maxd, lp_c, lp_d);
}


}  // namespace mth
