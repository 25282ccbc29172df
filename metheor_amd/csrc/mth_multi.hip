// mth_multi.hip -- mth_multi_accumulate: every requested measure over ONE batch (the entry point of `metheor all`), and the fused
// PDR + LPMD + ME / PM tile pass it runs on sparse batches (gfx950, wave64).
//
// Each measure's own entry point replaces one compute_helper pass of the reference over the file (pdr.rs:119, lpmd.rs:154, me.rs:90,
// pm.rs:85, mhl.rs:135, fdrp.rs:176, qfdrp.rs:188).  mth_multi_accumulate prepares the batch once (one device copy, one read index)
// and runs the requested measures over it.  PDR + LPMD (k_pdr_lpmd_wide, mth_pdr_wide.hip) and ME / PM (k_quartet_tile,
// mth_quartet.hip) have the same shape -- phase 1 reads cpg_off / start / mapq of every candidate read of a tile and queues the reads
// with work, phase 2 walks the queue with every lane live, rows are bucket-sorted out of an LDS table whose size does not grow with the
// tile -- so where launch_pdr_lpmd takes the wide form, k_multi_tile does both from ONE walk:
//   queue      a read enters if LPMD (>= 2 calls, lpmd mapq), PDR (>= min_cpgs calls, pdr mapq) or ME / PM (>= 4 calls, quartet mapq)
//              has work for it; each measure keeps its own filters in phase 2
//   phase 2    a queued read's calls are loaded once (two 16-byte loads) and feed the PDR site table, the LPMD sums and the quartet
//              table (512 slots, sixteen 16-bit bins each)
//   outputs    the PDR side exactly as k_pdr_lpmd_wide writes it (scratch slices, tile_cnt, bucket sums: k_gather, mth_pdr_fetch, site
//              discovery unchanged); the quartet side as k_quartet_tile writes it (per-tile tile_row0 / tile_rows, the batch's meta:
//              mth_quartet_fetch unchanged)
//   hand back  a tile with more than 65 535 candidate reads (16-bit bins), more distinct quartets than slots, or a wide quartet (two
//              consecutive CpGs >= 2048 bp apart) is flagged; the host then redoes the batch's ME / PM side through
//              mth_quartet_accumulate, whose global path gives those rows.  A stretch with more PDR sites than slots is redone in halves
//              (PDR + LPMD only: the quartet table is complete after the tile's first stretch, which is the whole tile).
// Where launch_pdr_lpmd takes the dense per-position kernel (dense batches), MTH_MULTI_AUTO runs the two existing passes; MTH_MULTI_FUSED
// takes the fused pass on any batch (16384-bp slices on a dense one).  Synchronous per batch.
#include <cstdlib>

#include "mth_ctx.h"
#include "mth_quartet_dev.h"
#include "mth_tile_dev.h"

namespace mth {

// the wide kernel's constants, with a 2048-read queue: LDS per workgroup ~36.6 KiB (site table 12, quartet table 20, queue 4) ->
// four workgroups per CU
constexpr int PW_S = 1024, PW_B = 256, PW_U = 2, PW_NB = 8, PW_QCAP = 2048;
constexpr uint32_t PW_EMPTY = 0xffffffffu;
constexpr int FQ_S = 512, FQ_OCC = 4;

template <int SHIFT, typename RelT>
__global__ __launch_bounds__(PW_B, FQ_OCC) void k_multi_tile(const TileArgs a, const FusedQuartet q, const uint32_t ntiles) {
    constexpr int W = 1 << SHIFT;
    constexpr bool PACKED = sizeof(RelT) == 1;                 // 8-bit relpos: the packed pair form
    __shared__ uint32_t tkey[PW_S], tcov[PW_S], tdisc[PW_S];   // the site table; in the row phase: keys / counters in bucket order
    __shared__ uint32_t bcnt[PW_B];
    // the work queue of the read phases shares its LDS with the row phase's bucket bases
    __shared__ uint32_t q_or_sort[PW_QCAP / 2];
    static_assert(PW_QCAP / 2 >= PW_B, "bbase fits under the queue");
    uint16_t *const rq = reinterpret_cast<uint16_t *>(q_or_sort);
    uint32_t *const bbase = q_or_sort;
    __shared__ uint32_t red[4][PW_B / 64], ws[PW_B / 64 + 1];
    __shared__ __attribute__((aligned(16))) SlotTabs tabs;
    __shared__ uint32_t s_over, s_qn;
    // the quartet table (k_quartet_tile's: 64-bit key, sixteen 16-bit bins in 8 words); it lives for the whole tile
    __shared__ unsigned long long qkeys[FQ_S];
    __shared__ uint32_t qbins[FQ_S * 8];
    __shared__ uint32_t s_qheavy;
    __shared__ unsigned long long s_qrow0;
    static_assert(PW_QCAP / 2 >= PW_B + FQ_S / 2, "the quartet row phase's bucket bases and source slots fit under the queue");
    static_assert(PW_QCAP <= 65536, "queue entries are 16-bit read numbers");
    static_assert(FQ_S % PW_B == 0 && PW_B == 256 && FQ_S <= 65536, "each thread owns FQ_S / PW_B slots and one bucket; 16-bit source slots");
    uint16_t *const sslot = reinterpret_cast<uint16_t *>(q_or_sort + PW_B);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block b runs on XCD b % 8 (observed; speed only): give each XCD a contiguous run of tiles
    const uint32_t per_xcd = (ntiles + 7) / 8;
    const uint32_t t = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (t >= ntiles) return;
    // (a tile may be narrower than its scratch slice: the host picks the width that fills whole rounds of resident workgroups)
    const uint32_t Wt = a.tile_w_rt ? a.tile_w_rt : (uint32_t)W;
    const int32_t T0 = a.region_beg + (int32_t)(t * Wt);
    const int32_t T1 = (int32_t)min((int64_t)T0 + Wt, (int64_t)a.region_end);
    const RelT *__restrict__ rel = reinterpret_cast<const RelT *>(a.cpg_rel);
    SiteRec *__restrict__ out = a.scratch + (size_t)t * W;
    slot_tabs_init(tabs, tid);
    for (int i = tid; i < FQ_S; i += PW_B) qkeys[i] = QKEY_EMPTY;
    for (int i = tid; i < FQ_S * 8; i += PW_B) qbins[i] = 0u;
    {
        // the tile's candidate reads (the first stretch is the whole tile): a bin counts at most one update per read -> 16 bits hold
        // 65535 candidates (k_quartet_tile's rule); beyond that, or on a test's request, the tile is handed back
        const uint32_t lo = min(a.idx[((uint32_t)T0 - (uint32_t)a.max_span + 1u - (uint32_t)a.idx_base) >> IDX_QSHIFT], a.n_reads);
        const uint32_t hi = min(a.idx[(((uint32_t)T1 - (uint32_t)a.idx_base) >> IDX_QSHIFT) + 1], a.n_reads);
        if (tid == 0) s_qheavy = (hi > lo && hi - lo > 65535u) || q.force_heavy ? 1u : 0u;
    }
    // one window of four consecutive calls (readutil.rs:105-129) into the tile's quartet table; the quartet belongs to the tile of p1
    auto window = [&](const uint32_t x, const uint32_t y, const uint32_t z, const uint32_t w) {
        const int32_t p1 = (int32_t)(x & 0x7fffffffu);
        if (p1 < T0 || p1 >= T1) return;
        const uint32_t d2 = (y & 0x7fffffffu) - (x & 0x7fffffffu), d3 = (z & 0x7fffffffu) - (y & 0x7fffffffu),
                       d4 = (w & 0x7fffffffu) - (z & 0x7fffffffu);
        const unsigned long long key = ((unsigned long long)(uint32_t)p1 << 33) | ((unsigned long long)d2 << 22) |
                                       ((unsigned long long)d3 << 11) | (unsigned long long)d4;
        if (d2 - 1u >= 2047u || d3 - 1u >= 2047u || d4 - 1u >= 2047u || key == QKEY_EMPTY) { s_qheavy = 1u; return; }   // a wide quartet
        const uint32_t pat = ((x >> 31) << 3) | ((y >> 31) << 2) | ((z >> 31) << 1) | (w >> 31);
        uint32_t h = quartet_slot(key, FQ_S - 1), probes = 0;
        while (probes++ < (uint32_t)FQ_S) {
            const unsigned long long cur = atomicCAS(&qkeys[h], QKEY_EMPTY, key);
            if (cur == QKEY_EMPTY || cur == key) { atomicAdd(&qbins[h * 8 + (pat >> 1)], (pat & 1u) ? 0x10000u : 1u); return; }   // me.rs:121-125
            h = (h + 1) & (FQ_S - 1);
        }
        s_qheavy = 1u;                                       // more distinct quartets than slots
    };
    bool q_on = true;                                        // block-uniform: the quartet side is fed by the tile's first stretch only
    // (distances between live calls are < 2^16, so capping max_distance keeps dead-slot differences outside)
    const int32_t maxd = PACKED ? min(a.max_dist, 255) : min(a.max_dist, 1 << 20);   // 8-bit relpos: no distance beyond 255
    const int32_t mind = max(a.min_dist, 0);
    const bool lp_possible = a.want_lpmd && maxd >= a.min_dist && maxd >= 0;          // min > max: no pair can qualify
    uint32_t lp_c = 0, lp_d = 0, n_read = 0, n_valid = 0;      // the thread's LPMD sums over the finished stretches
    uint32_t rows_out = 0, bad = 0;
    int sub_shift = SHIFT;                                     // log2 of the stretch of positions worked on (block-uniform)
    for (int64_t P0l = T0; P0l < T1;) {
        const int32_t P0 = (int32_t)P0l;
        const int32_t P1 = (int32_t)min(P0l + (1ll << sub_shift), (int64_t)T1);
        const uint32_t Wp = (uint32_t)(P1 - P0);
        // candidate reads: start in [P0 - max_span + 1, P1]  (a call sits in [start - 1, start - 1 + max_span])
        const uint32_t lo = min(a.idx[((uint32_t)P0 - (uint32_t)a.max_span + 1u - (uint32_t)a.idx_base) >> IDX_QSHIFT], a.n_reads);
        const uint32_t hi = min(a.idx[(((uint32_t)P1 - (uint32_t)a.idx_base) >> IDX_QSHIFT) + 1], a.n_reads);
        for (int i = tid; i < PW_S; i += PW_B) { tkey[i] = PW_EMPTY; tcov[i] = 0u; tdisc[i] = 0u; }
        bcnt[tid] = 0u;
        if (tid == 0) { s_over = 0u; s_qn = 0u; }
        __syncthreads();
        uint32_t a_c = 0, a_d = 0, a_r = 0, a_v = 0;           // this attempt's LPMD sums
        for (uint32_t c0 = lo; c0 < hi; c0 += PW_QCAP) {
            const uint32_t c1 = min(c0 + (uint32_t)PW_QCAP, hi);
            if (c0 != lo) {
                __syncthreads();                               // the previous stretch's queue is done with
                if (tid == 0) s_qn = 0u;
                __syncthreads();
            }
            // ---- phase 1
            uint32_t o0s[PW_U], o1s[PW_U];
#pragma unroll
            for (int u = 0; u < PW_U; ++u) {
                const uint32_t ii = min(c0 + (uint32_t)u * PW_B + tid, c1 - 1);
                o0s[u] = a.cpg_off[ii]; o1s[u] = a.cpg_off[ii + 1];
            }
            for (uint32_t b0 = c0; b0 < c1; b0 += PW_B * PW_U) {
                int32_t st[PW_U];
                uint32_t mq[PW_U], o0n[PW_U], o1n[PW_U];
#pragma unroll
                for (int u = 0; u < PW_U; ++u) {
                    const uint32_t i = b0 + (uint32_t)u * PW_B + tid, ii = min(i, c1 - 1);
                    st[u] = a.read_start[ii]; mq[u] = a.read_mapq[ii];
                    const uint32_t in = min(i + (uint32_t)PW_U * PW_B, c1 - 1);
                    o0n[u] = a.cpg_off[in]; o1n[u] = a.cpg_off[in + 1];
                }
#pragma unroll
                for (int u = 0; u < PW_U; ++u) {
                    const uint32_t i = b0 + (uint32_t)u * PW_B + tid;
                    const bool in = i < c1;
                    const uint32_t n = in ? o1s[u] - o0s[u] : 0u;
                    const bool owned = in && st[u] >= P0 && st[u] < P1;
                    // lpmd.rs:176-179
                    const bool lp_ok = a.want_lpmd && owned && mq[u] >= a.lpmd_min_qual;
                    if (a.want_lpmd && owned) { a_r += 1; a_v += lp_ok ? 1u : 0u; }
                    // pdr.rs:147-157
                    const bool pdr_ok = a.want_pdr && n >= a.min_cpgs && mq[u] >= a.pdr_min_qual && n > 0;
                    const bool q_ok = q_on && in && n >= 4 && mq[u] >= q.min_qual;       // readutil.rs:101, me.rs:115
                    const bool work = (lp_ok && lp_possible && n > 1) || pdr_ok || q_ok;
                    const unsigned long long bal = __ballot(work);
                    if (bal) {
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(&s_qn, (uint32_t)__builtin_popcountll(bal));
                        base = __builtin_amdgcn_readfirstlane(base);
                        if (work) rq[base + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = (uint16_t)(i - c0);
                    }
                }
#pragma unroll
                for (int u = 0; u < PW_U; ++u) { o0s[u] = o0n[u]; o1s[u] = o1n[u]; }
            }
            __syncthreads();
            // ---- phase 2
            const uint32_t qn = s_qn;
            for (uint32_t j0 = 0; j0 < qn; j0 += PW_B) {
                const uint32_t j = j0 + tid;
                const bool act = j < qn;
                const uint32_t i = c0 + (act ? (uint32_t)rq[j] : 0u);
                const uint32_t o0 = a.cpg_off[i], o1 = a.cpg_off[i + 1];
                const uint32_t n = act ? o1 - o0 : 0u;
                uint32_t v[PW_NB] = {0, 0, 0, 0, 0, 0, 0, 0};
                int32_t r[PW_NB] = {0, 0, 0, 0, 0, 0, 0, 0};
                uint32_t rraw0 = 0, rraw1 = 0;
                static_assert(PW_NB == 8, "two 16-byte loads per read");
                if (__all(!act || (unsigned long long)o0 + PW_NB <= (unsigned long long)a.n_cpgs)) {
                    if (act) {
                        const u32x4_a4 x = *reinterpret_cast<const u32x4_a4 *>(a.cpg_pos + o0), y = *reinterpret_cast<const u32x4_a4 *>(a.cpg_pos + o0 + 4);
                        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
                        if constexpr (PACKED) { const u32x2_a1 z = *reinterpret_cast<const u32x2_a1 *>(rel + o0); rraw0 = z.x; rraw1 = z.y; }
                        else {
                            const u32x4_a2 z = *reinterpret_cast<const u32x4_a2 *>(rel + o0);
                            r[0] = (int32_t)(z.x & 0xffffu); r[1] = (int32_t)(z.x >> 16); r[2] = (int32_t)(z.y & 0xffffu); r[3] = (int32_t)(z.y >> 16);
                            r[4] = (int32_t)(z.z & 0xffffu); r[5] = (int32_t)(z.z >> 16); r[6] = (int32_t)(z.w & 0xffffu); r[7] = (int32_t)(z.w >> 16);
                        }
                    }
                } else if (act) {                               // the batch's last reads: a window of 8 would leave the arrays
#pragma unroll
                    for (int k = 0; k < PW_NB; ++k) {
                        const uint32_t kk = o0 + min((uint32_t)k, n - 1);
                        v[k] = a.cpg_pos[kk];
                        const uint32_t rv = (uint32_t)rel[kk];
                        if constexpr (PACKED) { if (k < 4) rraw0 |= rv << (8 * k); else rraw1 |= rv << (8 * (k - 4)); }
                        else r[k] = (int32_t)rv;
                    }
                }
                const int32_t s = a.read_start[i];
                const uint32_t mq = a.read_mapq[i];
                const bool owned = act && s >= P0 && s < P1;
                const bool lp_ok = lp_possible && owned && mq >= a.lpmd_min_qual && n > 1;
                const bool pdr_ok = act && a.want_pdr && n >= a.min_cpgs && mq >= a.pdr_min_qual;
                const uint32_t sm1 = (uint32_t)(s - 1);
                // slot liveness, span check, concordance state (pdr.rs:37-45 via readutil.rs:226-251): the tile kernel's table form
                const uint32_t nrow = min(n, 8u);
                const uint4 ma = reinterpret_cast<const uint4 *>(&tabs.mtab[nrow][0])[0], mb = reinterpret_cast<const uint4 *>(&tabs.mtab[nrow][0])[1];
                const uint32_t mk[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
                uint32_t acc = 0, xmax = act ? (v[0] & 0x7fffffffu) - sm1 : 0u;
#pragma unroll
                for (int k = 1; k < PW_NB; ++k) {
                    xmax = max(xmax, __builtin_amdgcn_bitop3_b32(v[k] - sm1, mk[k], 0x7fffffffu, 0x80));   // a & b & c
                    v[k] = __builtin_amdgcn_bitop3_b32(v[k], v[0], mk[k], 0xe4);                             // live ? own word : the first call's
                    acc |= v[k] ^ v[0];
                }
                uint32_t bad_it = (xmax > (uint32_t)a.max_span) ? 1u : 0u;
                uint32_t disc = acc >> 31;
                const bool any_long = __any(n > (uint32_t)PW_NB);
                if (any_long && n > (uint32_t)PW_NB) {
                    const uint32_t first = v[0] >> 31;
                    for (uint32_t k = PW_NB; k < n; ++k) {
                        const uint32_t x = a.cpg_pos[o0 + k];
                        disc |= (x >> 31) ^ first;
                        bad_it |= ((x & 0x7fffffffu) - sm1 > (uint32_t)a.max_span) ? 1u : 0u;
                    }
                }
                bad |= act ? bad_it : 0u;
                // windowed pair counts (readutil.rs:166-224): pairs (j < k) with min <= rel_k - rel_j <= max, diagonal by diagonal
                if (__any(lp_ok)) {
                    const uint32_t n_lp = lp_ok ? min(n, (uint32_t)PW_NB) : 0u;
                    if constexpr (PACKED) {
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
                            const uint4 da = reinterpret_cast<const uint4 *>(&tabs.dtab[n_lp][0])[0], db = reinterpret_cast<const uint4 *>(&tabs.dtab[n_lp][0])[1];
                            Q[0] += da.x; Q[1] += da.y; Q[2] += da.z; Q[3] += da.w; O[0] += db.x; O[1] += db.y; O[2] += db.z; O[3] += db.w;
                        }
                        const uint32_t KA = (0x8000u - (uint32_t)mind) * 0x10001u, KB = (0x8000u + (uint32_t)maxd) * 0x10001u;
                        uint32_t accIN = 0, accDD = 0;
#pragma unroll
                        for (int g = 1; g < 8; ++g) {
                            uint32_t orB = 0;
#pragma unroll
                            for (int m = 0; m < 4; ++m) {
                                const int li = (g & 1) ? (g - 1) / 2 + m : g / 2 + m;      // index of the later operand in O (g odd) / Q (g even)
                                if (li > 3) break;
                                const uint32_t later = (g & 1) ? O[li] : Q[li], sl = (g & 1) ? SO[li] : SQ[li];
                                const uint32_t D = later - Q[m];
                                const uint32_t Bw = KB - D;
                                const uint32_t IN = __builtin_amdgcn_bitop3_b32(D + KA, Bw, 0x80008000u, 0x80);   // min <= distance <= max (readutil.rs:184, 196)
                                const uint32_t DD = IN & (sl ^ SQ[m]);
                                accIN += __builtin_popcount(IN);
                                accDD += __builtin_popcount(DD);
                                orB |= Bw;
                            }
                            if (!__any((orB & 0x80008000u) != 0u)) break;      // no lane has a pair within max_distance on this diagonal
                        }
                        a_c += accIN - accDD;
                        a_d += accDD;
                    } else {
#pragma unroll
                        for (int k = 0; k < PW_NB; ++k) r[k] = ((uint32_t)k < n_lp) ? r[k] : (int32_t)((k + 1) << 24);
                        const uint32_t span_ok = (uint32_t)(maxd - a.min_dist);
                        uint32_t lp_n = 0, lp_dd = 0;
#pragma unroll
                        for (int g = 1; g < PW_NB; ++g) {
                            int32_t dmin = 0x7fffffff;
#pragma unroll
                            for (int k = g; k < PW_NB; ++k) {
                                const int32_t dist = r[k] - r[k - g];
                                dmin = min(dmin, dist);
                                const bool in = (uint32_t)(dist - a.min_dist) <= span_ok;      // min <= dist <= max (min <= max)
                                lp_n += in ? 1u : 0u;
                                lp_dd += (in ? (v[k] ^ v[k - g]) : 0u) >> 31;
                            }
                            if (!__any(dmin <= maxd)) break;
                        }
                        a_c += lp_n - lp_dd;
                        a_d += lp_dd;
                    }
                    // a read with more than 8 calls: the pairs whose LATER call is the 9th or beyond, from memory (divergent, rare)
                    if (any_long && lp_ok && n > (uint32_t)PW_NB) {
                        for (uint32_t k = PW_NB; k < n; ++k) {
                            const int32_t rk = (int32_t)rel[o0 + k];
                            const uint32_t mkk = a.cpg_pos[o0 + k] >> 31;
                            for (uint32_t jj = k; jj-- > 0;) {
                                const int32_t dist = rk - (int32_t)rel[o0 + jj];
                                if (dist > a.max_dist) break;          // readutil.rs:184 (anchors evicted)
                                if (dist < a.min_dist) continue;       // readutil.rs:196
                                if ((a.cpg_pos[o0 + jj] >> 31) == mkk) a_c += 1; else a_d += 1;
                            }
                        }
                    }
                }
                // PDR (pdr.rs:180-191): +1 coverage, +1 discordant for a discordant read, at each of the read's calls the stretch holds
                if (__any(pdr_ok && !bad_it)) {
                    auto insert = [&](const uint32_t word) {
                        const uint32_t p = word & 0x7fffffffu, d = p - (uint32_t)P0;
                        if (d >= Wp) return;
                        // CpG sites lie at least two positions apart: (d >> 1) spreads a dense stretch over consecutive slots
                        uint32_t h = (d >> 1) & (PW_S - 1), probes = 0;
                        while (probes++ < (uint32_t)PW_S) {
                            const uint32_t cur = atomicCAS(&tkey[h], PW_EMPTY, p);
                            if (cur == PW_EMPTY || cur == p) { atomicAdd(&tcov[h], 1u); if (disc) atomicAdd(&tdisc[h], 1u); return; }
                            h = (h + 1) & (PW_S - 1);
                        }
                        s_over = 1u;
                    };
                    const bool go = pdr_ok && !bad_it;
#pragma unroll
                    for (int k = 0; k < PW_NB; ++k) {
                        if (!__any(go && (uint32_t)k < n)) break;            // wave-uniform
                        if (go && (uint32_t)k < n) insert(v[k]);
                    }
                    if (any_long && go && n > (uint32_t)PW_NB)
                        for (uint32_t k = PW_NB; k < n; ++k) insert(a.cpg_pos[o0 + k]);
                }
                // ME / PM from the same calls: the live slots of v[] are the read's own words (dead slots were overwritten above)
                const bool q_ok = q_on && act && n >= 4 && mq >= q.min_qual;
                if (__any(q_ok)) {
#pragma unroll
                    for (int k = 3; k < PW_NB; ++k) {
                        if (!__any(q_ok && (uint32_t)k < n)) break;        // wave-uniform
                        if (q_ok && (uint32_t)k < n) window(v[k - 3], v[k - 2], v[k - 1], v[k]);
                    }
                    if (any_long && q_ok && n > (uint32_t)PW_NB) {
                        uint32_t x = v[PW_NB - 3], y = v[PW_NB - 2], z = v[PW_NB - 1];
                        for (uint32_t k = PW_NB; k < n; ++k) {
                            const uint32_t w = a.cpg_pos[o0 + k];
                            window(x, y, z, w);
                            x = y; y = z; z = w;
                        }
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t over = s_over;
        __syncthreads();                                    // (s_over is cleared at the top of the next trip; the queue is done with)
        q_on = false;                                       // the whole tile's quartets are in the table (the first stretch is the tile)
        if (over && sub_shift > 8) { --sub_shift; continue; }      // more distinct sites than slots: the same stretch again in halves
        if (over) bad |= 2u;                                // cannot happen: 256 positions, 1024 slots
        lp_c += a_c; lp_d += a_d; n_read += a_r; n_valid += a_v;
        // rows: slots with coverage >= min_depth, sorted by position.  Bucket sort on the position (256 buckets per stretch): every
        // thread holds its slots in registers, so the table is rebuilt in place in bucket order; a key's final rank = start of its
        // bucket + the keys of that bucket below it (a few).
        constexpr int PER = PW_S / PW_B;
        uint32_t kk[PER], kc[PER], kd[PER], pib[PER];
        const int bshift = sub_shift - 8;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            kk[k] = tkey[tid * PER + k]; kc[k] = tcov[tid * PER + k]; kd[k] = tdisc[tid * PER + k];
            pib[k] = 0;
            if (kk[k] != PW_EMPTY && kc[k] < a.min_cov) kk[k] = PW_EMPTY;
            if (kk[k] != PW_EMPTY) pib[k] = atomicAdd(&bcnt[(kk[k] - (uint32_t)P0) >> bshift], 1u);
        }
        __syncthreads();                                    // every slot is in registers now: the table can be overwritten
        const uint32_t m_b = bcnt[tid];
        const uint32_t incl = wave_scan_incl(m_b);
        if (lane == 63) ws[wave + 1] = incl;
        __syncthreads();
        if (tid == 0) { ws[0] = 0; for (int w = 1; w <= PW_B / 64; ++w) ws[w] += ws[w - 1]; }
        __syncthreads();
        const uint32_t n_rows = ws[PW_B / 64];
        bbase[tid] = ws[wave] + incl - m_b;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (kk[k] != PW_EMPTY) {
                const uint32_t dst = bbase[(kk[k] - (uint32_t)P0) >> bshift] + pib[k];
                tkey[dst] = kk[k]; tcov[dst] = kc[k]; tdisc[dst] = kd[k];
            }
        __syncthreads();
        for (uint32_t j = tid; j < n_rows; j += PW_B) {
            const uint32_t key = tkey[j];
            const uint32_t bk = (key - (uint32_t)P0) >> bshift, b0 = bbase[bk], b1 = b0 + bcnt[bk];
            uint32_t rnk = b0;
            for (uint32_t i = b0; i < b1; ++i) rnk += tkey[i] < key ? 1u : 0u;
            SiteRec rr;
            rr.pos = (int32_t)key; rr.n_disc = tdisc[j]; rr.n_conc = tcov[j] - rr.n_disc; rr.pad = 0;
            out[rows_out + rnk] = rr;
        }
        rows_out += n_rows;
        P0l = P1;
        __syncthreads();                                    // the table is cleared by the next trip
    }
    // ---- quartet rows (k_quartet_tile's row phase): sorted by (p1, d2, d3, d4) through a bucket sort on p1, 256 buckets of the slice
    {
        constexpr int QPER = FQ_S / PW_B, QBSHIFT = SHIFT - 8;
        bcnt[tid] = 0u;
        __syncthreads();
        const bool heavy = s_qheavy != 0u;                  // block-uniform
        unsigned long long kq[QPER];
        uint32_t qib[QPER];
#pragma unroll
        for (int k = 0; k < QPER; ++k) {
            kq[k] = heavy ? QKEY_EMPTY : qkeys[tid * QPER + k];
            qib[k] = 0;
            if (kq[k] != QKEY_EMPTY) qib[k] = atomicAdd(&bcnt[((uint32_t)(kq[k] >> 33) - (uint32_t)T0) >> QBSHIFT], 1u);
        }
        __syncthreads();
        const uint32_t m_b = bcnt[tid];
        const uint32_t incl = wave_scan_incl(m_b);
        if (lane == 63) ws[wave + 1] = incl;
        __syncthreads();
        if (tid == 0) {
            ws[0] = 0;
            for (int w = 1; w <= PW_B / 64; ++w) ws[w] += ws[w - 1];
            const uint32_t n_all = ws[PW_B / 64];
            unsigned long long r0 = 0ull;
            if (heavy) atomicAdd(q.qs + 5, 1ull);
            else if (n_all) {
                r0 = atomicAdd(q.qs + 1, (unsigned long long)n_all);
                if (r0 + n_all > q.row_cap) atomicAdd(q.qs + 6, 1ull);      // (cannot happen: the host sizes for every call of the batch)
            }
            q.tile_flag[t] = heavy ? 1u : 0u; q.tile_rows[t] = heavy ? 0u : n_all; q.tile_row0[t] = r0;
            s_qrow0 = r0;
        }
        __syncthreads();
        const uint32_t nq = ws[PW_B / 64];
        if (!heavy && nq && s_qrow0 + nq <= q.row_cap) {     // block-uniform
            bbase[tid] = ws[wave] + incl - m_b;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < QPER; ++k) {
                if (kq[k] == QKEY_EMPTY) continue;
                const uint32_t dst = bbase[((uint32_t)(kq[k] >> 33) - (uint32_t)T0) >> QBSHIFT] + qib[k];
                qkeys[dst] = kq[k];
                sslot[dst] = (uint16_t)(tid * QPER + k);
            }
            __syncthreads();
            for (uint32_t j = tid; j < nq; j += PW_B) {
                const unsigned long long key = qkeys[j];
                const uint32_t bk = ((uint32_t)(key >> 33) - (uint32_t)T0) >> QBSHIFT, b0 = bbase[bk], b1 = b0 + bcnt[bk];
                uint32_t r = b0;
                for (uint32_t i = b0; i < b1; ++i) r += qkeys[i] < key ? 1u : 0u;
                const uint32_t h = sslot[j];
                const unsigned long long o = s_qrow0 + r;
                const int32_t p1 = (int32_t)(key >> 33);
                const int32_t p2 = p1 + (int32_t)((key >> 22) & 2047u), p3 = p2 + (int32_t)((key >> 11) & 2047u),
                              p4 = p3 + (int32_t)(key & 2047u);
                reinterpret_cast<int4 *>(q.out_pos)[o] = make_int4(p1, p2, p3, p4);
                uint32_t c[16];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    const uint32_t v = qbins[h * 8 + w];
                    c[2 * w] = v & 0xffffu; c[2 * w + 1] = v >> 16;
                }
#pragma unroll
                for (int qq = 0; qq < 4; ++qq)
                    reinterpret_cast<uint4 *>(q.out_cnt + o * 16)[qq] = make_uint4(c[4 * qq], c[4 * qq + 1], c[4 * qq + 2], c[4 * qq + 3]);
                float me, pm;
                uint32_t total;
                quartet_values(c, me, pm, total);
                q.out_me[o] = me; q.out_pm[o] = pm; q.out_depth[o] = total;
            }
        }
        __syncthreads();
    }
    if (bad & 1u) atomicOr(const_cast<uint32_t *>(&a.st->err), (uint32_t)ERRB_SPAN);
    if (bad & 2u) atomicOr(const_cast<uint32_t *>(&a.st->err), (uint32_t)ERRB_CAPACITY);
    // LPMD partials: wave sums -> LDS -> one atomic per counter into the tile's bucket
    if (a.want_lpmd) {
        const uint32_t r0 = wave_sum(lp_c), r1 = wave_sum(lp_d), r2 = wave_sum(n_read), r3 = wave_sum(n_valid);
        if (lane == 0) { red[0][wave] = r0; red[1][wave] = r1; red[2][wave] = r2; red[3][wave] = r3; }
        __syncthreads();
        if (tid < 4) {
            uint32_t sum = 0;
            for (int w = 0; w < PW_B / 64; ++w) sum += red[tid][w];
            if (sum) atomicAdd(a.bucket + a.nbk + (size_t)(t >> TILE_BUCKET_SHIFT) * 4 + tid, (unsigned long long)sum);
        }
    }
    if (tid == 0) {
        a.tile_cnt[t] = rows_out;
        if (rows_out) atomicAdd(a.bucket + (t >> TILE_BUCKET_SHIFT), (unsigned long long)rows_out);
    }
}


void launch_tile_fused(const TileArgs &a, const FusedQuartet &q, uint32_t ntiles, int shift, bool rel8, hipStream_t s) {
    const uint32_t grid = ((ntiles + 7) / 8) * 8;   // whole rows of 8 XCDs (remap in the kernel)
    if (shift == 14) {
        if (rel8) hipLaunchKernelGGL((k_multi_tile<14, uint8_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
        else hipLaunchKernelGGL((k_multi_tile<14, uint16_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
    } else if (shift == 16) {
        if (rel8) hipLaunchKernelGGL((k_multi_tile<16, uint8_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
        else hipLaunchKernelGGL((k_multi_tile<16, uint16_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
    } else {
        if (rel8) hipLaunchKernelGGL((k_multi_tile<15, uint8_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
        else hipLaunchKernelGGL((k_multi_tile<15, uint16_t>), dim3(grid), dim3(PW_B), 0, s, a, q, ntiles);
    }
}

// the quartet state words at the start of a fused batch: rows so far, no tile handed back, nothing beyond the output
__global__ void k_fq_begin(unsigned long long *qs, unsigned long long rows_before) { qs[1] = rows_before; qs[5] = 0; qs[6] = 0; }

// PDR and / or LPMD plus ME / PM of one (prepared) batch through the fused pass where launch_pdr_lpmd takes its wide form (or
// everywhere: force).  *fused: the pass ran (else the quartet side went through mth_quartet_accumulate as in the split form).
static int fused_batch(mth_ctx *ctx, const mth_batch_t &pb, const mth_multi_params_t &mp, bool force, bool *fused) {
    *fused = false;
    MTH_ENTER(ctx);                                         // queued ME / PM batches settled: ctx->q_rows is exact
    hipStream_t s = ctx->stream;
    if (!ctx->q_state.p) {
        MTH_HIP(ctx, ctx->q_state.reserve(8 * sizeof(unsigned long long), s));
        MTH_HIP(ctx, hipMemsetAsync(ctx->q_state.p, 0, 8 * sizeof(unsigned long long), s));
    }
    unsigned long long *qs = ctx->q_state.as<unsigned long long>();
    const uint64_t rows_before = ctx->q_rows;
    const uint64_t tiles_before = ctx->q_meta.empty() ? 0 : ctx->q_meta.back().tile_end;
    const int64_t region_len = (int64_t)pb.region_end - pb.region_beg;
    // a wide-form tile is at least 8192 positions (half a 16384-bp slice); at most one quartet row per CpG call of the batch
    const uint32_t max_tiles = (uint32_t)std::max<int64_t>(region_len, 0) / 8192u + 2u;
    const uint64_t cap = rows_before + pb.n_cpgs + 1024;
    if (cap > ctx->q_cap) {
        MTH_HIP(ctx, ctx->q_pos.reserve(cap * 16, s, true, rows_before * 16));
        MTH_HIP(ctx, ctx->q_cnt.reserve(cap * 64, s, true, rows_before * 64));
        MTH_HIP(ctx, ctx->q_me.reserve(cap * 4, s, true, rows_before * 4));
        MTH_HIP(ctx, ctx->q_pm.reserve(cap * 4, s, true, rows_before * 4));
        MTH_HIP(ctx, ctx->q_depth.reserve(cap * 4, s, true, rows_before * 4));
        ctx->q_cap = cap;
    }
    MTH_HIP(ctx, ctx->q_tflag.reserve((size_t)max_tiles * 4, s));
    MTH_HIP(ctx, ctx->q_tile_row0.reserve((tiles_before + max_tiles) * 8, s, true, tiles_before * 8));
    MTH_HIP(ctx, ctx->q_tile_rows.reserve((tiles_before + max_tiles) * 4, s, true, tiles_before * 4));
    hipLaunchKernelGGL(k_fq_begin, dim3(1), dim3(1), 0, s, qs, (unsigned long long)rows_before);
    MTH_HIP(ctx, hipGetLastError());
    FusedQuartet fq;
    fq.force = force ? 1 : 0;
    fq.force_heavy = getenv("MTH_MULTI_FORCE_HANDBACK") ? 1 : 0;       // tests: every tile handed back
    fq.min_qual = mp.quartet.min_qual;
    fq.qs = qs; fq.row_cap = ctx->q_cap; fq.max_tiles = max_tiles;
    fq.tile_flag = ctx->q_tflag.as<uint32_t>();
    fq.tile_row0 = ctx->q_tile_row0.as<unsigned long long>() + tiles_before;
    fq.tile_rows = ctx->q_tile_rows.as<uint32_t>() + tiles_before;
    fq.out_pos = ctx->q_pos.as<int32_t>(); fq.out_cnt = ctx->q_cnt.as<uint32_t>(); fq.out_me = ctx->q_me.as<float>();
    fq.out_pm = ctx->q_pm.as<float>(); fq.out_depth = ctx->q_depth.as<uint32_t>();
    fq.taken = false; fq.ntiles = 0;
    mth_pdr_lpmd_params_t p = mp.pdr_lpmd;
    p.want_pdr = (mp.want & MTH_MULTI_PDR) ? 1 : 0;
    p.want_lpmd = (mp.want & MTH_MULTI_LPMD) ? 1 : 0;
    ctx->fuse_q = &fq;
    int rc = mth_pdr_lpmd_accumulate(ctx, &pb, &p);
    ctx->fuse_q = nullptr;
    if (rc) return rc;
    if (!fq.taken) return mth_quartet_accumulate(ctx, &pb, &mp.quartet);     // (the dense form ran, or a PDR-only exact pass)
    *fused = true;
    unsigned long long *st = ctx->h_words;
    MTH_HIP(ctx, hipMemcpyAsync(st, qs, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    ctx->multi_stats[2] += fq.ntiles;
    if (st[5] || st[6]) {
        // hand back: the batch's ME / PM side again through the single entry point (its rows restart at rows_before; no meta was kept)
        ctx->multi_stats[3] += st[6] ? fq.ntiles : st[5];
        return mth_quartet_accumulate(ctx, &pb, &mp.quartet);
    }
    const uint64_t total = st[1];
    ctx->q_meta.push_back(mth_ctx::TileBatch{pb.tid, total - rows_before, total, tiles_before + fq.ntiles});
    ctx->q_rows = total;
    ctx->q_epoch += 1;
    if (pb.n_cpgs) { ctx->q_rows_per_cpg = std::max(ctx->q_rows_per_cpg * 0.5, (double)(total - rows_before) / (double)pb.n_cpgs); ctx->q_learned = true; }
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_multi_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_multi_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    const uint32_t all = MTH_MULTI_PDR | MTH_MULTI_LPMD | MTH_MULTI_QUARTET | MTH_MULTI_MHL | MTH_MULTI_FDRP | MTH_MULTI_PAIRS;
    const uint32_t want = params->want;
    if (want == 0 || (want & ~all)) return fail(ctx, MTH_ERR_INVALID, "mth_multi_params_t.want: no measure, or an unknown bit");
    if (params->form != MTH_MULTI_AUTO && params->form != MTH_MULTI_FUSED && params->form != MTH_MULTI_SPLIT)
        return fail(ctx, MTH_ERR_INVALID, "mth_multi_params_t.form");
    mth_batch_t pb = *batch;
    const bool own = batch->mem != MTH_MEM_PREPARED;
    if (own) {
        const int rc = mth_batch_prepare(ctx, batch, &pb);
        if (rc) return rc;
    }
    int rc = MTH_OK;
    bool fused = false;
    // the fused pass needs both of its consumers: PDR and / or LPMD, and ME / PM
    if (params->form != MTH_MULTI_SPLIT && (want & MTH_MULTI_QUARTET) && (want & (MTH_MULTI_PDR | MTH_MULTI_LPMD))) {
        rc = fused_batch(ctx, pb, *params, params->form == MTH_MULTI_FUSED, &fused);
    } else {
        if (want & (MTH_MULTI_PDR | MTH_MULTI_LPMD)) {
            mth_pdr_lpmd_params_t p = params->pdr_lpmd;
            p.want_pdr = (want & MTH_MULTI_PDR) ? 1 : 0;
            p.want_lpmd = (want & MTH_MULTI_LPMD) ? 1 : 0;
            rc = mth_pdr_lpmd_accumulate(ctx, &pb, &p);
        }
        if (!rc && (want & MTH_MULTI_QUARTET)) rc = mth_quartet_accumulate(ctx, &pb, &params->quartet);
    }
    if (!rc && (want & MTH_MULTI_MHL)) rc = mth_mhl_accumulate(ctx, &pb, &params->mhl);
    if (!rc && (want & MTH_MULTI_FDRP)) rc = mth_fdrp_accumulate(ctx, &pb, &params->fdrp);
    if (!rc && (want & MTH_MULTI_PAIRS)) rc = mth_lpmd_pairs_accumulate(ctx, &pb, &params->pairs);
    // synchronous per batch: queued ME / PM and pairs batches are settled and the batch's data errors reported here, so that the
    // prepared batch can go (its index and, for a host batch, its device copies) and the caller may reuse its arrays
    if (!rc) rc = mth_ctx_sync(ctx);
    if (own) {
        const int rr = mth_batch_release(ctx, &pb);
        if (!rc) rc = rr;
    }
    if (!rc) ctx->multi_stats[fused ? 0 : 1] += 1;
    return rc;
}

int mth_multi_stats(mth_ctx_t *ctx, uint64_t out[4]) {
    if (!ctx || !out) return MTH_ERR_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = ctx->multi_stats[k];
    return MTH_OK;
}

}  // extern "C"
