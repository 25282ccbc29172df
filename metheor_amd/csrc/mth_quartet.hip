// mth_quartet.hip -- ME / PM: per-quartet 16-bin epiallele histograms on gfx950.
//
// Reference: readutil.rs:97-132 (get_cpg_quartets_and_patterns: every window of 4 consecutive CpGs of
// a read, pattern = 8*m0 + 4*m1 + 2*m2 + m3), me.rs:90-132 / pm.rs:85-128 (global
// HashMap<Quartet,[u32;16]> over reads with mapq >= min_qual, never flushed), me.rs:42-55
// (me = -0.25 * sum_{c>0} p*log2(p)), pm.rs:42-51 (pm = 1 - sum p*p), p = c as f32 / total as f32,
// bins visited 0..15 in order; min_depth is applied when rows are written (me.rs:82).
//
// Device design.  A quartet is owned by the position of its first CpG, so -- as for the per-site counters of PDR -- the
// tile (8192 / 16384 / 32768 bp, by the batch's call density) that contains p1 sees ALL updates of its quartets: k_quartet_tile keeps a 512-slot hash table in LDS
// (64-bit key, sixteen 16-bit bins packed in 8 words), fed by the tile's candidate reads (linear read index), and emits
// its rows straight from LDS (one global atomic per tile to claim the output range).  The first version sent every
// update to a global table: 6 M CAS + 6 M adds through L2 per 10 M reads were what it spent its time on.  Tiles that do
// not fit (> 65535 candidate reads: 16-bit bins; more distinct quartets than the table holds) are flagged and take
// that global path, restricted to their quartets: a global open-addressing table (64-bit key CAS, then one L2 atomic add on the
// bin) sized from an exact counting pre-pass.  Key = p1 (31 bits) | three position deltas (11 bits
// each): consecutive CpGs of one read further than 2047 bp apart are refused (MTH_ERR_CAPACITY).
// A quartet is owned by the batch whose region contains p1 (same rule as sites), so region / contig
// sharding needs no exchange.  Each tile sorts its rows in LDS and the fetch walks the tiles in order, so rows come out
// sorted by (tid, p1..p4); rows of tiles that took the global path follow in table order (the reference's order is
// HashMap-random, compare as sets).
#include <algorithm>
#include <cmath>

#include "mth_ctx.h"
#include "mth_scan.h"
#include "mth_tile_dev.h"
#include "mth_quartet_dev.h"

namespace mth {

// tile kernel: reference positions per tile, LDS table slots, threads.  Measured on S-chr19-10M (profiles/r01_quartet_tile.md):
// wider tiles re-read fewer halo reads and clear LDS less often, a smaller table lets more tiles share a CU (25 KB each).
constexpr int QT_NC = 8;   // calls of a read held in registers
constexpr int QT_QCAP = 2048;   // candidate reads per fill of the contributor queue
constexpr int QT_OCC = 6;  // waves per SIMD (LDS: 23 KiB per workgroup = 6 per CU)
constexpr int QT_B = 256, QT_U = 2, QT_CHUNK = 512, QT_GRID = 8192;   // (the tile width is a template parameter: 8192 / 16384 / 32768, chosen per batch)

__device__ __forceinline__ unsigned long long qhash(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

// global path: upper bound of the number of (read, window) updates: sum over passing reads of max(0, n - 3)
__global__ __launch_bounds__(256) void k_quartet_bound(const uint32_t *__restrict__ cpg_off,
                                                       const uint8_t *__restrict__ mapq, uint32_t n_reads,
                                                       uint8_t min_qual, unsigned long long *__restrict__ out) {
    unsigned long long acc = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_reads; i += gridDim.x * 256) {
        const uint32_t n = cpg_off[i + 1] - cpg_off[i];
        if (n >= 4 && mapq[i] >= min_qual) acc += n - 3;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ unsigned long long ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, ws[0] + ws[1] + ws[2] + ws[3]);
}

constexpr uint32_t QPROBE_MAX = 1024;
__global__ __launch_bounds__(256) void k_quartet_insert(const uint32_t *__restrict__ cpg_off,
                                                        const uint32_t *__restrict__ cpg_pos,
                                                        const uint8_t *__restrict__ mapq, uint32_t n_reads,
                                                        uint8_t min_qual, int32_t region_beg, int32_t region_end,
                                                        unsigned long long *__restrict__ keys,
                                                        uint32_t *__restrict__ hist, unsigned long long mask,
                                                        unsigned long long *__restrict__ overflow, DevState *__restrict__ st,
                                                        const uint32_t *__restrict__ tile_flag /* nullptr: every quartet */,
                                                        int tile_shift /* log2 of the tile width the flags were made with */,
                                                        uint4 *__restrict__ wide_pos, uint32_t *__restrict__ wide_pat,
                                                        unsigned long long wide_cap, unsigned long long *__restrict__ wide_n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_reads) return;
    const uint32_t o0 = cpg_off[i], o1 = cpg_off[i + 1];
    if (o1 - o0 < 4 || mapq[i] < min_qual) return;          // readutil.rs:101, me.rs:115
    uint32_t a = cpg_pos[o0], b = cpg_pos[o0 + 1], c = cpg_pos[o0 + 2];
    for (uint32_t k = o0 + 3; k < o1; ++k) {                // readutil.rs:105-129
        const uint32_t d = cpg_pos[k];
        const int32_t p1 = (int32_t)(a & 0x7fffffffu);
        if (p1 >= region_beg && p1 < region_end && (!tile_flag || tile_flag[(uint32_t)(p1 - region_beg) >> tile_shift])) {
            const uint32_t d2 = (b & 0x7fffffffu) - (a & 0x7fffffffu), d3 = (c & 0x7fffffffu) - (b & 0x7fffffffu),
                           d4 = (d & 0x7fffffffu) - (c & 0x7fffffffu);
            const unsigned long long key = ((unsigned long long)(uint32_t)p1 << 33) | ((unsigned long long)d2 << 22) |
                                           ((unsigned long long)d3 << 11) | (unsigned long long)d4;
            const uint32_t pat = ((a >> 31) << 3) | ((b >> 31) << 2) | ((c >> 31) << 1) | (d >> 31);
            if (d2 - 1u >= 0x7fffffffu || d3 - 1u >= 0x7fffffffu || d4 - 1u >= 0x7fffffffu) {
                atomicOr(&st->err, (uint32_t)ERRB_SPAN);                 // calls of a read not in ascending position order
            } else if (d2 >= 2048u || d3 >= 2048u || d4 >= 2048u || key == QKEY_EMPTY) {
                // CpGs of the window >= 2048 bp apart do not fit the packed key: the instance goes to the wide list
                // (aggregated by k_quartet_wide_insert under a 128-bit key); counted even when the list is full (the host redoes)
                const unsigned long long w = atomicAdd(wide_n, 1ull);
                if (w < wide_cap) {
                    wide_pos[w] = make_uint4((uint32_t)p1, b & 0x7fffffffu, c & 0x7fffffffu, d & 0x7fffffffu);
                    wide_pat[w] = pat;
                }
            } else {
                unsigned long long h = qhash(key) & mask;
                // The table is sized for the DISTINCT quartets one expects (half the instances), not for the instances:
                // a bounded probe, and a flag that makes the host redo the pass with a larger table, keep that safe.
                uint32_t probes = 0;
                bool placed = false;
                while (probes++ < QPROBE_MAX) {
                    const unsigned long long cur = atomicCAS(&keys[h], QKEY_EMPTY, key);
                    if (cur == QKEY_EMPTY || cur == key) { placed = true; break; }
                    h = (h + 1) & mask;
                }
                if (placed) atomicAdd(&hist[h * 16 + pat], 1u);         // me.rs:121-125
                else *overflow = 1ull;
            }
        }
        a = b; b = c; c = d;
    }
}

// Wide quartets (some pair of consecutive CpGs >= 2048 bp apart: reference skips, deletions, long reads) under a 128-bit
// key: k0 = p1 << 32 | p2 claims the slot with a CAS, k1 = p3 << 32 | p4 is published right after by the claimer.  A lane that
// finds its k0 in a slot waits for the slot's k1 to appear and compares; the claimer's store comes before every wait in
// program order (same iteration, straight-line), so lanes of one wave cannot wait on each other's unpublished slot.
__global__ __launch_bounds__(256) void k_quartet_wide_insert(const uint4 *__restrict__ wide_pos, const uint32_t *__restrict__ wide_pat,
                                                             unsigned long long n, unsigned long long *__restrict__ k0,
                                                             unsigned long long *__restrict__ k1, uint32_t *__restrict__ hist,
                                                             unsigned long long mask, unsigned long long *__restrict__ overflow) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 p = wide_pos[i];
    const unsigned long long key0 = ((unsigned long long)p.x << 32) | p.y, key1 = ((unsigned long long)p.z << 32) | p.w;
    unsigned long long h = qhash(key0 ^ qhash(key1)) & mask;
    for (uint32_t probes = 0; probes < QPROBE_MAX; ++probes) {
        const unsigned long long cur = atomicCAS(&k0[h], QKEY_EMPTY, key0);
        if (cur == QKEY_EMPTY) __hip_atomic_store(&k1[h], key1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == QKEY_EMPTY || cur == key0) {
            unsigned long long v;
            do { v = __hip_atomic_load(&k1[h], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); } while (v == QKEY_EMPTY);
            if (v == key1) { atomicAdd(&hist[h * 16 + wide_pat[i]], 1u); return; }
        }
        h = (h + 1) & mask;
    }
    *overflow = 1ull;
}

// rows per block of 256*8 slots
constexpr int QE_PER = 8;
__global__ __launch_bounds__(256) void k_quartet_blockcount(const unsigned long long *__restrict__ keys,
                                                            unsigned long long n_slots, uint32_t *__restrict__ blk) {
    const unsigned long long s0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * QE_PER;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < QE_PER; ++k) m += (s0 + k < n_slots && keys[s0 + k] != QKEY_EMPTY) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_down(m, o, 64);
    __shared__ uint32_t ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(256) void k_quartet_emit(const unsigned long long *__restrict__ keys,
                                                      const unsigned long long *__restrict__ keys1 /* wide table: p3 << 32 | p4; else nullptr */,
                                                      const uint32_t *__restrict__ hist, unsigned long long n_slots,
                                                      const uint32_t *__restrict__ blk,
                                                      const unsigned long long *__restrict__ q_base,
                                                      int32_t *__restrict__ out_pos, uint32_t *__restrict__ out_cnt,
                                                      float *__restrict__ out_me, float *__restrict__ out_pm,
                                                      uint32_t *__restrict__ out_depth) {
    const unsigned long long s0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * QE_PER;
    uint32_t m = 0;
    unsigned long long kk[QE_PER];
#pragma unroll
    for (int k = 0; k < QE_PER; ++k) {
        kk[k] = s0 + k < n_slots ? keys[s0 + k] : QKEY_EMPTY;
        m += kk[k] != QKEY_EMPTY ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __shared__ uint32_t ws[5];
    if (lane == 63) ws[wave + 1] = incl;
    __syncthreads();
    if (threadIdx.x == 0) { ws[0] = 0; for (int w = 1; w <= 4; ++w) ws[w] += ws[w - 1]; }
    __syncthreads();
    unsigned long long o = *q_base + blk[blockIdx.x] + ws[wave] + incl - m;
#pragma unroll
    for (int k = 0; k < QE_PER; ++k) {
        if (kk[k] == QKEY_EMPTY) continue;
        const unsigned long long key = kk[k];
        int32_t p1, p2, p3, p4;
        if (keys1) {
            const unsigned long long key1 = keys1[s0 + k];
            p1 = (int32_t)(key >> 32); p2 = (int32_t)(uint32_t)key; p3 = (int32_t)(key1 >> 32); p4 = (int32_t)(uint32_t)key1;
        } else {
            p1 = (int32_t)(key >> 33);
            p2 = p1 + (int32_t)((key >> 22) & 2047u); p3 = p2 + (int32_t)((key >> 11) & 2047u); p4 = p3 + (int32_t)(key & 2047u);
        }
        reinterpret_cast<int4 *>(out_pos)[o] = make_int4(p1, p2, p3, p4);
        uint32_t c[16];
        const uint4 *src = reinterpret_cast<const uint4 *>(hist + (s0 + k) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 x = src[q];
            c[4 * q] = x.x; c[4 * q + 1] = x.y; c[4 * q + 2] = x.z; c[4 * q + 3] = x.w;
            reinterpret_cast<uint4 *>(out_cnt + o * 16)[q] = x;
        }
        float me, pm;
        uint32_t total;
        quartet_values(c, me, pm, total);
        out_me[o] = me; out_pm[o] = pm; out_depth[o] = total;
        ++o;
    }
}


// ---- tile kernel ---------------------------------------------------------------------------------------------------
struct QTileArgs {
    const int32_t  *read_start;
    const uint8_t  *read_mapq;
    const uint32_t *cpg_off, *cpg_pos, *idx;
    int32_t region_beg, region_end, idx_base, max_span;
    uint32_t n_reads, ntiles, n_cpgs;
    uint8_t min_qual, force_heavy;            // force_heavy: tests send every tile down the global path
    unsigned long long *row_total;            // rows claimed so far (all batches, gaps included)
    unsigned long long row_cap;               // rows the output holds; a range beyond it is claimed but not written ...
    unsigned long long *unfit;                // ... and reported here (the host redoes the batch with the exact size)
    unsigned long long *n_heavy;              // tiles left to the global path
    uint32_t *tile_flag;                      // per tile of the batch: 1 = left to the global path
    unsigned long long *tile_row0;            // per tile: first row of its range ...
    uint32_t *tile_rows;                      // ... and its length (the fetch walks tiles in order: rows come out sorted)
    int32_t *out_pos; uint32_t *out_cnt; float *out_me, *out_pm; uint32_t *out_depth;
    DevState *st;
};
template <int QT_W>
__global__ __launch_bounds__(QT_B, QT_OCC) void k_quartet_tile(const QTileArgs a) {
    __shared__ unsigned long long keys[QT_S];  // the hash table; later its keys in bucket order
    __shared__ uint32_t bcnt[QT_B];            // bucket sort on p1: keys per bucket
    // the contributor queue of the read phases (16-bit read numbers) shares its LDS with two arrays of the row phase: the first
    // rank of each bucket, and the slot each sorted key came from
    __shared__ uint32_t q_or_sort[QT_QCAP / 2];
    static_assert(QT_QCAP / 2 >= QT_B + QT_S / 2, "bbase and sslot fit under the queue");
    uint16_t *const rq = reinterpret_cast<uint16_t *>(q_or_sort);
    uint32_t *const bbase = q_or_sort;
    uint16_t *const sslot = reinterpret_cast<uint16_t *>(q_or_sort + QT_B);
    __shared__ uint32_t s_qn;
    __shared__ uint32_t bins[QT_S * 8];        // bin 2w in the low half of word w, bin 2w+1 in the high half
    __shared__ uint32_t s_heavy, ws[QT_B / 64 + 1];
    __shared__ unsigned long long s_chunk_pos, s_chunk_end;   // rows claimed from the global counter, handed out tile by tile
    const int tid = threadIdx.x;
    if (tid == 0) { s_chunk_pos = 0; s_chunk_end = 0; }
    // Persistent workgroups: each takes tiles t, t + grid, ... and claims output rows for several tiles at once.  (One claim
    // per tile was the kernel's floor on sparse WGBS: same-address returning atomics serialise at ~12 ns each, and a
    // human genome is 378 k tiles.)  The unused tail of a chunk stays a gap; the fetch walks per-tile ranges.
    for (uint32_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    __syncthreads();                                    // the previous tile's rows have left LDS
    const int32_t T0 = a.region_beg + (int32_t)(t * QT_W);
    const int32_t T1 = (int32_t)min((int64_t)T0 + QT_W, (int64_t)a.region_end);
    // candidate reads: a read with a CpG at p1 >= T0 starts after T0 - max_span and not after T1 - 1
    const uint32_t lo = min(a.idx[((uint32_t)T0 - (uint32_t)a.max_span + 1u - (uint32_t)a.idx_base) >> IDX_QSHIFT], a.n_reads);
    const uint32_t hi = min(a.idx[(((uint32_t)T0 + (uint32_t)QT_W - (uint32_t)a.idx_base) >> IDX_QSHIFT) + 1], a.n_reads);
    if (lo >= hi) {                                             // nothing starts here: no LDS work at all
        if (tid == 0) { a.tile_flag[t] = 0u; a.tile_rows[t] = 0u; a.tile_row0[t] = 0ull; }
        continue;
    }
    for (int i = tid; i < QT_S; i += QT_B) keys[i] = QKEY_EMPTY;
    bcnt[tid] = 0;
    for (int i = tid; i < QT_S * 8; i += QT_B) bins[i] = 0;
    if (tid == 0) { s_heavy = (hi - lo > 65535u || a.force_heavy) ? 1u : 0u; s_qn = 0u; }      // a bin counts at most one update per candidate read
    __syncthreads();
    if (!s_heavy) {
        uint32_t bad = 0;
        // one window of four consecutive calls into the tile's table
        auto window = [&](const uint32_t x, const uint32_t y, const uint32_t z, const uint32_t w) {
            if (quartet_window<QT_S>(x, y, z, w, T0, T1, keys, bins) == QW_HAND_BACK) s_heavy = 1u;
        };
        // Two phases per stretch of QT_QCAP candidate reads.  Phase 1, every candidate (offsets one round ahead, mapq): the reads with
        // >= 4 CpGs that pass mapq (readutil.rs:101, me.rs:115) -- a third of config 2's reads, a twentieth at WGBS density -- are
        // queued.  Phase 2, the queue with every lane live: the read's first QT_NC calls as two 16-byte loads from a per-read base
        // (the PDR tile kernel's form; a wave that holds one of the batch's last reads takes clamped single loads instead), its
        // windows from registers; only a read with more than QT_NC calls goes back to memory, one dependent load per further window.
        // (One phase over all candidates ran the window code with 5-30 % of the lanes live; measured gain of the split: config 2
        // 0.124 -> 0.121 ms, config-3 density 0.160 -> 0.158 -- the tile's fixed chain, not the windows, is what this kernel waits for.)
        for (uint32_t c0 = lo; c0 < hi; c0 += QT_QCAP) {
            const uint32_t c1 = min(c0 + (uint32_t)QT_QCAP, hi);
            if (c0 != lo) {
                __syncthreads();                            // the previous stretch's queue is done with
                if (tid == 0) s_qn = 0u;
                __syncthreads();
            }
            uint32_t o0s[QT_U], o1s[QT_U];
#pragma unroll
            for (int u = 0; u < QT_U; ++u) {
                const uint32_t ii = min(c0 + (uint32_t)u * QT_B + tid, c1 - 1);
                o0s[u] = a.cpg_off[ii]; o1s[u] = a.cpg_off[ii + 1];
            }
            for (uint32_t b0 = c0; b0 < c1; b0 += QT_B * QT_U) {
                uint32_t mq[QT_U], o0n[QT_U], o1n[QT_U];
#pragma unroll
                for (int u = 0; u < QT_U; ++u) {
                    const uint32_t i = b0 + (uint32_t)u * QT_B + tid;
                    mq[u] = a.read_mapq[min(i, c1 - 1)];
                    const uint32_t in = min(i + (uint32_t)QT_U * QT_B, c1 - 1);
                    o0n[u] = a.cpg_off[in]; o1n[u] = a.cpg_off[in + 1];
                }
#pragma unroll
                for (int u = 0; u < QT_U; ++u) {
                    const uint32_t i = b0 + (uint32_t)u * QT_B + tid;
                    const bool contrib = i < c1 && o1s[u] - o0s[u] >= 4 && mq[u] >= a.min_qual;
                    const unsigned long long bal = __ballot(contrib);
                    if (bal) {
                        uint32_t base = 0;
                        if ((tid & 63) == 0) base = atomicAdd(&s_qn, (uint32_t)__builtin_popcountll(bal));
                        base = __builtin_amdgcn_readfirstlane(base);
                        if (contrib) rq[base + (uint32_t)__builtin_popcountll(bal & ((1ull << (tid & 63)) - 1ull))] = (uint16_t)(i - c0);
                    }
                }
#pragma unroll
                for (int u = 0; u < QT_U; ++u) { o0s[u] = o0n[u]; o1s[u] = o1n[u]; }
            }
            __syncthreads();
            const uint32_t qn = s_qn;
            for (uint32_t j0 = 0; j0 < qn; j0 += QT_B) {
                const uint32_t j = j0 + tid;
                const bool act = j < qn;
                const uint32_t i = c0 + (act ? (uint32_t)rq[j] : 0u);
                const uint32_t o0 = a.cpg_off[i], o1 = a.cpg_off[i + 1];
                const uint32_t n_calls = act ? o1 - o0 : 0u;
                uint32_t vv[QT_NC];
                static_assert(QT_NC == 8, "two 16-byte loads per read");
                if (__all(!act || (unsigned long long)o0 + QT_NC <= (unsigned long long)a.n_cpgs)) {
                    if (act) {
                        const u32x4_a4 x = *reinterpret_cast<const u32x4_a4 *>(a.cpg_pos + o0), y = *reinterpret_cast<const u32x4_a4 *>(a.cpg_pos + o0 + 4);
                        vv[0] = x.x; vv[1] = x.y; vv[2] = x.z; vv[3] = x.w; vv[4] = y.x; vv[5] = y.y; vv[6] = y.z; vv[7] = y.w;
                    }
                } else if (act) {
#pragma unroll
                    for (int k = 0; k < QT_NC; ++k) vv[k] = a.cpg_pos[o0 + min((uint32_t)k, n_calls - 1)];
                }
                // candidate ranges rely on every call lying in [start - 1, start - 1 + max_span] (a reverse read's first call
                // may sit one base before its start, readutil.rs:338; rule of the PDR tile kernel).  Unsigned: a call further
                // left is caught too; the windows' deltas are checked to be 1..2047 below, so the calls in between are ordered.
                const uint32_t sm1 = (uint32_t)a.read_start[i] - 1u;
                uint32_t xmax = 0;
#pragma unroll
                for (int k = 0; k < QT_NC; ++k) xmax = max(xmax, (uint32_t)k < n_calls ? (vv[k] & 0x7fffffffu) - sm1 : 0u);
                bad |= (xmax > (uint32_t)a.max_span) ? 1u : 0u;
#pragma unroll
                for (int k = 3; k < QT_NC; ++k) {
                    if (!__any((uint32_t)k < n_calls)) break;               // wave-uniform
                    if ((uint32_t)k < n_calls) window(vv[k - 3], vv[k - 2], vv[k - 1], vv[k]);
                }
                if (__any(n_calls > (uint32_t)QT_NC) && n_calls > (uint32_t)QT_NC) {
                    uint32_t x = vv[QT_NC - 3], y = vv[QT_NC - 2], z = vv[QT_NC - 1];
                    for (uint32_t k = o0 + QT_NC; k < o1; ++k) {
                        const uint32_t w = a.cpg_pos[k];
                        bad |= ((w & 0x7fffffffu) - sm1 > (uint32_t)a.max_span) ? 1u : 0u;
                        window(x, y, z, w);
                        x = y; y = z; z = w;
                    }
                }
            }
        }
        if (bad) atomicOr(&a.st->err, (uint32_t)ERRB_SPAN);
    }
    __syncthreads();
    if (s_heavy) {                                      // block-uniform: the whole tile goes to the global path
        if (tid == 0) { a.tile_flag[t] = 1u; a.tile_rows[t] = 0u; a.tile_row0[t] = 0ull; atomicAdd(a.n_heavy, 1ull); }
        continue;
    }
    // thread 0 hands the tile its rows out of the workgroup's chunk
    auto claim_rows = [&](const uint32_t n_all) {
        a.tile_flag[t] = 0u; a.tile_rows[t] = n_all;
        if (n_all && s_chunk_pos + n_all > s_chunk_end) {       // next chunk (what is left of the old one stays unused)
            // enough for this workgroup's remaining tiles if they are like this one, at most QT_CHUNK rows: the gaps stay
            // small next to the rows (a single-tile workgroup claims exactly its rows)
            const unsigned long long left = (unsigned long long)((a.ntiles - 1u - t) / gridDim.x + 1u);
            const unsigned long long claim = max((unsigned long long)n_all, min((unsigned long long)n_all * left, (unsigned long long)QT_CHUNK));
            s_chunk_pos = atomicAdd(a.row_total, claim);
            s_chunk_end = s_chunk_pos + claim;
            if (s_chunk_end > a.row_cap) atomicAdd(a.unfit, 1ull);
        }
        const unsigned long long row0 = s_chunk_pos;
        s_chunk_pos += n_all;
        a.tile_row0[t] = row0;
        return row0;
    };
    quartet_rows<QT_S, QT_B, __builtin_ctz((unsigned)QT_W) - 8>(keys, bins, bcnt, bbase, sslot, ws, T0, true, claim_rows, a.row_cap, a.out_pos,
                                                                a.out_cnt, a.out_me, a.out_pm, a.out_depth);
    }
}

// ---- what ME / PM brings to the tile-row driver (mth_tile_rows.hip) -----------------------------------------------
// the tile width: quartet_tile_shift of mth_plan.h
static int quartet_tile_shift(const mth_batch_t &d, const TileParams &) { return quartet_tile_shift(batch_shape(d), tile_shift_knob("MTH_QUARTET")); }

static hipError_t quartet_grow_rows(mth_ctx *ctx, uint64_t cap, uint64_t used) {
    hipStream_t s = ctx->stream;
    hipError_t e;
    if ((e = ctx->q_pos.reserve(cap * 16, s, true, used * 16)) != hipSuccess) return e;
    if ((e = ctx->q_cnt.reserve(cap * 64, s, true, used * 64)) != hipSuccess) return e;
    if ((e = ctx->q_me.reserve(cap * 4, s, true, used * 4)) != hipSuccess) return e;
    if ((e = ctx->q_pm.reserve(cap * 4, s, true, used * 4)) != hipSuccess) return e;
    return ctx->q_depth.reserve(cap * 4, s, true, used * 4);
}

static void quartet_launch_tiles(mth_ctx *ctx, const mth_batch_t &d, const TileParams &p, int tile_shift, uint32_t ntiles, int32_t idx_base,
                                 uint64_t tiles_before, uint64_t row_cap) {
    const TileRowTable &t = ctx->quartets;
    hipStream_t s = ctx->stream;
    unsigned long long *qs = t.words();
    QTileArgs a;
    a.read_start = d.read_start; a.read_mapq = d.read_mapq; a.cpg_off = d.cpg_off; a.cpg_pos = d.cpg_pos;
    a.idx = idx_ptr(ctx);
    a.region_beg = d.region_beg; a.region_end = d.region_end; a.idx_base = idx_base; a.max_span = d.max_span;
    a.n_reads = d.n_reads; a.ntiles = ntiles; a.n_cpgs = (uint32_t)d.n_cpgs; a.min_qual = p.quartet.min_qual;
    a.force_heavy = force_global_knob("MTH_QUARTET") ? 1 : 0;
    a.row_total = qs + 1; a.row_cap = row_cap; a.unfit = qs + 6; a.n_heavy = qs + 5;
    a.tile_flag = t.tflag.as<uint32_t>();
    a.tile_row0 = t.tile_row0.as<unsigned long long>() + tiles_before;
    a.tile_rows = t.tile_rows.as<uint32_t>() + tiles_before;
    a.out_pos = ctx->q_pos.as<int32_t>(); a.out_cnt = ctx->q_cnt.as<uint32_t>(); a.out_me = ctx->q_me.as<float>();
    a.out_pm = ctx->q_pm.as<float>(); a.out_depth = ctx->q_depth.as<uint32_t>(); a.st = ctx->d_state;
    LaunchTimer lt(ctx, K_QTILE);
    if (tile_shift == 13) hipLaunchKernelGGL(k_quartet_tile<8192>, dim3(std::min<uint32_t>(ntiles, QT_GRID)), dim3(QT_B), 0, s, a);
    else if (tile_shift == 14) hipLaunchKernelGGL(k_quartet_tile<16384>, dim3(std::min<uint32_t>(ntiles, QT_GRID)), dim3(QT_B), 0, s, a);
    else if (tile_shift == 15) hipLaunchKernelGGL(k_quartet_tile<32768>, dim3(std::min<uint32_t>(ntiles, QT_GRID)), dim3(QT_B), 0, s, a);
    else hipLaunchKernelGGL(k_quartet_tile<65536>, dim3(std::min<uint32_t>(ntiles, QT_GRID)), dim3(QT_B), 0, s, a);
}

// The tiles the LDS table could not hold: the global table, for their quartets only.  Its size: `bound` counts
// quartet INSTANCES of the whole batch; bound / 2 slots to start with, redone 4x larger if an insert ran out of
// probes -- at 2 x bound slots that cannot happen.
static int quartet_global_path(mth_ctx *ctx, const mth_batch_t &d, const TileParams &p, int tile_shift, uint64_t &total) {
    TileRowTable &t = ctx->quartets;
    const mth_quartet_params_t *params = &p.quartet;
    hipStream_t s = ctx->stream;
    unsigned long long *qs = t.words();
    MTH_HIP(ctx, hipMemsetAsync(qs, 0, sizeof(unsigned long long), s));
    {
        LaunchTimer lt(ctx, K_QBOUND);
        hipLaunchKernelGGL(k_quartet_bound, dim3(1024), dim3(256), 0, s, d.cpg_off, d.read_mapq, d.n_reads,
                           params->min_qual, qs);
    }
    unsigned long long bound = 0;
    MTH_HIP(ctx, hipMemcpyAsync(&bound, qs, sizeof bound, hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    unsigned long long n_slots = 1024;
    while (n_slots < bound / 2) n_slots <<= 1;
    unsigned long long wide_cap = std::max<unsigned long long>(ctx->q_wpat.cap / 4, 65536), wide_n = 0;
    if (const unsigned long long k = slots_min_knob("MTH_QUARTET")) n_slots = k;   // tests: force the retry
    for (;;) {
        MTH_HIP(ctx, ctx->q_keys.reserve(n_slots * 8, s));
        MTH_HIP(ctx, ctx->q_hist.reserve(n_slots * 64, s));
        MTH_HIP(ctx, hipMemsetAsync(ctx->q_keys.p, 0xFF, n_slots * 8, s));
        MTH_HIP(ctx, hipMemsetAsync(ctx->q_hist.p, 0, n_slots * 64, s));
        MTH_HIP(ctx, hipMemsetAsync(qs + 3, 0, sizeof(unsigned long long), s));
        MTH_HIP(ctx, hipMemsetAsync(qs + 7, 0, sizeof(unsigned long long), s));
        MTH_HIP(ctx, ctx->q_wpos.reserve(wide_cap * 16, s));
        MTH_HIP(ctx, ctx->q_wpat.reserve(wide_cap * 4, s));
        {
            LaunchTimer lt(ctx, K_QINSERT);
            hipLaunchKernelGGL(k_quartet_insert, dim3((d.n_reads + 255) / 256), dim3(256), 0, s, d.cpg_off, d.cpg_pos,
                               d.read_mapq, d.n_reads, params->min_qual, d.region_beg, d.region_end,
                               ctx->q_keys.as<unsigned long long>(), ctx->q_hist.as<uint32_t>(), n_slots - 1, qs + 3,
                               ctx->d_state, (const uint32_t *)t.tflag.as<uint32_t>(), tile_shift,
                               ctx->q_wpos.as<uint4>(), ctx->q_wpat.as<uint32_t>(), wide_cap, qs + 7);
        }
        unsigned long long ovf = 0;
        MTH_HIP(ctx, hipMemcpyAsync(&ovf, qs + 3, sizeof ovf, hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipMemcpyAsync(&wide_n, qs + 7, sizeof wide_n, hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipStreamSynchronize(s));
        if (wide_n > wide_cap) { wide_cap = wide_n; continue; }        // the wide list was too short: same table, again
        if (!ovf) break;
        n_slots <<= 2;
    }
    if (total + bound > t.cap) MTH_HIP(ctx, tile_rows_grow(ctx, t, total + bound, total));     // distinct quartets <= instances
    const uint32_t nblk = (uint32_t)((n_slots + 256 * QE_PER - 1) / (256 * QE_PER));
    MTH_HIP(ctx, ctx->q_blk.reserve((size_t)nblk * 4, s));
    MTH_HIP(ctx, ctx->q_batch_rows.reserve(4, s));
    {
        LaunchTimer lt(ctx, K_QEMIT);
        hipLaunchKernelGGL(k_quartet_blockcount, dim3(nblk), dim3(256), 0, s, ctx->q_keys.as<unsigned long long>(),
                           n_slots, ctx->q_blk.as<uint32_t>());
        hipLaunchKernelGGL(k_block_scan, dim3(1), dim3(1024), 0, s, ctx->q_blk.as<uint32_t>(), nblk, qs + 1, qs + 2,
                           ctx->q_batch_rows.as<uint32_t>(), 0u);
        hipLaunchKernelGGL(k_quartet_emit, dim3(nblk), dim3(256), 0, s, ctx->q_keys.as<unsigned long long>(),
                           (const unsigned long long *)nullptr,
                           ctx->q_hist.as<uint32_t>(), n_slots, ctx->q_blk.as<uint32_t>(), qs + 2,
                           ctx->q_pos.as<int32_t>(), ctx->q_cnt.as<uint32_t>(), ctx->q_me.as<float>(),
                           ctx->q_pm.as<float>(), ctx->q_depth.as<uint32_t>());
    }
    unsigned long long t2 = 0;
    MTH_HIP(ctx, hipMemcpyAsync(&t2, qs + 1, sizeof t2, hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    total = t2;
    if (wide_n) {
        // the wide instances under their 128-bit keys: same emit, rows appended after the packed-key rows of the batch
        unsigned long long w_slots = 1024;
        while (w_slots < 2 * wide_n) w_slots <<= 1;
        for (;;) {
            MTH_HIP(ctx, ctx->q_wk0.reserve(w_slots * 8, s));
            MTH_HIP(ctx, ctx->q_wk1.reserve(w_slots * 8, s));
            MTH_HIP(ctx, ctx->q_hist.reserve(w_slots * 64, s));
            MTH_HIP(ctx, hipMemsetAsync(ctx->q_wk0.p, 0xFF, w_slots * 8, s));
            MTH_HIP(ctx, hipMemsetAsync(ctx->q_wk1.p, 0xFF, w_slots * 8, s));
            MTH_HIP(ctx, hipMemsetAsync(ctx->q_hist.p, 0, w_slots * 64, s));
            MTH_HIP(ctx, hipMemsetAsync(qs + 3, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL(k_quartet_wide_insert, dim3((uint32_t)((wide_n + 255) / 256)), dim3(256), 0, s, ctx->q_wpos.as<uint4>(),
                               ctx->q_wpat.as<uint32_t>(), wide_n, ctx->q_wk0.as<unsigned long long>(), ctx->q_wk1.as<unsigned long long>(),
                               ctx->q_hist.as<uint32_t>(), w_slots - 1, qs + 3);
            unsigned long long ovf = 0;
            MTH_HIP(ctx, hipMemcpyAsync(&ovf, qs + 3, sizeof ovf, hipMemcpyDeviceToHost, s));
            MTH_HIP(ctx, hipStreamSynchronize(s));
            if (!ovf) break;
            w_slots <<= 2;
        }
        if (total + wide_n > t.cap) MTH_HIP(ctx, tile_rows_grow(ctx, t, total + wide_n, total));
        const uint32_t wblk = (uint32_t)((w_slots + 256 * QE_PER - 1) / (256 * QE_PER));
        MTH_HIP(ctx, ctx->q_blk.reserve((size_t)wblk * 4, s));
        hipLaunchKernelGGL(k_quartet_blockcount, dim3(wblk), dim3(256), 0, s, ctx->q_wk0.as<unsigned long long>(), w_slots, ctx->q_blk.as<uint32_t>());
        hipLaunchKernelGGL(k_block_scan, dim3(1), dim3(1024), 0, s, ctx->q_blk.as<uint32_t>(), wblk, qs + 1, qs + 2,
                           ctx->q_batch_rows.as<uint32_t>(), 0u);
        hipLaunchKernelGGL(k_quartet_emit, dim3(wblk), dim3(256), 0, s, ctx->q_wk0.as<unsigned long long>(),
                           (const unsigned long long *)ctx->q_wk1.as<unsigned long long>(),
                           ctx->q_hist.as<uint32_t>(), w_slots, ctx->q_blk.as<uint32_t>(), qs + 2,
                           ctx->q_pos.as<int32_t>(), ctx->q_cnt.as<uint32_t>(), ctx->q_me.as<float>(),
                           ctx->q_pm.as<float>(), ctx->q_depth.as<uint32_t>());
        MTH_HIP(ctx, hipMemcpyAsync(&t2, qs + 1, sizeof t2, hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipStreamSynchronize(s));
        total = t2;
    }
    return MTH_OK;
}

const TileMeasure *quartet_measure() {
    static const TileMeasure m = {quartet_tile_shift, quartet_grow_rows, quartet_launch_tiles, quartet_global_path};
    return &m;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_quartet_accumulate(mth_ctx_t *ctx, const mth_batch_t *batch, const mth_quartet_params_t *params) {
    if (!ctx || !batch || !params) return MTH_ERR_INVALID;
    ctx->q_epoch += 1;
    TileParams p{};
    p.quartet = *params;
    return tile_rows_accumulate(ctx, ctx->quartets, *batch, p);
}

// rows of all batches with depth >= min_depth (me.rs:82 / pm.rs:77); any pointer may be NULL.
// Call with every pointer NULL to get the count.
int mth_quartet_fetch(mth_ctx_t *ctx, uint32_t min_depth, uint64_t *n_rows, int32_t *tid, int32_t *pos4,
                      uint32_t *counts16, float *me, float *pm) {
    if (!ctx) return MTH_ERR_INVALID;
    int rc = sync_and_check(ctx);          // resolves the queued batches first
    if (rc) return rc;
    // Row order: per batch, sorted by (p1..p4): the tiles in position order give that for free (tile_rows_walk); a batch with
    // rows from the global path is sorted here.  The reference's order is HashMap-random.
    const TileRowTable &t = ctx->quartets;
    const uint64_t total = t.rows;
    std::vector<int32_t> hp;                // pos1..pos4 of every device row
    std::vector<uint64_t> &order = ctx->q_order;            // device row of every output row that passes the depth filter
    std::vector<int32_t> &order_tid = ctx->q_order_tid;
    const bool cached = ctx->q_order_epoch == ctx->q_epoch && ctx->q_order_min_depth == min_depth;
    if (!cached) {
        std::vector<uint32_t> depth(total);
        if (total) MTH_HIP(ctx, hipMemcpy(depth.data(), ctx->q_depth.p, total * 4, hipMemcpyDeviceToHost));
        order.clear(); order_tid.clear();
        bool any_heavy = false;
        {
            uint64_t batch_end = 0;
            for (const auto &mb : t.meta) { batch_end += mb.rows; any_heavy |= mb.heavy0 < batch_end; }
        }
        if (total && (pos4 || any_heavy)) {
            hp.resize(total * 4);
            MTH_HIP(ctx, hipMemcpy(hp.data(), ctx->q_pos.p, total * 16, hipMemcpyDeviceToHost));
        }
        size_t first = 0;                       // the batch's first output row
        bool unsorted = false;
        rc = tile_rows_walk(ctx, t, [&](const TileBatch &mb, uint64_t i, bool heavy) {
            if (depth[i] >= min_depth) { order.push_back(i); order_tid.push_back(mb.tid); unsorted |= heavy; }
        }, [&](size_t) {
            if (unsorted)                       // rows of the global path came in table order: put the batch in (pos1..pos4) order
                std::sort(order.begin() + (ptrdiff_t)first, order.end(), [&](uint64_t x, uint64_t y) {
                    return std::lexicographical_compare(hp.begin() + (ptrdiff_t)(x * 4), hp.begin() + (ptrdiff_t)(x * 4 + 4),
                                                        hp.begin() + (ptrdiff_t)(y * 4), hp.begin() + (ptrdiff_t)(y * 4 + 4));
                });
            first = order.size(); unsorted = false;
        });
        if (rc) return rc;
        ctx->q_order_epoch = ctx->q_epoch; ctx->q_order_min_depth = min_depth;
    }
    const uint64_t n = order.size();
    if (n_rows) *n_rows = n;
    if (!tid && !pos4 && !counts16 && !me && !pm) return MTH_OK;
    std::vector<uint32_t> hc(counts16 ? total * 16 : 0);
    std::vector<float> hme(me ? total : 0), hpm(pm ? total : 0);
    // rows of contig groups go back under their own contig: tid and positions are both needed for that, whichever was asked for
    const bool grouped = (tid || pos4) && has_group_batch(ctx, 3);
    std::vector<int32_t> tmp_tid, tmp_pos;
    if (grouped && !tid) { tmp_tid.resize(n); tid = tmp_tid.data(); }
    if (grouped && !pos4) { tmp_pos.resize(n * 4); pos4 = tmp_pos.data(); }
    if (total) {
        if (pos4 && hp.empty()) { hp.resize(total * 4); MTH_HIP(ctx, hipMemcpy(hp.data(), ctx->q_pos.p, total * 16, hipMemcpyDeviceToHost)); }
        if (counts16) MTH_HIP(ctx, hipMemcpy(hc.data(), ctx->q_cnt.p, total * 64, hipMemcpyDeviceToHost));
        if (me) MTH_HIP(ctx, hipMemcpy(hme.data(), ctx->q_me.p, total * 4, hipMemcpyDeviceToHost));
        if (pm) MTH_HIP(ctx, hipMemcpy(hpm.data(), ctx->q_pm.p, total * 4, hipMemcpyDeviceToHost));
    }
    for (uint64_t o = 0; o < n; ++o) {
        const uint64_t i = order[o];
        if (tid) tid[o] = order_tid[o];
        if (pos4) memcpy(pos4 + o * 4, hp.data() + i * 4, 16);
        if (counts16) memcpy(counts16 + o * 16, hc.data() + i * 16, 64);
        if (me) me[o] = hme[i];
        if (pm) pm[o] = hpm[i];
    }
    if (grouped) return ungroup_rows(ctx, n, tid, pos4, 4, 4, nullptr);
    return MTH_OK;
}

}  // extern "C"
