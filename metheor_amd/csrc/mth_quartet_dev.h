// mth_quartet_dev.h -- device pieces of the ME / PM quartet tables shared by k_quartet_tile (mth_quartet.hip) and the quartet side of
// the tile pass of mth_pdr_wide.hip (k_multi_tile): the empty key, the LDS slot hash, the window insert, the row phase and the values
// of a histogram.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mth_tile_dev.h"

namespace mth {

constexpr unsigned long long QKEY_EMPTY = ~0ull;

// slot of a key in an LDS table of mask + 1 slots: two 32-bit multiplies (a 64-bit mixer costs ~30 VALU)
__device__ __forceinline__ uint32_t quartet_slot(unsigned long long key, uint32_t mask) {
    uint32_t h = (uint32_t)(key >> 33) * 0x9E3779B1u ^ (uint32_t)key * 0x85EBCA6Bu;
    h ^= h >> 15;
    return h & mask;
}

// One window of four consecutive calls (readutil.rs:105-129) into a tile's LDS table of SLOTS slots (64-bit key, sixteen 16-bit bins in
// 8 words: bin 2w in the low half of word w, bin 2w+1 in the high half).  The quartet belongs to the tile [T0, T1) that holds p1.
enum QuartetWindow { QW_PLACED, QW_NOT_MINE, QW_HAND_BACK };
template <int SLOTS>
__device__ __forceinline__ QuartetWindow quartet_window(const uint32_t x, const uint32_t y, const uint32_t z, const uint32_t w, const int32_t T0,
                                                        const int32_t T1, unsigned long long *keys, uint32_t *bins) {
    const int32_t p1 = (int32_t)(x & 0x7fffffffu);
    if (p1 < T0 || p1 >= T1) return QW_NOT_MINE;
    const uint32_t d2 = (y & 0x7fffffffu) - (x & 0x7fffffffu), d3 = (z & 0x7fffffffu) - (y & 0x7fffffffu),
                   d4 = (w & 0x7fffffffu) - (z & 0x7fffffffu);
    const unsigned long long key = ((unsigned long long)(uint32_t)p1 << 33) | ((unsigned long long)d2 << 22) |
                                   ((unsigned long long)d3 << 11) | (unsigned long long)d4;
    // CpGs >= 2048 bp apart (or out of order): the global path sorts it out
    if (d2 - 1u >= 2047u || d3 - 1u >= 2047u || d4 - 1u >= 2047u || key == QKEY_EMPTY) return QW_HAND_BACK;
    const uint32_t pat = ((x >> 31) << 3) | ((y >> 31) << 2) | ((z >> 31) << 1) | (w >> 31);
    uint32_t h = quartet_slot(key, SLOTS - 1), probes = 0;
    while (probes++ < (uint32_t)SLOTS) {
        const unsigned long long cur = atomicCAS(&keys[h], QKEY_EMPTY, key);
        if (cur == QKEY_EMPTY || cur == key) { atomicAdd(&bins[h * 8 + (pat >> 1)], (pat & 1u) ? 0x10000u : 1u); return QW_PLACED; }   // me.rs:121-125
        h = (h + 1) & (SLOTS - 1);
    }
    return QW_HAND_BACK;                                     // more distinct quartets than slots
}

// me.rs:42-55 and pm.rs:42-51 with the reference's operation order.  Plain operators, and the whole
// engine is compiled with -ffp-contract=off: with hipcc's default (contract=fast) `pm - p*p` became an
// FMA -- HIP's __fmul_rn/__fsub_rn header functions did not prevent it -- and 2.8 % of PM values were
// one ulp off the reference expression (measured; tools/pm_probe.py).
__device__ __forceinline__ void quartet_values(const uint32_t *c, float &me, float &pm, uint32_t &total) {
#pragma clang fp contract(off)
    total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) total += c[k];
    const float tf = (float)total;
    me = 0.0f;
    pm = 1.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float p = (float)c[k] / tf;
        if (c[k] > 0) {
            const float t = p * log2f(p);
            me = me + t;
        }
        const float sq = p * p;
        pm = pm - sq;
    }
    me = me * -0.25f;
}

// The row phase of a tile's table: rows go out sorted by key = (p1, d2, d3, d4) = (p1, p2, p3, p4).  Bucket sort on p1: B buckets of
// 1 << BSHIFT positions, a few keys each.  Every thread holds its slots in registers, so the table is rebuilt in place in bucket
// order; a key's final rank = start of its bucket + the keys of that bucket below it.  (Before: an all-pairs rank sort / bitonic
// network over the tile's keys -- most of the kernel's time on sparse WGBS.)
// In: bcnt cleared and the table complete (a barrier since); live = false leaves the table out (a tile that is handed back).  Between the
// scan and the scatter thread 0 calls claim(rows of the tile), which returns the tile's first output row and records the tile; rows that
// would end beyond row_cap are not written.  bbase (B words) and sslot (SLOTS 16-bit source slots) may lie under the read phases' queue.
template <int SLOTS, int B, int BSHIFT, typename Claim>
__device__ __forceinline__ void quartet_rows(unsigned long long *keys, const uint32_t *bins, uint32_t *bcnt, uint32_t *bbase, uint16_t *sslot,
                                             uint32_t *ws, const int32_t T0, const bool live, Claim claim, const unsigned long long row_cap,
                                             int32_t *out_pos, uint32_t *out_cnt, float *out_me, float *out_pm, uint32_t *out_depth) {
    static_assert(SLOTS % B == 0 && B == 256 && SLOTS <= 65536, "each thread owns SLOTS / B slots and one bucket; 16-bit source slots");
    constexpr int PER = SLOTS / B;
    __shared__ unsigned long long s_row0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long kk[PER];
    uint32_t pib[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        kk[k] = live ? keys[tid * PER + k] : QKEY_EMPTY;
        pib[k] = 0;
        if (kk[k] != QKEY_EMPTY) pib[k] = atomicAdd(&bcnt[((uint32_t)(kk[k] >> 33) - (uint32_t)T0) >> BSHIFT], 1u);
    }
    __syncthreads();                                    // every slot is in registers now: the table can be overwritten
    const uint32_t m = bcnt[tid];
    const uint32_t incl = wave_scan_incl(m);
    if (lane == 63) ws[wave + 1] = incl;
    __syncthreads();
    if (tid == 0) {
        ws[0] = 0;
        for (int w = 1; w <= B / 64; ++w) ws[w] += ws[w - 1];
        s_row0 = claim(ws[B / 64]);
    }
    __syncthreads();
    const uint32_t n = ws[B / 64];
    if (n == 0 || s_row0 + n > row_cap) return;         // block-uniform
    bbase[tid] = ws[wave] + incl - m;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (kk[k] == QKEY_EMPTY) continue;
        const uint32_t dst = bbase[((uint32_t)(kk[k] >> 33) - (uint32_t)T0) >> BSHIFT] + pib[k];
        keys[dst] = kk[k];
        sslot[dst] = (uint16_t)(tid * PER + k);
    }
    __syncthreads();
    for (uint32_t j = tid; j < n; j += B) {
        const unsigned long long key = keys[j];
        const uint32_t bk = ((uint32_t)(key >> 33) - (uint32_t)T0) >> BSHIFT, b0 = bbase[bk], b1 = b0 + bcnt[bk];
        uint32_t r = b0;
        for (uint32_t i = b0; i < b1; ++i) r += keys[i] < key ? 1u : 0u;
        const uint32_t h = sslot[j];
        const unsigned long long o = s_row0 + r;
        const int32_t p1 = (int32_t)(key >> 33);
        const int32_t p2 = p1 + (int32_t)((key >> 22) & 2047u), p3 = p2 + (int32_t)((key >> 11) & 2047u),
                      p4 = p3 + (int32_t)(key & 2047u);
        reinterpret_cast<int4 *>(out_pos)[o] = make_int4(p1, p2, p3, p4);
        uint32_t c[16];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const uint32_t v = bins[h * 8 + w];
            c[2 * w] = v & 0xffffu; c[2 * w + 1] = v >> 16;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            reinterpret_cast<uint4 *>(out_cnt + o * 16)[q] = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        float me, pm;
        uint32_t total;
        quartet_values(c, me, pm, total);
        out_me[o] = me; out_pm[o] = pm; out_depth[o] = total;
    }
}

}  // namespace mth
