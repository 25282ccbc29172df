// mth_lpmd_bytes.h -- LPMD windowed pair counts on 8-bit relative positions, four pairs per 32-bit instruction.
// Shared by the three PDR + LPMD kernel bodies (through mth_tile_dev.h); includes nothing from HIP and also compiles as plain
// C++ (one lane, tests/test_lpmd_bytes_host.py), where the gfx950 instructions below have stand-ins.
//
// A read holds up to 8 calls in registers: E0 / E1 = their relative positions, one per byte, as they lie in memory (slot k in
// byte k & 3 of word k >> 2); S0 / S1 = the top bytes of the 8 call words in the same layout (methylation state in bit 7 of
// each byte, the other 7 bits are ignored).  The live slots are a prefix 0..n-1 with ASCENDING relative positions; the dead
// slots may hold anything (in the kernels: the next reads' bytes).  Per diagonal g = 1..7 (pairs (j, j + g)):
//     L   = the bytes shifted down by g slots                    v_alignbyte_b32 / v_lshrrev_b32
//     D   = L - E                                                one subtraction = four byte distances
//     d7  = D & 0x7f7f7f7f
//     t   = d7 + (0x80 - min) * 0x01010101                       bit 7 of a byte: d7 >= min      (0 <= min <= 128)
//     u   = (0x80 + max) * 0x01010101 - d7                       bit 7 of a byte: d7 <= max      (0 <= max <= 127)
//     Y   = u & ~D & M[n][g]                                     ~D drops distances >= 128; M: 0x80 in byte j iff j + g < n
//     IN  = t & Y                                                the pair counts (readutil.rs:184, 196)
//     DD  = IN & (SL ^ S)                                        ... and its two states differ
// The single subtraction is exact: on a diagonal the live pairs are a prefix of the bytes and have L >= E, so a borrow can
// start only in a dead byte and runs upward, into dead bytes only; M removes those.  t and u never carry between bytes
// (d7 <= 0x7f, both constants are bytes).
// M need not be a table: "slot k is live" is k < n, so M[n][g] is the live-byte mask LB(n) (0x80 in byte i iff i < n, lpmd_live_bytes)
// shifted down g bytes -- v_alignbyte_b32 / v_lshrrev_b32 on the two words of LB, like L.  A lane that counts nothing passes LB = 0.
// The dense tile and run kernels take that form (an LDS read there is an uncovered wait); the hashed-site and fused kernels, which
// cover a read with seven waves a SIMD and are bound by instruction issue, keep M as a 9 x 8 LDS table (profiles/tile_loop_lds.md).
// Where the walk stops.  A diagonal without a live pair within max adds nothing, so the counts depend only on the walk reaching
// every diagonal that has one.  Relative positions ascend with the slot: if (j, j + g + 1) is live and within max, then (j, j + g)
// and (j + 1, j + g + 1) are live and within max as well (each lies inside it), and they are ADJACENT bytes j, j + 1 of Y on
// diagonal g.  So diagonal g + 1 can hold a pair only in a lane where Y & (Y >> 8) != 0 over the 64 bits of diagonal g (byte 3 of
// word 0 is adjacent to byte 0 of word 1), and by induction no later diagonal can hold one where diagonal g + 1 holds none: the walk
// goes on iff some lane of the wave has two such adjacent bytes.  (The rule it replaces, "some lane has one pair within max", walked
// about one diagonal more per chunk of 64 reads on 150-bp reads in a 2 / 16 window: profiles/tile_loop_lds.md.)  The word of the
// slots 4..7 is skipped by a vote of its own where no lane has a live pair in it; its Y is then zero, which is exact.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MTH_LB_FN __host__ __device__ __forceinline__
#else
#define MTH_LB_FN inline
#endif

namespace mth {

// the window bounds the byte form is exact for (min clamped at 0 below, max at 255 above, as the callers pass them)
MTH_LB_FN bool lpmd_bytes_domain(const int32_t mind, const int32_t maxd) { return mind >= 0 && mind <= 128 && maxd >= 0 && maxd <= 127; }

struct alignas(8) LpMask { uint32_t w0, w1; };     // slots 0..3, slots 4..7

// M[n][g], word w: 0x80 in every byte j with (4 w + j) + g < n
MTH_LB_FN uint32_t lpmd_bytes_mask(const uint32_t n, const uint32_t g, const uint32_t w) {
    uint32_t m = 0;
    for (uint32_t j = 0; j < 4; ++j) m |= (4u * w + j + g < n) ? 0x80u << (8u * j) : 0u;
    return m;
}

MTH_LB_FN uint32_t lb_alignbyte(const uint32_t hi, const uint32_t lo, const int sh) {      // bytes sh .. sh + 3 of hi:lo
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#endif
}
MTH_LB_FN uint32_t lb_perm(const uint32_t a, const uint32_t b, const uint32_t sel) {        // v_perm_b32: selectors 0-3 bytes of b, 4-7 bytes of a, 0x0c zero
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(a, b, sel);
#else
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = (sel >> (8 * k)) & 0xffu;
        const uint32_t byte = s < 4 ? (b >> (8 * s)) & 0xffu : (s < 8 ? (a >> (8 * (s - 4))) & 0xffu : 0u);
        r |= byte << (8 * k);
    }
    return r;
#endif
}
template <int TT>
MTH_LB_FN uint32_t lb_bitop3(const uint32_t a, const uint32_t b, const uint32_t c) {        // v_bitop3_b32: truth table TT (a = 0xf0, b = 0xcc, c = 0xaa)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
        if ((TT >> i) & 1) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
#endif
}
MTH_LB_FN bool lb_any(const bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(x);
#else
    return x;
#endif
}

// the state bytes of calls 0..3 / 4..7 in the layout of E0 / E1: two v_perm and one or per word
MTH_LB_FN uint32_t lpmd_state_bytes(const uint32_t v0, const uint32_t v1, const uint32_t v2, const uint32_t v3) {
    return lb_perm(v1, v0, 0x0c0c0703u) | lb_perm(v3, v2, 0x07030c0cu);
}

// LB(n), the live bytes of a read with n calls: 0x80 in byte i of the 64 bits (w0 = slots 0..3, w1 = slots 4..7) iff i < min(n, 8).
// Vector arithmetic on the call count, no table: one 64-bit shift of a constant (and a select for n = 0, which the shift cannot reach).
MTH_LB_FN LpMask lpmd_live_bytes(const uint32_t n) {
    const uint32_t nrow = n < 8u ? n : 8u;
    const uint64_t x = nrow ? 0x8080808080808080ull >> (64u - 8u * nrow) : 0ull;
    return LpMask{(uint32_t)x, (uint32_t)(x >> 32)};
}
// M[n][g] = LB(n) >> 8 g (slot j + g is live iff byte j + g of LB is set): its two words from the two of LB, one instruction each
MTH_LB_FN uint32_t lpmd_mask_w0(const uint32_t lb0, const uint32_t lb1, const int g) { return g < 4 ? lb_alignbyte(lb1, lb0, g) : lb1 >> (8 * (g & 3)); }
MTH_LB_FN uint32_t lpmd_mask_w1(const uint32_t lb0, const uint32_t lb1, const int g) { (void)lb0; return g < 4 ? lb1 >> (8 * g) : 0u; }

// Adds the read's pairs inside the window [mind, maxd] to lp_c (same state) / lp_d (states differ).  The masks of the diagonals come
// from LB(n) in registers (TAB = false: lb0 / lb1 = its two words; both zero: the lane counts nothing) or from a row of a table
// M[9][8] (TAB = true: mrow = &M[n][0], one 8-byte read per diagonal -- the form of the kernels that run enough waves to cover it).
// Needs lpmd_bytes_domain(mind, maxd); the word of the slots 4..7 and the early exit are votes among the lanes that call it together.
// walked (host tests only): the number of diagonals evaluated.
template <bool TAB>
MTH_LB_FN void lpmd_pairs_bytes_walk(const uint32_t E0, const uint32_t E1, const uint32_t S0, const uint32_t S1, const LpMask *mrow, const uint32_t lb0,
                                     const uint32_t lb1, const uint32_t mind, const uint32_t maxd, uint32_t &lp_c, uint32_t &lp_d, uint32_t *walked) {
    const uint32_t KA = (0x80u - mind) * 0x01010101u, KB = (0x80u + maxd) * 0x01010101u;
    uint32_t accIN = 0, accDD = 0;
#pragma unroll
    for (int g = 1; g < 8; ++g) {
        uint32_t m0, m1;
        if constexpr (TAB) { const LpMask m = mrow[g]; m0 = m.w0; m1 = m.w1; }
        else { m0 = lpmd_mask_w0(lb0, lb1, g); m1 = lpmd_mask_w1(lb0, lb1, g); }
        uint32_t adj;
        if (walked) *walked = (uint32_t)g;
        // pairs whose earlier call is one of the slots 0..3
        const uint32_t L0 = g < 4 ? lb_alignbyte(E1, E0, g) : E1 >> (8 * (g & 3));
        const uint32_t SL0 = g < 4 ? lb_alignbyte(S1, S0, g) : S1 >> (8 * (g & 3));
        const uint32_t D0 = L0 - E0;
        const uint32_t d70 = D0 & 0x7f7f7f7fu;
        const uint32_t Y0 = lb_bitop3<0x20>(KB - d70, D0, m0);            // a & ~b & c
        const uint32_t IN0 = (d70 + KA) & Y0;
        accIN += (uint32_t)__builtin_popcount(IN0);                         // v_bcnt_u32_b32 adds its second operand: one instruction per count
        accDD += (uint32_t)__builtin_popcount(lb_bitop3<0x60>(IN0, SL0, S0));   // a & (b ^ c)
        // ... one of the slots 4..7: live only in reads with more than 4 + g calls, so most waves skip it (on 150-bp WGBS reads at
        // 3 calls per read 60 % of the waves have no read with more than 5 calls): one compare and a scalar branch against 11 VALU
        if (g < 4 && lb_any(m1 != 0u)) {
            const uint32_t L = E1 >> (8 * g), SL = S1 >> (8 * g);
            const uint32_t D = L - E1;
            const uint32_t d7 = D & 0x7f7f7f7fu;
            const uint32_t Y1 = lb_bitop3<0x20>(KB - d7, D, m1);
            const uint32_t IN = (d7 + KA) & Y1;
            accIN += (uint32_t)__builtin_popcount(IN);
            accDD += (uint32_t)__builtin_popcount(lb_bitop3<0x60>(IN, SL, S1));
            adj = (Y0 & lb_alignbyte(Y1, Y0, 1)) | (Y1 & (Y1 >> 8));        // byte 3 of word 0 is adjacent to byte 0 of word 1
        } else {
            adj = Y0 & (Y0 >> 8);                                           // (no lane has a live pair in word 1: its Y is zero)
        }
        if (!lb_any(adj != 0u)) break;      // no lane has two adjacent live pairs within max_distance on this diagonal: none has a pair on the next
    }
    lp_c += accIN - accDD;
    lp_d += accDD;
}
MTH_LB_FN void lpmd_pairs_bytes(const uint32_t E0, const uint32_t E1, const uint32_t S0, const uint32_t S1, const uint32_t lb0, const uint32_t lb1,
                                const uint32_t mind, const uint32_t maxd, uint32_t &lp_c, uint32_t &lp_d, uint32_t *walked = nullptr) {
    lpmd_pairs_bytes_walk<false>(E0, E1, S0, S1, nullptr, lb0, lb1, mind, maxd, lp_c, lp_d, walked);
}
MTH_LB_FN void lpmd_pairs_bytes(const uint32_t E0, const uint32_t E1, const uint32_t S0, const uint32_t S1, const LpMask *mrow,
                                const uint32_t mind, const uint32_t maxd, uint32_t &lp_c, uint32_t &lp_d, uint32_t *walked = nullptr) {
    lpmd_pairs_bytes_walk<true>(E0, E1, S0, S1, mrow, 0u, 0u, mind, maxd, lp_c, lp_d, walked);
}

}  // namespace mth
