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
// (d7 <= 0x7f, both constants are bytes).  The calls are sorted, so distances grow with g: the walk stops at the first diagonal
// on which no lane of the wave has a live pair within max (the counts do not depend on where it stops).
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

// Adds the read's pairs inside the window [mind, maxd] to lp_c (same state) / lp_d (states differ).  mrow = &M[n][0], n = the
// number of live slots (0: the lane counts nothing).  Needs lpmd_bytes_domain(mind, maxd); the early exit is a vote among the lanes that call it together.
MTH_LB_FN void lpmd_pairs_bytes(const uint32_t E0, const uint32_t E1, const uint32_t S0, const uint32_t S1, const LpMask *mrow,
                                const uint32_t mind, const uint32_t maxd, uint32_t &lp_c, uint32_t &lp_d) {
    const uint32_t KA = (0x80u - mind) * 0x01010101u, KB = (0x80u + maxd) * 0x01010101u;
    uint32_t accIN = 0, accDD = 0;
#pragma unroll
    for (int g = 1; g < 8; ++g) {
        const LpMask m = mrow[g];
        uint32_t orY;
        {   // pairs whose earlier call is one of the slots 0..3
            const uint32_t L = g < 4 ? lb_alignbyte(E1, E0, g) : E1 >> (8 * (g & 3));
            const uint32_t SL = g < 4 ? lb_alignbyte(S1, S0, g) : S1 >> (8 * (g & 3));
            const uint32_t D = L - E0;
            const uint32_t d7 = D & 0x7f7f7f7fu;
            const uint32_t Y = lb_bitop3<0x20>(KB - d7, D, m.w0);          // a & ~b & c
            const uint32_t IN = (d7 + KA) & Y;
            accIN += (uint32_t)__builtin_popcount(IN);                      // v_bcnt_u32_b32 adds its second operand: one instruction per count
            accDD += (uint32_t)__builtin_popcount(lb_bitop3<0x60>(IN, SL, S0));   // a & (b ^ c)
            orY = Y;
        }
        // ... one of the slots 4..7: live only in reads with more than 4 + g calls, so most waves skip it (on 150-bp WGBS reads at
        // 3 calls per read 60 % of the waves have no read with more than 5 calls): one compare and a scalar branch against 11 VALU
        if (g < 4 && lb_any(m.w1 != 0u)) {
            const uint32_t L = E1 >> (8 * g), SL = S1 >> (8 * g);
            const uint32_t D = L - E1;
            const uint32_t d7 = D & 0x7f7f7f7fu;
            const uint32_t Y = lb_bitop3<0x20>(KB - d7, D, m.w1);
            const uint32_t IN = (d7 + KA) & Y;
            accIN += (uint32_t)__builtin_popcount(IN);
            accDD += (uint32_t)__builtin_popcount(lb_bitop3<0x60>(IN, SL, S1));
            orY |= Y;
        }
        if (!lb_any(orY != 0u)) break;      // no lane has a live pair within max_distance on this diagonal
    }
    lp_c += accIN - accDD;
    lp_d += accDD;
}

}  // namespace mth
