// mth_quartet_dev.h -- device pieces of the ME / PM quartet tables shared by k_quartet_tile (mth_quartet.hip) and the fused
// PDR + LPMD + ME / PM tile pass (mth_multi.hip): the empty key, the LDS slot hash and the values of a histogram.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mth {

constexpr unsigned long long QKEY_EMPTY = ~0ull;

// slot of a key in an LDS table of mask + 1 slots: two 32-bit multiplies (a 64-bit mixer costs ~30 VALU)
__device__ __forceinline__ uint32_t quartet_slot(unsigned long long key, uint32_t mask) {
    uint32_t h = (uint32_t)(key >> 33) * 0x9E3779B1u ^ (uint32_t)key * 0x85EBCA6Bu;
    h ^= h >> 15;
    return h & mask;
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

}  // namespace mth
