// mth_decode_dev.h -- what the record decode kernels share (mth_decode.hip: calls from XM:Z; mth_decode_genome.hip: calls
// from the genome; mth_decode_mm.hip: calls from MM:Z / ML:B:C): the argument block, unaligned loads, the --cpg-set lookup.
#pragma once
#include "mth_common.h"

namespace mth {

struct DecArgs {
    const uint8_t *raw;
    const uint64_t *off;          // n_rec + 1 byte offsets of the records (each starts with its block_size)
    uint32_t n_rec;
    int32_t *tid, *start, *end;
    uint8_t *mapq, *fwd;
    uint32_t *ncpg;               // pass 1 out
    uint2 *xm_loc;                // pass 1 out / pass 2 in: {offset of the XM string from the record core, its length}
    const unsigned long long *cpg_off;   // pass 2 in (exclusive scan of ncpg, n_rec + 1; global call indices)
    uint32_t *cpg_pos;
    uint16_t *cpg_rel;
    uint32_t *err;                // DevState.err
    uint32_t *notes;              // DevState.pad_: non-fatal findings (bit 0: a CIGAR P operation), read back with the error bits
    const unsigned long long *filt;   // --cpg-set: sorted keys tid << 32 | pos, or nullptr (no filter)
    uint64_t n_filt;
    uint32_t xm_min_mapq;         // a record WITHOUT XM:Z is an error only if its mapq >= this (lpmd.rs:176-181 filters on mapq first)
    // mth_decode_set_genome, staged form: record i's XM string is xm_base[xm_off[i] .. + xm_lens[i]) (what k_tag_xm wrote) and
    // the record's own aux fields are not looked at; nullptr: the string is the record's XM:Z field
    const uint8_t *xm_base;
    const unsigned long long *xm_off;
    const uint32_t *xm_lens;
    // mth_decode_set_modtags: the calls come from MM:Z / ML:B:C.  strand_fwd != 0: a record is forward iff its flag has no 0x10
    // (the position rule of readutil.rs:332 on the strand alone); 0: the flags 0 / 99 / 147 are.  mm_threshold: ML >= this is 'Z'
    uint32_t strand_fwd;
    uint32_t mm_threshold;
};

typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// filter_isin (readutil.rs:87-95): is (tid, pos) in the sorted key array ?
__device__ __forceinline__ bool in_cpg_set(const unsigned long long *__restrict__ keys, uint64_t n, unsigned long long key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == key;
}

}  // namespace mth
