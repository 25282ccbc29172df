// mth_inflate.hip -- BGZF (RFC 1951 DEFLATE) block inflate and per-block record walk on the device
// (the step before the record decode; replaces bamutil.rs:4-11's htslib reader thread).
//
// BGZF = independent <= 64-KiB gzip members, each one raw DEFLATE stream: embarrassingly parallel across blocks,
// strictly serial inside one.  Mapping: ONE WAVE per BGZF block.  The decoder state (bit buffer, input cursor,
// output cursor) is wave-uniform, so the symbol loop is effectively one decoder per wave; the lanes are used for
// what is parallel -- filling the Huffman lookup tables (lane = symbol) and copying matches (lane = byte).
// Huffman decode: a direct lookup table on the low ROOT bits (codes are read LSB-first, so the index is the
// bit-reversed code) for codes up to ROOT bits, canonical bit-by-bit decode (count / first-code walk) for the few
// longer ones.  Output goes straight to HBM; back-references read it back (the window of a block is the block).
// A block is checked against its ISIZE; any inconsistency sets ERRB_FORMAT.
//
// k_block_walk: BAM writers built on htslib flush the BGZF block before a record that would not fit, so records
// never straddle blocks and every block starts at a record boundary: one thread per block follows the block_size
// chain, counting / writing record offsets, and VERIFIES that the chain ends exactly at the block's end.  A file for
// which that does not hold sets ERRB_UNALIGNED and the caller takes the host walk instead -- or mth_bgzf_decode_straddle:
//
// Records that STRADDLE blocks (htsjdk / Picard / GATK, sambamba, biobambam cut blocks at a byte count).  The inflated stream of a
// call is contiguous in inf_raw; only the record offsets are missing, and the entry offset of block b is the exit offset of block
// b - 1: a serial chain over the file.  It is built by speculation and exact verification.  k_straddle_guess: a wave per block finds
// the block's first offset that looks like a record start (the block that holds first_byte starts there).  k_straddle_walk: a thread
// per block follows block_size from its entry while a record STARTS inside the block (it may end in a later one) and leaves a count
// and an exit offset, absolute in the stream; a speculative walk sets no error bit, an unreadable or bogus block_size just ends it
// with an exit past everything.  The state is final when block 0 enters at first_byte and every block enters where its predecessor
// left (a block whose entry lies at or past its own end passes it on): by induction those are the offsets of the serial chain, and
// nothing of the guess rule enters the result.  Until then k_straddle_check / k_straddle_repair run in rounds -- separate launches,
// the host reads one mismatch counter per round, no grid barrier, no workgroup waits for another -- at most
// MTH_STRADDLE_MAX_ROUNDS of them; past that the call is MTH_ERR_UNALIGNED like mth_bgzf_decode's and the caller takes the host
// walk.  A record that covers k whole blocks costs about k rounds.  Then count -> scan_u32_to_u64 -> fill (the only pass that raises
// ERRB_FORMAT: block_size < 32, or a finished stream that ends inside a record) and decode_core as ever.  A call whose stream ends
// inside a record keeps the bytes from that record's start on the device (ctx->inf_carry); they come first in the next call's
// stream, whose block 0 then begins at offset 0.
//
// mth_bgzf_straddle_scan: the same scheme one level up, for the shards of a multi-GPU run over such a file.  A RUN of blocks is
// inflated and its chain found from a guessed entry (block 0 guesses like the others), nothing is decoded, and the caller verifies
// the runs against each other as the rounds verify the blocks: run r must enter where run r - 1 left.  Two things differ.  No block
// of a guessed run has a certain entry, so an exit is believed only as far as the next block: where a block has no guess, or leaves
// at or past the end of the block behind it, the chain breaks and that block keeps its own guess; k_straddle_keys counts the breaks
// and such a run is scanned again.  And
// the stream carries look-ahead blocks behind the run, so a record that ends beyond it leaves at p + 4 + block_size, a value the
// next run is held against.  The second pass, mth_bgzf_straddle_rescan, takes the true entry and the state the context kept
// (inflated bytes, block table, links): repair rounds from block 0, no copy and no inflate.
#include "mth_ctx.h"
#include "mth_inflate.h"

namespace mth {

// Reads of a CORRUPT last block can run past the staged file bytes: garbage keeps decoding until the output bound (isize <= 64 KiB)
// stops it.  A literal costs at most 15 bits (the direct-lookup width LROOT is not the code length limit: DEFLATE codes go up to 15
// bits) = 120 KiB of input for 64 Ki literals; a match costs at most 15 + 5 + 15 + 13 bits and yields >= 3 bytes: less per output
// byte.  The staging buffers carry 160 KiB of zeroed padding, so the bit reader's scalar loads always stay inside the allocation
// and read defined bytes (the CRC / ISIZE checks then flag the block): INF_FILE_PAD, mth_inflate.h.

constexpr int LROOT = 10, DROOT = 9;          // direct-lookup bits of the literal/length and distance tables
struct InflArgs {
    const uint8_t *file;                      // the compressed file, padded by >= 16 readable bytes
    const uint64_t *coff;                     // per block: offset of the DEFLATE payload in the file
    const uint32_t *csize, *isize;            // payload bytes / inflated bytes
    const uint64_t *uoff;                     // offset of the block's output in the inflated stream
    uint32_t n_blocks;
    uint8_t *out;
    uint32_t *err;
    int fast_literals;                         // the hand-written literal loop (METHEOR_INFLATE_ASM=0 turns it off: A/B)
};

__constant__ uint8_t c_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one Huffman code: lens[0..n) -> direct table (entry = sym << 4 | len, 0 = not a short code) + canonical arrays
struct Huff {
    uint16_t *tab;        // 1 << root entries
    uint16_t *sorted;     // symbols ordered by (length, symbol)
    uint16_t *count;      // [16] codes per length
    int root;
    uint16_t *tmp;        // [32] builder scratch (next code / sorted offset per length)
};

// wave-cooperative build; returns false for an over-subscribed code (incomplete codes are accepted as zlib does for
// the single-distance-code case; an unused entry decodes as an error later)
__device__ bool huff_build(const Huff &h, const uint8_t *lens, int n, uint16_t *code_of /* scratch, n entries */, bool flag_literals = false) {
    const int lane = threadIdx.x & 63;
    if (lane < 16) h.count[lane] = 0;
    for (int i = lane; i < (1 << h.root); i += 64) h.tab[i] = 0;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {                  // canonical codes (RFC 1951 3.2.2); per-length arrays in LDS (dynamic indexing)
        uint16_t *cnt = h.count, *next = h.tmp, *offs = h.tmp + 16;
        for (int s = 0; s < n; ++s) cnt[lens[s]]++;
        cnt[0] = 0;
        int left = 1;
        bool over = false;
        for (int l = 1; l < 16; ++l) { left <<= 1; left -= cnt[l]; if (left < 0) over = true; }
        uint32_t code = 0;
        uint16_t o = 0;
        next[0] = 0; offs[0] = 0;
        for (int l = 1; l < 16; ++l) { code = (code + cnt[l - 1]) << 1; next[l] = (uint16_t)code; offs[l] = o; o += cnt[l]; }
        for (int s = 0; s < n; ++s) {
            const int l = lens[s];
            if (l) { code_of[s] = next[l]++; h.sorted[offs[l]++] = (uint16_t)s; } else code_of[s] = 0;
        }
        cnt[0] = over ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (h.count[0]) return false;
    // direct table: lane = symbol; a code of length l <= root owns every index whose low l bits are its reversal
    for (int s = lane; s < n; s += 64) {
        const int l = lens[s];
        if (l == 0 || l > h.root) continue;
        const uint32_t rev = __builtin_bitreverse32((uint32_t)code_of[s]) >> (32 - l);
        const uint16_t e = (uint16_t)((s << 4) | l | ((flag_literals && s < 256) ? 0x8000 : 0));   // bit 15: a literal (the asm loop tests it)
        for (uint32_t k = rev; k < (1u << h.root); k += (1u << l)) h.tab[k] = e;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return true;
}

// The bit reader.  Wave-uniform by construction: every field lives in scalar registers and the input is read with SCALAR
// loads of aligned dwords (the file bytes are not written by this launch), so a refill neither occupies a vector lane nor
// waits for the literal stores in flight (a vector load's s_waitcnt vmcnt does).
// (the decoder state IS wave-uniform, but values that came through LDS or a vector load look divergent to the compiler:
// readfirstlane states the fact at the scalar-asm boundaries)
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }
template <class T> __device__ __forceinline__ T *uni_ptr(T *p) { return reinterpret_cast<T *>(uni64(reinterpret_cast<uint64_t>(p))); }
__device__ __forceinline__ uint32_t sload_dword(const uint8_t *p) {   // p: wave-uniform, 4-byte aligned
    uint32_t w;
    const uint8_t *q = uni_ptr(p);
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(q) : "memory");
#ifndef MTH_INFLATE_DIVERGENT_STATE
    w = uni(w);                          // (an asm result counts as divergent: say it is not, or the whole decoder moves to the vector unit)
#endif
    return w;
}
struct Bits {
    const uint8_t *file;         // the compressed bytes (a kernel argument: loads through file + offset stay global, uniform loads --
                                 // a pointer that came back from the scalar asm would be a flat one, and flat loads count as divergent)
    uint64_t in, end;            // byte offsets in file: next aligned dword to load; first byte past the payload (reads run a few bytes beyond: the file is padded)
    uint64_t bb;
    int bc;
    __device__ __forceinline__ void seek(uint64_t p) {          // start reading at byte offset p
        const uint32_t skip = ((uint32_t)(reinterpret_cast<uintptr_t>(file) + p) & 3u) * 8u;
        in = p - (skip >> 3);
        const uint32_t w = sload_dword(file + in);
        in += 4;
        bb = w >> skip; bc = 32 - (int)skip;
    }
    __device__ __forceinline__ void refill() {
        if (bc < 32) {
            const uint32_t w = sload_dword(file + in);
            bb |= (uint64_t)w << bc;
            in += 4; bc += 32;
        }
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(int n) { bb >>= n; bc -= n; }
    __device__ __forceinline__ uint32_t take(int n) { const uint32_t v = peek(n); drop(n); return v; }
    // bytes consumed so far (whole bytes of the bit buffer given back), as an offset in file
    __device__ __forceinline__ uint64_t cursor() const { return in - (uint64_t)(bc >> 3); }
};

// A run of literals in hand-written ISA: while the next code is a direct-table hit for a literal (bit 15 of the entry), decode
// it, store it and go on -- three per trip around the loop (a refill leaves >= 32 bits, a table hit takes <= 10), refilling
// from scalar memory as it goes; table index, literal test and code length are worked out on the vector side (the scalar unit
// is the busy one): ~5 scalar + 8 vector instructions per literal against the ~30 + 15 the compiler made of the
// general symbol loop; the scalar unit, one per CU, is what k_inflate is bound by (PMC: 10.8 G scalar / 5.8 G vector
// instructions per 13 441 blocks before, profiles/r02_e2e.md).  The output bound is checked where the bits are refilled: at
// most 63 + 2 literals can follow a refill, so the loop only runs while 72 bytes of room are left and the block's last bytes
// go through the general loop.  Leaves at anything else (length code, end of block, long code) with the state as the general
// loop expects it.
#define MTH_LIT_STEP                                     \
    "v_mov_b32 %[vt], s40\n\t"                           \
    "v_and_b32 %[vt], 0x3ff, %[vt]\n\t"                  \
    "v_lshl_add_u32 %[vt], %[vt], 1, %[vlt]\n\t"         \
    "ds_read_u16 %[ve], %[vt]\n\t"                       \
    "s_waitcnt lgkmcnt(0)\n\t"                           \
    "v_cmp_gt_u32 vcc, 0x8000, %[ve]\n\t"                \
    "v_and_b32 %[vt], 15, %[ve]\n\t"                     \
    "s_cbranch_vccnz L_exit_%=\n\t"                      \
    "v_readfirstlane_b32 %[e], %[vt]\n\t"                \
    "s_lshr_b64 s[40:41], s[40:41], %[e]\n\t"            \
    "s_sub_u32 %[bc], %[bc], %[e]\n\t"                   \
    "v_lshrrev_b32 %[ve], 4, %[ve]\n\t"                  \
    "global_store_byte %[vpos], %[ve], %[out]\n\t"       \
    "v_add_u32 %[vpos], 1, %[vpos]\n\t"
__device__ __forceinline__ void literal_run(Bits &b, uint32_t &pos, const uint32_t isize, uint8_t *out0, const uint32_t ltab_lds) {
    // The loop checks the output bound where it refills; entered with >= 32 bits in hand it would store up to 63 + 2 literals
    // before its first check: same bound here, once per call (a corrupt stream must not write into the next block's output).
    if (pos + 72u > isize) return;
    uint64_t bb = uni64(b.bb), tmp;
    const uint64_t base = uni64(reinterpret_cast<uint64_t>(b.file));
    uint64_t in = base + uni64(b.in);                   // the address as an integer: scalar registers s[42:43]
    int32_t bc = (int32_t)uni((uint32_t)b.bc);
    uint32_t t, e, vt, ve;
    uint32_t vpos = pos;
    const uint32_t u_isize = uni(isize), u_lt = uni(ltab_lds);
    uint8_t *const u_out = uni_ptr(out0);
    asm volatile(
        "L_top_%=:\n\t"
        "s_cmp_lt_i32 %[bc], 32\n\t"
        "s_cbranch_scc0 L_go_%=\n\t"
        "v_readfirstlane_b32 %[t], %[vpos]\n\t"
        "s_add_u32 %[t], %[t], 72\n\t"
        "s_cmp_gt_u32 %[t], %[isize]\n\t"
        "s_cbranch_scc1 L_exit_%=\n\t"
        "s_load_dword s44, s[42:43], 0x0\n\t"
        "s_add_u32 s42, s42, 4\n\t"
        "s_addc_u32 s43, s43, 0\n\t"
        "s_mov_b32 s45, 0\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_lshl_b64 s[44:45], s[44:45], %[bc]\n\t"
        "s_or_b64 s[40:41], s[40:41], s[44:45]\n\t"
        "s_add_u32 %[bc], %[bc], 32\n\t"
        "L_go_%=:\n\t"
        MTH_LIT_STEP MTH_LIT_STEP MTH_LIT_STEP
        "s_branch L_top_%=\n\t"
        "L_exit_%=:\n\t"
        : "+{s[40:41]}"(bb), "+{s[42:43]}"(in), [bc] "+s"(bc), [vpos] "+v"(vpos), "=&{s[44:45]}"(tmp), [t] "=&s"(t), [e] "=&s"(e),
          [vt] "=&v"(vt), [ve] "=&v"(ve)
        : [vlt] "v"(u_lt), [isize] "s"(u_isize), [out] "s"(u_out)
        : "memory", "scc", "vcc");
#ifndef MTH_INFLATE_DIVERGENT_STATE
    b.bb = uni64(bb); b.in = uni64(in) - base; b.bc = (int)uni((uint32_t)bc); pos = uni(vpos);
#else
    b.bb = bb; b.in = in - base; b.bc = bc; pos = vpos;
#endif
}
#undef MTH_LIT_STEP

// decode one symbol; -1 on an invalid code
__device__ __forceinline__ int huff_decode(const Huff &h, Bits &b) {
    const uint32_t e = h.tab[b.peek(h.root)];
    if (e) { b.drop((int)(e & 15u)); return (int)((e >> 4) & 0x7ffu); }
    // longer than root bits (or invalid): canonical walk, one bit at a time (RFC 1951 3.2.2; MSB of the code first)
    int code = 0, first = 0, index = 0;
#pragma unroll 1                                       // rare path: unrolled 15 deep it tripled the kernel and cost it a wave per SIMD
    for (int l = 1; l < 16; ++l) {
        code |= (int)b.take(1);
        const int c = h.count[l];
        if (code - c < first) return h.sorted[index + (code - first)];
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// The symbols of one DEFLATE block (RFC 1951 3.2.3-3.2.5) up to its end-of-block code; true = the stream is invalid.
// Early returns instead of loop-carried error flags: the flags were most of what the compiler's version spent per symbol.
__device__ __forceinline__ bool inflate_symbols(Bits &b, const Huff &HL, const Huff &HD, uint32_t &pos, const uint32_t isize, uint8_t *out0,
                                                const uint32_t ltab_lds, const bool fast_literals, const int lane, const uint32_t *s_lbx,
                                                const uint32_t *s_dbx) {
    for (;;) {
        if (fast_literals) literal_run(b, pos, isize, out0, ltab_lds);
        b.refill();
        const int sym = huff_decode(HL, b);
        if (sym < 0) return true;
        if (sym < 256) {
            if (pos >= isize) return true;
            out0[pos] = (uint8_t)sym;          // every lane, same address, same value: no exec-mask juggling for lane 0
            ++pos;
            continue;
        }
        if (sym == 256) return false;
        if (sym > 285) return true;
        const int li = sym - 257;
        // base and extra bits of a length / distance symbol (RFC 1951 3.2.5) from two small LDS tables built at kernel start:
        // by arithmetic they were ~25 scalar instructions per match, on the unit the kernel is bound by
        const uint32_t lbx = s_lbx[li];
        const uint32_t len = (lbx & 0xffffu) + b.take((int)(lbx >> 16));
        b.refill();
        const int ds = huff_decode(HD, b);
        if (ds < 0 || ds > 29) return true;
        const uint32_t dbx = s_dbx[ds];
        const uint32_t dist = (dbx & 0xffffu) + b.take((int)(dbx >> 16));
        if (dist > pos || pos + len > isize) return true;
        // the bytes written so far must be visible to the loads below (same wave, but loads and stores return
        // out of order with respect to each other)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (dist >= len) {                              // no overlap: all lanes copy at once
            for (uint32_t k = lane; k < len; k += 64) out0[pos + k] = out0[pos - dist + k];
        } else {                                        // overlapping run: the source repeats with period dist
            for (uint32_t k = lane; k < len; k += 64) out0[pos + k] = out0[pos - dist + (k % dist)];
        }
        pos += len;
    }
}

__global__ __launch_bounds__(64, 8) void k_inflate(const InflArgs a) {
    __shared__ uint16_t s_ltab[1 << LROOT], s_dtab[1 << DROOT];
    __shared__ uint16_t s_lsorted[288], s_dsorted[32], s_lcount[16], s_dcount[16], s_code[320];
    __shared__ uint8_t s_lens[320];
    __shared__ uint16_t s_tmp[32];
    __shared__ uint32_t s_lbx[32], s_dbx[32];     // length / distance symbols: base | extra bits << 16 (RFC 1951 3.2.5)
    const uint32_t blk = blockIdx.x;
    if (blk >= a.n_blocks) return;
    const int lane = threadIdx.x;
    if (lane < 29) {                               // from the 9th length symbol on, four symbols per extra-bit count
        const uint32_t li = (uint32_t)lane, lx = (li < 8 || li == 28) ? 0u : (li >> 2) - 1u;
        s_lbx[lane] = (li < 8 ? li + 3u : (li == 28 ? 258u : ((4u + (li & 3u)) << lx) + 3u)) | (lx << 16);
    }
    if (lane < 30) {                               // from the 5th distance symbol on, two per extra-bit count
        const uint32_t ds = (uint32_t)lane, dx = ds < 4 ? 0u : (ds >> 1) - 1u;
        s_dbx[lane] = (ds < 4 ? ds + 1u : ((2u + (ds & 1u)) << dx) + 1u) | (dx << 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint8_t *const out0 = a.out + a.uoff[blk];
    const uint32_t isize = a.isize[blk];
    Bits b;
    b.file = a.file;
    b.end = a.coff[blk] + a.csize[blk];
    b.seek(a.coff[blk]);
    const uint32_t ltab_lds = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint16_t *)s_ltab);
    const Huff HL{s_ltab, s_lsorted, s_lcount, LROOT, s_tmp}, HD{s_dtab, s_dsorted, s_dcount, DROOT, s_tmp};
    uint32_t pos = 0;
    bool bad = false, last = false;
    while (!last && !bad) {
        b.refill();
        last = b.take(1) != 0;
        const uint32_t type = b.take(2);
        if (type == 0) {                                   // stored
            b.drop(b.bc & 7);                              // to the byte boundary
            const uint64_t po = b.cursor();
            const uint8_t *p = a.file + po;
            const uint32_t len = (uint32_t)p[0] | ((uint32_t)p[1] << 8), nlen = (uint32_t)p[2] | ((uint32_t)p[3] << 8);
            p += 4;
            if ((len ^ nlen) != 0xffffu || pos + len > isize || po + 4 + len > b.end) { bad = true; break; }
            for (uint32_t i = lane; i < len; i += 64) out0[pos + i] = p[i];
            pos += len;
            b.seek(po + 4 + len);
            continue;
        }
        if (type == 3) { bad = true; break; }
        if (type == 1) {                                   // fixed codes (RFC 1951 3.2.6)
            for (int s = lane; s < 288; s += 64) s_lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (!huff_build(HL, s_lens, 288, s_code, true)) { bad = true; break; }
            for (int s = lane; s < 30; s += 64) s_lens[s] = 5;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (!huff_build(HD, s_lens, 30, s_code)) { bad = true; break; }
        } else {                                           // dynamic codes (3.2.7)
            b.refill();
            const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
            if (hlit > 286 || hdist > 30) { bad = true; break; }
            if (lane < 19) s_lens[lane] = 0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int i = 0; i < hclen; ++i) {
                b.refill();
                const uint32_t v = b.take(3);
                if (lane == 0) s_lens[c_clen_order[i]] = (uint8_t)v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the code-length code reuses the distance table's storage (root 7 <= DROOT)
            const Huff HC{s_dtab, s_dsorted, s_dcount, 7, s_tmp};
            if (!huff_build(HC, s_lens, 19, s_code)) { bad = true; break; }
            int i = 0, prev = 0;
            const int total = hlit + hdist;
            while (i < total) {
                b.refill();
                const int sym = huff_decode(HC, b);
                if (sym < 0) { bad = true; break; }
                int rep = 1, val = sym;
                if (sym == 16) { if (i == 0) { bad = true; break; } val = prev; rep = 3 + (int)b.take(2); }
                else if (sym == 17) { val = 0; rep = 3 + (int)b.take(3); }
                else if (sym == 18) { val = 0; rep = 11 + (int)b.take(7); }
                if (i + rep > total) { bad = true; break; }
                // lens of the literal/length code then of the distance code, one array (s_lens is 320 long)
                for (int k = lane; k < rep; k += 64) s_lens[i + k] = (uint8_t)val;   // into a second region below
                i += rep; prev = val;
            }
            if (bad) break;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (s_lens[256] == 0) { bad = true; break; }   // no end-of-block code
            // the distance lengths follow the literal/length ones: build the distance code first (it lives in s_dtab,
            // which the code-length code no longer needs), from a copy at the front of a scratch region
            if (!huff_build(HD, s_lens + hlit, hdist, s_code)) { bad = true; break; }
            if (!huff_build(HL, s_lens, hlit, s_code, true)) { bad = true; break; }
        }
        // ---- symbols ----
        if (inflate_symbols(b, HL, HD, pos, isize, out0, ltab_lds, a.fast_literals != 0, lane, s_lbx, s_dbx)) { bad = true; break; }
    }
    if (!bad && (pos != isize || b.cursor() > b.end)) bad = true;
    if (bad && lane == 0) atomicOr(a.err, (uint32_t)ERRB_FORMAT);
}


// ---- CRC32 of the inflated blocks (gzip trailer; htslib and the host reader verify it, so does this path) ----------
// One wave per block.  Raw CRC (init 0, no final xor) is linear and ignores leading zeros, so the block is cut into 64
// chunks of 1 KiB aligned to its END (the first chunks of a short block are empty); lane = chunk, slicing-by-4 table
// CRC from LDS tables, then a 6-level tree R(A||B) = shift_|B|(R(A)) ^ R(B) with precomputed GF(2) operators for
// "append 2^k zero bytes" (crc_mat[k][32]).  The standard CRC is ~(R0(data) ^ shift_L(0xffffffff)).
struct CrcArgs {
    const uint8_t *raw;             // inflated stream
    const uint8_t *file;            // compressed file (the stored CRC follows each payload)
    const uint64_t *coff, *uoff;
    const uint32_t *csize, *isize;
    const uint32_t *mat;            // [17][32]: operator for 2^k zero bytes, k = 0..16
    uint32_t n_blocks;
    uint32_t *err;
    uint32_t *out;                  // non-null: the CRCs are stored here and nothing is compared (the deflate side, mth_deflate.hip)
};
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t *__restrict__ m, uint32_t v) {
    uint32_t s = 0;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) s ^= ((v >> i) & 1u) ? m[i] : 0u;
    return s;
}
__global__ __launch_bounds__(64) void k_crc32(const CrcArgs a) {
    __shared__ uint32_t tab[4][256];          // slicing-by-4: tab[j][b] = CRC of byte b followed by j zero bytes
    __shared__ uint32_t smat[17 * 32];
    const uint32_t blk = blockIdx.x;
    if (blk >= a.n_blocks) return;
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        tab[0][i] = c;
    }
    for (int i = lane; i < 17 * 32; i += 64) smat[i] = a.mat[i];
    __syncthreads();
    for (int i = lane; i < 256; i += 64) {
        const uint32_t c1 = (tab[0][i] >> 8) ^ tab[0][tab[0][i] & 0xffu];
        const uint32_t c2 = (c1 >> 8) ^ tab[0][c1 & 0xffu];
        tab[1][i] = c1; tab[2][i] = c2; tab[3][i] = (c2 >> 8) ^ tab[0][c2 & 0xffu];
    }
    __syncthreads();
    const uint32_t L = a.isize[blk];
    const uint8_t *p = a.raw + a.uoff[blk];
    const int64_t beg = (int64_t)L - (int64_t)(64 - lane) * 1024;
    uint32_t c = 0;
    int64_t i = beg < 0 ? 0 : beg;
    const int64_t end = beg + 1024;                          // <= 0 for the empty leading chunks of a short block
    for (; i < end && ((end - i) & 3); ++i) c = tab[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    auto step4 = [&](uint32_t w) {                          // four bytes: four independent lookups
        c ^= w;
        c = tab[3][c & 0xffu] ^ tab[2][(c >> 8) & 0xffu] ^ tab[1][(c >> 16) & 0xffu] ^ tab[0][c >> 24];
    };
    // sixteen bytes per load: the lanes of a wave read 64 different cache lines (their chunks lie 1 KiB apart) and 28 waves
    // per CU do not fit L1, so every load is an L2 round trip -- a quarter as many of them
    typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
    for (; i + 16 <= end; i += 16) {
        const u32x4_a1 w = *reinterpret_cast<const u32x4_a1 *>(p + i);
        step4(w.x); step4(w.y); step4(w.z); step4(w.w);
    }
    for (; i < end; i += 4) {
        uint32_t w;
        __builtin_memcpy(&w, p + i, 4);
        step4(w);
    }
    // tree: at level k lanes are grouped in runs of 2^(k+1); the left half's CRC is shifted by the right half's length
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t other = (uint32_t)__shfl_xor((int)c, 1 << k, 64);
        const bool right = (lane >> k) & 1;                      // this lane holds the right half of its pair
        const uint32_t left_crc = right ? other : c, right_crc = right ? c : other;
        c = gf2_apply(smat + (10 + k) * 32, left_crc) ^ right_crc;   // right half is 1024 << k bytes long
    }
    if (lane == 0) {
        uint32_t init = 0xffffffffu;                              // shift_L(0xffffffff): binary decomposition of L
        for (int k = 0; k < 17; ++k) if ((L >> k) & 1u) init = gf2_apply(smat + k * 32, init);
        const uint32_t crc = ~(c ^ init);
        if (a.out) { a.out[blk] = crc; return; }
        uint32_t want;
        __builtin_memcpy(&want, a.file + a.coff[blk] + a.csize[blk], 4);
        if (crc != want) atomicOr(a.err, (uint32_t)ERRB_CRC);
    }
}

// ---- per-block record walk ------------------------------------------------------------------------------
struct WalkBArgs {
    const uint8_t *raw;            // inflated stream
    const uint64_t *uoff;          // per block: offset of its bytes in raw
    const uint32_t *isize;
    uint32_t n_blocks;
    uint64_t first_byte;           // records start here (end of the BAM header)
    uint32_t *cnt;                 // pass 1: records per block
    const unsigned long long *base;   // pass 2: exclusive scan of cnt
    uint64_t *rec_off;             // pass 2: record offsets (+ closing offset written by the last block)
    uint64_t total_bytes;
    uint32_t *err;
};
template <bool FILL>
__global__ __launch_bounds__(256) void k_block_walk(const WalkBArgs a) {
    const uint32_t blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.n_blocks) return;
    const uint64_t b0 = a.uoff[blk], b1 = b0 + a.isize[blk];
    uint32_t n = 0;
    if (b1 > a.first_byte) {
        uint64_t p = b0 < a.first_byte ? a.first_byte : b0;
        unsigned long long w = FILL ? a.base[blk] : 0ull;
        while (p + 4 <= b1) {
            uint32_t bs;
            __builtin_memcpy(&bs, a.raw + p, 4);
            if (bs < 32 || p + 4 + (uint64_t)bs > b1) break;
            if (FILL) a.rec_off[w++] = p;
            ++n;
            p += 4 + (uint64_t)bs;
        }
        if (p != b1) atomicOr(a.err, (uint32_t)ERRB_UNALIGNED);      // a record straddles the block (or garbage)
    }
    if (!FILL) a.cnt[blk] = n;
    if (FILL && blk == a.n_blocks - 1) a.rec_off[a.base[blk] + n] = a.total_bytes;
}

// ---- record walk for records that straddle blocks: speculation, then exact verification ------------------------------
// (mth_bgzf_decode_straddle; the formulation is described at the top of the file)
constexpr uint64_t STR_NONE = ~0ull;          // entry of a block without a guess: equal to no exit
constexpr uint64_t STR_PAST = 1ull << 62;     // exit of a walk that cannot go on (no readable, sane block_size): past every block

// mismatch / first_bad: blocks that do not enter where their predecessor left, and the first of them (k_straddle_check);
// tail: where the unfinished (or bogus) record starts, else the stream's end
// broken: blocks of a scan from a guess that do not continue their predecessor's chain (k_straddle_keys)
struct StrState { uint32_t mismatch, first_bad, repaired, broken; unsigned long long tail; };
struct StrArgs {
    const uint8_t *raw;            // the call's stream: the carry, then the inflated blocks
    const uint64_t *uoff;          // per block: offset of its bytes in raw (block 0 also owns the carry in front of it)
    const uint32_t *isize;
    uint32_t n_blocks;
    uint64_t first_byte, total;    // records start at first_byte; raw holds total bytes
    const uint64_t *entry_in, *exit_in;      // the generation a launch reads ...
    const uint32_t *cnt_in;
    uint64_t *entry_out, *exit_out;          // ... and the one it writes
    uint32_t *cnt_out;
    StrState *st;
    const unsigned long long *base;          // fill: exclusive scan of the final counts
    uint64_t *rec_off;                       // fill: record offsets + the closing offset
    int last;                                // fill: the stream ends here and may not end inside a record (MTH_STRADDLE_LAST)
    uint32_t *err;
    // mth_bgzf_straddle_scan (n_blocks = the run's blocks; raw / total also hold the look-ahead behind them):
    int scan;                                // a record whose block_size is readable and leads past the stream leaves at that offset, not STR_PAST
    int guess_first;                         // block 0 guesses like every other block and is its own reference (str_want)
    mth_straddle_row_t *rows;                // k_straddle_keys: one row per block of the run
};
__device__ __forceinline__ uint32_t str_ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
// do the 36 bytes at p look like the fixed part of a BAM record (SAM spec 4.2)?  next = where its block_size leads.
// Bounded by the stream length before anything is loaded: p is any offset at all.
__device__ __forceinline__ bool str_plausible(const uint8_t *raw, uint64_t p, uint64_t total, uint64_t &next) {
    if (p + 36 > total) return false;
    const int32_t bs = (int32_t)str_ld32(raw + p), ref = (int32_t)str_ld32(raw + p + 4), pos = (int32_t)str_ld32(raw + p + 8);
    const int64_t l_name = str_ld32(raw + p + 12) & 0xffu, n_cigar = str_ld32(raw + p + 16) & 0xffffu;
    const int32_t l_seq = (int32_t)str_ld32(raw + p + 20), next_ref = (int32_t)str_ld32(raw + p + 24), next_pos = (int32_t)str_ld32(raw + p + 28);
    next = p + 4 + (uint64_t)(uint32_t)bs;
    return bs >= 32 && ref >= -1 && next_ref >= -1 && pos >= -1 && next_pos >= -1 && l_name >= 1 && l_seq >= 0 &&
           32 + l_name + 4 * n_cigar + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq <= (int64_t)bs;
}
// one wave per block: the lanes test 64 consecutive offsets at a time; the first that passes, and whose record leads to another
// offset that passes or exactly to the stream's end, is the block's guess.  (A block_size that leads PAST the stream is not
// taken: among sequence and quality bytes one offset in a few dozen passes the field tests with a block_size of hundreds of
// megabytes.  The record a call's stream ends inside therefore is nobody's guess; the block it starts in is repaired if it
// holds no earlier start.)
__global__ __launch_bounds__(256) void k_straddle_guess(const StrArgs a) {
    const uint32_t blk = uni(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (blk == 0 && lane == 0) a.st->tail = a.total;
    if (blk >= a.n_blocks) return;
    const uint64_t b0 = blk ? uni64(a.uoff[blk]) : 0ull, b1 = uni64(a.uoff[blk]) + uni(a.isize[blk]);
    uint64_t g = STR_NONE;
    if (b0 <= a.first_byte && !a.guess_first) {
        g = a.first_byte;                        // the records start in (or after) this block: no guess needed
    } else {
        for (uint64_t q = b0; q < b1; q += 64) {
            const uint64_t p = q + lane;
            uint64_t nx = 0, nx2;
            bool ok = p < b1 && str_plausible(a.raw, p, a.total, nx);
            if (ok && nx != a.total) ok = nx < a.total && str_plausible(a.raw, nx, a.total, nx2);
            const unsigned long long m = __ballot(ok);
            if (m) { g = q + (uint64_t)(__ffsll((long long)m) - 1); break; }
        }
    }
    if (lane == 0) a.entry_out[blk] = g;
}
// the records that START in [entry, b1), following block_size; a record may end in a later block.  Returns where the chain
// leaves the block: the next block's entry.  FILL (the final pass) writes the offsets and is the only one to raise an error.
template <bool FILL>
__device__ __forceinline__ uint64_t str_walk(const StrArgs &a, uint32_t blk, uint64_t entry, uint64_t b1, uint32_t &n) {
    n = 0;
    if (entry == STR_NONE) return STR_PAST;
    uint64_t p = entry;
    unsigned long long w = FILL ? a.base[blk] : 0ull;
    while (p < b1) {
        bool cut = p + 4 > a.total, bogus = false;         // cut: the stream ends inside this record
        uint32_t bs = 0;
        if (!cut) {
            bs = str_ld32(a.raw + p);
            bogus = (int32_t)bs < 32;
            cut = !bogus && p + 4 + (uint64_t)bs > a.total;
        }
        if (!FILL && a.scan && cut && p + 4 <= a.total) { ++n; return p + 4 + (uint64_t)bs; }   // ends in blocks the caller did not pass: a value
        if (cut || bogus) {
            if (FILL) {
                if (bogus || a.last) atomicOr(a.err, (uint32_t)ERRB_FORMAT);
                a.st->tail = p;                              // (one block at most gets here: no record starts behind this one)
                a.rec_off[w] = p;                            // the closing offset: the end of the last whole record
            }
            return STR_PAST;
        }
        if (FILL) a.rec_off[w++] = p;
        ++n;
        p += 4 + (uint64_t)bs;
    }
    return p;
}
template <bool FILL>
__global__ __launch_bounds__(256) void k_straddle_walk(const StrArgs a) {
    const uint32_t blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.n_blocks) return;
    const uint64_t b1 = a.uoff[blk] + a.isize[blk];
    uint32_t n;
    const uint64_t x = str_walk<FILL>(a, blk, a.entry_in[blk], b1, n);
    if (!FILL) { a.exit_out[blk] = x; a.cnt_out[blk] = n; }
    if (FILL && blk == a.n_blocks - 1 && x == a.total) a.rec_off[a.base[blk] + n] = a.total;    // the chain ends with the stream: the closing offset
}
// A round.  k_straddle_check counts the blocks that do not enter where their predecessor left (none: the offsets are final) and
// finds the first of them: every block before it is final, so its own new entry is certain.  k_straddle_repair then walks again
// that block, and every other such block whose predecessor agrees with ITS predecessor -- from a predecessor that is itself about
// to change, a wrong entry would only move on, one block per round, with the correction chasing it.  A predecessor can agree and
// still be wrong (two guesses on one chain of decoys); walking from a wrong offset nearly always ends on an unreadable block_size,
// so an exit that says "cannot go on" is believed only of the block whose predecessors are final.
// A scan from a guess has no block whose entry is certain: block 0 has no reference but itself, and what a chain head says about the
// blocks behind it is believed only as far as the NEXT block.  A block whose predecessor found no guess, or left at or past this
// block's end (STR_PAST; a block_size read at a wrong offset -- the look-alike 4 bytes before a record start of profiles/
// straddle_walk.md leads 5.5 MB on, and block after block would take that exit over its own good guess, one per round; or a record
// that does cover the block), keeps its own guess: the chain breaks there and a new one starts.  k_straddle_keys counts the breaks;
// a run with one is scanned again from its true entry, where the first block in doubt IS certain and a record over k blocks costs
// its k rounds.
__device__ __forceinline__ bool str_breaks(const StrArgs &a, uint32_t blk) {
    return a.guess_first && blk && (a.entry_in[blk - 1] == STR_NONE || a.exit_in[blk - 1] >= a.uoff[blk] + a.isize[blk]);
}
__device__ __forceinline__ uint64_t str_want(const StrArgs &a, uint32_t blk) {
    if (a.guess_first && (blk == 0 || str_breaks(a, blk))) return a.entry_in[blk];
    return blk ? a.exit_in[blk - 1] : a.first_byte;
}
__global__ __launch_bounds__(256) void k_straddle_check(const StrArgs a) {
    const uint32_t blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.n_blocks || a.entry_in[blk] == str_want(a, blk)) return;
    atomicAdd(&a.st->mismatch, 1u);
    atomicMin(&a.st->first_bad, blk);
}
__global__ __launch_bounds__(256) void k_straddle_repair(const StrArgs a) {
    const uint32_t blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.n_blocks) return;
    uint64_t entry = a.entry_in[blk], x = a.exit_in[blk];
    uint32_t n = a.cnt_in[blk];
    const uint64_t want = str_want(a, blk);
    if (entry != want) {
        const bool pred_agrees = blk == 0 || a.entry_in[blk - 1] == str_want(a, blk - 1);
        // (want <= total: an exit past the stream -- STR_PAST, or under `scan` where a block_size read at a wrong offset leads -- is
        // believed only of the first block in doubt)
        if (blk == a.st->first_bad || (pred_agrees && want <= a.total)) {
            entry = want;
            x = str_walk<false>(a, blk, entry, a.uoff[blk] + a.isize[blk], n);
            atomicAdd(&a.st->repaired, 1u);
        }
    }
    a.entry_out[blk] = entry; a.exit_out[blk] = x; a.cnt_out[blk] = n;
}
// mth_bgzf_straddle_scan: the settled chain as one row per block -- a thread per block reads refID and pos of the first record that
// starts in it from the contiguous stream (the 12 bytes may lie across the block's end: the look-ahead holds them)
__global__ __launch_bounds__(256) void k_straddle_keys(const StrArgs a) {
    const uint32_t blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.n_blocks) return;
    const uint64_t b0 = a.uoff[blk], b1 = b0 + a.isize[blk], e = a.entry_in[blk], x = a.exit_in[blk];
    mth_straddle_row_t r;
    r.start = MTH_STRADDLE_NO_START; r.ref_id = r.pos = INT32_MIN; r.pad_ = 0;
    if (e != STR_NONE && e >= b0 && e < b1) {
        r.start = (uint32_t)(e - b0);
        if (e + 12 <= a.total) { r.ref_id = (int32_t)str_ld32(a.raw + e + 4); r.pos = (int32_t)str_ld32(a.raw + e + 8); }
    }
    r.exit = (x >= STR_PAST || x < b1) ? MTH_STRADDLE_EXIT_BAD : x - b1;
    a.rows[blk] = r;
    if (str_breaks(a, blk)) atomicAdd(&a.st->broken, 1u);
}

}  // namespace mth

using namespace mth;

// GF(2) operators for appending 2^k zero bytes to a raw CRC-32 (zlib's crc32_combine construction)
static void crc_zero_operators(uint32_t (*mat)[32]) {
    auto times = [](const uint32_t *m, uint32_t v) { uint32_t s = 0; for (int i = 0; v; v >>= 1, ++i) if (v & 1u) s ^= m[i]; return s; };
    uint32_t bit[32], t[32];
    bit[0] = 0xedb88320u;                               // one zero BIT
    for (int n = 1; n < 32; ++n) bit[n] = 1u << (n - 1);
    auto square = [&](uint32_t *dst, const uint32_t *src) { for (int n = 0; n < 32; ++n) dst[n] = times(src, src[n]); };
    square(t, bit); square(bit, t); square(t, bit);     // 2, 4, 8 bits: t = one zero byte
    for (int n = 0; n < 32; ++n) mat[0][n] = t[n];
    for (int k = 1; k < 17; ++k) square(mat[k], mat[k - 1]);
}

// (Splitting a pageable host-to-device copy over 4 / 8 host threads that enqueue slices into the same stream was measured:
// no gain at 4, slower at 8 -- profiles/r02_e2e.md.)
namespace mth {

// the zero-byte operators of k_crc32 into the context, once
static int crc_operators(mth_ctx *ctx) {
    if (ctx->crc_mat.p) return MTH_OK;
    hipStream_t s = ctx->stream;
    uint32_t mat[17][32];
    crc_zero_operators(mat);
    MTH_HIP(ctx, ctx->crc_mat.reserve(sizeof mat, s));
    MTH_HIP(ctx, hipMemcpyAsync(ctx->crc_mat.p, mat, sizeof mat, hipMemcpyHostToDevice, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));            // mat is a local
    return MTH_OK;
}

// CRC-32 of n_blocks device-resident blocks (block b: isize[b] <= 65536 bytes at raw + uoff[b]) into out[b]: k_crc32 without a
// trailer to compare with
int crc32_blocks(mth_ctx *ctx, const uint8_t *raw, const uint64_t *d_uoff, const uint32_t *d_isize, uint32_t n_blocks, uint32_t *d_out) {
    { const int rc = crc_operators(ctx); if (rc) return rc; }
    CrcArgs ca{};
    ca.raw = raw; ca.uoff = d_uoff; ca.isize = d_isize; ca.mat = ctx->crc_mat.as<uint32_t>(); ca.n_blocks = n_blocks;
    ca.err = &ctx->d_state->err; ca.out = d_out;
    LaunchTimer lt(ctx, K_CRC);
    hipLaunchKernelGGL(k_crc32, dim3(n_blocks), dim3(64), 0, ctx->stream, ca);
    return MTH_OK;
}

int stage_take(mth_ctx *ctx, const void *file, uint64_t n_bytes, bool &staged) {
    hipStream_t s = ctx->stream;
    // the helper thread of the previous call (copying THIS call's bytes, if they were announced) has to be done first
    if (ctx->stage_thread.joinable()) {
        ctx->stage_thread.join();
        if (ctx->stage_rc != MTH_OK) return fail(ctx, MTH_ERR_HIP, "staging the next chunk's file bytes failed");
    }
    staged = ctx->staged_src && ctx->staged_src == file && ctx->staged_bytes == n_bytes;
    if (ctx->staged_src && !staged) ctx->load_stats.stage_misses += 1;      // copied, and this call came with another pointer or size
    if (staged) {
        // copied on the side stream while the previous chunk was in flight: take that buffer
        std::swap(ctx->inf_file, ctx->inf_file2);
        MTH_HIP(ctx, hipStreamWaitEvent(s, ctx->staged_ev, 0));
    } else {
        MTH_HIP(ctx, ctx->inf_file.reserve((size_t)n_bytes + INF_FILE_PAD, s));
    }
    ctx->staged_src = nullptr;
    return MTH_OK;
}

int stage_start_next(mth_ctx *ctx) {
    // the chunk announced by mth_bgzf_stage: its bytes travel on the side stream, from a helper thread (a pageable copy
    // blocks its caller), while this call's kernels run.  The thread owns inf_file2 / copy_stream / staged_* until joined.
    if (ctx->next_src && ctx->next_bytes) {
        if (!ctx->copy_stream) {
            MTH_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
            MTH_HIP(ctx, hipEventCreateWithFlags(&ctx->staged_ev, hipEventDisableTiming));
        }
        const void *src = ctx->next_src;
        const uint64_t nbytes = ctx->next_bytes;
        ctx->next_src = nullptr;
        ctx->stage_rc = MTH_OK;
        ctx->stage_thread = std::thread([ctx, src, nbytes] {
            auto ok = [&](hipError_t e) { if (e != hipSuccess) ctx->stage_rc = MTH_ERR_HIP; return e == hipSuccess; };
            if (!ok(hipSetDevice(ctx->device))) return;
            if (!ok(ctx->inf_file2.reserve((size_t)nbytes + INF_FILE_PAD, ctx->copy_stream))) return;
            if (!ok(hipMemcpyAsync(ctx->inf_file2.p, src, (size_t)nbytes, hipMemcpyHostToDevice, ctx->copy_stream))) return;
            if (!ok(hipMemsetAsync(static_cast<uint8_t *>(ctx->inf_file2.p) + nbytes, 0, INF_FILE_PAD, ctx->copy_stream))) return;
            if (!ok(hipEventRecord(ctx->staged_ev, ctx->copy_stream))) return;
            ctx->staged_src = src; ctx->staged_bytes = nbytes;
        });
    }
    return MTH_OK;
}

// stage the file bytes + block table and launch the inflate; on return d_uoff / d_isize point at the device table
// (the blocks' output starts at stream_base in inf_raw; total includes it)
int inflate_blocks(mth_ctx *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                   const uint32_t *isize, uint64_t n_blocks, uint64_t &total, uint64_t *&d_uoff, uint32_t *&d_isize, uint64_t stream_base) {
    if (n_blocks >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "too many BGZF blocks in one call: split the file");
    MTH_ENTER(ctx);
    ctx->scan_valid = false;                  // inf_raw / inf_tab are this call's now
    hipStream_t s = ctx->stream;
    const size_t nb = (size_t)n_blocks;
    // output offsets of the blocks + validation of the table against the byte range given
    std::vector<uint64_t> uoff(nb + 1, 0);
    uoff[0] = stream_base;                    // (mth_bgzf_decode_straddle: the carry comes first in the stream)
    for (size_t i = 0; i < nb; ++i) {
        if (coff[i] + (uint64_t)csize[i] > n_bytes || isize[i] > 65536u) return fail(ctx, MTH_ERR_INVALID, "BGZF block table does not fit the file bytes");
        uoff[i + 1] = uoff[i] + isize[i];
    }
    total = uoff[nb];
    // stage: compressed bytes (padded: the bit reader loads whole words), the table, the inflated stream
    bool staged = false;
    { const int rc = stage_take(ctx, file, n_bytes, staged); if (rc) return rc; }
    MTH_HIP(ctx, ctx->inf_tab.reserve(nb * 24 + 64, s));
    MTH_HIP(ctx, ctx->inf_raw.reserve((size_t)total + 64, s));
    // METHEOR_COPY_PIECE_MB=k (default 0 = off): an in-line copy (the first chunk of a file, or every chunk under METHEOR_NO_STAGE)
    // of two pieces or more travels on its own stream piece by piece, and the blocks of a piece are inflated as soon as the piece
    // has landed.  Built to hide the first chunk's inflate behind its copy; measured slower (profiles/r02_e2e.md, last section):
    // a pageable copy pins, moves and unpins inside the call, ~2.5 ms of that per call is not overlapped with anything, and the
    // runtime pipelines one large copy better than the caller can pipeline several small ones.  Kept as a switch, parity-tested
    // (tests/test_gpu_chunked_load.py: bytes, and the launch count against a restatement of the rule below).
    static const size_t piece_bytes = [] { const char *e = getenv("METHEOR_COPY_PIECE_MB"); const long k = e ? atol(e) : 0; return k > 0 ? (size_t)k << 20 : (size_t)0; }();
    const bool pieced = !staged && piece_bytes && n_bytes >= 2 * (uint64_t)piece_bytes && nb >= 2;
    (staged ? ctx->load_stats.staged_calls : pieced ? ctx->load_stats.pieced_calls : ctx->load_stats.inline_calls) += 1;
    if (!staged && !pieced) {
        // (copying through own page-locked pieces from 2-8 worker threads was measured: no faster than the runtime's pageable path,
        // profiles/r02_e2e.md -- the page-cache reads bound both)
        if (n_bytes) MTH_HIP(ctx, hipMemcpyAsync(ctx->inf_file.p, file, (size_t)n_bytes, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemsetAsync(static_cast<uint8_t *>(ctx->inf_file.p) + n_bytes, 0, INF_FILE_PAD, s));
    }
    // (before the inflate is launched: allocating it afterwards synchronised with the inflate and delayed the first CRC launch by ~7 ms)
    { const int rc = crc_operators(ctx); if (rc) return rc; }
    { const int rc = stage_start_next(ctx); if (rc) return rc; }
    uint8_t *tab = static_cast<uint8_t *>(ctx->inf_tab.p);
    uint64_t *d_coff = reinterpret_cast<uint64_t *>(tab);
    d_uoff = reinterpret_cast<uint64_t *>(tab + nb * 8);
    uint32_t *d_csize = reinterpret_cast<uint32_t *>(tab + nb * 16);
    d_isize = reinterpret_cast<uint32_t *>(tab + nb * 20);
    if (nb) {
        MTH_HIP(ctx, hipMemcpyAsync(d_coff, coff, nb * 8, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(d_uoff, uoff.data(), nb * 8, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(d_csize, csize, nb * 4, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(d_isize, isize, nb * 4, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipStreamSynchronize(s));            // uoff is a local
        InflArgs ia{};
        ia.file = ctx->inf_file.as<uint8_t>(); ia.coff = d_coff; ia.csize = d_csize; ia.isize = d_isize; ia.uoff = d_uoff;
        ia.n_blocks = (uint32_t)nb; ia.out = ctx->inf_raw.as<uint8_t>(); ia.err = &ctx->d_state->err;
        { static const int fast = [] { const char *e = getenv("METHEOR_INFLATE_ASM"); return e ? atoi(e) : 1; }(); ia.fast_literals = fast; }
        auto launch = [&](size_t b0, size_t b1) {       // blocks [b0, b1): absolute output offsets, so a launch is any run of blocks
            InflArgs x = ia;
            x.coff = d_coff + b0; x.csize = d_csize + b0; x.isize = d_isize + b0; x.uoff = d_uoff + b0; x.n_blocks = (uint32_t)(b1 - b0);
            LaunchTimer lt(ctx, K_INFLATE);
            hipLaunchKernelGGL(k_inflate, dim3(x.n_blocks), dim3(64), 0, s, x);
        };
        if (pieced) {
            if (!ctx->piece_stream) MTH_HIP(ctx, hipStreamCreateWithFlags(&ctx->piece_stream, hipStreamNonBlocking));
            auto event = [&](size_t k) -> hipError_t {
                while (ctx->piece_ev.size() <= k) {
                    hipEvent_t e = nullptr;
                    const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
                    if (rc != hipSuccess) return rc;
                    ctx->piece_ev.push_back(e);
                }
                return hipSuccess;
            };
            // whatever the compute stream still runs on the old contents of the buffer comes first
            MTH_HIP(ctx, event(0));
            MTH_HIP(ctx, hipEventRecord(ctx->piece_ev[0], s));
            MTH_HIP(ctx, hipStreamWaitEvent(ctx->piece_stream, ctx->piece_ev[0], 0));
            uint8_t *const dst = static_cast<uint8_t *>(ctx->inf_file.p);
            const uint8_t *const src = static_cast<const uint8_t *>(file);
            size_t off = 0, bl = 0, k = 1;
            while (off < (size_t)n_bytes) {
                size_t len = std::min(piece_bytes, (size_t)n_bytes - off);
                if ((size_t)n_bytes - off - len < piece_bytes / 2) len = (size_t)n_bytes - off;     // no stub piece at the end
                MTH_HIP(ctx, hipMemcpyAsync(dst + off, src + off, len, hipMemcpyHostToDevice, ctx->piece_stream));
                off += len;
                const bool last = off == (size_t)n_bytes;
                if (last) MTH_HIP(ctx, hipMemsetAsync(dst + n_bytes, 0, INF_FILE_PAD, ctx->piece_stream));
                MTH_HIP(ctx, event(k));
                MTH_HIP(ctx, hipEventRecord(ctx->piece_ev[k], ctx->piece_stream));
                MTH_HIP(ctx, hipStreamWaitEvent(s, ctx->piece_ev[k], 0));
                ++k;
                // the blocks whose payload -- and the 64 bytes the bit reader may load past it -- have arrived
                size_t b1 = bl;
                while (b1 < nb && (last || coff[b1] + (uint64_t)csize[b1] + 64u <= (uint64_t)off)) ++b1;
                if (b1 > bl) { launch(bl, b1); ctx->load_stats.pieced_launches += 1; }
                bl = b1;
            }
        } else {
            launch(0, nb);
        }
        // CRC32 of every inflated block against the gzip trailer (the 4 bytes after the payload)
        for (size_t i = 0; i < nb; ++i)
            if (coff[i] + (uint64_t)csize[i] + 4 > n_bytes) return fail(ctx, MTH_ERR_INVALID, "BGZF block table: the CRC trailer of a block lies outside the file bytes");
        CrcArgs ca{};
        ca.raw = ctx->inf_raw.as<uint8_t>(); ca.file = ctx->inf_file.as<uint8_t>(); ca.coff = d_coff; ca.uoff = d_uoff;
        ca.csize = d_csize; ca.isize = d_isize; ca.mat = ctx->crc_mat.as<uint32_t>(); ca.n_blocks = (uint32_t)nb; ca.err = &ctx->d_state->err;
        LaunchTimer lt(ctx, K_CRC);
        hipLaunchKernelGGL(k_crc32, dim3((uint32_t)nb), dim3(64), 0, s, ca);
    }
    return MTH_OK;
}

}  // namespace mth

// per block, two generations of (entry, exit, count) behind the state words: a round reads one and writes the other
struct StrLinks { StrState *st; uint64_t *entry[2], *exit_[2]; uint32_t *cnt[2]; };
static int straddle_links(mth_ctx *ctx, size_t nb, StrLinks &k) {
    const size_t gen = nb * 8;
    MTH_HIP(ctx, ctx->inf_links.reserve(64 + 4 * gen + 2 * nb * 4 + 16, ctx->stream));
    uint8_t *const lk = static_cast<uint8_t *>(ctx->inf_links.p);
    k.st = reinterpret_cast<StrState *>(lk);
    k.entry[0] = reinterpret_cast<uint64_t *>(lk + 64); k.entry[1] = reinterpret_cast<uint64_t *>(lk + 64 + gen);
    k.exit_[0] = reinterpret_cast<uint64_t *>(lk + 64 + 2 * gen); k.exit_[1] = reinterpret_cast<uint64_t *>(lk + 64 + 3 * gen);
    k.cnt[0] = reinterpret_cast<uint32_t *>(lk + 64 + 4 * gen); k.cnt[1] = reinterpret_cast<uint32_t *>(lk + 64 + 4 * gen + nb * 4);
    return MTH_OK;
}
// rounds: separate launches, the host reads one mismatch counter per round; generation `cur` is final when nothing mismatches
// (settled), else the round bound was reached
static int straddle_rounds(mth_ctx *ctx, StrArgs &a, const StrLinks &k, int &cur, uint32_t &rounds, bool &settled) {
    hipStream_t s = ctx->stream;
    const dim3 per_thread((a.n_blocks + 255) / 256);
    rounds = 0;
    settled = false;
    for (;;) {
        const uint32_t none[2] = {0u, 0xffffffffu};                  // mismatch, first_bad
        MTH_HIP(ctx, hipMemcpyAsync(k.st, none, sizeof none, hipMemcpyHostToDevice, s));
        a.entry_in = k.entry[cur]; a.exit_in = k.exit_[cur]; a.cnt_in = k.cnt[cur];
        a.entry_out = k.entry[cur ^ 1]; a.exit_out = k.exit_[cur ^ 1]; a.cnt_out = k.cnt[cur ^ 1];
        { LaunchTimer lt(ctx, K_STR_REPAIR); hipLaunchKernelGGL(k_straddle_check, per_thread, dim3(256), 0, s, a); }
        uint32_t mismatch = 0;
        MTH_HIP(ctx, hipMemcpyAsync(&mismatch, &k.st->mismatch, 4, hipMemcpyDeviceToHost, s));
        MTH_HIP(ctx, hipStreamSynchronize(s));
        if (mismatch == 0) { settled = true; break; }
        if (rounds == MTH_STRADDLE_MAX_ROUNDS) break;
        { LaunchTimer lt(ctx, K_STR_REPAIR); hipLaunchKernelGGL(k_straddle_repair, per_thread, dim3(256), 0, s, a); }
        cur ^= 1;
        ++rounds;
    }
    return MTH_OK;
}
static const char *const kNotSettled = "the record offsets did not settle within the round bound (records far longer than a BGZF block, or data that looks like record headers): use the host walk";

// the rounds of a scan from the state the context holds, then the rows and the run's summary
static int straddle_scan_finish(mth_ctx *ctx, uint64_t first_byte, int guess_first, mth_straddle_row_t *rows, mth_straddle_run_t *run, mth_straddle_info_t *info) {
    hipStream_t s = ctx->stream;
    const size_t nb = ctx->scan_n_run;
    StrLinks k;
    int rc = straddle_links(ctx, nb, k);
    if (rc) return rc;
    StrArgs a{};
    a.raw = ctx->inf_raw.as<uint8_t>(); a.uoff = ctx->scan_uoff; a.isize = ctx->scan_isize; a.n_blocks = (uint32_t)nb;
    a.first_byte = first_byte; a.total = ctx->scan_total; a.st = k.st; a.err = &ctx->d_state->err;
    a.scan = 1; a.guess_first = guess_first;
    uint32_t rounds = 0;
    bool settled = false;
    if ((rc = straddle_rounds(ctx, a, k, ctx->scan_cur, rounds, settled))) return rc;
    StrState hs{};
    if ((rc = sync_and_check(ctx))) return rc;              // a corrupt block
    if (!settled) {
        MTH_HIP(ctx, hipMemcpy(&hs, k.st, sizeof hs, hipMemcpyDeviceToHost));
        if (info) { info->rounds = rounds; info->repaired_blocks = hs.repaired; }
        ctx->scan_valid = false;
        return fail(ctx, MTH_ERR_UNALIGNED, kNotSettled);
    }
    MTH_HIP(ctx, ctx->inf_base.reserve(nb * sizeof(mth_straddle_row_t) + 16, s));
    a.entry_in = k.entry[ctx->scan_cur]; a.exit_in = k.exit_[ctx->scan_cur];
    a.rows = ctx->inf_base.as<mth_straddle_row_t>();
    { LaunchTimer lt(ctx, K_STR_WALK); hipLaunchKernelGGL(k_straddle_keys, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, a); }
    uint64_t e0 = 0;
    MTH_HIP(ctx, hipMemcpyAsync(rows, a.rows, nb * sizeof(mth_straddle_row_t), hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipMemcpyAsync(&e0, a.entry_in, 8, hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipMemcpyAsync(&hs, k.st, sizeof hs, hipMemcpyDeviceToHost, s));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    if (info) { info->rounds = rounds; info->repaired_blocks = hs.repaired; }
    if (run) {
        // a chain that breaks inside the run says nothing past the break: no entry to hold the true one against
        run->entry = (e0 == STR_NONE || hs.broken) ? MTH_STRADDLE_ENTRY_GUESS : e0;
        run->exit = rows[nb - 1].exit;                      // past the last block of the run = past the run
    }
    return MTH_OK;
}

extern "C" {

int mth_bgzf_straddle_scan(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                           const uint32_t *isize, uint64_t n_blocks, uint64_t n_run, uint64_t entry, mth_straddle_row_t *rows,
                           mth_straddle_run_t *run, mth_straddle_info_t *info) {
    if (!ctx || !rows || !file || !coff || !csize || !isize || n_run == 0 || n_run > n_blocks) return MTH_ERR_INVALID;
    if (info) *info = mth_straddle_info_t{0, 0, 0};
    ctx->carry_bytes = 0;                     // the stream of a scan is its own
    uint64_t total = 0, *d_uoff = nullptr;
    uint32_t *d_isize = nullptr;
    int rc = inflate_blocks(ctx, file, n_bytes, coff, csize, isize, n_blocks, total, d_uoff, d_isize);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const size_t nb = (size_t)n_run;
    ctx->scan_n_run = n_run; ctx->scan_total = total; ctx->scan_uoff = d_uoff; ctx->scan_isize = d_isize; ctx->scan_cur = 0;
    StrLinks k;
    if ((rc = straddle_links(ctx, nb, k))) return rc;
    MTH_HIP(ctx, hipMemsetAsync(k.st, 0, sizeof(StrState), s));
    const bool guess = entry == MTH_STRADDLE_ENTRY_GUESS;
    StrArgs a{};
    a.raw = ctx->inf_raw.as<uint8_t>(); a.uoff = d_uoff; a.isize = d_isize; a.n_blocks = (uint32_t)nb;
    a.first_byte = guess ? 0 : entry; a.total = total; a.st = k.st; a.err = &ctx->d_state->err;
    a.scan = 1; a.guess_first = guess ? 1 : 0;
    a.entry_out = k.entry[0];
    { LaunchTimer lt(ctx, K_STR_GUESS); hipLaunchKernelGGL(k_straddle_guess, dim3((uint32_t)((nb + 3) / 4)), dim3(256), 0, s, a); }
    a.entry_in = k.entry[0]; a.exit_out = k.exit_[0]; a.cnt_out = k.cnt[0];
    { LaunchTimer lt(ctx, K_STR_WALK); hipLaunchKernelGGL((k_straddle_walk<false>), dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, a); }
    ctx->scan_valid = true;
    return straddle_scan_finish(ctx, a.first_byte, a.guess_first, rows, run, info);
}

int mth_bgzf_straddle_rescan(mth_ctx_t *ctx, uint64_t entry, mth_straddle_row_t *rows, mth_straddle_run_t *run, mth_straddle_info_t *info) {
    if (!ctx || !rows || entry == MTH_STRADDLE_ENTRY_GUESS) return MTH_ERR_INVALID;
    if (info) *info = mth_straddle_info_t{0, 0, 0};
    if (!ctx->scan_valid) return fail(ctx, MTH_ERR_INVALID, "mth_bgzf_straddle_rescan: the context holds no scan (another load call came in between)");
    MTH_ENTER(ctx);
    StrLinks k;
    int rc = straddle_links(ctx, (size_t)ctx->scan_n_run, k);
    if (rc) return rc;
    MTH_HIP(ctx, hipMemsetAsync(k.st, 0, sizeof(StrState), ctx->stream));
    return straddle_scan_finish(ctx, entry, 0, rows, run, info);
}

int mth_bgzf_stage(mth_ctx_t *ctx, const void *file, uint64_t n_bytes) {
    if (!ctx || (n_bytes && !file)) return MTH_ERR_INVALID;
    ctx->next_src = n_bytes ? file : nullptr;
    ctx->next_bytes = n_bytes;
    return MTH_OK;
}

int mth_load_stats(mth_ctx_t *ctx, mth_load_stats_t *out) {
    if (!ctx || !out) return MTH_ERR_INVALID;
    *out = ctx->load_stats;
    return MTH_OK;
}

int mth_bgzf_inflate(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                     const uint32_t *isize, uint64_t n_blocks, void *dst_host, uint64_t *n_out) {
    if (!ctx || (n_blocks && (!file || !coff || !csize || !isize))) return MTH_ERR_INVALID;
    uint64_t total = 0, *d_uoff = nullptr;
    uint32_t *d_isize = nullptr;
    int rc = inflate_blocks(ctx, file, n_bytes, coff, csize, isize, n_blocks, total, d_uoff, d_isize);
    if (rc) return rc;
    if ((rc = sync_and_check(ctx))) return rc;
    if (n_out) *n_out = total;
    if (dst_host && total) MTH_HIP(ctx, hipMemcpy(dst_host, ctx->inf_raw.p, (size_t)total, hipMemcpyDeviceToHost));
    return MTH_OK;
}

int mth_bgzf_decode(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                    const uint32_t *isize, uint64_t n_blocks, uint64_t first_byte, int append, mth_decoded_t *out) {
    if (!ctx || !out || (n_blocks && (!file || !coff || !csize || !isize))) return MTH_ERR_INVALID;
    uint64_t total = 0, *d_uoff = nullptr;
    uint32_t *d_isize = nullptr;
    int rc0 = inflate_blocks(ctx, file, n_bytes, coff, csize, isize, n_blocks, total, d_uoff, d_isize);
    if (rc0) return rc0;
    if (first_byte > total) return fail(ctx, MTH_ERR_INVALID, "first_byte beyond the inflated stream");
    hipStream_t s = ctx->stream;
    const size_t nb = (size_t)n_blocks;
    uint64_t n_rec = 0;
    if (nb) {
        // record offsets: count per block -> scan -> fill (verifying that no record straddles a block)
        MTH_HIP(ctx, ctx->inf_cnt.reserve(nb * 4 + 16, s));
        MTH_HIP(ctx, ctx->inf_base.reserve((nb + 1) * 8 + 16, s));
        WalkBArgs wa{};
        wa.raw = ctx->inf_raw.as<uint8_t>(); wa.uoff = d_uoff; wa.isize = d_isize; wa.n_blocks = (uint32_t)nb;
        wa.first_byte = first_byte; wa.cnt = ctx->inf_cnt.as<uint32_t>(); wa.total_bytes = total; wa.err = &ctx->d_state->err;
        hipLaunchKernelGGL((k_block_walk<false>), dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, wa);
        unsigned long long tot_rec = 0;
        int rc = scan_u32_to_u64(ctx, wa.cnt, (uint32_t)nb, 0ull, ctx->inf_base.as<unsigned long long>(), &tot_rec);
        if (rc) return rc;                       // (synchronises: inflate / walk errors surface here)
        n_rec = tot_rec;
        MTH_HIP(ctx, ctx->inf_recoff.reserve((size_t)(n_rec + 1) * 8 + 16, s));
        wa.base = ctx->inf_base.as<unsigned long long>(); wa.rec_off = ctx->inf_recoff.as<uint64_t>();
        hipLaunchKernelGGL((k_block_walk<true>), dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, s, wa);
    }
    return decode_core(ctx, ctx->inf_raw.as<uint8_t>(), ctx->inf_recoff.as<uint64_t>(), n_rec, append, out);
}

int mth_bgzf_decode_straddle(mth_ctx_t *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                             const uint32_t *isize, uint64_t n_blocks, uint64_t first_byte, unsigned flags, mth_decoded_t *out,
                             mth_straddle_info_t *info) {
    if (!ctx || !out || (n_blocks && (!file || !coff || !csize || !isize))) return MTH_ERR_INVALID;
    const unsigned ends = flags & (MTH_STRADDLE_LAST | MTH_STRADDLE_DROP_TAIL);
    if ((flags & ~(MTH_STRADDLE_APPEND | MTH_STRADDLE_LAST | MTH_STRADDLE_DROP_TAIL)) || ends == (MTH_STRADDLE_LAST | MTH_STRADDLE_DROP_TAIL))
        return fail(ctx, MTH_ERR_INVALID, "mth_bgzf_decode_straddle: flags");
    if (info) *info = mth_straddle_info_t{0, 0, 0};
    const int append = (flags & MTH_STRADDLE_APPEND) ? 1 : 0;
    if (!append) ctx->carry_bytes = 0;
    const uint64_t carry = ctx->carry_bytes;
    if (carry && first_byte) return fail(ctx, MTH_ERR_INVALID, "first_byte must be 0 while a record of the previous call is carried");
    ctx->carry_bytes = 0;                     // consumed by this call, whatever becomes of it
    uint64_t total = 0, *d_uoff = nullptr;
    uint32_t *d_isize = nullptr;
    int rc = inflate_blocks(ctx, file, n_bytes, coff, csize, isize, n_blocks, total, d_uoff, d_isize, carry);
    if (rc) return rc;
    if (first_byte > total) return fail(ctx, MTH_ERR_INVALID, "first_byte beyond the inflated stream");
    hipStream_t s = ctx->stream;
    // the carry was copied aside at the end of the previous call: inf_raw may have been reallocated since
    if (carry) MTH_HIP(ctx, hipMemcpyAsync(ctx->inf_raw.p, ctx->inf_carry.p, (size_t)carry, hipMemcpyDeviceToDevice, s));
    const size_t nb = (size_t)n_blocks;
    uint64_t n_rec = 0, tail = total;
    if (nb == 0) {
        tail = 0;                             // nothing but the carry: still unfinished
        if (carry && (flags & MTH_STRADDLE_LAST)) return fail(ctx, MTH_ERR_FORMAT, "the BAM stream ends inside a record");
    } else {
        StrLinks k;
        if ((rc = straddle_links(ctx, nb, k))) return rc;
        MTH_HIP(ctx, ctx->inf_base.reserve((nb + 1) * 8 + 16, s));
        StrState *const st = k.st;
        uint64_t *const *const entry = k.entry;
        uint32_t *const *const cnt = k.cnt;
        MTH_HIP(ctx, hipMemsetAsync(st, 0, sizeof(StrState), s));
        StrArgs a{};
        a.raw = ctx->inf_raw.as<uint8_t>(); a.uoff = d_uoff; a.isize = d_isize; a.n_blocks = (uint32_t)nb;
        a.first_byte = first_byte; a.total = total; a.st = st; a.err = &ctx->d_state->err;
        const dim3 per_thread((uint32_t)((nb + 255) / 256));
        a.entry_out = entry[0];
        { LaunchTimer lt(ctx, K_STR_GUESS); hipLaunchKernelGGL(k_straddle_guess, dim3((uint32_t)((nb + 3) / 4)), dim3(256), 0, s, a); }
        a.entry_in = entry[0]; a.exit_out = k.exit_[0]; a.cnt_out = cnt[0];
        { LaunchTimer lt(ctx, K_STR_WALK); hipLaunchKernelGGL((k_straddle_walk<false>), per_thread, dim3(256), 0, s, a); }
        int cur = 0;
        uint32_t rounds = 0;
        bool settled = false;
        if ((rc = straddle_rounds(ctx, a, k, cur, rounds, settled))) return rc;
        StrState hs{};
        if (!settled) {
            if ((rc = sync_and_check(ctx))) return rc;      // a corrupt block explains it better
            MTH_HIP(ctx, hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
            if (info) { info->rounds = MTH_STRADDLE_MAX_ROUNDS; info->repaired_blocks = hs.repaired; }
            return fail(ctx, MTH_ERR_UNALIGNED, kNotSettled);
        }
        unsigned long long tot_rec = 0;
        rc = scan_u32_to_u64(ctx, cnt[cur], (uint32_t)nb, 0ull, ctx->inf_base.as<unsigned long long>(), &tot_rec);
        if (rc) return rc;                       // (synchronises: inflate errors surface here)
        n_rec = tot_rec;
        if (n_rec >= (1ull << 32) - 16) return fail(ctx, MTH_ERR_CAPACITY, "more than 2^32 records in one decode call: split the stream");
        MTH_HIP(ctx, ctx->inf_recoff.reserve((size_t)(n_rec + 1) * 8 + 16, s));
        a.entry_in = entry[cur]; a.base = ctx->inf_base.as<unsigned long long>(); a.rec_off = ctx->inf_recoff.as<uint64_t>();
        a.last = (flags & MTH_STRADDLE_LAST) ? 1 : 0;
        { LaunchTimer lt(ctx, K_STR_WALK); hipLaunchKernelGGL((k_straddle_walk<true>), per_thread, dim3(256), 0, s, a); }
        if ((rc = sync_and_check(ctx))) return rc;          // block_size < 32, or a finished stream that ends inside a record
        MTH_HIP(ctx, hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
        tail = hs.tail;
        if (info) { info->rounds = rounds; info->repaired_blocks = hs.repaired; }
    }
    if (!ends && tail < total) {
        // the unfinished record comes first in the next call's stream: copied aside now, inf_raw is that call's to reuse
        const uint64_t keep = total - tail;
        if (keep > MTH_STRADDLE_MAX_CARRY) return fail(ctx, MTH_ERR_UNALIGNED, "a record left unfinished by this call is larger than the carry buffer: use the host walk");
        if (nb) {                                 // (nb == 0: the carry is where it was)
            MTH_HIP(ctx, ctx->inf_carry.reserve((size_t)keep, s));
            MTH_HIP(ctx, hipMemcpyAsync(ctx->inf_carry.p, ctx->inf_raw.as<uint8_t>() + tail, (size_t)keep, hipMemcpyDeviceToDevice, s));
        }
        ctx->carry_bytes = keep;
        if (info) info->carry_bytes = keep;
    }
    return decode_core(ctx, ctx->inf_raw.as<uint8_t>(), ctx->inf_recoff.as<uint64_t>(), n_rec, append, out);
}

}  // extern "C"
