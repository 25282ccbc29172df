// mth_bai.hip -- the BAM index (.bai, SAM spec 5.2) of a record stream, built on the device (gfx950).
//
// `tag -O bam --write-index`: at the end of a window the tagged records, every record's offset in the stream, the block cuts and
// the compressed size of every block are in HBM (mth_tag.hip, mth_deflate.hip).  That is everything an index is made of, so it is
// built there, beside the data; what comes back at the end is the finished tables (a few MB for a human genome), never a record.
//
// Per window (bai_window), one thread per record:
//   k_bai_keys   refID / pos / flag / the CIGAR's reference length from the record's bytes -> end, bin (reg2bin), the virtual offsets
//                of its first byte and of the byte after its last (binary search of its stream offsets in the cuts), the checks
//                (sorted, inside the contig, inside what a .bai can address), the linear index (64-bit atomicMin over the 16-kbp
//                windows it touches) and the per-contig metadata (first / last offset, mapped / unmapped counts, highest window).
//                A lane leaves out what the lane before it covers (same contig, an earlier offset), and a wave whose records lie on
//                one contig reduces the metadata with shuffles first: one thread's worth of atomics per wave, not 64.
//   k_bai_heads  a record is a run head where (refID, bin) differs from its predecessor's (record 0: the last record of the window
//                before, kept in the device state)
//   scan         of the head flags (scan_u32_to_u64): every run's row
//   k_bai_rows   heads write (refID << 32 | bin, vbeg), the last record of a run writes vend; a window whose first record is no head
//                extends the last row of the window before.  Rows are appended to buffers that grow by doubling.
// At the end (mth_bai_finish): the rows sorted by refID << 32 | bin (rocPRIM's radix sort through hipCUB -- stable, so a bin keeps
// its chunks in file order), bin boundaries and counts (flags -> scan -> k_bai_bins / k_bai_bin_counts), and the linear table
// forward-filled per contig (k_bai_fill: a workgroup per contig, inclusive max-scan with 0 for "untouched").
// Min, max and integer add are the only atomics, the sort is stable on rows appended in file order: the result is a function of
// the input alone.  Not the hot path of anything: streaming, latency-bound kernels, no MFMA.
#include <hipcub/hipcub.hpp>

#include "mth_ctx.h"

namespace mth {

constexpr unsigned long long BAI_NONE = ~0ull;
constexpr long long BAI_MAX_END = 1ll << 29;           // what a .bai's bins and 16-kbp windows can address
// what a record can be refused for (the error word is ordinal << 3 | code, smallest wins)
enum : uint32_t { BAI_E_FORMAT = 1, BAI_E_REFID, BAI_E_UNSORTED, BAI_E_NEGPOS, BAI_E_CSI, BAI_E_LN };

// device state of the index under construction.  prev_*[2]: the last record of the window before, two generations (a window reads
// one and writes the other: no thread reads what another one of the same launch writes)
struct BaiState {
    unsigned long long err;            // BAI_NONE: none
    unsigned long long n_no_coor;
    unsigned long long prev_key[2];    // refID << 32 | bin, BAI_NONE for a record without a row (and before the first record)
    unsigned long long prev_sort[2];   // its place in coordinate order (bai_sort_key), 0 before the first record
    unsigned long long tail_at_end;    // it ended exactly where the blocks given so far end
};

struct BaiArgs {
    const uint8_t *raw;
    const unsigned long long *off;     // n_rec + 1
    uint32_t n_rec;
    unsigned long long rec_base;       // ordinal of record 0
    const unsigned long long *cut;     // n_blocks + 1 stream offsets
    const unsigned long long *coff;    // n_blocks file offsets, each + coff_base
    unsigned long long coff_base;
    uint32_t n_blocks;
    int32_t n_refs;
    const unsigned long long *lin_off; // n_refs + 1
    const long long *ref_len;          // n_refs
    unsigned long long *lin, *meta;    // meta: 4 words per contig
    uint32_t *n_intv;
    BaiState *st;
    int par;                           // generation of prev_* to read
    unsigned long long *key, *vb, *ve; // per record
    uint32_t *flag;
    const unsigned long long *rank;    // exclusive scan of flag
    unsigned long long *r_key, *r_vb, *r_ve;
    unsigned long long row_base, row_cap;
};

__device__ __forceinline__ uint32_t bai_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// coordinate order as one unsigned number: contigs ascending, positions ascending inside one, records without a contig last
__device__ __forceinline__ unsigned long long bai_sort_key(int32_t ref, int32_t pos) {
    if (ref < 0) return 0xffffffff00000000ull;
    return ((unsigned long long)(uint32_t)ref << 32) | ((uint32_t)pos ^ 0x80000000u);
}

// SAM spec 5.3, [beg, end) with end > beg
__device__ __forceinline__ uint32_t bai_reg2bin(long long beg, long long end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0u;
}

// the last block that starts at or before stream offset x (n_blocks for x at or past the end of the stream)
__device__ __forceinline__ uint32_t bai_block_of(const unsigned long long *cut, uint32_t n_blocks, unsigned long long x) {
    uint32_t lo = 0, hi = n_blocks + 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cut[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;                                                 // cut[0] == 0 <= x
}

__device__ __forceinline__ unsigned long long bai_shfl_xor64(unsigned long long v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k_bai_init(BaiState *st, unsigned long long *meta, uint32_t *n_intv, int32_t n_refs) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        st->err = BAI_NONE; st->n_no_coor = 0; st->prev_key[0] = st->prev_key[1] = BAI_NONE;
        st->prev_sort[0] = st->prev_sort[1] = 0; st->tail_at_end = 0;
    }
    if (t < (uint32_t)n_refs) { meta[4ull * t] = BAI_NONE; meta[4ull * t + 1] = 0; meta[4ull * t + 2] = 0; meta[4ull * t + 3] = 0; n_intv[t] = 0; }
}

// every thread of the block runs to the end (the shuffles want whole waves); ok = the record takes part in the index
__global__ __launch_bounds__(256) void k_bai_keys(const BaiArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = i < a.n_rec;
    uint32_t code = 0;
    int32_t ref = -1, pos = 0;
    uint32_t flag = 0;
    long long end = 1;
    unsigned long long o0 = 0, o1 = 0;
    if (live) {
        o0 = a.off[i]; o1 = a.off[i + 1];
        bool bad = o1 < o0 + 36ull || o1 > a.cut[a.n_blocks];
        uint64_t reflen = 0;
        if (!bad) {
            const uint8_t *p = a.raw + o0;
            bad = (unsigned long long)bai_u32(p) + 4ull != o1 - o0;
            ref = (int32_t)bai_u32(p + 4); pos = (int32_t)bai_u32(p + 8);
            const uint32_t l_read_name = p[12], n_cigar = p[16] | ((uint32_t)p[17] << 8);
            flag = p[18] | ((uint32_t)p[19] << 8);
            const unsigned long long o_cigar = 36ull + l_read_name;
            if (!bad && o_cigar + 4ull * n_cigar > o1 - o0) bad = true;
            if (!bad)
                for (uint32_t k = 0; k < n_cigar; ++k) {
                    const uint32_t c = bai_u32(p + o_cigar + 4ull * k), op = c & 15u;
                    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) reflen += c >> 4;        // M D N = X
                }
        }
        end = (long long)pos + (long long)(reflen ? reflen : 1);
        // the record before: its refID and pos are all the order needs
        unsigned long long before = a.st->prev_sort[a.par];
        if (i > 0 && !bad) {
            const unsigned long long q0 = a.off[i - 1];
            before = (q0 < o0 && o0 - q0 >= 12ull) ? bai_sort_key((int32_t)bai_u32(a.raw + q0 + 4), (int32_t)bai_u32(a.raw + q0 + 8)) : 0ull;
        }
        if (bad) { code = BAI_E_FORMAT; ref = -1; }
        else if (ref >= a.n_refs) code = BAI_E_REFID;
        else if (bai_sort_key(ref, pos) < before) code = BAI_E_UNSORTED;
        else if (ref >= 0) {
            if (pos < 0) code = BAI_E_NEGPOS;
            else if (end > BAI_MAX_END) code = BAI_E_CSI;
            else if (end > a.ref_len[ref]) code = BAI_E_LN;
        }
        if (code) atomicMin(&a.st->err, ((a.rec_base + i) << 3) | code);
        if (i == a.n_rec - 1) {
            a.st->prev_sort[a.par ^ 1] = bad ? 0ull : bai_sort_key(ref, pos);
            a.st->tail_at_end = (o1 == a.cut[a.n_blocks]) ? 1ull : 0ull;
        }
    }
    const bool ok = live && code == 0 && ref >= 0;
    unsigned long long key = BAI_NONE, vb = 0, ve = 0;
    uint32_t w0 = 0, w1 = 0;
    if (ok) {
        key = ((unsigned long long)(uint32_t)ref << 32) | bai_reg2bin(pos, end);
        w0 = (uint32_t)(pos >> 14); w1 = (uint32_t)((end - 1) >> 14);
        uint32_t b = bai_block_of(a.cut, a.n_blocks, o0);                        // < n_blocks: o0 < o1 <= cut[n_blocks]
        vb = ((a.coff_base + a.coff[b]) << 16) | (o0 - a.cut[b]);
        // a record that ends exactly at the end of a block keeps that block, as bgzf_tell does after reading it
        b = bai_block_of(a.cut, a.n_blocks, o1);
        if (o1 == a.cut[b] && b > 0) --b;
        ve = ((a.coff_base + a.coff[b]) << 16) | (o1 - a.cut[b]);
    }
    if (live) {
        a.key[i] = key; a.vb[i] = vb; a.ve[i] = ve;
        if (i == a.n_rec - 1) a.st->prev_key[a.par ^ 1] = key;
    }
    // records without a contig: counted, one atomic per wave
    {
        const unsigned long long m = __ballot(live && code == 0 && ref < 0);
        if (m && lane == (uint32_t)__builtin_ctzll(m)) atomicAdd(&a.st->n_no_coor, (unsigned long long)__builtin_popcountll(m));
    }
    // linear index: the smallest vbeg per window.  The lane before holds an earlier record: a window it touches on the same contig
    // already gets a smaller offset from it
    {
        const int p_ok = __shfl_up((int)ok, 1, 64), p_ref = __shfl_up(ref, 1, 64);
        const uint32_t p_w0 = (uint32_t)__shfl_up((int)w0, 1, 64), p_w1 = (uint32_t)__shfl_up((int)w1, 1, 64);
        if (ok) {
            const bool cover = lane > 0 && p_ok && p_ref == ref;
            unsigned long long *row = a.lin + a.lin_off[ref];
            for (uint32_t w = w0; w <= w1; ++w) {
                if (cover && w >= p_w0 && w <= p_w1) continue;
                atomicMin(row + w, vb);
            }
        }
    }
    // metadata of the contig: a wave on one contig (nearly all of them) reduces first
    const unsigned long long m_ok = __ballot(ok);
    if (m_ok) {
        const int first = __builtin_ctzll(m_ok);
        const int32_t r0 = __shfl(ref, first, 64);
        const bool same = __ballot(ok && ref == r0) == m_ok;
        unsigned long long lo = ok ? vb : BAI_NONE, hi = ok ? ve : 0ull;
        unsigned long long n_map = (ok && !(flag & 4u)) ? 1ull : 0ull, n_un = (ok && (flag & 4u)) ? 1ull : 0ull;
        uint32_t top = ok ? w1 + 1u : 0u;
        if (same) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long l2 = bai_shfl_xor64(lo, o), h2 = bai_shfl_xor64(hi, o);
                lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
                n_map += bai_shfl_xor64(n_map, o); n_un += bai_shfl_xor64(n_un, o);
                const uint32_t t2 = (uint32_t)__shfl_xor((int)top, o, 64);
                top = t2 > top ? t2 : top;
            }
        }
        if (same ? (int)lane == first : ok) {
            unsigned long long *mt = a.meta + 4ull * (uint32_t)ref;
            atomicMin(mt, lo); atomicMax(mt + 1, hi);
            if (n_map) atomicAdd(mt + 2, n_map);
            if (n_un) atomicAdd(mt + 3, n_un);
            atomicMax(a.n_intv + ref, top);
        }
    }
}

__global__ __launch_bounds__(256) void k_bai_heads(const BaiArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const unsigned long long k = a.key[i], before = i ? a.key[i - 1] : a.st->prev_key[a.par];
    a.flag[i] = (k != BAI_NONE && k != before) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bai_rows(const BaiArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rec) return;
    const unsigned long long k = a.key[i];
    if (k == BAI_NONE) return;
    const uint32_t head = a.flag[i];
    // the row of the run the record belongs to: the latest one opened at or before it (row_base - 1 = the last row of the window before)
    const unsigned long long row = a.row_base + a.rank[i] + head - 1ull;
    if (row >= a.row_cap) return;                                  // (also row_base == 0 without a head: cannot happen, never written)
    if (head) { a.r_key[row] = k; a.r_vb[row] = a.vb[i]; }
    if (i == a.n_rec - 1 || a.key[i + 1] != k) a.r_ve[row] = a.ve[i];
}

// an empty block follows the last record (the EOF block): bgzf_tell after that record names it, and so does the index
__global__ void k_bai_tail(BaiState *st, int par, unsigned long long *r_ve, unsigned long long n_rows, unsigned long long *meta, unsigned long long coff) {
    if (threadIdx.x || blockIdx.x) return;
    const unsigned long long k = st->prev_key[par];
    if (st->err != BAI_NONE || !st->tail_at_end || k == BAI_NONE || n_rows == 0) return;
    r_ve[n_rows - 1] = coff << 16;
    atomicMax(meta + 4ull * (k >> 32) + 1, coff << 16);
    st->tail_at_end = 0;
}

__global__ __launch_bounds__(256) void k_bai_iota(uint32_t *idx, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = i;
}

// the rows in (refID, bin) order: their offsets through the permutation, and where a bin begins
__global__ __launch_bounds__(256) void k_bai_gather(const unsigned long long *skey, const uint32_t *perm, uint32_t n, const unsigned long long *r_vb,
                                                    const unsigned long long *r_ve, unsigned long long *cb, unsigned long long *ce, uint32_t *flag) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = perm[j];
    cb[j] = r_vb[p]; ce[j] = r_ve[p];
    flag[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bai_bins(const unsigned long long *skey, const uint32_t *flag, const unsigned long long *rank, uint32_t n,
                                                  unsigned long long *bin_key, uint32_t *bin_start, uint32_t *ref_nbin) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !flag[j]) return;
    const unsigned long long r = rank[j], k = skey[j];
    bin_key[r] = k; bin_start[r] = j;
    atomicAdd(ref_nbin + (k >> 32), 1u);
}

__global__ __launch_bounds__(256) void k_bai_bin_counts(const uint32_t *bin_start, uint32_t n_bins, uint32_t n_rows, uint32_t *bin_cnt) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_bins) return;
    bin_cnt[r] = (r + 1 < n_bins ? bin_start[r + 1] : n_rows) - bin_start[r];
}

// a workgroup per contig: entry w <- the latest touched entry at or before w, 0 before the first (on sorted input the touched
// entries ascend, so "the latest" is the largest: an inclusive max-scan with 0 for an untouched window)
__global__ __launch_bounds__(256) void k_bai_fill(unsigned long long *lin, const unsigned long long *lin_off, const uint32_t *n_intv) {
    __shared__ unsigned long long ws[4];
    const uint32_t ref = blockIdx.x, n = n_intv[ref], lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long *row = lin + lin_off[ref];
    unsigned long long carry = 0;
    for (uint32_t w0 = 0; w0 < n; w0 += 256) {
        const uint32_t w = w0 + threadIdx.x;
        unsigned long long v = (w < n) ? row[w] : 0ull;
        if (v == BAI_NONE) v = 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
            const unsigned long long u = ((unsigned long long)hi << 32) | lo;
            if (lane >= (uint32_t)o && u > v) v = u;
        }
        if (lane == 63) ws[wave] = v;
        __syncthreads();
        unsigned long long pre = carry;
        for (uint32_t k = 0; k < wave; ++k) pre = ws[k] > pre ? ws[k] : pre;
        if (pre > v) v = pre;
        if (w < n) row[w] = v;
        unsigned long long all = carry;
        for (uint32_t k = 0; k < 4; ++k) all = ws[k] > all ? ws[k] : all;
        carry = all;
        __syncthreads();                                            // ws is rewritten by the next trip
    }
}

void bai_release(mth_ctx *ctx) {
    BaiBuild &b = ctx->bai;
    for (DevBuf *d : {&b.state, &b.lin, &b.tab, &b.meta, &b.n_intv, &b.key, &b.vb, &b.ve, &b.flag, &b.rank, &b.r_key, &b.r_vb, &b.r_ve, &b.cut,
                      &b.skey, &b.idx, &b.perm, &b.tmp, &b.cb, &b.ce, &b.bin_key, &b.bin_start, &b.bin_cnt, &b.ref_nbin})
        d->release();
}

static const char *bai_reason(uint32_t code) {
    switch (code) {
        case BAI_E_FORMAT: return "is malformed (block_size / field lengths inconsistent) or leaves the blocks given";
        case BAI_E_REFID: return "names a reference the header does not have (refID >= n_ref)";
        case BAI_E_UNSORTED: return "comes before its predecessor in coordinate order: the input is not coordinate-sorted and cannot be indexed";
        case BAI_E_NEGPOS: return "is placed on a reference at a negative position";
        case BAI_E_CSI: return "ends beyond position 2^29, the limit of the .bai format: a .csi index would be needed, and none is written";
        default: return "ends beyond the end of its reference (the header's LN)";
    }
}

// one window of the index: n records of the device-resident stream d_raw at d_off, cut into n_blocks blocks at the device-resident
// stream offsets d_cut, block b at file offset coff_base + d_coff[b].  Synchronises.  The first error is kept (b.err / b.err_msg).
int bai_window(mth_ctx *ctx, const uint8_t *d_raw, const unsigned long long *d_off, uint32_t n, const unsigned long long *d_cut,
               const unsigned long long *d_coff, unsigned long long coff_base, uint32_t n_blocks) {
    BaiBuild &b = ctx->bai;
    hipStream_t s = ctx->stream;
    if (b.err) return fail(ctx, b.err, b.err_msg.c_str());
    if (n == 0) return MTH_OK;
    const uint32_t nb = (n + 255) / 256;
    MTH_HIP(ctx, b.key.reserve((size_t)n * 8 + 16, s)); MTH_HIP(ctx, b.vb.reserve((size_t)n * 8 + 16, s)); MTH_HIP(ctx, b.ve.reserve((size_t)n * 8 + 16, s));
    MTH_HIP(ctx, b.flag.reserve((size_t)n * 4 + 16, s)); MTH_HIP(ctx, b.rank.reserve(((size_t)n + 1) * 8 + 16, s));
    BaiArgs a{};
    a.raw = d_raw; a.off = d_off; a.n_rec = n; a.rec_base = b.n_records; a.cut = d_cut; a.coff = d_coff; a.coff_base = coff_base; a.n_blocks = n_blocks;
    a.n_refs = b.n_refs; a.lin_off = b.tab.as<unsigned long long>(); a.ref_len = reinterpret_cast<const long long *>(b.tab.as<unsigned long long>() + b.n_refs + 1);
    a.lin = b.lin.as<unsigned long long>(); a.meta = b.meta.as<unsigned long long>(); a.n_intv = b.n_intv.as<uint32_t>();
    a.st = b.state.as<BaiState>(); a.par = b.par;
    a.key = b.key.as<unsigned long long>(); a.vb = b.vb.as<unsigned long long>(); a.ve = b.ve.as<unsigned long long>(); a.flag = b.flag.as<uint32_t>();
    {
        LaunchTimer lt(ctx, K_BAI_KEYS);
        hipLaunchKernelGGL(k_bai_keys, dim3(nb), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_bai_heads, dim3(nb), dim3(256), 0, s, a);
    MTH_HIP(ctx, hipGetLastError());
    MTH_HIP(ctx, hipMemcpyAsync(ctx->h_words, b.state.p, 8, hipMemcpyDeviceToHost, s));
    unsigned long long heads = 0;
    {
        const int rc = scan_u32_to_u64(ctx, a.flag, n, 0ull, b.rank.as<unsigned long long>(), &heads);   // synchronises
        if (rc) { b.err = rc; b.err_msg = ctx->last_error; return rc; }
    }
    b.par ^= 1;
    const unsigned long long e = ctx->h_words[0];
    if (e != BAI_NONE) {
        const uint32_t code = (uint32_t)(e & 7u);
        b.err = code == BAI_E_FORMAT ? MTH_ERR_FORMAT : code == BAI_E_UNSORTED ? MTH_ERR_UNSORTED : MTH_ERR_RANGE;
        b.err_msg = "index: record " + std::to_string(e >> 3) + " (counted from 0) " + bai_reason(code);
        return fail(ctx, b.err, b.err_msg.c_str());
    }
    const uint64_t need = b.n_rows + heads;
    if (need >= (1ull << 31)) { b.err = MTH_ERR_CAPACITY; b.err_msg = "index: more than 2^31 chunks"; return fail(ctx, b.err, b.err_msg.c_str()); }
    if (need > b.row_cap) {
        const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(b.row_cap * 2, 1024));
        for (DevBuf *d : {&b.r_key, &b.r_vb, &b.r_ve}) MTH_HIP(ctx, d->reserve((size_t)cap * 8, s, b.n_rows > 0, (size_t)b.n_rows * 8));
        b.row_cap = cap;
    }
    a.rank = b.rank.as<unsigned long long>();
    a.r_key = b.r_key.as<unsigned long long>(); a.r_vb = b.r_vb.as<unsigned long long>(); a.r_ve = b.r_ve.as<unsigned long long>();
    a.row_base = b.n_rows; a.row_cap = b.row_cap;
    {
        LaunchTimer lt(ctx, K_BAI_ROWS);
        hipLaunchKernelGGL(k_bai_rows, dim3(nb), dim3(256), 0, s, a);
    }
    MTH_HIP(ctx, hipGetLastError());
    b.n_rows = need;
    b.n_records += n;
    return MTH_OK;
}

}  // namespace mth

using namespace mth;

extern "C" {

int mth_bai_begin(mth_ctx_t *ctx, int32_t n_refs, const int64_t *ref_len, uint64_t file_off) {
    if (!ctx || n_refs < 0 || (n_refs && !ref_len)) return MTH_ERR_INVALID;
    MTH_ENTER(ctx);
    hipStream_t s = ctx->stream;
    BaiBuild &b = ctx->bai;
    b.on = false; b.err = 0; b.err_msg.clear();
    b.n_refs = n_refs; b.file_off = file_off; b.n_records = 0; b.n_rows = 0; b.par = 0;
    // the linear table: ceil(LN / 16384) entries per contig, as far as a .bai reaches
    b.h_lin_off.assign((size_t)n_refs + 1, 0);
    std::vector<unsigned long long> tab(2 * (size_t)n_refs + 1, 0);
    for (int32_t t = 0; t < n_refs; ++t) {
        if (ref_len[t] < 0) return fail(ctx, MTH_ERR_INVALID, "mth_bai_begin: negative reference length");
        const uint64_t ln = (uint64_t)std::min<int64_t>(ref_len[t], BAI_MAX_END);
        b.h_lin_off[(size_t)t + 1] = b.h_lin_off[(size_t)t] + (ln + 16383) / 16384;
        tab[(size_t)n_refs + 1 + (size_t)t] = (unsigned long long)ref_len[t];
    }
    for (int32_t t = 0; t <= n_refs; ++t) tab[(size_t)t] = b.h_lin_off[(size_t)t];
    const size_t n_lin = (size_t)b.h_lin_off[(size_t)n_refs];
    MTH_HIP(ctx, b.state.reserve(sizeof(BaiState), s));
    MTH_HIP(ctx, b.tab.reserve(tab.size() * 8, s));
    MTH_HIP(ctx, b.lin.reserve(n_lin * 8 + 16, s));
    MTH_HIP(ctx, b.meta.reserve((size_t)n_refs * 32 + 16, s));
    MTH_HIP(ctx, b.n_intv.reserve((size_t)n_refs * 4 + 16, s));
    MTH_HIP(ctx, hipMemcpyAsync(b.tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    if (n_lin) MTH_HIP(ctx, hipMemsetAsync(b.lin.p, 0xff, n_lin * 8, s));
    hipLaunchKernelGGL(k_bai_init, dim3((uint32_t)(n_refs / 256 + 1)), dim3(256), 0, s, b.state.as<BaiState>(), b.meta.as<unsigned long long>(),
                       b.n_intv.as<uint32_t>(), n_refs);
    MTH_HIP(ctx, hipGetLastError());
    MTH_HIP(ctx, hipStreamSynchronize(s));                      // `tab` goes away
    b.on = true;
    return MTH_OK;
}

int mth_bai_add_records(mth_ctx_t *ctx, const void *raw, const uint64_t *rec_off, uint64_t n_rec, int mem, const uint64_t *cut_off,
                        const uint64_t *block_coff, uint64_t n_blocks) {
    if (!ctx || (n_rec && (!raw || !rec_off || !n_blocks)) || (n_blocks && (!cut_off || !block_coff))) return MTH_ERR_INVALID;
    if (mem != MTH_MEM_HOST && mem != MTH_MEM_DEVICE) return fail(ctx, MTH_ERR_INVALID, "mem");
    BaiBuild &b = ctx->bai;
    if (!b.on) return fail(ctx, MTH_ERR_STATE, "mth_bai_begin has not been called");
    if (n_rec >= (1ull << 32) - 16 || n_blocks >= (1ull << 31)) return fail(ctx, MTH_ERR_CAPACITY, "more than 2^32 records or 2^31 blocks in one index call: split the stream");
    MTH_ENTER(ctx);
    if (b.err) return fail(ctx, b.err, b.err_msg.c_str());
    if (n_blocks == 0) return MTH_OK;
    hipStream_t s = ctx->stream;
    if (cut_off[0] != 0) return fail(ctx, MTH_ERR_INVALID, "index: the block cuts must start at 0");
    for (uint64_t k = 0; k < n_blocks; ++k) {
        if (cut_off[k + 1] < cut_off[k] || cut_off[k + 1] - cut_off[k] > 0xffffull) return fail(ctx, MTH_ERR_INVALID, "index: block cuts must ascend in steps a 16-bit in-block offset can address");
        if (block_coff[k] >= (1ull << 48)) return fail(ctx, MTH_ERR_INVALID, "index: a block's file offset does not fit the 48 bits of a virtual offset");
    }
    if (n_rec == 0) {
        // blocks without records behind the stream: only an empty one matters (the EOF block)
        if (cut_off[n_blocks] != 0 || b.n_rows == 0) return MTH_OK;
        hipLaunchKernelGGL(k_bai_tail, dim3(1), dim3(64), 0, s, b.state.as<BaiState>(), b.par, b.r_ve.as<unsigned long long>(), (unsigned long long)b.n_rows,
                           b.meta.as<unsigned long long>(), (unsigned long long)block_coff[n_blocks - 1]);
        MTH_HIP(ctx, hipGetLastError());
        return MTH_OK;
    }
    // cuts, then file offsets, in one table
    std::vector<unsigned long long> tab(2 * (size_t)n_blocks + 1);
    for (uint64_t k = 0; k <= n_blocks; ++k) tab[(size_t)k] = cut_off[k];
    for (uint64_t k = 0; k < n_blocks; ++k) tab[(size_t)(n_blocks + 1 + k)] = block_coff[k];
    MTH_HIP(ctx, b.cut.reserve(tab.size() * 8, s));
    MTH_HIP(ctx, hipMemcpyAsync(b.cut.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const uint8_t *d_raw = static_cast<const uint8_t *>(raw);
    const unsigned long long *d_off = reinterpret_cast<const unsigned long long *>(rec_off);
    if (mem == MTH_MEM_HOST) {
        const uint64_t n_bytes = rec_off[n_rec];
        for (uint64_t k = 0; k < n_rec; ++k)
            if (rec_off[k + 1] < rec_off[k]) return fail(ctx, MTH_ERR_INVALID, "index: record offsets must ascend");
        MTH_HIP(ctx, ctx->dec_raw.reserve(n_bytes + 16, s));
        MTH_HIP(ctx, ctx->dec_recoff.reserve((n_rec + 1) * 8, s));
        if (n_bytes) MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_raw.p, raw, n_bytes, hipMemcpyHostToDevice, s));
        MTH_HIP(ctx, hipMemcpyAsync(ctx->dec_recoff.p, rec_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, s));
        d_raw = ctx->dec_raw.as<uint8_t>(); d_off = ctx->dec_recoff.as<unsigned long long>();
    }
    // (the window's synchronisation comes before `tab` goes away)
    return bai_window(ctx, d_raw, d_off, (uint32_t)n_rec, b.cut.as<unsigned long long>(), b.cut.as<unsigned long long>() + n_blocks + 1, 0ull, (uint32_t)n_blocks);
}

int mth_bai_finish(mth_ctx_t *ctx, mth_bai_out_t *out) {
    if (!ctx || !out) return MTH_ERR_INVALID;
    BaiBuild &b = ctx->bai;
    *out = mth_bai_out_t{};
    if (!b.on) return fail(ctx, MTH_ERR_STATE, "mth_bai_begin has not been called");
    b.on = false;
    MTH_ENTER(ctx);
    if (b.err) return fail(ctx, b.err, b.err_msg.c_str());
    hipStream_t s = ctx->stream;
    const uint32_t R = (uint32_t)b.n_rows, nR = (R + 255) / 256;
    const size_t n_refs = (size_t)b.n_refs, n_lin = (size_t)b.h_lin_off[n_refs];
    unsigned long long n_bins = 0;
    MTH_HIP(ctx, b.ref_nbin.reserve(n_refs * 4 + 16, s));
    MTH_HIP(ctx, hipMemsetAsync(b.ref_nbin.p, 0, n_refs * 4 + 16, s));
    if (R) {
        for (DevBuf *d : {&b.skey, &b.cb, &b.ce, &b.bin_key}) MTH_HIP(ctx, d->reserve((size_t)R * 8 + 16, s));
        for (DevBuf *d : {&b.idx, &b.perm, &b.bin_start, &b.bin_cnt}) MTH_HIP(ctx, d->reserve((size_t)R * 4 + 16, s));
        MTH_HIP(ctx, b.flag.reserve((size_t)R * 4 + 16, s)); MTH_HIP(ctx, b.rank.reserve(((size_t)R + 1) * 8 + 16, s));
        int ref_bits = 1;
        while (ref_bits < 32 && (1ll << ref_bits) < (long long)b.n_refs) ++ref_bits;
        {
            LaunchTimer lt(ctx, K_BAI_SORT);
            hipLaunchKernelGGL(k_bai_iota, dim3(nR), dim3(256), 0, s, b.idx.as<uint32_t>(), R);
            size_t tmp_bytes = 0;
            MTH_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, b.r_key.as<unsigned long long>(), b.skey.as<unsigned long long>(),
                                                            b.idx.as<uint32_t>(), b.perm.as<uint32_t>(), (int)R, 0, 32 + ref_bits, s));
            MTH_HIP(ctx, b.tmp.reserve(tmp_bytes + 16, s));
            MTH_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(b.tmp.p, tmp_bytes, b.r_key.as<unsigned long long>(), b.skey.as<unsigned long long>(),
                                                            b.idx.as<uint32_t>(), b.perm.as<uint32_t>(), (int)R, 0, 32 + ref_bits, s));
            hipLaunchKernelGGL(k_bai_gather, dim3(nR), dim3(256), 0, s, b.skey.as<unsigned long long>(), b.perm.as<uint32_t>(), R, b.r_vb.as<unsigned long long>(),
                               b.r_ve.as<unsigned long long>(), b.cb.as<unsigned long long>(), b.ce.as<unsigned long long>(), b.flag.as<uint32_t>());
        }
        MTH_HIP(ctx, hipGetLastError());
        { const int rc = scan_u32_to_u64(ctx, b.flag.as<uint32_t>(), R, 0ull, b.rank.as<unsigned long long>(), &n_bins); if (rc) return rc; }   // synchronises
        hipLaunchKernelGGL(k_bai_bins, dim3(nR), dim3(256), 0, s, b.skey.as<unsigned long long>(), b.flag.as<uint32_t>(), b.rank.as<unsigned long long>(), R,
                           b.bin_key.as<unsigned long long>(), b.bin_start.as<uint32_t>(), b.ref_nbin.as<uint32_t>());
        hipLaunchKernelGGL(k_bai_bin_counts, dim3(((uint32_t)n_bins + 255) / 256), dim3(256), 0, s, b.bin_start.as<uint32_t>(), (uint32_t)n_bins, R, b.bin_cnt.as<uint32_t>());
        MTH_HIP(ctx, hipGetLastError());
    }
    if (n_refs) {
        LaunchTimer lt(ctx, K_BAI_FILL);
        hipLaunchKernelGGL(k_bai_fill, dim3((uint32_t)n_refs), dim3(256), 0, s, b.lin.as<unsigned long long>(), b.tab.as<unsigned long long>(), b.n_intv.as<uint32_t>());
    }
    MTH_HIP(ctx, hipGetLastError());
    // the finished tables to the host
    b.h_cb.resize(R); b.h_ce.resize(R); b.h_bin_key.resize((size_t)n_bins); b.h_bin_cnt.resize((size_t)n_bins); b.h_bin_ref.resize((size_t)n_bins); b.h_bin_id.resize((size_t)n_bins);
    b.h_ref_nbin.assign(n_refs, 0); b.h_n_intv.assign(n_refs, 0); b.h_lin.resize(n_lin); b.h_meta.assign(n_refs * 4, 0);
    BaiState st{};
    auto down = [&](void *dst, const DevBuf &src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    MTH_HIP(ctx, down(b.h_cb.data(), b.cb, (size_t)R * 8)); MTH_HIP(ctx, down(b.h_ce.data(), b.ce, (size_t)R * 8));
    MTH_HIP(ctx, down(b.h_bin_key.data(), b.bin_key, (size_t)n_bins * 8)); MTH_HIP(ctx, down(b.h_bin_cnt.data(), b.bin_cnt, (size_t)n_bins * 4));
    MTH_HIP(ctx, down(b.h_ref_nbin.data(), b.ref_nbin, n_refs * 4)); MTH_HIP(ctx, down(b.h_n_intv.data(), b.n_intv, n_refs * 4));
    MTH_HIP(ctx, down(b.h_lin.data(), b.lin, n_lin * 8)); MTH_HIP(ctx, down(b.h_meta.data(), b.meta, n_refs * 32));
    MTH_HIP(ctx, down(&st, b.state, sizeof st));
    MTH_HIP(ctx, hipStreamSynchronize(s));
    for (size_t k = 0; k < (size_t)n_bins; ++k) { b.h_bin_ref[k] = (int32_t)(b.h_bin_key[k] >> 32); b.h_bin_id[k] = (uint32_t)b.h_bin_key[k]; }
    out->n_refs = b.n_refs; out->n_records = b.n_records; out->n_chunks = R; out->n_bins = n_bins; out->n_no_coor = st.n_no_coor;
    out->chunk_beg = b.h_cb.data(); out->chunk_end = b.h_ce.data();
    out->bin_ref = b.h_bin_ref.data(); out->bin_id = b.h_bin_id.data(); out->bin_n_chunks = b.h_bin_cnt.data();
    out->ref_n_bins = b.h_ref_nbin.data(); out->ref_n_intv = b.h_n_intv.data(); out->lin_off = b.h_lin_off.data(); out->lin = b.h_lin.data();
    out->meta = b.h_meta.data();
    return MTH_OK;
}

}  // extern "C"
