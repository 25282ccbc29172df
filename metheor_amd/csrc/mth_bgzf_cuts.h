// mth_bgzf_cuts.h -- where a stream of BAM records is cut into BGZF blocks (host only, no HIP: the CLI, the C ABI and the CPU
// test all call this one function).
//
// htslib's rule (bgzf_flush_try before every record, bgzf_write across block ends):
//   - a block holds at most BGZF_MAX_BLOCK = 0xff00 uncompressed bytes;
//   - a record that does not fit into what is left of the current block starts a new block;
//   - a record longer than a block starts a new block and is cut across consecutive FULL blocks; what is left of it opens the
//     last of them, which later records may share;
//   - the stream's last block is closed short (a window of a file never carries bytes into the next window).
// The first record of a stream therefore starts a block, and no block begins or ends inside a record that fits a block: what a
// reader that wants whole records per block (mth_bgzf_decode) needs.
#pragma once
#include <stdint.h>

#include <vector>

namespace mth {

constexpr uint32_t BGZF_MAX_BLOCK = 0xff00u;

// rec_size[i] = bytes of record i (its block_size field included); cuts receives n_blocks + 1 ascending offsets into the
// stream, cuts[0] = 0 and cuts[n_blocks] = the stream's size (an empty stream: the single offset 0, no block)
inline void bgzf_record_cuts(const uint32_t *rec_size, uint64_t n_rec, std::vector<uint64_t> &cuts) {
    cuts.assign(1, 0);
    uint64_t pos = 0;          // bytes placed so far
    uint32_t fill = 0;         // bytes in the open block
    for (uint64_t i = 0; i < n_rec; ++i) {
        uint64_t s = rec_size[i];
        if (fill && fill + s > BGZF_MAX_BLOCK) { cuts.push_back(pos); fill = 0; }
        while (s > BGZF_MAX_BLOCK) {                 // (only with fill == 0: a record longer than a block has just closed it)
            pos += BGZF_MAX_BLOCK; s -= BGZF_MAX_BLOCK;
            cuts.push_back(pos);
        }
        pos += s; fill += (uint32_t)s;
        if (fill == BGZF_MAX_BLOCK) { cuts.push_back(pos); fill = 0; }
    }
    if (fill) cuts.push_back(pos);
}

// plain bytes (no records): a cut every BGZF_MAX_BLOCK bytes
inline void bgzf_byte_cuts(uint64_t n_bytes, std::vector<uint64_t> &cuts) {
    cuts.assign(1, 0);
    for (uint64_t p = 0; p < n_bytes;) { p += (n_bytes - p < BGZF_MAX_BLOCK) ? n_bytes - p : BGZF_MAX_BLOCK; cuts.push_back(p); }
}

}  // namespace mth
