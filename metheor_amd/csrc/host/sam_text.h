// sam_text.h -- SAM text <-> BAM records and a FASTA reader (see sam_text.cpp)
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "bam_reader.h"

namespace mthh {

// true if the file is text that starts like SAM (an @XX header line, or an 11-field alignment line)
bool looks_like_sam(const std::string &path);
// the whole SAM file as the bytes of an equivalent BGZF-compressed BAM file (whole records per block)
bool sam_text_to_bam(const std::string &path, std::vector<uint8_t> &bam, std::string &err);
// one BAM record (the bytes after block_size) as a SAM line ending in '\n'; xm != nullptr appends "\tXM:Z:<xm>"
bool sam_format_record(const std::vector<BamRef> &refs, const uint8_t *rec, uint32_t len, const char *xm, uint32_t xm_len, std::string &out);

struct BgzfMap;

class Fasta {
  public:
    Fasta();
    ~Fasta();
    // plain text (the .fai next to it, or one scan), or bgzip-compressed text: BGZF needs <path>.fai (coordinates in the
    // uncompressed stream; no .gzi: nothing here seeks), gzip that is not BGZF is refused
    bool open(const std::string &path, std::string &err);
    // faidx_fetch_seq(name, 0, end_incl): the bases [0, end_incl] clipped to the sequence, white space dropped (plain files only:
    // a compressed file is read on the device)
    bool fetch(const std::string &name, int64_t end_incl, std::vector<uint8_t> &seq, std::string &err) const;
    bool compressed() const { return bgzf_; }
    // the file mapped read-only and, for BGZF, the table of its blocks (the walk of bgzf_map); made once
    const BgzfMap *map(std::string &err);
    uint64_t stream_bytes() const { return stream_bytes_; }         // after map(): the uncompressed size
    // where fetch(name, end_incl) would read: offset of base 0 in the uncompressed stream, bases to take, line layout; checked
    // against the stream's size (map() is called).  `key` points at the name as the index holds it.
    struct Row { uint64_t src_off = 0; int64_t n_bases = 0, line_bases = 0, line_width = 0; const char *key = nullptr; };
    bool layout(const std::string &name, int64_t end_incl, Row &row, std::string &err);

  private:
    struct Entry { int64_t length = 0, offset = 0, line_bases = 0, line_width = 0; };
    std::string path_;
    std::unordered_map<std::string, Entry> index_;
    bool bgzf_ = false;
    BgzfMap *map_ = nullptr;
    uint64_t stream_bytes_ = 0;
};

}  // namespace mthh
