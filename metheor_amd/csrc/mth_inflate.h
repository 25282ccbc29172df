// mth_inflate.h -- what mth_inflate.hip lends to the other load paths (private): the verified BGZF inflate and the two halves of
// the overlapped staging copy (mth_bgzf_stage).
#pragma once
#include "mth_ctx.h"

namespace mth {

// the staging buffers carry this much zeroed padding behind the file bytes (why: mth_inflate.hip)
constexpr size_t INF_FILE_PAD = 160 * 1024;

// stage the file bytes + block table and launch the inflate and the CRC32 check; on return d_uoff / d_isize point at the device
// table (the blocks' output starts at stream_base in inf_raw; total includes it).  Findings surface at the next sync_and_check.
int inflate_blocks(mth_ctx *ctx, const void *file, uint64_t n_bytes, const uint64_t *coff, const uint32_t *csize,
                   const uint32_t *isize, uint64_t n_blocks, uint64_t &total, uint64_t *&d_uoff, uint32_t *&d_isize, uint64_t stream_base = 0);

// the bytes file[0, n_bytes) are wanted in ctx->inf_file: joins the helper thread of the previous call and, if it copied exactly
// these bytes (announced by mth_bgzf_stage), takes its buffer (staged = true: ctx->stream waits for the copy); otherwise inf_file
// is made large enough and the caller copies in line
int stage_take(mth_ctx *ctx, const void *file, uint64_t n_bytes, bool &staged);
// the chunk announced by mth_bgzf_stage, if any: a helper thread copies it into inf_file2 on the side stream from now on
int stage_start_next(mth_ctx *ctx);

}  // namespace mth
