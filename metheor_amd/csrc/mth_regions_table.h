// mth_regions_table.h -- the declared intervals of a per-interval measure and their table on the device (private): what
// mth_mhl_regions.hip, mth_pdr_regions.hip and mth_quartet_regions.hip keep between a begin and the fetches, and the domain registration mth_intervals.hip
// shares with them.
#pragma once
#include <string>

#include "mth_ctx.h"
#include "mth_intervals_dev.h"
#include "mth_regions_host.h"

namespace mth {

// "<prefix> <tail>": a measure's own prefix ("mhl regions:") before the text the measures share
inline int iv_fail(mth_ctx *ctx, int status, const char *prefix, const char *tail) { return fail(ctx, status, (std::string(prefix) + " " + tail).c_str()); }

// The slices of a batch's domain (its tid: a contig, or the handle -2 - k of contig group k, which the caller has checked), sorted
// into `dm` on first sight.  *added: the domain is new, so a table packed earlier lacks it.
inline int iv_slices_for(mth_ctx *ctx, IvDomains &dm, const char *prefix, int32_t dom, std::pair<uint32_t, uint32_t> &slices, bool *added) {
    *added = !dm.has(dom);
    if (*added) {
        if (dom >= 0) dm.add_domain(dom);
        else {
            if (dom > -2) return iv_fail(ctx, MTH_ERR_INVALID, prefix, "batch.tid");
            const mth_ctx::ContigGroup &g = ctx->groups[(size_t)(-2 - (int64_t)dom)];
            dm.add_domain(dom, g.tids.size(), g.tids.data(), g.voff.data());
        }
        if (dm.entries() >= (size_t)INT32_MAX) return iv_fail(ctx, MTH_ERR_CAPACITY, prefix, "2^31 or more interval entries");
    }
    slices = dm.dom_slices[dom];
    return MTH_OK;
}

// mth_*_regions_begin's look at the caller's intervals
inline int regions_check(mth_ctx *ctx, const char *prefix, uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    if (n && (!tid || !beg || !end)) return iv_fail(ctx, MTH_ERR_INVALID, prefix, "an array is missing");
    if (n >= (1ull << 31)) return iv_fail(ctx, MTH_ERR_CAPACITY, prefix, "2^31 or more intervals");
    const char *bad = iv_check_intervals(n, tid, beg, end);
    return bad ? iv_fail(ctx, MTH_ERR_INVALID, prefix, bad) : MTH_OK;
}

struct RegionsTable {
    std::vector<int32_t> tid, beg, end;            // the declared intervals (a copy: the caller's arrays may go)
    std::unique_ptr<IvDomains> dm;
    DevBuf tab;
    IvTab dev{};                                   // the table in `tab`, as of the latest upload
    bool dirty = true;                             // a domain was added since the table went up

    size_t size() const { return tid.size(); }
    void declare(uint64_t n, const int32_t *t, const int32_t *b, const int32_t *e) {
        tid.assign(t, t + n); beg.assign(b, b + n); end.assign(e, e + n);
        dm.reset(new IvDomains(n, tid.data(), beg.data(), end.data()));
        dirty = true;
    }
    // the slices of a staged batch's domain (stage_batch has checked a group's handle)
    int slices_for(mth_ctx *ctx, const char *prefix, int32_t batch_tid, std::pair<uint32_t, uint32_t> *slices) {
        bool added = false;
        const int rc = iv_slices_for(ctx, *dm, prefix, batch_tid, *slices, &added);
        dirty |= added;
        return rc;
    }
    // The table of every domain met so far, if the one on the device lacks one.  Kernels queued earlier may still read the table that
    // is replaced: the stream is drained first, whether the pass waits for its batches (MHL: nothing is left to wait for) or only
    // queues them (PDR).  Once per new domain -- a contig or contig group the intervals had not met -- not once per batch.
    int upload(mth_ctx *ctx) {
        if (!dirty) return MTH_OK;
        std::vector<uint32_t> words;
        const IvTabOffsets o = dm->pack(words);
        MTH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MTH_HIP(ctx, tab.reserve(std::max<size_t>(words.size(), 1) * 4, ctx->stream));
        if (!words.empty()) MTH_HIP(ctx, hipMemcpy(tab.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
        dev = o.at(tab.as<uint32_t>());
        dirty = false;
        return MTH_OK;
    }
    void release() { tab.release(); }
};

// what the read x interval passes tell their kernel about a staged batch
inline RgReadArgs rg_read_args(const mth_ctx *ctx, const mth_batch_t &d, const mth_mhl_params_t &p, const IvTab &tab, std::pair<uint32_t, uint32_t> slices) {
    RgReadArgs a;
    a.read_start = d.read_start; a.read_mapq = d.read_mapq; a.cpg_off = d.cpg_off; a.cpg_pos = d.cpg_pos;
    a.tab = tab; a.st = ctx->d_state;
    a.n_reads = d.n_reads; a.n_cpgs = d.n_cpgs; a.min_cpgs = p.min_cpgs; a.sl0 = slices.first; a.sl1 = slices.second;
    a.region_beg = d.region_beg; a.region_end = d.region_end; a.min_qual = p.min_qual;
    return a;
}

}  // namespace mth
