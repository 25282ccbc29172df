// mth_regions_host.h -- the host-only pieces of the per-interval measures (`lpmd --intervals`, `mhl-regions`, `pdr-regions`, `me-regions` / `pm-regions`): the intervals of a BED
// file as one batch's domain sees them, their packed table, and the finalisers of MHL, of PDR and of ME / PM per interval.  Plain C++, nothing of HIP, no environment: the
// library (mth_intervals.hip, mth_mhl_regions.hip, mth_pdr_regions.hip, mth_quartet_regions.hip) and the command line share this one copy, and it is tested
// without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mth {

// ---- interval domains ----------------------------------------------------------------------------------------------------------------
// A batch's tid names its domain: a contig, or a contig group whose contig k lies at [voff[k], ...) of one virtual coordinate space.
// Per domain the intervals are split into length classes (two bit lengths per class: lengths within a factor 4) and each class is
// sorted by start with a running maximum of the ends -- a SLICE.  A pass finds the last entry of a slice with start <= x by search
// and walks back while the running maximum is still beyond what it looks for: an entry k steps back starts at least k / depth
// interval lengths earlier, so a walk passes at most ~4x the intervals that hold its target, whatever other lengths the BED mixes in
// (a chromosome-long interval sits in a class of its own and costs one step).
struct IvEntry { int32_t start, end; uint32_t out; };

// The slices of every domain met so far as a pass reads them on the device: six arrays in one buffer of 32-bit words.
struct IvTab {
    const int32_t *s_beg, *s_end;                  // per slice (one domain, one length class): its entries [s_beg, s_end)
    const int32_t *e_start, *e_end, *e_maxend;     // per entry, sorted by start within the slice; maxend: running maximum of e_end
    const uint32_t *e_out;                         // the interval (caller's index) the entry adds to
};
// where IvDomains::pack put the six arrays (32-bit words from the buffer's start), and the table at a buffer that holds them
struct IvTabOffsets {
    size_t s_beg, s_end, e_start, e_end, e_maxend, e_out;
    IvTab at(const uint32_t *base) const {
        auto i32 = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o); };
        return IvTab{i32(s_beg), i32(s_end), i32(e_start), i32(e_end), i32(e_maxend), base + e_out};
    }
};

// what a set of intervals must satisfy; nullptr, or the tail of the message (the caller's prefix names the measure)
inline const char *iv_check_intervals(uint64_t n, const int32_t *tid, const int32_t *beg, const int32_t *end) {
    for (uint64_t i = 0; i < n; ++i)
        if (tid[i] < 0 || beg[i] < 0 || end[i] < beg[i]) return "want tid >= 0 and 0 <= beg <= end";
    return nullptr;
}

struct IvDomains {
    static constexpr int NCLS = 17;
    const int32_t *tid, *beg, *end;                // the caller's intervals (not owned)
    std::unordered_map<int32_t, std::vector<uint32_t>> by_tid;
    std::vector<int32_t> s_beg, s_end;             // per slice: its entries [s_beg, s_end)
    std::vector<int32_t> e_start, e_end, e_maxend; // per entry, sorted by start within its slice; maxend: running maximum of e_end
    std::vector<uint32_t> e_out;                   // the interval (caller's index) the entry belongs to
    std::unordered_map<int32_t, std::pair<uint32_t, uint32_t>> dom_slices;     // a batch tid -> its slices [first, second)

    IvDomains(uint64_t n, const int32_t *tid_, const int32_t *beg_, const int32_t *end_) : tid(tid_), beg(beg_), end(end_) {
        for (uint64_t i = 0; i < n; ++i)
            if (beg[i] < end[i]) by_tid[tid[i]].push_back((uint32_t)i);       // an empty interval holds nothing
    }
    bool has(int32_t dom) const { return dom_slices.count(dom) != 0; }
    size_t entries() const { return e_start.size(); }

    // the slices of a domain: a contig (n_contigs == 0: `dom` is its tid), or a group of n_contigs contigs (tids, voff ascending).  A
    // group shifts an interval by its contig's voff and cuts it at the word before the next contig: contig k + 1's position -1 lies
    // at voff[k + 1] - 1 and is the first word that is not contig k's.
    void add_domain(int32_t dom, size_t n_contigs = 0, const int32_t *g_tids = nullptr, const int64_t *g_voff = nullptr) {
        std::vector<IvEntry> cls[NCLS];
        auto put = [&](int64_t vb, int64_t ve, uint32_t out) {
            if (vb >= ve) return;
            const int bits = 64 - __builtin_clzll((unsigned long long)(ve - vb));     // 1 .. 31
            cls[(bits + 1) / 2].push_back(IvEntry{(int32_t)vb, (int32_t)ve, out});
        };
        if (n_contigs == 0) {
            const auto f = by_tid.find(dom);
            if (f != by_tid.end())
                for (uint32_t i : f->second) put(beg[i], end[i], i);
        } else {
            for (size_t k = 0; k < n_contigs; ++k) {
                const auto f = by_tid.find(g_tids[k]);
                if (f == by_tid.end()) continue;
                const int64_t limit = k + 1 < n_contigs ? g_voff[k + 1] - 1 : (int64_t)INT32_MAX;
                for (uint32_t i : f->second) put(g_voff[k] + beg[i], std::min<int64_t>(g_voff[k] + end[i], limit), i);
            }
        }
        const uint32_t first = (uint32_t)s_beg.size();
        for (auto &v : cls) {
            if (v.empty()) continue;
            std::sort(v.begin(), v.end(), [](const IvEntry &x, const IvEntry &y) { return x.start != y.start ? x.start < y.start : x.out < y.out; });
            s_beg.push_back((int32_t)e_start.size());
            int32_t mx = 0;
            for (const IvEntry &e : v) {
                mx = std::max(mx, e.end);
                e_start.push_back(e.start); e_end.push_back(e.end); e_maxend.push_back(mx); e_out.push_back(e.out);
            }
            s_end.push_back((int32_t)e_start.size());
        }
        dom_slices[dom] = {first, (uint32_t)s_beg.size()};
    }

    // the six arrays appended to `words` (the one place that knows the table's layout)
    IvTabOffsets pack(std::vector<uint32_t> &words) const {
        auto place = [&](const void *src, size_t n) {
            const size_t at = words.size();
            words.resize(at + n);
            if (n) memcpy(words.data() + at, src, n * 4);
            return at;
        };
        return IvTabOffsets{place(s_beg.data(), s_beg.size()), place(s_end.data(), s_end.size()), place(e_start.data(), e_start.size()),      // (in this order)
                            place(e_end.data(), e_end.size()), place(e_maxend.data(), e_maxend.size()), place(e_out.data(), e_out.size())};
    }
};

// ---- MHL per interval: the finaliser --------------------------------------------------------------------------------------------------
// compute_mhl (mhl.rs:43-73) of the AssociatedReads an interval collects (mhl.rs:75-80 add_num_cpgs, mhl.rs:36-41 add_stretch_info with
// readutil.rs:147-164 get_stretch_info), from the interval's two histograms, given as k sparse rows of ascending, distinct length:
//   runs[i]  = R[length[i]]: maximal methylated runs of that length among the kept calls of the contributing reads
//   reads[i] = C[length[i]]: contributing reads with that many kept calls
// stretch_info[l] = sum over r >= l of R[r] (r - l + 1), the denominator of l = sum over n >= l of C[n] (n - l + 1), max_num_cpgs = the
// largest n with C[n] > 0.  Terms in ascending l, l_sum as the running f32 sum, every operation a single f32 one (no a * b + c to
// contract), as the per-CpG MHL does it (mth_sites.hip).  Both sums are exact 64-bit integers converted to f32 once: the same bits as
// the reference's read-by-read f32 denominator whenever the interval's sum of n is below 2^24 (beyond that the reference's own value
// depends on the record order).  Fewer than max(min_depth, 1) contributing reads: NaN.
inline float mhl_regions_finalise(size_t k, const uint32_t *length, const uint64_t *runs, const uint64_t *reads, uint32_t min_depth,
                                  uint64_t *n_reads_out, uint32_t *max_cpgs_out) {
    uint64_t n_reads = 0;
    uint32_t maxn = 0, maxr = 0;
    for (size_t i = 0; i < k; ++i) {
        if (reads[i]) { n_reads += reads[i]; maxn = std::max(maxn, length[i]); }
        if (runs[i]) maxr = std::max(maxr, length[i]);
    }
    if (n_reads_out) *n_reads_out = n_reads;
    if (max_cpgs_out) *max_cpgs_out = maxn;
    if (n_reads < std::max<uint64_t>(min_depth, 1)) return std::nanf("");
    // suffix sums twice, from the longest length down: cnt = entries of length >= l, sum = their (length - l + 1) added up
    const uint32_t top = std::max(maxn, maxr);
    std::vector<uint64_t> S((size_t)top + 2, 0), D((size_t)top + 2, 0);
    {
        uint64_t cr = 0, sr = 0, cn = 0, sn = 0;
        size_t i = k;
        for (uint32_t l = top; l >= 1; --l) {
            while (i > 0 && length[i - 1] >= l) { --i; cr += runs[i]; cn += reads[i]; }
            sr += cr; sn += cn;
            S[l] = sr; D[l] = sn;
        }
    }
    float l_sum = 0.0f;
    for (uint32_t l = 1; l < maxn + 1; ++l) l_sum = l_sum + (float)l;
    float mhl = 0.0f;
    for (uint32_t l = 1; l <= top; ++l)
        if (S[l] > 0) { const float t = ((float)l * (float)S[l]) / (float)D[l]; mhl = mhl + t; }
    return mhl / l_sum;
}

// ---- PDR per interval: the finaliser --------------------------------------------------------------------------------------------------
// compute_pdr (pdr.rs:47-49) of the interval's counters: n_concordant = the contributing reads whose kept calls are all methylated or
// all unmethylated, n_discordant = the others.  Each 64-bit counter is converted to f32 once, then one f32 add and one f32 divide: the
// reference's bits whenever the counts fit its u32.  Fewer than max(min_depth, 1) contributing reads: NaN.
inline float pdr_regions_finalise(uint64_t n_concordant, uint64_t n_discordant, uint32_t min_depth) {
    if (n_concordant + n_discordant < std::max<uint64_t>(min_depth, 1)) return std::nanf("");
    const float c = (float)n_concordant, d = (float)n_discordant;
    const float den = c + d;
    return d / den;
}

// ---- ME / PM per interval: the finaliser -----------------------------------------------------------------------------------------------
// compute_me (me.rs:42-55) and compute_pm (pm.rs:42-51) of the interval's ONE pooled QuartetStat: bins[p] = windows of four consecutive
// kept calls with pattern p = 8*m1 + 4*m2 + 2*m3 + m4, over every contributing read.  n_patterns = the sum of the bins, the stat's
// get_read_depth().  The reference's operation order: bins 0..15 ascending, p = count / total with each converted to f32 once,
// me += p * log2(p) for the non-zero bins and me *= -0.25 last, pm -= p * p for every bin, zero ones included.  Plain operators, one
// f32 operation each -- the objects that include this are built with -ffp-contract=off (the note in mth_quartet_dev.h) --: the
// reference's bits whenever the counts fit its u32 (ME up to what log2 of the two C libraries differ by).  Fewer than max(min_depth, 1)
// patterns: both NaN (me.rs:82 applied to the pooled stat).
inline void quartet_regions_finalise(const uint64_t *bins, uint32_t min_depth, float *me_out, float *pm_out, uint64_t *n_patterns_out) {
    uint64_t total = 0;
    for (int k = 0; k < 16; ++k) total += bins[k];
    if (n_patterns_out) *n_patterns_out = total;
    float me = std::nanf(""), pm = std::nanf("");
    if (total >= std::max<uint64_t>(min_depth, 1)) {
        const float tf = (float)total;
        me = 0.0f;
        pm = 1.0f;
        for (int k = 0; k < 16; ++k) {
            const float p = (float)bins[k] / tf;
            if (bins[k] > 0) {
                const float t = p * log2f(p);
                me = me + t;
            }
            const float sq = p * p;
            pm = pm - sq;
        }
        me = me * -0.25f;
    }
    if (me_out) *me_out = me;
    if (pm_out) *pm_out = pm;
}

}  // namespace mth
