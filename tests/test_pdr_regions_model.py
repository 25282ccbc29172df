"""The per-interval PDR pass on the CPU, before any device is there.  metheor_amd/csrc/mth_pdr_regions_dev.h -- the per-lane part of
k_pdr_regions: the summary of a read, the whole / partial decision, the partial walk, the class -- compiles under
MTH_PDR_REGIONS_HOST_MODEL into a stand-alone program (its own main, g++ with the address and undefined-behaviour sanitizers) that plays
the kernel work item by work item around it: 256 reads at a time, the candidate range of every slice of the batch's domain
(mth_regions_host.h, the library's own copy), the span route, the LDS rows as bounds-checked arrays of exactly the cap's size, the
direct route.  Its counts must equal the numpy restatement (tests/pdr_regions_util.py) on every interval, in every form."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import pdr_regions_util as U

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#define MTH_PDR_REGIONS_HOST_MODEL
#include "mth_pdr_regions_dev.h"
#include "mth_regions_host.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
using namespace mth;

template <class T> static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2);
    return v;
}
static uint32_t take_u32(FILE *f) { return take<uint32_t>(f, 1)[0]; }
static int32_t upper(const std::vector<int32_t> &a, int32_t lo, int32_t hi, int32_t v) {      // iv_upper / iv_upper_wave
    return (int32_t)(std::upper_bound(a.begin() + lo, a.begin() + hi, v) - a.begin());
}

// argv: input, output, LDS cap, span route (0 / 1), workgroups (work item ch goes to workgroup ch mod that).  IN: n, tid / beg / end of the intervals, min_cpgs, min_qual, batches; per batch
// dom, n_contigs, tids, voff (int64), region_beg, region_end, n_reads, n_cpgs, read_start, read_mapq, cpg_off, cpg_pos.
// OUT: per interval four u64 words, then u64 stats: error flag, adds by the span route, to LDS rows, to memory directly, slices
// that used LDS rows, slices that went direct, adds of pending sums
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    const int32_t cap = atoi(argv[3]);
    const bool span = atoi(argv[4]) != 0;
    const uint32_t grid = (uint32_t)atoi(argv[5]);
    constexpr int PEND = IvDomains::NCLS;
    constexpr int B = 256;
    const uint32_t n_iv = take_u32(f);
    const std::vector<int32_t> tid = take<int32_t>(f, n_iv), beg = take<int32_t>(f, n_iv), end = take<int32_t>(f, n_iv);
    const uint32_t min_cpgs = take_u32(f), min_qual = take_u32(f), n_batches = take_u32(f);
    const uint32_t need = std::max(min_cpgs, 1u);
    IvDomains dm(n_iv, tid.data(), beg.data(), end.data());
    std::vector<uint64_t> rows((size_t)n_iv * PR_ROW, 0);
    uint64_t stats[7] = {0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> s_rows((size_t)cap * PR_ROW);                  // the LDS of a workgroup: exactly the cap
    for (uint32_t bi = 0; bi < n_batches; ++bi) {
        const int32_t dom = (int32_t)take_u32(f);
        const uint32_t n_contigs = take_u32(f);
        const std::vector<int32_t> g_tids = take<int32_t>(f, n_contigs);
        const std::vector<int64_t> g_voff = take<int64_t>(f, n_contigs);
        const int32_t region_beg = (int32_t)take_u32(f), region_end = (int32_t)take_u32(f);
        const uint32_t n_reads = take_u32(f), n_cpgs = take_u32(f);
        const std::vector<int32_t> read_start = take<int32_t>(f, n_reads);
        const std::vector<uint8_t> read_mapq = take<uint8_t>(f, n_reads);
        const std::vector<uint32_t> cpg_off = take<uint32_t>(f, (size_t)n_reads + 1), cpg_pos = take<uint32_t>(f, n_cpgs);
        if (!dm.has(dom)) dm.add_domain(dom, n_contigs, g_tids.data(), g_voff.data());
        const auto sl = dm.dom_slices[dom];
        if (sl.first == sl.second || n_reads == 0 || n_cpgs == 0) continue;
        const uint32_t n_chunks = (n_reads + B - 1) / B;
        const bool pend = sl.second - sl.first <= (uint32_t)PEND;
        for (uint32_t wg = 0; wg < std::min(grid, n_chunks); ++wg) {
        // the workgroup's pending sums: per slice the only candidate that held the span, and what is still to be added to it
        std::vector<int32_t> s_pj(PEND, -1);
        std::vector<uint32_t> s_pv((size_t)PEND * 3, 0u);
        auto pend_flush = [&](int k) {
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = s_pv.at((size_t)k * 3 + c);
                if (s_pj.at(k) >= 0 && v) { rows.at((size_t)dm.e_out.at(s_pj.at(k)) * PR_ROW + c) += v; stats[6] += 1; }
                s_pv.at((size_t)k * 3 + c) = 0u;
            }
        };
        for (uint32_t ch = wg; ch < n_chunks; ch += grid) {
            PrRead rd[B];
            bool elig[B];
            int32_t wmin = INT32_MAX, wmax = -1;
            uint32_t cnt[3] = {0, 0, 0};
            for (int t = 0; t < B; ++t) {
                const uint32_t r = ch * B + (uint32_t)t;
                elig[t] = false;
                rd[t].k0 = rd[t].k1 = 0; rd[t].first = INT32_MAX; rd[t].last = -1; rd[t].cls = PR_NONE;
                if (r >= n_reads) continue;
                const int32_t rs = read_start.at(r);
                if (!(rs >= region_beg && rs < region_end && read_mapq.at(r) >= min_qual)) continue;
                const uint32_t k0 = cpg_off.at(r), k1 = cpg_off.at(r + 1);
                if (!(k1 > k0 && k1 <= n_cpgs && k1 - k0 >= need)) continue;
                elig[t] = pr_summary(cpg_pos.data(), k0, k1, rd[t]);
                if (!elig[t]) { stats[0] = 1; rd[t].first = INT32_MAX; rd[t].last = -1; rd[t].cls = PR_NONE; continue; }
                wmin = std::min(wmin, rd[t].first); wmax = std::max(wmax, rd[t].last);
                cnt[rd[t].cls] += 1;
            }
            if (wmax < 0) continue;
            for (uint32_t s = sl.first; s < sl.second; ++s) {
                const int32_t lo = dm.s_beg.at(s), hi = dm.s_end.at(s);
                const int32_t w_hi = upper(dm.e_start, lo, hi, wmax);
                if (w_hi == lo) continue;
                const int32_t w_min = upper(dm.e_maxend, lo, w_hi, wmin);
                if (w_min == w_hi) continue;
                const int32_t acc_n = w_hi - w_min;
                bool rest = !span;
                if (span && pend && acc_n == 1 && pr_holds_span(dm.e_start.at(w_min), dm.e_end.at(w_min), wmin, wmax)) {
                    const int k = (int)(s - sl.first);
                    if (s_pj.at(k) != w_min) { pend_flush(k); s_pj.at(k) = w_min; }
                    for (int c = 0; c < 3; ++c) s_pv.at((size_t)k * 3 + c) += cnt[c];
                    continue;
                }
                if (span)
                    for (int32_t j = w_min; j < w_hi; ++j) {
                        if (!pr_holds_span(dm.e_start.at(j), dm.e_end.at(j), wmin, wmax)) { rest = true; continue; }
                        for (int c = 0; c < 3; ++c)
                            if (cnt[c]) { rows.at((size_t)dm.e_out.at(j) * PR_ROW + c) += cnt[c]; stats[1] += 1; }
                    }
                if (!rest) continue;
                const bool use_lds = acc_n <= cap;
                stats[use_lds ? 4 : 5] += 1;
                if (use_lds)
                    for (int32_t i = 0; i < acc_n * PR_ROW; ++i) s_rows.at(i) = 0u;
                for (int t = 0; t < B; ++t) {
                    if (!elig[t]) continue;
                    for (int32_t j = upper(dm.e_start, w_min, w_hi, rd[t].last) - 1; j >= w_min && dm.e_maxend.at(j) > rd[t].first; --j) {
                        const int32_t ie = dm.e_end.at(j);
                        if (ie <= rd[t].first) continue;
                        const int32_t ib = dm.e_start.at(j);
                        if (span && pr_holds_span(ib, ie, wmin, wmax)) continue;
                        const uint32_t cls = pr_entry_class(cpg_pos.data(), rd[t], ib, ie, need);
                        if (cls == PR_NONE) continue;
                        if (use_lds) { s_rows.at((size_t)(j - w_min) * PR_ROW + cls) += 1u; stats[2] += 1; }
                        else { rows.at((size_t)dm.e_out.at(j) * PR_ROW + cls) += 1; stats[3] += 1; }
                    }
                }
                if (!use_lds) continue;
                for (int32_t i = 0; i < acc_n * PR_ROW; ++i) {
                    const uint32_t v = s_rows.at(i);
                    if (v) rows.at((size_t)dm.e_out.at(w_min + i / PR_ROW) * PR_ROW + (uint32_t)(i % PR_ROW)) += v;
                }
            }
        }
        for (int k = 0; k < PEND; ++k) pend_flush(k);
        }
    }
    if (fwrite(rows.data(), 8, rows.size(), o) != rows.size() || fwrite(stats, 8, 7, o) != 7) return 2;
    fclose(o);
    return 0;
}
"""


def default_cap():
    text = open(os.path.join(CSRC, "mth_knobs.h")).read()
    return int(re.search(r"constexpr int PDR_REGIONS_LDS_CAP = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("pdr_regions_model")
    src = d / "pdr_regions_model.cpp"
    src.write_text(DRIVER)
    out = d / "pdr_regions_model"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


@pytest.fixture(scope="module")
def soa():
    return pyoracle.Reads.decode(U.records()).soa()


VOFF = [1, U.REFS[0][1] + 8192]                  # the two contigs with reads as one contig group: ivA's call at -1 lies at word 0


def batch_bytes(s, dom, tids, voff, region=(0, U.INT32_MAX)):
    """the reads of the contigs `tids` as one batch: a plain contig (voff None: dom is its tid, the words as they are) or a contig
    group (dom <= -2: every position shifted by its contig's voff, position -1 included)"""
    m = np.isin(s["tid"], tids)
    off = s["cpg_off"].astype(np.int64)
    n = np.diff(off)[m]
    sel = np.repeat(m, np.diff(off))
    words, start = s["cpg_pos"][sel].astype(np.int64), s["start"][m].astype(np.int64)
    if voff is not None:
        shift = np.zeros(max(tids) + 1, np.int64)
        shift[tids] = voff
        p = words & 0x7fffffff
        p = np.where(p == 0x7fffffff, -1, p) + np.repeat(shift[s["tid"][m]], n)
        words = (words & 0x80000000) | p
        start = start + shift[s["tid"][m]]
    assert (np.diff(start) >= 0).all()
    new_off = np.r_[0, np.cumsum(n)].astype(np.uint32)
    head = struct.pack("<iI", dom, 0 if voff is None else len(tids))
    if voff is not None:
        head += np.asarray(tids, np.int32).tobytes() + np.asarray(voff, np.int64).tobytes()
    head += struct.pack("<iiII", region[0], region[1], int(m.sum()), int(n.sum()))
    return head + start.astype(np.int32).tobytes() + s["mapq"][m].astype(np.uint8).tobytes() + new_off.tobytes() + words.astype(np.uint32).tobytes()


def model(exe, tmp_path, iv, batches, cap, span, min_cpgs=4, min_qual=10, grid=7):
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    t, b, e = (np.array([x[k] for x in iv], np.int32) for k in range(3))
    inp.write_bytes(struct.pack("<I", len(iv)) + t.tobytes() + b.tobytes() + e.tobytes() + struct.pack("<III", min_cpgs, min_qual, len(batches)) +
                    b"".join(batches))
    r = subprocess.run([exe, str(inp), str(outp), str(cap), "1" if span else "0", str(grid)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.frombuffer(outp.read_bytes(), np.uint64)
    rows = out[:-7].reshape(len(iv), 4).astype(np.int64)
    assert not rows[:, 3].any()                                           # the spare word
    return rows[:, :3], dict(zip(("err", "span", "lds", "direct", "lds_slices", "direct_slices", "pending"), out[-7:].tolist()))


def want_rows(iv, **kw):
    _, m, u, d = U.restate(U.default_calls(), iv, min_depth=1, **kw)
    return np.stack([m, u, d], axis=1)


def forms():
    return [(default_cap(), True), (default_cap(), False), (4, True), (4, False), (0, True), (0, False)]


@pytest.mark.parametrize("batching", ["one_group", "group_and_two_calls"])
def test_the_307_intervals_in_every_form(exe, soa, tmp_path, batching):
    iv = U.intervals()
    assert len(iv) == 307
    if batching == "one_group":
        batches = [batch_bytes(soa, -2, [0, 1], VOFF)]
    else:     # ivA alone in a group, ivB as a plain contig in two calls that own the reads starting in their half
        batches = [batch_bytes(soa, -2, [0], VOFF[:1]), batch_bytes(soa, 1, [1], None, (0, 30_000)), batch_bytes(soa, 1, [1], None, (30_000, U.INT32_MAX))]
    want = want_rows(iv, min_cpgs=4, min_qual=10)
    assert want[:, 2].sum() > 0 and (want > 0).all(axis=1).sum() >= 90
    seen = {}
    for cap, span in forms():
        got, st = model(exe, tmp_path, iv, batches, cap, span)
        assert (got == want).all(), (cap, span, np.nonzero((got != want).any(axis=1))[0][:10])
        assert st["err"] == 0
        seen[cap, span] = st
    # every route was taken where it should be, and only there
    full, off = seen[default_cap(), True], seen[default_cap(), False]
    assert full["span"] > 0 and full["lds"] > 0 and full["direct"] == 0 and off["span"] == 0 and off["lds"] > full["lds"]
    # the whole-contig intervals are their classes' only candidates: a workgroup adds its pending sum once per class it met (3 words
    # each), however many work items it ran -- and the sums are the same with one workgroup per work item or a single one for all
    assert 0 < full["pending"] <= 7 * 3 * 17 and off["pending"] == 0
    for grid in (1, 10 ** 6):
        got, st = model(exe, tmp_path, iv, batches, default_cap(), True, grid=grid)
        assert (got == want).all() and st["pending"] > 0, grid
    assert seen[4, True]["lds"] > 0 and seen[4, True]["direct"] > 0
    assert seen[0, True]["lds"] == 0 and seen[0, True]["lds_slices"] == 0 and seen[0, False]["span"] == 0 and seen[0, False]["direct"] > 0


@pytest.mark.parametrize("kw", [dict(min_cpgs=1, min_qual=0), dict(min_cpgs=9, min_qual=10), dict(min_cpgs=0, min_qual=43)], ids=["p1_q0", "p9_q10", "p0_q43"])
def test_parameters(exe, soa, tmp_path, kw):
    iv = U.intervals()
    want = want_rows(iv, **kw)
    assert (want.sum() == 0) == (kw["min_qual"] == 43)
    for cap, span in ((default_cap(), True), (4, False)):
        got, _ = model(exe, tmp_path, iv, [batch_bytes(soa, -2, [0, 1], VOFF)], cap, span, **kw)
        assert (got == want).all(), (cap, span)


def test_nesting_deeper_than_the_cap(exe, soa, tmp_path):
    cap = default_cap()
    iv = U.deep_nesting(cap) + [(0, 0, U.REFS[0][1], "whole")]
    assert len(iv) - 1 > cap
    want = want_rows(iv, min_cpgs=4, min_qual=10)
    assert (want.sum(axis=1) >= 10).all()
    for c, span in forms():
        got, st = model(exe, tmp_path, iv, [batch_bytes(soa, -2, [0, 1], VOFF)], c, span)
        assert (got == want).all(), (c, span)
        if c == cap:
            assert st["direct_slices"] > 0 and st["direct"] > 0            # more candidates under one workgroup than the cap: direct
            assert st["lds_slices"] > 0                                     # ... and fewer at the set's edges


def test_a_plain_contig_with_the_word_of_minus_one_is_an_error(exe, soa, tmp_path):
    """contig ivA holds a call at position -1: as a plain contig its batch carries the word no batch may carry"""
    _, st = model(exe, tmp_path, U.intervals(), [batch_bytes(soa, 0, [0], None)], default_cap(), True, min_cpgs=1)
    assert st["err"] == 1
