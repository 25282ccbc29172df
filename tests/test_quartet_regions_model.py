"""The per-interval ME / PM pass on the CPU, before any device is there.  metheor_amd/csrc/mth_quartet_regions_dev.h -- the per-lane part
of k_quartet_regions: the summary of a read with its packed pattern histogram, the whole / partial decision, the rolling walk --
compiles under MTH_QUARTET_REGIONS_HOST_MODEL into a stand-alone program (its own main, g++ with the address and undefined-behaviour
sanitizers) that plays the kernel work item by work item around it: 256 reads at a time, the candidate range of every slice of the
batch's domain (mth_regions_host.h, the library's own copy), the LDS rows as bounds-checked arrays of exactly the cap's size, the
carried row of a class with a single candidate, the direct route.  Its counts must equal the numpy restatement
(tests/quartet_regions_util.py) on every interval, in every form."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import pdr_regions_util as P
from tests import quartet_regions_util as U
from tests.test_pdr_regions_model import VOFF, batch_bytes

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#define MTH_QUARTET_REGIONS_HOST_MODEL
#include "mth_quartet_regions_dev.h"
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

// argv: input, output, LDS cap, packed summary (0 / 1), carried row (0 / 1), workgroups (work item ch goes to workgroup ch mod that),
// calls a carried row may take before it is flushed (0: the kernel's 2^31).  IN: n, tid / beg / end of the intervals, min_qual,
// batches; per batch dom, n_contigs, tids, voff (int64), region_beg, region_end, n_reads, n_cpgs, read_start, read_mapq, cpg_off,
// cpg_pos.  OUT: per interval seventeen u64 words, then u64 stats: error flag, adds to LDS rows, adds to memory directly, slices that
// used LDS rows, slices that went direct, slices that met a carried row, flushes of carried rows, entries taken from a packed summary,
// entries walked, the largest 32-bit word an LDS row held
int main(int argc, char **argv) {
    if (argc != 8) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    const int32_t cap = atoi(argv[3]);
    const bool summary = atoi(argv[4]) != 0, carry_knob = atoi(argv[5]) != 0;
    const uint32_t grid = (uint32_t)atoi(argv[6]);
    const uint32_t carry_max = atoi(argv[7]) ? (uint32_t)atoi(argv[7]) : QR_CARRY_CALLS_MAX;
    constexpr int CARRY = IvDomains::NCLS;
    constexpr int B = 256;
    const uint32_t n_iv = take_u32(f);
    const std::vector<int32_t> tid = take<int32_t>(f, n_iv), beg = take<int32_t>(f, n_iv), end = take<int32_t>(f, n_iv);
    const uint32_t min_qual = take_u32(f), n_batches = take_u32(f);
    IvDomains dm(n_iv, tid.data(), beg.data(), end.data());
    std::vector<uint64_t> rows((size_t)n_iv * QR_ROW, 0);
    uint64_t stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> s_rows((size_t)cap * QR_ROW);                  // the LDS of a workgroup: exactly the cap
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
        const bool carry = carry_knob && sl.second - sl.first <= (uint32_t)CARRY;
        for (uint32_t wg = 0; wg < std::min(grid, n_chunks); ++wg) {
        // the workgroup's carried rows: per slice its single candidate, the row not yet in memory, the calls it has taken
        std::vector<uint32_t> s_carry((size_t)CARRY * QR_ROW, 0u), s_cn(CARRY, 0u);
        std::vector<int32_t> s_cj(CARRY, -1);
        auto carry_flush = [&](int k, int32_t j) {
            for (int w = 0; w < QR_ROW; ++w) {
                const uint32_t v = s_carry.at((size_t)k * QR_ROW + w);
                if (j >= 0 && v) rows.at((size_t)dm.e_out.at(j) * QR_ROW + w) += v;
                s_carry.at((size_t)k * QR_ROW + w) = 0u;
            }
            if (j >= 0) stats[6] += 1;
        };
        for (uint32_t ch = wg; ch < n_chunks; ch += grid) {
            QrRead rd[B];
            bool elig[B];
            int32_t wmin = INT32_MAX, wmax = -1;
            uint32_t item_calls = 0;
            for (int t = 0; t < B; ++t) {
                const uint32_t r = ch * B + (uint32_t)t;
                elig[t] = false;
                rd[t].k0 = rd[t].k1 = 0; rd[t].first = INT32_MAX; rd[t].last = -1; rd[t].packed = 0; rd[t].packed_ok = false;
                if (r >= n_reads) continue;
                const int32_t rs = read_start.at(r);
                if (!(rs >= region_beg && rs < region_end && read_mapq.at(r) >= min_qual)) continue;
                const uint32_t k0 = cpg_off.at(r), k1 = cpg_off.at(r + 1);
                if (!(k1 > k0 && k1 <= n_cpgs && k1 - k0 >= QR_NEED)) continue;
                elig[t] = qr_summary(cpg_pos.data(), k0, k1, rd[t]);
                if (!elig[t]) { stats[0] = 1; rd[t].first = INT32_MAX; rd[t].last = -1; continue; }
                wmin = std::min(wmin, rd[t].first); wmax = std::max(wmax, rd[t].last);
                item_calls += qr_lane_calls(k0, k1);
            }
            if (wmax < 0) continue;
            const bool small = item_calls < QR_LANE_CALLS_MAX;
            for (uint32_t s = sl.first; s < sl.second; ++s) {
                const int32_t lo = dm.s_beg.at(s), hi = dm.s_end.at(s);
                const int32_t w_hi = upper(dm.e_start, lo, hi, wmax);
                if (w_hi == lo) continue;
                const int32_t w_min = upper(dm.e_maxend, lo, w_hi, wmin);
                if (w_min == w_hi) continue;
                const int32_t acc_n = w_hi - w_min;
                const bool use_lds = small && acc_n <= cap;
                const bool carried = use_lds && carry && acc_n == 1;
                uint32_t *base = s_rows.data();
                size_t base_n = s_rows.size();
                if (carried) {
                    const int k = (int)(s - sl.first);
                    const bool flush = s_cj.at(k) != w_min || s_cn.at(k) + item_calls >= carry_max;
                    if (flush) carry_flush(k, s_cj.at(k));
                    s_cn.at(k) = (flush ? 0u : s_cn.at(k)) + item_calls;
                    s_cj.at(k) = w_min;
                    base = s_carry.data() + (size_t)k * QR_ROW; base_n = QR_ROW;
                    stats[5] += 1;
                } else if (use_lds) {
                    for (int32_t i = 0; i < acc_n * QR_ROW; ++i) s_rows.at(i) = 0u;
                    stats[3] += 1;
                } else stats[4] += 1;
                for (int t = 0; t < B; ++t) {
                    if (!elig[t]) continue;
                    for (int32_t j = upper(dm.e_start, w_min, w_hi, rd[t].last) - 1; j >= w_min && dm.e_maxend.at(j) > rd[t].first; --j) {
                        const int32_t ie = dm.e_end.at(j);
                        if (ie <= rd[t].first) continue;
                        const int32_t ib = dm.e_start.at(j);
                        stats[summary && rd[t].packed_ok && ib <= rd[t].first && rd[t].last < ie ? 7 : 8] += 1;
                        qr_entry(cpg_pos.data(), rd[t], ib, ie, summary, [&](uint32_t w, uint32_t v) {
                            if (w >= (uint32_t)QR_ROW || v == 0) abort();
                            if (use_lds) {
                                const size_t at = (size_t)(j - w_min) * QR_ROW + w;
                                if (at >= base_n) abort();                                   // a row beyond the LDS there is
                                if (base[at] > 0x7fffffffu - v) abort();                     // a 32-bit word about to pass 2^31
                                base[at] += v; stats[1] += 1;
                                stats[9] = std::max<uint64_t>(stats[9], base[at]);
                            } else { rows.at((size_t)dm.e_out.at(j) * QR_ROW + w) += v; stats[2] += 1; }
                        });
                    }
                }
                if (!use_lds || carried) continue;
                for (int32_t i = 0; i < acc_n * QR_ROW; ++i) {
                    const uint32_t v = s_rows.at(i);
                    if (v) rows.at((size_t)dm.e_out.at(w_min + i / QR_ROW) * QR_ROW + (uint32_t)(i % QR_ROW)) += v;
                }
            }
        }
        for (int k = 0; k < CARRY; ++k) carry_flush(k, s_cj.at(k));
        }
    }
    if (fwrite(rows.data(), 8, rows.size(), o) != rows.size() || fwrite(stats, 8, 10, o) != 10) return 2;
    fclose(o);
    return 0;
}
"""

STATS = ("err", "lds", "direct", "lds_slices", "direct_slices", "carried_slices", "carry_flushes", "packed", "walked", "max_word")


def default_cap():
    text = open(os.path.join(CSRC, "mth_knobs.h")).read()
    return int(re.search(r"constexpr int QUARTET_REGIONS_LDS_CAP = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("quartet_regions_model")
    src = d / "quartet_regions_model.cpp"
    src.write_text(DRIVER)
    out = d / "quartet_regions_model"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


@pytest.fixture(scope="module")
def soa():
    return pyoracle.Reads.decode(U.records()).soa()


def model(exe, tmp_path, iv, batches, cap, summary=True, carry=True, min_qual=10, grid=7, carry_max=0):
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    t, b, e = (np.array([x[k] for x in iv], np.int32) for k in range(3))
    inp.write_bytes(struct.pack("<I", len(iv)) + t.tobytes() + b.tobytes() + e.tobytes() + struct.pack("<II", min_qual, len(batches)) + b"".join(batches))
    r = subprocess.run([exe, str(inp), str(outp), str(cap), "1" if summary else "0", "1" if carry else "0", str(grid), str(carry_max)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.frombuffer(outp.read_bytes(), np.uint64)
    return out[:-10].reshape(len(iv), 17).astype(np.int64), dict(zip(STATS, out[-10:].tolist()))


def want_rows(iv, calls=None, min_qual=10):
    _, _, _, n_reads, bins = U.restate(calls or U.default_calls(), iv, min_depth=1, min_qual=min_qual)
    return np.concatenate([bins, n_reads[:, None]], axis=1)


def forms():
    """(cap, packed summary, carried row): the default and the differential forms"""
    d = default_cap()
    return [(d, True, True), (d, False, True), (d, True, False), (4, True, True), (4, False, False), (0, True, True), (0, False, True)]


@pytest.mark.parametrize("batching", ["one_group", "group_and_two_calls"])
def test_the_307_intervals_in_every_form(exe, soa, tmp_path, batching):
    iv = U.intervals()
    assert len(iv) == 307
    if batching == "one_group":
        batches = [batch_bytes(soa, -2, [0, 1], VOFF)]
    else:     # ivA alone in a group, ivB as a plain contig in two calls that own the reads starting in their half
        batches = [batch_bytes(soa, -2, [0], VOFF[:1]), batch_bytes(soa, 1, [1], None, (0, 30_000)), batch_bytes(soa, 1, [1], None, (30_000, U.INT32_MAX))]
    want = want_rows(iv)
    assert (want[:, :16] > 0).all(axis=1).sum() == 178 and (want[:, :16].sum(axis=1) >= 10).sum() == 295
    seen = {}
    for cap, summary, carry in forms():
        got, st = model(exe, tmp_path, iv, batches, cap, summary, carry)
        assert (got == want).all(), (cap, summary, carry, np.nonzero((got != want).any(axis=1))[0][:10])
        assert st["err"] == 0
        seen[cap, summary, carry] = st
    d = default_cap()
    full, no_sum, no_carry = seen[d, True, True], seen[d, False, True], seen[d, True, False]
    # every route was taken where it should be, and only there
    assert full["lds"] > 0 and full["direct"] == 0 and full["packed"] > 0 and full["walked"] > 0      # (reads of more than 18 calls, partial overlaps)
    assert no_sum["packed"] == 0 and no_sum["walked"] == full["packed"] + full["walked"] and no_sum["lds"] > full["lds"]
    # the whole-contig intervals are their classes' only candidates: a workgroup carries their rows from work item to work item and
    # adds each at most once per class and workgroup -- not once per work item
    assert full["carried_slices"] > 7 * 17 >= full["carry_flushes"] > 0
    assert no_carry["carried_slices"] == 0 and no_carry["carry_flushes"] == 0 and no_carry["lds_slices"] == full["lds_slices"] + full["carried_slices"]
    for grid in (1, 10 ** 6):
        got, st = model(exe, tmp_path, iv, batches, d, grid=grid)
        assert (got == want).all() and st["carry_flushes"] > 0, grid
    assert seen[4, True, True]["lds"] > 0 and seen[4, True, True]["direct"] > 0
    for k in ((0, True, True), (0, False, True)):
        assert seen[k]["lds"] == 0 and seen[k]["lds_slices"] == 0 and seen[k]["carried_slices"] == 0 and seen[k]["direct"] > 0


def test_a_carried_row_is_flushed_before_its_words_could_overflow(exe, soa, tmp_path):
    """with the limit lowered to 5000 calls the carried rows go to memory every few work items: the sums are the same, no word of a
    carried row ever holds more than the calls it has taken, and the model aborts on a word about to pass 2^31"""
    iv = U.intervals()
    want = want_rows(iv)
    batches = [batch_bytes(soa, -2, [0, 1], VOFF)]
    got, st = model(exe, tmp_path, iv, batches, default_cap(), grid=1, carry_max=5000)
    _, ref = model(exe, tmp_path, iv, batches, default_cap(), grid=1)
    assert (got == want).all()
    # whole_a's row takes the calls of every eligible read of ivA, fewer than 5000 between two flushes
    n = np.diff(soa["cpg_off"].astype(np.int64))
    calls_a = int(n[(soa["tid"] == 0) & (soa["mapq"] >= 10) & (n >= 4)].sum())
    assert calls_a > 40 * 5000
    assert st["carry_flushes"] >= -(-calls_a // 5000) - 1 > ref["carry_flushes"] and st["max_word"] < 5000 <= ref["max_word"]


@pytest.mark.parametrize("min_qual", [0, 43])
def test_parameters(exe, soa, tmp_path, min_qual):
    iv = U.intervals()
    want = want_rows(iv, min_qual=min_qual)
    assert (want.sum() == 0) == (min_qual == 43)
    for cap, summary, carry in ((default_cap(), True, True), (4, False, False)):
        got, _ = model(exe, tmp_path, iv, [batch_bytes(soa, -2, [0, 1], VOFF)], cap, summary, carry, min_qual=min_qual)
        assert (got == want).all(), (cap, summary, carry)


@pytest.mark.parametrize("cap", [0, 4, None], ids=["cap_0", "cap_4", "default_cap"])
def test_nesting_deeper_than_the_cap(exe, soa, tmp_path, cap):
    cap = default_cap() if cap is None else cap
    iv = P.deep_nesting(max(cap, 4)) + [(0, 0, U.REFS[0][1], "whole")]
    assert len(iv) - 1 > cap
    want = want_rows(iv)
    assert (want[:, :16].sum(axis=1) >= 10).all()
    for summary, carry in ((True, True), (False, False)):
        got, st = model(exe, tmp_path, iv, [batch_bytes(soa, -2, [0, 1], VOFF)], cap, summary, carry)
        assert (got == want).all(), (cap, summary, carry)
        assert st["direct_slices"] > 0 and st["direct"] > 0                # more candidates under one workgroup than the cap: direct
        assert (st["lds_slices"] > 0) == (cap > 0)                         # ... and fewer at the set's edges


def test_calls_in_descending_order(exe, tmp_path):
    """the calls of every read reversed within the read (a batch may carry them in any order of position): the windows follow the
    call order, the extremes come from min / max"""
    s = pyoracle.Reads.decode(U.records()).soa()
    off = s["cpg_off"].astype(np.int64)
    words = s["cpg_pos"].copy()
    for a, b in zip(off[:-1], off[1:]):
        words[a:b] = words[a:b][::-1]
    rev = dict(s, cpg_pos=words)
    c = U.default_calls()
    rc = U.Calls.__new__(U.Calls)
    rc.__dict__.update(c.__dict__)
    p = (words & 0x7fffffff).astype(np.int64)
    rc.pos, rc.meth = np.where(p == 0x7fffffff, -1, p), (words >> 31).astype(bool)
    iv = U.intervals()
    want = want_rows(iv, calls=rc)
    assert (want != want_rows(iv)).any() and (want[:, 16] == want_rows(iv)[:, 16]).all()      # other patterns, the same reads
    for cap, summary, carry in ((default_cap(), True, True), (4, False, True)):
        got, st = model(exe, tmp_path, iv, [batch_bytes(rev, -2, [0, 1], VOFF)], cap, summary, carry)
        assert (got == want).all() and st["err"] == 0, (cap, summary, carry)


def minus_one_soa():
    """two reads of contig 0 with five calls each; the first one's first call is at position -1 (the word 0x7fffffff)"""
    words = np.array([0x7fffffff, 3 | 1 << 31, 8, 12, 20, 10, 12 | 1 << 31, 14, 16, 18], np.uint32)
    return dict(tid=np.zeros(2, np.int32), start=np.array([0, 10], np.int32), mapq=np.full(2, 40, np.uint8),
                cpg_off=np.array([0, 5, 10], np.uint64), cpg_pos=words)


def test_a_plain_contig_with_the_word_of_minus_one_is_an_error(exe, soa, tmp_path):
    """the reads of the default set that call at -1 hold three calls, too few for this pass to look at: a read of five calls with that
    word, in a plain contig's batch, which may not carry it -- and as a contig group, shifted by one, it is an ordinary call"""
    s = minus_one_soa()
    iv = [(0, 0, 100, "all")]
    _, st = model(exe, tmp_path, iv, [batch_bytes(s, 0, [0], None)], default_cap())
    assert st["err"] == 1
    got, st = model(exe, tmp_path, iv, [batch_bytes(s, -2, [0], VOFF[:1])], default_cap())
    assert st["err"] == 0 and got[0, 16] == 2 and got[0, :16].sum() == 3       # the call at -1 lies in no interval: 4 kept calls, 1 window; and 2
    _, st = model(exe, tmp_path, U.intervals(), [batch_bytes(soa, 0, [0], None)], default_cap(), min_qual=0)
    assert st["err"] == 0
