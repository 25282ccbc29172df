"""ME / PM per interval (`metheor me-regions`, `pm-regions`) on the CPU: the restatement of the definition
(tests/quartet_regions_util.py) against the oracle's pinned primitives, against the reference's own known answers (the unit tests of
me.rs and pm.rs) and the host finaliser (mth_regions_host.h) against the f32 expression.  No device."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import quartet_regions_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metheor_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib_finalise():
    from metheor_amd import build, capi
    build.build()
    return capi.quartet_regions_finalise


def reads_of(xms, pos=100, mapq=40, length=100_000):
    """forward reads with one M operation each: the call of byte k of an XM string lies at pos + k"""
    n = len(xms)
    return bamio.Records([("c", length)], [0] * n, [pos] * n, [0] * n, [mapq] * n, [[(len(x) << 4) | 0] for x in xms], [x.encode() for x in xms])


# ---- 1. the definition against pinned code ------------------------------------------------------------------------------------------
def test_restatement_equals_the_route_through_the_oracles_primitives():
    iv, rec = U.intervals(), U.records()
    _, _, n_patterns, n_reads, bins = U.default_expected()
    ks = [k for k in range(0, len(iv), 6) if iv[k][2] - iv[k][1] <= 200_000]      # every 6th interval (the open-ended one is not among them)
    assert len(ks) == 52
    for k in ks:
        t, b, e, _ = iv[k]
        got_bins, got_reads = U.oracle_route(rec, t, b, e, min_qual=10)
        assert (got_bins == bins[k]).all() and got_reads == n_reads[k], iv[k]
    assert sum(1 for k in ks if (bins[k] > 0).all()) >= 20 and sum(1 for k in ks if n_patterns[k] == 0) >= 1


def test_the_set_is_not_vacuous():
    iv = U.intervals()
    me, pm, n_patterns, n_reads, bins = U.default_expected()
    assert len(iv) == 307 and (n_patterns >= 10).sum() == 295 and np.isfinite(me).sum() == 295 and np.isfinite(pm).sum() == 295
    assert (bins > 0).all(axis=1).sum() == 178
    s = pyoracle.Reads.decode(U.records()).soa()
    assert len(s["tid"]) == 52_534 and (np.diff(s["cpg_off"].astype(np.int64)) > 18).sum() == 2_850      # reads beyond the packed histogram
    named = {name: k for k, (_, _, _, name) in enumerate(iv) if name}
    k = named["empty"]
    assert n_patterns[k] == 0 and n_reads[k] == 0 and np.isnan(me[k]) and np.isnan(pm[k])
    k = named["long_reads"]                                # the two reads of 100 calls hold 97 windows each
    assert n_patterns[k] >= 2 * 97
    assert (n_patterns >= n_reads).all() and ((n_reads > 0) == (n_patterns > 0)).all()
    assert (me[np.isfinite(me)] >= 0).all() and (me[np.isfinite(me)] <= 1).all() and (pm[np.isfinite(pm)] < 1).all()


def test_one_pattern_everywhere_gives_negative_zero():
    """every window of every read is 1111: p = 1, log2(p) = 0, me = 0 * -0.25 -- the reference prints "-0" """
    rec = reads_of(["Z.Z.Z.Z.Z.Z"] * 3)
    bins, n_reads = U.counts_of(U.Calls(rec), 0, 0, 1000)
    assert bins.tolist() == [0] * 15 + [9] and n_reads == 3
    me, pm, n = U.finalise(bins, min_depth=1)
    assert n == 9 and me == 0 and np.signbit(me) and pyoracle.format_f32(me) == "-0"
    assert pm == 0 and not np.signbit(pm) and pyoracle.format_f32(pm) == "0"
    ob, orr = U.oracle_route(rec, 0, 0, 1000)
    assert (ob == bins).all() and orr == 3
    text = U.table_text([(0, 0, 1000, "mono")], np.array([me]), np.array([n]), np.array([n_reads]), names=["c"])
    assert text == U.HEADER_ME + "c\t0\t1000\tmono\t-0\t9\t3\n"


def test_a_read_split_by_an_edge_into_3_and_5():
    """eight calls at 100, 102, ... 114; the edge at 106 leaves three on one side (no window) and five on the other (two windows)"""
    rec = reads_of(["Z.z.Z.Z.z.Z.z.z"])
    c = U.Calls(rec)
    assert c.pos.tolist() == list(range(100, 116, 2))
    left, n_left = U.counts_of(c, 0, 0, 106)
    right, n_right = U.counts_of(c, 0, 106, 1000)
    assert left.sum() == 0 and n_left == 0
    # kept: Z z Z z z -> 1010 and 0100
    assert n_right == 1 and right.sum() == 2 and right[0b1010] == 1 and right[0b0100] == 1
    for b, e, want, wr in ((0, 106, left, 0), (106, 1000, right, 1)):
        ob, orr = U.oracle_route(rec, 0, b, e)
        assert (ob == want).all() and orr == wr
    whole, _ = U.counts_of(c, 0, 0, 1000)
    assert whole.sum() == 5                                 # the windows across the edge are in neither part
    low, n_low = U.counts_of(c, 0, 0, 1000, min_qual=41)     # mapq 40: the read does not contribute
    assert low.sum() == 0 and n_low == 0


# ---- 2. the reference's known answers -----------------------------------------------------------------------------------------------
KNOWN = {1: (1.0, 0.9375, 16), 2: (0.25, 0.5, None), 3: (0.25, 0.5, None)}      # me.rs / pm.rs tests 1-3: the file's single quartet


@pytest.mark.parametrize("k", range(1, 7))
def test_reference_fixtures(k):
    rec = bamio.read_bam(os.path.join(GOLDEN, "test%d.bam" % k))
    c = U.Calls(rec)
    bins, n_reads = U.counts_of(c, 0, 0, U.INT32_MAX)
    me, pm, n = U.finalise(bins, min_depth=0)
    table = pyoracle.Reads.decode(rec).me(min_depth=0, min_qual=10)
    assert (bins == (table.cnt.astype(np.int64).sum(axis=0) if len(table) else 0)).all()      # the whole contig pools every quartet
    if k in KNOWN:
        wme, wpm, depth = KNOWN[k]
        assert len(table) == 1 and me == np.float32(wme) and pm == np.float32(wpm) and (depth is None or n == depth)
        assert float(table.val[0]) == wme
    elif k == 4:
        # two quartets of ME 1.0 / PM 0.9375 each (me.rs test4): an interval over one quartet gives that value ...
        assert len(table) == 2
        for row in table.pos.tolist():
            b1, n1 = U.counts_of(c, 0, row[0], row[3] + 1)
            m1, p1, _ = U.finalise(b1, min_depth=0)
            assert m1 == np.float32(1.0) and p1 == np.float32(1.0 - 16.0 * (1.0 / 16.0) * (1.0 / 16.0)) and n1 > 0
        # ... and the whole contig the pooled one
        assert n == int(table.cnt.sum()) and np.isfinite(me) and np.isfinite(pm)
    elif k == 5:
        assert len(table) == 0 and n == 0 and n_reads == 0 and np.isnan(me) and np.isnan(pm)      # no read passes the quality cutoff
    else:
        assert n == int(table.cnt.sum()) and (n > 0) == (n_reads > 0)


# ---- 3. the host finaliser ----------------------------------------------------------------------------------------------------------
def finalise_cases():
    rng = np.random.default_rng(9)
    cases = [([0] * 16, 0), ([0] * 16, 1), ([1] + [0] * 15, 0), ([1] + [0] * 15, 2), ([0] * 15 + [9], 1), ([1] * 16, 10), ([3] * 16, 49),
             ([2 ** 24 + 1] + [3] * 15, 10), ([2 ** 32 + 5, 7] + [0] * 14, 10), ([2 ** 32 + 5] * 16, 2 ** 32 - 1)]
    cases += [(rng.integers(0, 1000, 16).tolist(), 10) for _ in range(40)]
    cases += [((rng.integers(0, 50, 16) * (rng.random(16) < 0.4)).tolist(), 10) for _ in range(40)]
    return cases


def check_values(got, want, what):
    me, pm, n = got
    wme, wpm, wn = want
    assert n == wn, what
    assert U.same_bits([pm], [wpm]), what
    assert np.isnan(me) == np.isnan(wme) and (np.isnan(wme) or (abs(float(me) - float(wme)) <= 1e-6 and np.signbit(me) == np.signbit(wme))), what


def test_host_finaliser_equals_the_f32_expression(lib_finalise):
    _, _, _, _, bins = U.default_expected()
    for k in range(len(bins)):
        check_values(lib_finalise(bins[k], 10), U.finalise(bins[k], 10), k)
    for b, depth in finalise_cases():
        check_values(lib_finalise(b, depth), U.finalise(b, depth), (b, depth))
    me, pm, n = lib_finalise([0] * 15 + [9], 1)
    assert me == 0 and np.signbit(me) and pm == 0 and n == 9
    me, pm, n = lib_finalise([1] * 16, 17)
    assert np.isnan(me) and np.isnan(pm) and n == 16                        # below depth: NaN, the count is still reported
    assert lib_finalise([1] * 16, 16)[:2] == (np.float32(1.0), np.float32(0.9375))


DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "mth_regions_host.h"
int main() {
    unsigned long long b[16];
    unsigned depth;
    for (;;) {
        for (int k = 0; k < 16; ++k) if (scanf("%llu", &b[k]) != 1) return 0;
        if (scanf("%u", &depth) != 1) return 0;
        uint64_t bins[16], n = 0;
        for (int k = 0; k < 16; ++k) bins[k] = b[k];
        float me, pm;
        mth::quartet_regions_finalise(bins, depth, &me, &pm, &n);
        uint32_t mb, pb;
        memcpy(&mb, &me, 4); memcpy(&pb, &pm, 4);
        printf("%u %u %llu\n", mb, pb, (unsigned long long)n);
    }
}
"""


def test_host_header_compiles_alone_with_plain_cxx(tmp_path):
    src = tmp_path / "fin.cpp"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", str(tmp_path / "fin"), str(src)])
    cases = finalise_cases()[:20]
    text = "".join(" ".join(str(x) for x in b) + " %d\n" % d for b, d in cases)
    out = subprocess.run([str(tmp_path / "fin")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for line, (b, d) in zip(out, cases):
        mb, pb, n = (int(x) for x in line.split())
        got = (np.array([mb], np.uint32).view(np.float32)[0], np.array([pb], np.uint32).view(np.float32)[0], n)
        check_values(got, U.finalise(b, d), (b, d))
