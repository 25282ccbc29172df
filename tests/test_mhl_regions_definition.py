"""MHL per interval (`metheor mhl-regions`) on the CPU: the restatement of the definition
(tests/mhl_regions_util.py) against the oracle's pinned primitives, against the reference's own known answers, against the per-CpG
oracle where an interval is small enough for the two to coincide, and the host finaliser (mth_regions_host.h) against the restatement.
No device."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import mhl_regions_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metheor_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
KNOWN = [0.1625, 0.5, 0.5, 0.1625, np.nan, 0.5]          # mhl.rs's unit tests for test1..test5; test6: the oracle's per-CpG value


def rows_of(R, C):
    """the histograms as the sparse rows the library hands out: ascending lengths with runs or reads"""
    top = max(len(R), len(C))
    ln = [l for l in range(1, top) if (l < len(R) and R[l]) or (l < len(C) and C[l])]
    return ln, [int(R[l]) if l < len(R) else 0 for l in ln], [int(C[l]) if l < len(C) else 0 for l in ln]


@pytest.fixture(scope="module")
def lib_finalise():
    from metheor_amd import build, capi
    build.build()
    return capi.mhl_regions_finalise


# ---- 1. the definition against pinned code ------------------------------------------------------------------------------------------
def pinned_set():
    iv = U.intervals()
    named = {n: k for k, (_, _, _, n) in enumerate(iv) if n}
    must = ["nest_outer", "whole_a", "whole_b_open_end", "after_minus_one", "first_base", "empty", "no_reads", "read_exact", "cut_after_first",
            "cut_before_last", "end_on_a_call", "end_past_a_call", "start_on_a_call", "start_past_a_call", "long_reads", "long_run_70",
            "long_tail_70_calls", "deletion", "insertion", "nest_mid", "nest_inner", "twin", "slide_66000", "slide_65500", "hub_0", "hub_3"]
    ks = [named[n] for n in must] + list(range(0, 200, 12)) + list(range(200, 260, 9))
    return sorted(set(ks))


def test_restatement_equals_the_route_through_the_oracles_primitives():
    iv, rec = U.intervals(), U.records()
    mhl, n_reads, max_cpgs = U.default_expected()
    ks = pinned_set()
    assert len(ks) >= 40
    for k in ks:
        t, b, e, _ = iv[k]
        v, n, mx = U.oracle_route(rec, t, b, e, **U.DEFAULT_KW)
        assert U.same_bits([v], [mhl[k]]) and n == n_reads[k] and (mx == max_cpgs[k] or n == 0), (iv[k], v, mhl[k], n, n_reads[k])
    assert np.isfinite(mhl[ks]).sum() >= 30


def test_every_interval_is_below_2_24_and_equals_the_read_order_denominator():
    """the reference adds its denominator in f32 read by read: exact, and the same bits as the integer converted once, while the
    interval's sum of n stays below 2^24 -- which every interval of the set does, so the claim is never vacuous"""
    c, iv = U.default_calls(), U.intervals()
    mhl, _, _ = U.default_expected()
    for k, (t, b, e, _) in enumerate(iv):
        R, C, n_list = U.histograms(c, t, b, e, U.DEFAULT_KW["min_cpgs"], U.DEFAULT_KW["min_qual"])
        assert int(n_list.sum()) < 2 ** 24
        top = max(len(R), len(C)) - 1
        v, _, _ = U.finalise(R, C, U.DEFAULT_KW["min_depth"], denominators=U.read_order_denominators(n_list, top))
        assert U.same_bits([v], [mhl[k]]), iv[k]


# ---- 2. the reference's known answers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 7))
def test_reference_fixtures(k, lib_finalise):
    rec = bamio.read_bam(os.path.join(GOLDEN, "test%d.bam" % k))
    c = U.Calls(rec)
    R, C, _ = U.histograms(c, 0, 0, U.INT32_MAX, min_cpgs=1, min_qual=10)
    want = np.float32(KNOWN[k - 1])
    v, n, _ = U.finalise(R, C, min_depth=1)
    assert U.same_bits([v], [want]), (k, v)
    got, n_lib, _ = lib_finalise(*rows_of(R, C), min_depth=1)
    assert U.same_bits([got], [want]) and n_lib == n, (k, got)
    if k == 6:        # mhl.rs has no unit test for it: the value is what the oracle's per-CpG mhl writes for every CpG of the file
        t = pyoracle.Reads.decode(rec).mhl(min_depth=1, min_cpgs=1, min_qual=10)
        assert len(t) > 0 and (t.val.view(np.uint32) == want.view(np.uint32)).all()


# ---- 3. hub check against the per-CpG oracle -----------------------------------------------------------------------------------------
def test_small_intervals_equal_the_per_cpg_oracle():
    """an interval with at most 12 called positions, under -p set to that count: every contributing read holds every CpG of the
    interval, so each CpG's AssociatedReads is the interval's and every row `mhl -c <the interval's positions>` writes is its value"""
    c, iv, rec = U.default_calls(), U.intervals(), U.records()
    hit, names = 0, []
    for t, b, e, name in iv:
        idx = c.by_tid.get(t, np.zeros(0, np.int64))
        pos = np.unique(c.pos[idx][(c.pos[idx] >= b) & (c.pos[idx] < e)])
        if not 1 <= len(pos) <= 12:
            continue
        p = len(pos)
        R, C, _ = U.histograms(c, t, b, e, min_cpgs=p, min_qual=10)
        v, n, _ = U.finalise(R, C, min_depth=10)
        table = pyoracle.Reads.decode(rec, cpg_set=[(t, int(q)) for q in pos]).mhl(min_depth=10, min_cpgs=p, min_qual=10)
        if n >= 10:
            assert len(table) > 0
        if len(table):
            assert n >= 1 and (table.val.view(np.uint32) == np.float32(v).view(np.uint32)).all(), (t, b, e, name, v, table.val)
            hit += 1
            names.append(name)
    assert hit >= 5 and "after_minus_one" in names, names


# ---- 4. the host finaliser alone -------------------------------------------------------------------------------------------------------
def test_host_finaliser_equals_the_restatement(lib_finalise):
    c, iv = U.default_calls(), U.intervals()
    for kw in (U.DEFAULT_KW, dict(min_depth=1, min_cpgs=1, min_qual=0)):
        mhl, n_reads, max_cpgs = U.restate(c, iv, **kw)
        for k, (t, b, e, _) in enumerate(iv):
            R, C, _ = U.histograms(c, t, b, e, kw["min_cpgs"], kw["min_qual"])
            v, n, mx = lib_finalise(*rows_of(R, C), min_depth=kw["min_depth"])
            assert U.same_bits([v], [mhl[k]]) and n == n_reads[k] and mx == max_cpgs[k], (iv[k], v, mhl[k])
    v, n, mx = lib_finalise([], [], [], min_depth=0)
    assert np.isnan(v) and n == 0 and mx == 0                          # an empty histogram: NaN, also at depth 0
    v, n, mx = lib_finalise([3], [0], [9], min_depth=10)
    assert np.isnan(v) and n == 9 and mx == 3                          # below depth: NaN, the actual reads and their largest n
    v, _, _ = lib_finalise([3], [0], [10], min_depth=10)
    assert v == 0.0                                                     # deep enough, nothing methylated


DRIVER = r"""
#include <cstdio>
#include "mth_regions_host.h"
// stdin: n, then n rows "length runs reads"; stdout: the value's bits, n_reads, max_cpgs
int main() {
    unsigned long long n;
    if (scanf("%llu", &n) != 1) return 2;
    std::vector<uint32_t> len(n);
    std::vector<uint64_t> runs(n), reads(n);
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned long long a, b;
        if (scanf("%u %llu %llu", &len[i], &a, &b) != 3) return 2;
        runs[i] = a; reads[i] = b;
    }
    uint64_t nr = 0;
    uint32_t mx = 0;
    const float v = mth::mhl_regions_finalise(n, len.data(), runs.data(), reads.data(), 10, &nr, &mx);
    uint32_t bits;
    memcpy(&bits, &v, 4);
    printf("%u %llu %u\n", bits, (unsigned long long)nr, mx);
    return 0;
}
"""


def test_host_header_is_pure_and_gives_the_same_bits_as_plain_cxx(tmp_path):
    """mth_regions_host.h compiles alone with a plain C++ compiler, at the compiler's default contraction setting: it includes nothing of
    HIP, reads no environment, and its value on the island is the restatement's"""
    text = open(os.path.join(CSRC, "mth_regions_host.h")).read()
    assert "getenv" not in text and "hip/" not in text and "mth_common.h" not in text and "mth_ctx.h" not in text
    src = tmp_path / "fin.cpp"
    src.write_text("#include <cstring>\n" + DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "fin"), str(src)])
    c, iv = U.default_calls(), U.intervals()
    k = [n for _, _, _, n in iv].index("nest_outer")
    R, C, _ = U.histograms(c, *iv[k][:3])
    ln, ru, re_ = rows_of(R, C)
    out = subprocess.run([str(tmp_path / "fin")], input="%d\n" % len(ln) + "".join("%d %d %d\n" % x for x in zip(ln, ru, re_)),
                         capture_output=True, text=True, check=True).stdout.split()
    mhl, n_reads, max_cpgs = U.default_expected()
    assert int(out[0]) == int(np.float32(mhl[k]).view(np.uint32)) and int(out[1]) == n_reads[k] and int(out[2]) == max_cpgs[k]
