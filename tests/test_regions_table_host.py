"""The packed interval table on the CPU.  IvDomains::pack appends the six arrays of the sorted intervals to a word vector and
IvTabOffsets::at turns the offsets it returns into the pointers a kernel reads (metheor_amd/csrc/mth_regions_host.h): through them
every array must come back element for element, whatever the vector held before.  iv_check_intervals is what every entry point
that takes intervals asks of them.  A stand-alone program (its own main) under the address and undefined-behaviour sanitizers;
it includes nothing but that header."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#include "mth_regions_host.h"
#include <cstdio>
#include <cstdlib>
using namespace mth;

#define WANT(c) do { if (!(c)) { fprintf(stderr, "%s: line %d: %s\n", what, __LINE__, #c); exit(1); } } while (0)

template <class T> static void same(const char *what, const std::vector<T> &v, const T *p) {
    for (size_t i = 0; i < v.size(); ++i) WANT(p[i] == v[i]);
}

// pack behind `before` words of something else, then every array through the offsets; prints the slices of `dom` and the entries
static void round_trip(const char *what, const IvDomains &dm, int32_t dom, size_t before) {
    std::vector<uint32_t> words(before, 0xabad1deau);
    const IvTabOffsets o = dm.pack(words);
    WANT(words.size() == before + 2 * dm.s_beg.size() + 4 * dm.entries());
    for (size_t i = 0; i < before; ++i) WANT(words[i] == 0xabad1deau);
    for (size_t at : {o.s_beg, o.s_end, o.e_start, o.e_end, o.e_maxend, o.e_out}) WANT(at >= before && at <= words.size());
    std::vector<uint32_t> copy(words);                      // the table works at any base that holds the words: here a copy, on the device a buffer
    const IvTab t = o.at(copy.data());
    same(what, dm.s_beg, t.s_beg); same(what, dm.s_end, t.s_end);
    same(what, dm.e_start, t.e_start); same(what, dm.e_end, t.e_end); same(what, dm.e_maxend, t.e_maxend);
    same(what, dm.e_out, t.e_out);
    const auto sl = dm.dom_slices.at(dom);
    for (uint32_t s = sl.first; s < sl.second; ++s) {
        WANT(t.s_beg[s] < t.s_end[s] && (size_t)t.s_end[s] <= dm.entries());
        for (int32_t j = t.s_beg[s]; j < t.s_end[s]; ++j) {
            WANT(t.e_start[j] < t.e_end[j] && t.e_end[j] <= t.e_maxend[j]);
            if (j > t.s_beg[s]) WANT(t.e_start[j - 1] <= t.e_start[j] && t.e_maxend[j - 1] <= t.e_maxend[j]);
        }
    }
    printf("%s %u %zu\n", what, sl.second - sl.first, dm.entries());
}

int main() {
    // five intervals on contig 0 in three length classes (one empty interval holds nothing), two on contig 1, one on contig 3
    const std::vector<int32_t> tid = {0, 0, 1, 0, 0, 0, 1, 0, 3}, beg = {100, 0, 5, 40, 120, 7, 0, 90, 10},
                               end = {200, 1000000, 9, 40, 260, 9, 300, 95, 20};
    {
        IvDomains dm(tid.size(), tid.data(), beg.data(), end.data());
        dm.add_domain(0);
        round_trip("contig", dm, 0, 0);
        dm.add_domain(1);                                   // a second domain behind the first, the table behind other words
        round_trip("contig_then_contig", dm, 1, 7);
    }
    {   // contigs 0 and 1 as one group: contig 1 at voff 2000, so contig 0's long interval is cut at 1999 (the word before contig 1)
        const int32_t g_tids[2] = {0, 1};
        const int64_t g_voff[2] = {1, 2000};
        IvDomains dm(tid.size(), tid.data(), beg.data(), end.data());
        dm.add_domain(-2, 2, g_tids, g_voff);
        const char *what = "group";
        bool cut = false, shifted = false;
        for (size_t j = 0; j < dm.entries(); ++j) {
            cut |= dm.e_out[j] == 1 && dm.e_start[j] == 1 && dm.e_end[j] == 1999;
            shifted |= dm.e_out[j] == 6 && dm.e_start[j] == 2000 && dm.e_end[j] == 2300;
        }
        WANT(cut && shifted);
        round_trip(what, dm, -2, 3);
    }
    {
        IvDomains dm(tid.size(), tid.data(), beg.data(), end.data());
        dm.add_domain(2);                                   // no interval on the batch's contig
        round_trip("nothing_here", dm, 2, 0);
        round_trip("nothing_here_behind_words", dm, 2, 5);
    }
    {
        IvDomains dm(0, nullptr, nullptr, nullptr);
        dm.add_domain(0);
        round_trip("no_intervals", dm, 0, 2);
    }
    const char *what = "check";
    {
        const int32_t t[3] = {0, 2, 7}, b[3] = {0, 5, INT32_MAX}, e[3] = {0, 5, INT32_MAX};      // beg == end is an interval (an empty one)
        WANT(iv_check_intervals(3, t, b, e) == nullptr);
        WANT(iv_check_intervals(0, nullptr, nullptr, nullptr) == nullptr);
    }
    for (int k = 0; k < 3; ++k) {
        int32_t t[3] = {0, 2, 7}, b[3] = {0, 5, 9}, e[3] = {1, 6, 10};
        if (k == 0) t[2] = -1;
        if (k == 1) b[1] = -1;
        if (k == 2) e[0] = 0, b[0] = 1;
        const char *msg = iv_check_intervals(3, t, b, e);
        WANT(msg != nullptr);
        printf("check %d %s\n", k, msg);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    d = tmp_path_factory.mktemp("regions_table_host")
    src = d / "regions_table_host.cpp"
    src.write_text(DRIVER)
    exe = d / "regions_table_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_pack_and_at_reproduce_the_six_arrays(out):
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out if not ln.startswith("check")}
    # (slices of the domain, entries of all domains): contig 0 holds 1 Mbp, two of 100..140 bp, 5 and 2 bp -- four length classes
    assert got["contig"] == (4, 5)
    assert got["contig_then_contig"] == (2, 7)              # contig 1: 4 bp and 300 bp
    assert got["group"] == (5, 7)                           # one coordinate space: the cut 1 Mbp and the 300 bp interval each open a class
    assert got["nothing_here"] == (0, 0) and got["nothing_here_behind_words"] == (0, 0)
    assert got["no_intervals"] == (0, 0)


def test_check_intervals(out):
    msgs = [ln.split(None, 2)[2] for ln in out if ln.startswith("check")]
    assert msgs == ["want tid >= 0 and 0 <= beg <= end"] * 3
