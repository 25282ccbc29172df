"""Where `tag --output-format bam` cuts its record stream into BGZF blocks (metheor_amd/csrc/mth_bgzf_cuts.h), on the CPU: the
header compiled as plain C++ (it includes nothing of HIP) with a driver that reads record sizes and prints the cuts, compared
with a restatement of htslib's rule written here."""
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")
MAX = 0xff00

DRIVER = r"""
#include <cstdio>
#include "mth_bgzf_cuts.h"
// a case: n, then n record sizes; prints the cuts of the case on one line
int main() {
    unsigned long long n;
    while (scanf("%llu", &n) == 1) {
        std::vector<uint32_t> sz(n);
        for (auto &s : sz) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; s = (uint32_t)v; }
        std::vector<uint64_t> cuts;
        mth::bgzf_record_cuts(sz.data(), n, cuts);
        for (uint64_t c : cuts) printf("%llu ", (unsigned long long)c);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_cuts")
    src = d / "cuts_driver.cpp"
    src.write_text(DRIVER)
    out = d / "cuts_driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


def restated(sizes):
    """htslib: flush before a record that does not fit; a record longer than a block starts one and is written through full blocks"""
    cuts, pos, fill = [0], 0, 0
    for s in sizes:
        if fill > 0 and fill + s > MAX:
            cuts.append(pos); fill = 0
        while fill + s >= MAX:               # the writer closes a block the moment it is full
            take = MAX - fill
            pos += take; s -= take; fill = 0
            cuts.append(pos)
        pos += s; fill += s
    if fill:
        cuts.append(pos)
    return cuts


def cuts_of(exe, cases):
    text = "".join("%d %s\n" % (len(c), " ".join(str(int(x)) for x in c)) for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [[int(x) for x in line.split()] for line in out]


CASES = {
    "empty": [],
    "one": [300],
    "exact_fit": [MAX - 1000, 600, 400, 77],
    "one_byte_over": [MAX - 1000, 600, 401, 77],
    "record_is_a_block": [100, MAX, 100],
    "record_one_over_a_block": [100, MAX + 1, 100],
    "three_blocks": [3 * MAX],
    "three_blocks_between": [50, 3 * MAX, 50],
    "long_then_fill": [2 * MAX + 10, MAX - 10, 5],
    "long_then_over": [2 * MAX + 10, MAX - 9, 5],
}


@pytest.mark.parametrize("name", list(CASES))
def test_cut_rule_cases(exe, name):
    sizes = CASES[name]
    got, = cuts_of(exe, [sizes])
    assert got == restated(sizes)
    assert got[0] == 0 and got[-1] == sum(sizes) and len(set(got)) == len(got)
    assert all(0 < b - a <= MAX for a, b in zip(got, got[1:]))
    # a record that fits a block lies inside one block; a longer one starts a block and fills every block but its last
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for s, e in zip(starts[:-1], starts[1:]):
        inside = [c for c in got if s < c < e]
        if e - s <= MAX:
            assert not inside
        else:
            assert s in got and inside == [s + k * MAX for k in range(1, len(inside) + 1)] and len(inside) == (e - s - 1) // MAX


def test_cut_rule_hand_worked(exe):
    got = cuts_of(exe, [CASES["empty"], CASES["exact_fit"], CASES["one_byte_over"], CASES["record_one_over_a_block"], CASES["three_blocks"]])
    assert got[0] == [0]
    assert got[1] == [0, MAX, MAX + 77]
    assert got[2] == [0, MAX - 400, MAX + 78]
    assert got[3] == [0, 100, 100 + MAX, 100 + MAX + 1 + 100]
    assert got[4] == [0, MAX, 2 * MAX, 3 * MAX]


def test_cut_rule_random(exe):
    rng = np.random.default_rng(11)
    sizes = rng.integers(40, 700, 10000)
    sizes[rng.integers(0, 10000, 40)] = rng.integers(MAX - 300, MAX + 300, 40)      # around a block
    sizes[rng.integers(0, 10000, 5)] = rng.integers(2 * MAX, 5 * MAX, 5)            # several blocks
    sizes = [int(x) for x in sizes]
    got, = cuts_of(exe, [sizes])
    assert got == restated(sizes)
    assert got[-1] == sum(sizes) and all(0 < b - a <= MAX for a, b in zip(got, got[1:]))
