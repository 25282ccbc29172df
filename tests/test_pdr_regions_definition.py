"""PDR per interval (`metheor pdr-regions`) on the CPU: the restatement of the definition
(tests/pdr_regions_util.py) against the oracle's pinned primitives, against the reference's own known answers (pdr.rs tests 1-6) and
the oracle's per-CpG table, and the host finaliser (mth_regions_host.h) against the f32 expression.  No device."""
import collections
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import pdr_regions_util as U
from tests.test_mhl_regions_definition import pinned_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metheor_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib_finalise():
    from metheor_amd import build, capi
    build.build()
    return capi.pdr_regions_finalise


# ---- 1. the definition against pinned code ------------------------------------------------------------------------------------------
def test_restatement_equals_the_route_through_the_oracles_primitives():
    iv, rec = U.intervals(), U.records()
    _, m, u, d = U.default_expected()
    ks = pinned_set()                                 # the named boundary intervals and a spread of the others
    assert len(ks) >= 40
    for k in ks:
        t, b, e, _ = iv[k]
        assert U.oracle_route(rec, t, b, e, min_cpgs=4, min_qual=10) == (m[k], u[k], d[k]), iv[k]
    assert sum(1 for k in ks if m[k] and u[k] and d[k]) >= 10


def test_the_set_is_not_vacuous():
    iv = U.intervals()
    pdr, m, u, d = U.default_expected()
    n = m + u + d
    assert len(iv) == 307 and (n > 0).sum() == 295 and (n[n > 0] >= 10).all() and np.isfinite(pdr).sum() == 295
    assert len(np.unique(pdr[np.isfinite(pdr)].view(np.uint32))) == 265
    assert ((m > 0) & (u > 0) & (d > 0)).sum() == 90
    named = {name: k for k, (_, _, _, name) in enumerate(iv) if name}
    k = named["whole_a"]
    assert (m[k], u[k], d[k]) == (2742, 103, 22624)
    _, m1, u1, d1 = U.restate(U.default_calls(), [iv[named["after_minus_one"]], iv[named["deletion"]]], min_depth=1, min_cpgs=1, min_qual=10)
    assert (m1[0], u1[0], d1[0]) == (4, 0, 8) and (m1[1], u1[1], d1[1]) == (7, 23, 5)
    k = named["empty"]
    assert n[k] == 0 and np.isnan(pdr[k])


# ---- 2. the reference's known answers -----------------------------------------------------------------------------------------------
KNOWN = {1: (2, 14), 2: (16, 0), 3: (2, 0), 5: (0, 0)}            # (n_concordant, n_discordant) pdr.rs's unit tests assert for every CpG


def read_groups(c, min_cpgs, min_qual):
    """the reads by the set of positions they call -> per set (n_concordant, n_discordant) among the contributing reads"""
    out = collections.OrderedDict()
    for r in range(c.n_reads):
        sel = c.read == r
        meth = c.meth[sel]
        g = out.setdefault(tuple(c.pos[sel].tolist()), [0, 0])
        if c.mapq[r] >= min_qual and len(meth) >= max(min_cpgs, 1):
            g[0 if (meth.all() or not meth.any()) else 1] += 1
    return out


@pytest.mark.parametrize("k", range(1, 7))
def test_reference_fixtures(k):
    rec = bamio.read_bam(os.path.join(GOLDEN, "test%d.bam" % k))
    c = U.Calls(rec)
    for min_cpgs in ((1, 2) if k == 6 else (0,)):      # pdr.rs test 6 sets min_cpgs 1 (every read passes), test 7 on the same file 2 (none does)
        m, u, d = U.counts_of(c, 0, 0, U.INT32_MAX, min_cpgs=min_cpgs, min_qual=10)
        table = pyoracle.Reads.decode(rec).pdr(min_depth=0, min_cpgs=min_cpgs, min_qual=10)
        if k in KNOWN:
            assert (m + u, d) == KNOWN[k]
            assert all(tuple(row) == KNOWN[k] for row in table.cnt.tolist()) and (len(table) > 0) == (k != 5)
            continue
        # tests 4 and 6: reads in groups that call disjoint sets of positions -- the whole-contig interval holds every group, a CpG
        # of the per-CpG table exactly one: the table's row is its group's counters and the interval's are the groups' added
        groups = read_groups(c, min_cpgs, 10)
        sets = [set(g) for g in groups]
        assert len(groups) == 2 and not (sets[0] & sets[1])
        assert (m + u, d) == tuple(np.sum(list(groups.values()), axis=0).tolist())
        by_pos = {p: tuple(v) for g, v in groups.items() for p in g}
        if m + u + d:
            assert len(table) == len(by_pos)
        for pos, row in zip(table.pos[:, 0].tolist(), table.cnt.tolist()):
            assert tuple(row) == by_pos[pos], (k, pos)
        assert (m + u, d) == {4: (4, 28), (6, 1): (32, 0), (6, 2): (0, 0)}[k if k == 4 else (k, min_cpgs)]
        assert (len(table) == 0) == (k == 6 and min_cpgs == 2)


# ---- 3. the host finaliser ----------------------------------------------------------------------------------------------------------
def test_host_finaliser_equals_the_f32_expression(lib_finalise):
    pdr, m, u, d = U.default_expected()
    for k in range(len(pdr)):
        assert U.same_bits([lib_finalise(int(m[k] + u[k]), int(d[k]), 10)], [pdr[k]])
    cases = [(3, 6, 10), (3, 7, 10), (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 1), (5, 5, 0), (2 ** 24 + 1, 3, 10), (3, 2 ** 24 + 1, 10),
             (2 ** 24 + 1, 2 ** 24 + 1, 10), (2 ** 32 + 5, 7, 10), (7, 2 ** 32 + 5, 10), (2 ** 32 + 5, 2 ** 32 + 5, 2 ** 32 - 1)]
    for c, d_, depth in cases:
        want = U.finalise(c, d_, depth)
        assert U.same_bits([lib_finalise(c, d_, depth)], [want]), (c, d_, depth)
    assert np.isnan(lib_finalise(3, 6, 10)) and lib_finalise(3, 7, 10) == np.float32(0.7)       # below depth: NaN (the counts stay the caller's)
    assert np.isnan(lib_finalise(0, 0, 0)) and lib_finalise(1, 0, 0) == 0.0 and lib_finalise(0, 1, 1) == 1.0
    # 2^24 + 1 is not an f32: each counter is rounded once, then one add and one divide
    assert lib_finalise(2 ** 24 + 1, 3, 10) == np.float32(3) / np.float32(np.float32(2 ** 24) + np.float32(3))
    assert lib_finalise(7, 2 ** 32 + 5, 10) == np.float32(2 ** 32) / np.float32(np.float32(7) + np.float32(2 ** 32))


DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "mth_regions_host.h"
int main() {
    unsigned long long c, d;
    unsigned depth;
    while (scanf("%llu %llu %u", &c, &d, &depth) == 3) {
        const float v = mth::pdr_regions_finalise(c, d, depth);
        uint32_t bits;
        memcpy(&bits, &v, 4);
        printf("%u\n", bits);
    }
    return 0;
}
"""


def test_host_header_still_compiles_alone_with_plain_cxx(tmp_path):
    text = open(os.path.join(CSRC, "mth_regions_host.h")).read()
    assert "getenv" not in text and "hip/" not in text and "mth_common.h" not in text and "mth_ctx.h" not in text
    src = tmp_path / "fin.cpp"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "fin"), str(src)])
    cases = [(2742 + 103, 22624, 10), (3, 6, 10), (2 ** 24 + 1, 3, 0), (2 ** 32 + 5, 7, 10)]
    out = subprocess.run([str(tmp_path / "fin")], input="".join("%d %d %d\n" % x for x in cases), capture_output=True, text=True, check=True).stdout.split()
    want = [U.finalise(*x) for x in cases]
    assert len(out) == len(cases)
    for o, w in zip(out, want):
        assert U.same_bits(np.array([int(o)], np.uint32).view(np.float32), [w])
