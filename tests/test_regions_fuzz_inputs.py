"""The inputs of tests/test_gpu_regions_fuzz.py, looked at without a device: which seed reaches which branch of the per-interval frame
(every branch by at least two seeds), the narrowed restatements of tests/regions_fuzz_util.py against the utility modules' own on a
sample of every seed's intervals, and those against the oracle_route of the definition tests on a few intervals per seed."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import lpmd_intervals_util as L
from tests import mhl_regions_util as M
from tests import pdr_regions_util as P
from tests import quartet_regions_util as Q
from tests import regions_fuzz_util as U

BRANCHES = ("over_mhl_cap", "over_quartet_cap", "over_pdr_cap", "over_lpmd_cap", "over_lpmd_starts", "slice_over_4096", "run_over_64",
            "read_over_18_calls", "more_items_than_grid", "carried_row_changes_entry", "pending_sum_changes_entry", "bare_contig", "sliced_ownership",
            "long_reads", "long_reads_more_items_than_grid", "long_reads_lpmd_default", "long_reads_mhl_default", "long_reads_pdr_default",
            "long_reads_quartet_default", "long_reads_over_pdr_cap", "long_reads_slice_over_4096", "zero_length", "open_ended", "duplicates_over_1000")


def facts_of(seed):
    s = U.scenario(seed)
    calls = M.Calls.from_soa(*s.soa)
    f = dict.fromkeys(BRANCHES, False)
    f["classes"] = set()
    f["removed"], f["n_reads"], f["n_iv"], f["kind"] = s.removed, s.n_reads, len(s.iv), s.kind
    f["bare_contig"] = any(len(c["read_start"]) and not any(x[0] == t and x[1] < x[2] for x in s.iv) for t, c in enumerate(s.cs))
    f["sliced_ownership"], f["long_reads"] = s.regions is not None, s.long
    f["zero_length"] = any(x[1] == x[2] for x in s.iv)
    f["open_ended"] = any(x[2] == U.INT32_MAX for x in s.iv)
    lines = {}
    for x in s.iv:
        lines[x[:3]] = lines.get(x[:3], 0) + 1
    f["duplicates_over_1000"] = max(lines.values()) > 1000
    n_calls = np.bincount(calls.read, minlength=calls.n_reads)
    f["read_over_18_calls"] = bool((n_calls[calls.mapq >= s.min_qual] > U.PACKED_CALLS).any())
    depth = {}
    items_max = 0
    for t, c in enumerate(s.cs):
        sl = U.slices_of([(b, e) for tt, b, e, _ in s.iv if tt == t])
        f["classes"] |= set(sl)
        if not len(c["read_start"]):
            continue
        pos = U.called(c)
        for k, v in sl.items():
            depth[t, k] = U.point_depth(v, pos)
            f["slice_over_4096"] |= len(v[0]) > U.WAVE_ROUND
        if sl:
            R = M.histograms(calls, t, 0, U.INT32_MAX, max(s.min_cpgs, 1), s.min_qual)[0]
            f["run_over_64"] |= len(R) - 1 > U.BINS
    for k in ("mhl", "quartet", "pdr", "lpmd"):
        f["over_%s_cap" % k] = any(d > U.CAPS[k] for d in depth.values())
    f["over_lpmd_starts"] = any(d > U.CAPS["lpmd_starts"] for d in depth.values())
    for sub, region in U.batches(s):
        t = sub["tid"]
        sl = U.slices_of([(b, e) for tt, b, e, _ in s.iv if tt == t])
        off = sub["cpg_off"].astype(np.int64)
        pos = (sub["cpg_pos"] & np.uint32(0x7fffffff)).astype(np.int64)
        n_items = -(-len(sub["read_start"]) // U.RG_B)
        items_max = max(items_max, -(-n_items // (s.grid or n_items or 1)))
        if not s.grid:
            continue
        f["more_items_than_grid"] |= n_items > s.grid
        # the quartet pass carries a row where a class has one candidate (reads of four calls; not with the carry off or a cap of 0); the
        # PDR pass keeps a pending sum where that candidate also holds the span (reads of min_cpgs calls; not with the span route off)
        fq, fp = s.forms["quartet"], s.forms["pdr"]
        if fq.get("MTH_QUARTET_REGIONS_CARRY") != "0" and fq.get("MTH_QUARTET_REGIONS_LDS_CAP") != "0":
            items = U.work_items(*U.read_spans(pos, off, sub["read_mapq"], sub["read_start"], region, s.min_qual, 4), sl)
            f["carried_row_changes_entry"] |= any(U.single_changes(q) for k in sl for q in U.routes(items, sl, k, s.grid))
        if fp.get("MTH_PDR_REGIONS_SPAN") != "0":
            items = U.work_items(*U.read_spans(pos, off, sub["read_mapq"], sub["read_start"], region, s.min_qual, s.min_cpgs), sl)
            f["pending_sum_changes_entry"] |= any(U.single_changes([r for r in q if r[0] != "single" or r[2]]) for k in sl for q in U.routes(items, sl, k, s.grid))
    f["items_per_workgroup"] = items_max
    f["long_reads_more_items_than_grid"] = s.long and f["more_items_than_grid"]
    for k in ("lpmd", "mhl", "pdr", "quartet"):
        f["long_reads_%s_default" % k] = s.long and not s.forms[k]
    f["long_reads_over_pdr_cap"], f["long_reads_slice_over_4096"] = s.long and f["over_pdr_cap"], s.long and f["slice_over_4096"]
    return f


@pytest.fixture(scope="module")
def facts():
    return {seed: facts_of(seed) for seed in U.SEEDS}


def test_every_branch_is_reached_by_two_seeds(facts):
    for b in BRANCHES:
        hit = [s for s, f in facts.items() if f[b]]
        print("%-26s %s" % (b, hit))
        assert len(hit) >= 2, (b, hit)
    # every length class an interval can fall in (1 .. 16: class 0 of the table's seventeen takes no interval), in one seed
    full = [s for s, f in facts.items() if f["classes"] >= set(range(1, 17))]
    print("all sixteen classes", full, "work items per workgroup at most", max(f["items_per_workgroup"] for f in facts.values()))
    assert len(full) >= 2
    assert all(f["n_iv"] <= U.MAX_INTERVALS for f in facts.values())


def test_few_reads_call_position_minus_one(facts):
    for s, f in facts.items():
        assert f["removed"] * 100 <= f["n_reads"], (s, f["removed"])


def sample(s, rng, k, at_most=None):
    iv = [x for x in s.iv if at_most is None or x[2] - x[1] <= at_most]
    pick = rng.choice(len(iv), size=min(k, len(iv)), replace=False)
    return [iv[i] for i in pick]


@pytest.mark.parametrize("seed", U.SEEDS)
def test_the_narrowed_restatements_are_the_modules_own(seed):
    s = U.scenario(seed)
    rng = np.random.default_rng(500 + seed)
    iv = sample(s, rng, 10) + [x for x in s.iv if x[3] in ("whole", "open", "empty", "the_last_call", "dup")][:6]
    calls = M.Calls.from_soa(*s.soa)
    nar = U.Narrowed(calls)
    kw = dict(min_depth=s.min_depth, min_cpgs=s.min_cpgs, min_qual=s.min_qual)
    a, b = U.restate_mhl(nar, iv, **kw), M.restate(calls, iv, **kw)
    assert M.same_bits(a[0], b[0]) and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    a, b = U.restate_pdr(nar, iv, **kw), P.restate(calls, iv, **kw)
    assert P.same_bits(a[0], b[0]) and all((x == y).all() for x, y in zip(a[1:], b[1:]))
    a, b = U.restate_quartet(nar, iv, s.min_depth, s.min_qual), Q.restate(calls, iv, min_depth=s.min_depth, min_qual=s.min_qual)
    assert Q.same_bits(a[0], b[0]) and Q.same_bits(a[1], b[1]) and all((x == y).all() for x, y in zip(a[2:], b[2:]))
    table = U.pairs_table(pyoracle.Reads.from_soa(*s.soa), s.lk)
    a, b = U.reduce_table(table, iv), L.reduce_table(table, iv)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("seed", U.SEEDS)
def test_the_restatements_are_the_oracle_route(seed):
    """three intervals of at most 5 kbp per seed, one of them around a called position: the modules' restate on the scenario's calls
    against the pinned primitives on the same reads written as records"""
    s = U.scenario(seed)
    rng = np.random.default_rng(900 + seed)
    rec = U.to_records(s.cs)
    calls = M.Calls.from_soa(*s.soa)
    assert calls.n_reads == len(rec)
    named = [x for x in s.iv if x[3] in ("start+0", "end+0", "dup")][:1]
    for t, b, e, name in sample(s, rng, 2, at_most=5000) + named:
        if t >= len(s.cs):
            continue
        iv = [(t, b, e, name)]
        mhl, n_reads, max_cpgs = M.restate(calls, iv, min_depth=s.min_depth, min_cpgs=s.min_cpgs, min_qual=s.min_qual)
        v, n, mx = M.oracle_route(rec, t, b, e, min_depth=s.min_depth, min_cpgs=s.min_cpgs, min_qual=s.min_qual)
        assert M.same_bits([v], mhl) and n == n_reads[0] and (mx == max_cpgs[0] or n == 0), (iv, v, mhl)
        _, m, u, d = P.restate(calls, iv, min_depth=s.min_depth, min_cpgs=s.min_cpgs, min_qual=s.min_qual)
        assert P.oracle_route(rec, t, b, e, min_cpgs=s.min_cpgs, min_qual=s.min_qual) == (m[0], u[0], d[0]), iv
        q = Q.restate(calls, iv, min_depth=s.min_depth, min_qual=s.min_qual)
        ob, orr = Q.oracle_route(rec, t, b, e, min_qual=s.min_qual)
        assert (ob == q[4][0]).all() and orr == q[3][0], iv
