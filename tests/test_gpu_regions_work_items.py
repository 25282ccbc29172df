"""The per-interval passes (`lpmd --intervals`, `mhl-regions`, `pdr-regions`, `me-regions` / `pm-regions`) with several work items per
workgroup.  Their kernels are persistent loops over work items (a tile's rows; 256 consecutive reads) and launch up to 4096 / 8192
workgroups, so on a test-sized input every workgroup takes one work item and leaves: what a workgroup keeps from one work item to the
next -- the LDS rows and their barriers, the quartet pass's carried row, the PDR pass's pending sum -- only runs on inputs of millions of
reads.  MTH_REGIONS_GRID (mth_knobs.h) bounds the workgroups of those launches: with 1, one workgroup walks every work item of a batch
in order.  Everything here is compared with the restatements of the utility modules through the per-pass modules' own feeders and check
functions, at their bars (counters exact; LPMD, PDR, PM and MHL bit for bit; ME within 1e-6), never with an unbounded run alone."""
import functools
import os

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import lpmd_intervals_util as L
from tests import mhl_regions_util as M
from tests import pdr_regions_util as P
from tests import quartet_regions_util as Q
from tests import regions_fuzz_util as U
from tests import test_gpu_lpmd_intervals as T_lpmd
from tests import test_gpu_mhl_regions as T_mhl
from tests import test_gpu_pdr_regions as T_pdr
from tests import test_gpu_quartet_regions as T_quartet
from tests import util
from tests.test_gpu_regions_fuzz import arrays, check_lpmd, engine

pytestmark = pytest.mark.gpu

GRID = "MTH_REGIONS_GRID"
SHARDS = {"METHEOR_SHARD_HALO": "4000", "METHEOR_DEVICES": "1"}


def _bam(d, rec, bed_text):
    raw, bam, bed = str(d / "raw.bam"), str(d / "iv.bam"), d / "iv.bed"
    bamio.write_bam(raw, rec)
    util.reblock_aligned(raw, bam)
    bed.write_text(bed_text)
    body, offs = L.record_stream(bam)
    return dict(dir=d, rec=rec, bam=bam, bed=str(bed), body=body, offs=offs)


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    """the records and the 307 intervals of the three read x interval modules, once for all of them"""
    assert os.path.exists(T_mhl.EXE)
    return dict(_bam(tmp_path_factory.mktemp("work_items"), M.records(), M.bed_text()), iv=M.intervals())


@pytest.fixture(scope="module")
def mhl_files(shared):
    want = M.default_expected()
    return dict(shared, want=want, text=M.table_text(shared["iv"], *want))


@pytest.fixture(scope="module")
def pdr_files(shared):
    want = P.default_expected()
    return dict(shared, want=want, text=P.table_text(shared["iv"], *want))


@pytest.fixture(scope="module")
def quartet_files(shared):
    want = Q.default_expected()
    me_text, pm_text = Q.expected_texts(shared["iv"], want)
    return dict(shared, want=want, me_text=me_text, pm_text=pm_text)


@pytest.fixture(scope="module")
def lpmd_files(tmp_path_factory):
    """the per-interval LPMD module's own records and intervals"""
    iv = L.intervals()
    nc, nd = L.reduce_table(L.default_table(), iv)
    return dict(_bam(tmp_path_factory.mktemp("work_items_lpmd"), L.records(), L.bed_text()), iv=iv, nc=nc, nd=nd, text=L.table_text(iv, nc, nd))


# ---- 1. the default sets ---------------------------------------------------------------------------------------------------------------------
ROUTES = [("groups", 1), ("groups", 3), ("groups", 7), ("one_contig_per_batch", 1)]
ROUTE_IDS = ["%s_grid_%d" % r for r in ROUTES]


def work_items_of_the_group_batch(rec):
    return -(-len(rec) // U.RG_B)


@pytest.mark.parametrize("route,grid", ROUTES, ids=ROUTE_IDS)
def test_mhl_default_set(mhl_files, route, grid):
    with engine(grid) as eng:
        eng.mhl_regions_begin(*arrays(mhl_files["iv"]))
        T_mhl.feed(eng, mhl_files, route, min_cpgs=4, min_qual=10)
        T_mhl.check(eng.mhl_regions_fetch(min_depth=10), mhl_files["want"], (route, grid))
        assert eng.mhl_regions_stats()[0] >= 7                             # the long reads' lengths went through the overflow list
    assert work_items_of_the_group_batch(mhl_files["rec"]) >= 150          # ... all of which one workgroup takes at grid 1


@pytest.mark.parametrize("route,grid", ROUTES, ids=ROUTE_IDS)
def test_pdr_default_set(pdr_files, route, grid):
    with engine(grid) as eng:
        eng.pdr_regions_begin(*arrays(pdr_files["iv"]))
        T_pdr.feed(eng, pdr_files, route, min_cpgs=4, min_qual=10)
        T_pdr.check(eng.pdr_regions_fetch(min_depth=10), pdr_files["want"], (route, grid))
        c = eng.pdr_regions_counts()
        _, m, u, d = pdr_files["want"]
        assert (c["methylated"] == m).all() and (c["unmethylated"] == u).all() and (c["discordant"] == d).all()


@pytest.mark.parametrize("route,grid", ROUTES, ids=ROUTE_IDS)
def test_quartet_default_set(quartet_files, route, grid):
    with engine(grid) as eng:
        eng.quartet_regions_begin(*arrays(quartet_files["iv"]))
        T_quartet.feed(eng, quartet_files, route, min_qual=10)
        T_quartet.check(eng.quartet_regions_fetch(min_depth=10), quartet_files["want"], (route, grid))
        T_quartet.check_counts(eng.quartet_regions_counts(), quartet_files["want"], (route, grid))


def lpmd_reduced(eng, files, iv, each):
    eng.decode_records(files["body"], files["offs"])
    tids, rb, re_, fl = eng.decoded_contigs()
    for bt, r0, r1, _ in eng.decoded_group(tids, rb, re_, each=each):
        eng.lpmd_pairs_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **L.DEFAULT_KW)
    return eng.lpmd_intervals_fetch(*arrays(iv))


@pytest.mark.parametrize("global_path", [False, True], ids=["tiles", "global_path"])
@pytest.mark.parametrize("route,grid", ROUTES, ids=ROUTE_IDS)
def test_lpmd_default_set(lpmd_files, route, grid, global_path):
    """(a few dozen tiles with rows, or on the global path three chunks of 2048 rows: test_lpmd_many_work_items has the long loop)"""
    with engine(grid, {"MTH_PAIRS_FORCE_GLOBAL": "1"} if global_path else None) as eng:
        check_lpmd(lpmd_reduced(eng, lpmd_files, lpmd_files["iv"], route != "groups"), (lpmd_files["nc"], lpmd_files["nd"]))


LPMD_SLICES = 192


@functools.lru_cache(maxsize=None)
def many_batches():
    """one contig of 400 kbp in LPMD_SLICES ownership slices of about equal numbers of reads, each fed as a batch of its own: every
    batch brings its own tiles (or, on the global path, its own chunk of rows) to the pairs table, so the reduction has at least as many
    work items with rows as there are slices that own a row"""
    from metheor_amd import shard, synth
    c = synth.make_contig(0, 400_000, 30_000, 0.03, np.random.default_rng(411))
    regions = shard.plan_regions(c, LPMD_SLICES)
    table = U.pairs_table(pyoracle.Reads.from_soa(*synth.to_oracle_soa(c)), L.DEFAULT_KW)
    p = int(table[1][len(table[1]) // 2])
    iv = U.tiling(0, c["length"], 1000, None) + U.sliding(0, p, 1100) + [(0, 0, c["length"], "whole"), (0, 0, U.INT32_MAX, "open"), (0, p, p, "empty")] + \
        [(0, b, e + 700, None) for b, e in regions[::7]] + [(0, max(b - 300, 0), e, None) for b, e in regions[3::11]]
    owning = sum(1 for b, e in regions if ((table[1] >= b) & (table[1] < e)).any())      # (a row is its cpg1's slice's)
    return c, regions, table, iv, owning


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("global_path", [False, True], ids=["tiles", "global_path"])
def test_lpmd_many_work_items(global_path, grid):
    """k_pairs_intervals round its loop at least 150 times in one workgroup: a pairs table accumulated from 192 ownership slices, reduced
    by tiling windows, 1100 nested ones, whole-contig intervals and intervals cut at the slices' edges"""
    from tests import test_gpu_pairs as T_pairs
    c, regions, table, iv, owning = many_batches()
    assert owning >= 150 and len(table[0]) > 4000
    with engine(grid, {"MTH_PAIRS_FORCE_GLOBAL": "1"} if global_path else None) as eng:
        T_pairs.run_device(eng, [c], L.DEFAULT_KW, regions=[regions])
        want = U.reduce_table(table, iv)
        assert (want[0] + want[1] > 0).sum() > 1400
        check_lpmd(eng.lpmd_intervals_fetch(*arrays(iv)), want)


# ---- 2. the forms, one workgroup each -----------------------------------------------------------------------------------------------------------
# (the per-pass modules' own tests, which compare with the restatements, called under the grid bound: their engines are created inside)
@pytest.mark.parametrize("form", list(T_quartet.FORMS))
def test_quartet_forms_in_one_workgroup(quartet_files, form, monkeypatch):
    monkeypatch.setenv(GRID, "1")
    T_quartet.test_the_forms_agree(quartet_files, form, monkeypatch)


@pytest.mark.parametrize("form", ["default", "span_off", "cap_4", "cap_0"])
def test_pdr_forms_in_one_workgroup(pdr_files, form, monkeypatch):
    monkeypatch.setenv(GRID, "1")
    T_pdr.test_the_forms_agree(pdr_files, form, monkeypatch)


def test_mhl_second_run_in_one_workgroup(mhl_files, monkeypatch):
    """a list of two entries: the append-only second run of the batch honours the bound too (and still counts what the first counted)"""
    monkeypatch.setenv(GRID, "1")
    T_mhl.test_overflow_list_too_short_runs_the_batch_again(mhl_files, monkeypatch)


@pytest.mark.parametrize("force_global", [False, True], ids=["tiles", "global_path"])
def test_lpmd_deep_overlap_in_one_workgroup(lpmd_files, force_global, monkeypatch):
    monkeypatch.setenv(GRID, "1")
    T_lpmd.test_overlap_deeper_than_the_kernel_sums_in_lds(lpmd_files, monkeypatch, force_global)


# ---- 3. the carried row and the pending sum -----------------------------------------------------------------------------------------------------
WHOLE = [(0, 0, L.REFS[0][1], "whole")]
BLOCKS = [(0, 0, 60_000, "block_0"), (0, 70_000, 130_000, "block_1"), (0, 140_000, 200_000, "block_2")]
TWO_CONTIGS = [(0, 0, 60_000, "head_a"), (1, 0, 60_000, "head_b")]
SETS = dict(whole=WHOLE, blocks=BLOCKS, two_contigs=TWO_CONTIGS)


def group_model(iv, grid):
    """what each workgroup of the default records' one group batch meets, work item by work item (tests/regions_fuzz_util.py), in a
    virtual coordinate space laid out as the library's: contig ivA behind an offset (it holds a call at -1), ivB behind it"""
    c = M.default_calls()
    voff = [4096, 4096 + 204_800, 4096 + 204_800 + 65_536]
    n = np.bincount(c.read, minlength=c.n_reads)
    off = np.r_[0, np.cumsum(n)].astype(np.int64)
    first, last, elig = U.read_spans(c.pos + np.array(voff)[c.tid], off, c.mapq, np.zeros(c.n_reads, np.int64), (0, 1), 10, 4)
    sl = U.slices_of([(voff[t] + b, min(voff[t] + e, voff[t + 1] - 1)) for t, b, e, _ in iv])
    assert len(sl) == 1
    k = next(iter(sl))
    items = U.work_items(first, last, elig, sl)
    return U.routes(items, sl, k, grid), len(items)


def longest_same_single(seq):
    best = cur = 0
    prev = None
    for r in seq:
        if r[0] != "single":
            continue
        cur = cur + 1 if r[1] == prev else 1
        prev, best = r[1], max(best, cur)
    return best


def survives_a_gap(seq):
    """a single candidate, work items without one, then another single candidate"""
    s = [r for r in seq if r[0] != "rows"]
    return any(a[0] == "single" and b[0] == "none" for a, b in zip(s, s[1:])) and any(a[0] == "none" and b[0] == "single" for a, b in zip(s, s[1:]))


def leaves_the_span_route_and_returns(seq):
    """the single candidate holds the span, then it does not (the PDR pass counts it read by read in LDS rows), then it does again"""
    h = [r[2] for r in seq if r[0] == "single"]
    return any(a and not b for a, b in zip(h, h[1:])) and any(b and not a for a, b in zip(h, h[1:]))


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("which", list(SETS))
def test_the_transitions_happen_inside_one_workgroup(which, grid):
    """on the CPU, from the reads' calls: at this grid each workgroup's sequence of work items holds the transitions the next test is
    about"""
    seqs, n_items = group_model(SETS[which], grid)
    assert n_items >= 150 and len(seqs) == grid
    for seq in seqs:
        if which == "whole":
            assert longest_same_single(seq) >= 120 // grid                    # the row is carried that long, the sum pending
        elif which == "blocks":
            assert U.single_changes(seq) == 2 and survives_a_gap(seq) and not any(r[0] == "rows" for r in seq)
        else:
            assert U.single_changes(seq) == 1 and [r[1] for r in seq if r[0] == "single"][0] == 0
    if which == "blocks":
        assert any(leaves_the_span_route_and_returns(seq) for seq in seqs)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("which", list(SETS))
def test_carried_row_and_pending_sum(shared, which, grid, monkeypatch):
    """a whole-contig interval alone (one entry, every work item); three disjoint equal intervals (one class whose single candidate
    changes twice, with work items that have none in between and work items that straddle an interval's edge); one interval on each
    contig of a group batch (the entry changes where the workgroup passes from ivA's reads to ivB's)"""
    iv = SETS[which]
    monkeypatch.setenv(GRID, str(grid))
    for k in T_quartet.KNOBS + ("MTH_PDR_REGIONS_SPAN", "MTH_PDR_REGIONS_LDS_CAP"):
        monkeypatch.delenv(k, raising=False)
    want = Q.restate(M.default_calls(), iv, **Q.DEFAULT_KW)
    assert (want[3] > 256).all()
    got, counts = T_quartet.counted(iv, shared)
    T_quartet.check(got, want, (which, grid))
    T_quartet.check_counts(counts, want, (which, grid))
    want = P.restate(M.default_calls(), iv, **P.DEFAULT_KW)
    assert ((want[1] + want[2] + want[3]) > 256).all()
    T_pdr.check(T_pdr.counted(iv, shared), want, (which, grid))


# ---- 4. the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_two_workgroups(mhl_files, pdr_files, quartet_files, lpmd_files):
    env = {GRID: "2"}
    assert T_mhl.cli(mhl_files, "wi_mhl", env=env) == mhl_files["text"]
    assert T_pdr.cli(pdr_files, "wi_pdr", env=env) == pdr_files["text"]
    T_quartet.both(quartet_files, "wi", env=env)
    assert T_lpmd.cli(lpmd_files, "wi_lpmd", env=env)[0] == lpmd_files["text"]


def test_cli_all_two_workgroups(shared, mhl_files, pdr_files, quartet_files):
    d = shared["dir"]
    out = {k: d / ("wi_all_%s.tsv" % k) for k in ("lpmd", "li", "mhl", "pdr", "me", "pm")}
    r = T_mhl.run("all", "-i", shared["bam"], "--intervals", shared["bed"], "--lpmd", out["lpmd"], "--lpmd-intervals", out["li"], "--mhl-intervals", out["mhl"],
                  "--pdr-intervals", out["pdr"], "--me-intervals", out["me"], "--pm-intervals", out["pm"], env={GRID: "2"})
    assert r.returncode == 0, r.stderr
    assert out["mhl"].read_text() == mhl_files["text"] and out["pdr"].read_text() == pdr_files["text"] and out["pm"].read_text() == quartet_files["pm_text"]
    Q.assert_me_text(out["me"].read_text(), quartet_files["me_text"])
    nc, nd = L.reduce_table(L.pairs_table(shared["rec"], **L.DEFAULT_KW), shared["iv"])
    assert out["li"].read_text() == L.table_text(shared["iv"], nc, nd)


def test_cli_two_shards_two_workgroups(pdr_files, quartet_files):
    env = dict(SHARDS, **{GRID: "2"})
    assert T_pdr.cli(pdr_files, "wi_sh2", "--gpus", "2", env=env) == pdr_files["text"]
    Q.assert_me_text(T_quartet.cli(quartet_files, "me-regions", "wi_sh2", "--gpus", "2", env=env), quartet_files["me_text"])
