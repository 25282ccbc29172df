"""GPU: the chunked BAM load -- a file given to the device in several calls (mth_bgzf_decode with append), the next chunk's bytes
staged on a side stream by a helper thread (mth_bgzf_stage), the decoded arrays sized once (mth_decode_reserve) or grown with a
keep-copy, the in-line copy in pieces (METHEOR_COPY_PIECE_MB), and the CLI's chunk loop with its size switches and its header
bookkeeping.  Every expected value comes from outside the code under test: the oracle's decode of the file, gzip / zlib for the
inflated bytes, the oracle's text for the CLI.  mth_load_stats (and the CLI's "[metheor load]" lines under METHEOR_TIMING) say which
way every call went, so that a case about staging or pieces cannot pass through the in-line copy.
tests/test_chunked_load_inputs.py checks on the CPU that every input here holds the case its test is about.

Wall time of this file on an MI355X box: 27 s for its 61 tests (37 `metheor` runs and one child Python process among them; the
slowest test 2.8 s)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import chunked_load_util as U
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
KEYS = ("tid", "start", "end", "mapq", "fwd", "cpg_off", "cpg_pos", "cpg_rel")
DEVICE, STRADDLE = "  device inflate + walk + decode", "  device inflate + straddle walk + decode"


@pytest.fixture
def eng():
    """a fresh engine per test: the decoded arrays start empty, so the appends really grow them"""
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("chunked_load"))


def oracle_soa(path):
    return pyoracle.Reads.decode(bamio.read_bam(path)).soa()


@pytest.fixture(scope="module")
def files(d):
    """name -> (Layout, the oracle's SoA of the file, extra), written and decoded once"""
    out = {}
    p = U.one_contig(os.path.join(d, "one.bam"))
    out["one"] = (U.Layout(p), oracle_soa(p), None)
    p, firsts = U.three_contigs(d)
    out["three"] = (U.Layout(p), oracle_soa(p), firsts)
    p, second = U.low_yield_first(d)
    out["yield"] = (U.Layout(p), oracle_soa(p), second)
    p, i = U.swapped_pair(d)
    out["swap"] = (U.Layout(p), oracle_soa(p), i)
    return out


def same(got, want, what=""):
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def run_plan(eng, lay, plan, staged=False, between=None):
    """the plan's calls in order; staged: every next chunk announced before the current call, with the very view it is decoded from"""
    calls = [lay.call(b0, b1) for b0, b1 in plan]
    n = (0, 0)
    for k, (fb, coff, csize, isize, first) in enumerate(calls):
        if staged and k + 1 < len(calls):
            eng.bgzf_stage(calls[k + 1][0])
        n = eng.bgzf_decode(fb, coff, csize, isize, first, append=k > 0)
        if between:
            between(k, n)
    return n


def contig_cut_blocks(lay, firsts):
    first_rec, _ = lay.record_block_starts()
    return [int(np.nonzero(first_rec == f)[0][0]) for f in firsts[1:]]


# name -> (file, plan from the layout and the file's extra)
PLANS = {
    "every-block": ("one", lambda lay, x: U.plan_every(lay.n_blocks, 1)),
    "every-2": ("one", lambda lay, x: U.plan_every(lay.n_blocks, 2)),
    "every-3": ("one", lambda lay, x: U.plan_every(lay.n_blocks, 3)),
    "every-7": ("one", lambda lay, x: U.plan_every(lay.n_blocks, 7)),
    "every-64": ("one", lambda lay, x: U.plan_every(lay.n_blocks, 64)),
    "random-1": ("one", lambda lay, x: U.plan_random(lay.n_blocks, 1)),
    "random-2": ("three", lambda lay, x: U.plan_random(lay.n_blocks, 2)),
    "random-4": ("three", lambda lay, x: U.plan_random(lay.n_blocks, 4, n_cuts=25)),
    "contig-change": ("three", lambda lay, x: U.plan_cuts(lay.n_blocks, contig_cut_blocks(lay, x))),
    "header-only-first": ("three", lambda lay, x: U.plan_cuts(lay.n_blocks, [lay.first_data_block(), lay.n_blocks // 2])),
    "empty-call-inside": ("one", lambda lay, x: U.plan_with_empty_call(U.plan_every(lay.n_blocks, 30), 2)),
    "every-block-three": ("three", lambda lay, x: U.plan_every(lay.n_blocks, 1)),
}


# ---- the library: cuts everywhere, in line and staged ---------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True], ids=["inline", "staged"])
@pytest.mark.parametrize("name", list(PLANS))
def test_cut_plans(eng, files, name, staged):
    key, make = PLANS[name]
    lay, want, extra = files[key]
    plan = make(lay, extra)
    n = run_plan(eng, lay, plan, staged)
    assert n == (len(want["tid"]), len(want["cpg_pos"]))
    same(eng.decoded_fetch(), want, name)
    st = eng.load_stats()
    print(name, staged, len(plan), st)
    taken, inline = U.expected_paths(lay, plan, staged)
    assert (st["staged_calls"], st["inline_calls"], st["pieced_calls"], st["pieced_launches"], st["stage_misses"]) == (taken, inline, 0, 0, 0), st
    if staged and name != "empty-call-inside":
        assert st["staged_calls"] == len(plan) - 1 and st["inline_calls"] == 1
    if name.startswith("every-block"):
        assert st["decode_reallocs"] > 16, st            # eight first allocations, and the arrays grew again and again under the appends
    if name == "header-only-first":
        fb, coff, csize, isize, first = lay.call(*plan[0])
        assert first == int(isize.astype(np.int64).sum()) == lay.hbytes     # the first call is given first_byte == total: zero records


# ---- staging misses: the result stays exact, the counters say what happened ----------------------------------------------------------
def quarters(lay):
    n = lay.n_blocks
    return U.plan_cuts(n, [n // 4, n // 2, 3 * n // 4])


def test_stage_miss_other_view_then_shorter_size(eng, files):
    lay, want, _ = files["one"]
    q = quarters(lay)
    c = [lay.call(*x) for x in q]
    eng.bgzf_stage(c[1][0])
    eng.bgzf_decode(*c[0])
    elsewhere = c[1][0].copy()                              # the same bytes at another address
    eng.bgzf_stage(c[2][0])
    eng.bgzf_decode(elsewhere, *c[1][1:], append=True)
    assert eng.load_stats()["stage_misses"] == 1
    mid = (q[2][0] + q[2][1]) // 2                          # chunk 2 in two calls: the first has the announced pointer and a shorter size
    a, b = lay.call(q[2][0], mid), lay.call(mid, q[2][1])
    assert a[0].ctypes.data == c[2][0].ctypes.data and a[0].size < c[2][0].size
    eng.bgzf_decode(*a, append=True)
    assert eng.load_stats()["stage_misses"] == 2
    eng.bgzf_stage(c[3][0])
    eng.bgzf_decode(*b, append=True)
    eng.bgzf_decode(*c[3], append=True)                     # a right announcement is taken again
    same(eng.decoded_fetch(), want)
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (1, 4, 2), st


def test_stage_withdrawn_and_announced_twice(eng, files):
    lay, want, _ = files["one"]
    c = [lay.call(*x) for x in quarters(lay)]
    eng.bgzf_stage(c[1][0])
    eng.bgzf_stage(None)                                    # withdrawn: nothing is copied, nothing is missed
    eng.bgzf_decode(*c[0])
    eng.bgzf_decode(*c[1], append=True)
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (0, 2, 0), st
    eng.bgzf_stage(c[3][0])
    eng.bgzf_stage(c[3][0], n_bytes=0)                      # the other spelling
    eng.bgzf_stage(c[2][0])                                 # announced twice before one call: the later one holds
    eng.bgzf_stage(c[3][0])
    eng.bgzf_decode(*c[2], append=True)
    eng.bgzf_decode(*c[3], append=True)
    same(eng.decoded_fetch(), want)
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (1, 3, 0), st


def test_stage_started_by_bgzf_inflate(eng, files):
    lay, want, _ = files["one"]
    c = [lay.call(*x) for x in quarters(lay)]
    eng.bgzf_stage(c[0][0])
    fb, coff, csize, isize, _ = lay.call(lay.n_blocks - 5, lay.n_blocks)
    got = eng.bgzf_inflate(fb, coff, csize, isize)          # this call starts the helper too
    assert got.tobytes() == lay.raw[int(lay.u0[lay.n_blocks - 5]):]
    eng.bgzf_decode(*c[0])
    for x in c[1:]:
        eng.bgzf_decode(*x, append=True)
    same(eng.decoded_fetch(), want)
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (1, 4, 0), st


def test_stage_then_reset_then_whole_file(eng, files):
    lay, want, _ = files["one"]
    c = [lay.call(*x) for x in quarters(lay)]
    eng.bgzf_stage(c[1][0])
    eng.bgzf_decode(*c[0])
    eng.reset()
    assert eng.load_stats() == dict(staged_calls=0, inline_calls=0, pieced_calls=0, pieced_launches=0, stage_misses=0, decode_reallocs=0)
    eng.bgzf_decode(*lay.call(0, lay.n_blocks))
    same(eng.decoded_fetch(), want)
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (0, 1, 1), st      # the copy made before the reset was not taken


def test_stage_then_close(files):
    """the engine is closed while the helper thread's copy may still be in flight; the next engine loads the file"""
    import metheor_amd
    lay, want, _ = files["one"]
    c = [lay.call(*x) for x in quarters(lay)]
    e = metheor_amd.Engine(0)
    e.bgzf_stage(c[1][0])
    e.bgzf_decode(*c[0])
    e.close()
    assert e.h is None
    e = metheor_amd.Engine(0)
    try:
        run_plan(e, lay, quarters(lay), staged=True)
        same(e.decoded_fetch(), want)
        assert e.load_stats()["staged_calls"] == 3
    finally:
        e.close()


def test_bgzf_stage_refuses_bytes(eng, files):
    lay, _, _ = files["one"]
    with pytest.raises(TypeError):
        eng.bgzf_stage(lay.arr.tobytes())


# ---- reserve ------------------------------------------------------------------------------------------------------------------------
RESERVES = {     # name -> (reserve(R, C) after the first call, reallocations after it: "none" / "some")
    "twice": (lambda R, C, r, c: (2 * R, 2 * C), "none"),
    "exact": (lambda R, C, r, c: (R, C), "none"),
    "half": (lambda R, C, r, c: (R // 2, C // 2), "some"),
    "zero": (lambda R, C, r, c: (0, 0), "some"),
    "less-than-decoded": (lambda R, C, r, c: (r // 2, c // 2), "some"),
}


@pytest.mark.parametrize("name", list(RESERVES))
def test_reserve_after_the_first_call(eng, files, name):
    lay, want, _ = files["one"]
    R, C = len(want["tid"]), len(want["cpg_pos"])
    plan = U.plan_every(lay.n_blocks, 12)
    size, after = RESERVES[name]
    seen = {}

    def between(k, n):
        if k == 0:
            before = eng.load_stats()["decode_reallocs"]
            assert before == 8                                # a fresh engine's first call: every array once
            eng.decode_reserve(*size(R, C, *n))
            seen["reserved"] = eng.load_stats()["decode_reallocs"]
            if name in ("zero", "less-than-decoded"):
                assert seen["reserved"] == before             # no change ...
                same(eng.decoded_fetch(), {k2: (v[:n[0] + 1] if k2 == "cpg_off" else v[:n[1]] if k2.startswith("cpg") else v[:n[0]]) for k2, v in want.items()}, "kept")
            else:
                assert seen["reserved"] > before
    run_plan(eng, lay, plan, between=between)
    same(eng.decoded_fetch(), want, name)                      # ... and nothing lost
    grown = eng.load_stats()["decode_reallocs"] - seen["reserved"]
    print(name, "reallocations after the reserve:", grown)
    assert (grown == 0) if after == "none" else (grown > 0), (name, grown)


def test_reserve_before_any_decode_and_again_between_appends(eng, files):
    lay, want, _ = files["one"]
    R, C = len(want["tid"]), len(want["cpg_pos"])
    eng.decode_reserve(R // 3, C // 3)
    assert eng.load_stats()["decode_reallocs"] == 8

    def between(k, n):
        if k == 3:                                            # between two later appends: up to the true totals, what is decoded is kept
            eng.decode_reserve(R, C)
            between.at = eng.load_stats()["decode_reallocs"]
    run_plan(eng, lay, U.plan_every(lay.n_blocks, 12), between=between)
    same(eng.decoded_fetch(), want)
    assert eng.load_stats()["decode_reallocs"] == between.at


def test_reserve_as_the_cli_would_on_a_low_yield_first_chunk(eng, files):
    """the first chunk holds reads without a single call: 1.03 * total / done * yield + 4096 is far too few calls, and the appends
    grow the call arrays with everything before them kept"""
    lay, want, second = files["yield"]
    first_rec, _ = lay.record_block_starts()
    cut = int(np.nonzero(first_rec == second)[0][0]) // 2       # half of the quiet contig's blocks
    plan = [(0, cut)] + [(b, min(b + 10, lay.n_blocks)) for b in range(cut, lay.n_blocks, 10)]
    seen = {}

    def between(k, n):
        if k == 0:
            assert n[1] == 0 and n[0] > 1000
            r, c = U.cli_reserve(int(lay.u1[-1]), int(lay.u1[cut - 1]), *n)
            assert c == 4096 < len(want["cpg_pos"]) // 10 and r >= len(want["tid"])
            eng.decode_reserve(r, c)
            seen["at"] = eng.load_stats()["decode_reallocs"]
    run_plan(eng, lay, plan, between=between)
    same(eng.decoded_fetch(), want)
    assert eng.load_stats()["decode_reallocs"] - seen["at"] >= 4      # cpg_pos and cpg_rel, more than once each; the read arrays never


# ---- the order flag at a seam ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one-call", "cut-between-the-pair", "cut-after-the-pair", "every-block", "staged-cut-between"])
def test_order_flag_at_a_seam(eng, files, how):
    lay, want, i = files["swap"]
    assert not U.in_order(want)
    first_rec, _ = lay.record_block_starts()
    b = int(np.nonzero(first_rec == i + 1)[0][0])             # the block the pair's second record opens: the later-starting one is the last before it
    plan = {"one-call": [(0, lay.n_blocks)], "cut-between-the-pair": U.plan_cuts(lay.n_blocks, [b]), "cut-after-the-pair": U.plan_cuts(lay.n_blocks, [b + 1]),
            "every-block": U.plan_every(lay.n_blocks, 1), "staged-cut-between": U.plan_cuts(lay.n_blocks, [b])}[how]
    run_plan(eng, lay, plan, staged=how.startswith("staged"))
    same(eng.decoded_fetch(), want)
    tids, beg, end, flags = eng.decoded_contigs()
    assert flags & 4 and not flags & 3, flags
    assert list(tids) == [0] and int(end[0]) == len(want["tid"])


def test_order_flag_stays_clear_on_a_sorted_file(eng, files):
    lay, want, _ = files["three"]
    assert U.in_order(want)
    run_plan(eng, lay, U.plan_every(lay.n_blocks, 1))
    tids, beg, end, flags = eng.decoded_contigs()
    assert flags == 0 and list(tids) == [0, 1, 2]


# ---- other sources of calls: the genome, MM / ML ---------------------------------------------------------------------------------------
def small_blocks(src, dst):
    """the BAM form of a SAM file, relaid in blocks of at most 6 000 bytes: dozens of calls from a few thousand short records"""
    from metheor_amd import hostapi
    f = hostapi.BamFile(str(src))
    open(dst + ".raw", "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    U.relayout(dst + ".raw", dst, block_bytes=6000)
    return U.Layout(dst)


@pytest.fixture(scope="module")
def genome_case(d):
    from tests import genome_util as gu
    g = gu.generate(2)
    recs, xms = gu.runnable(g)
    refs = [(g["name"], len(g["contig"]))]
    sam = os.path.join(d, "genome.sam")
    open(sam, "w").write(gu.sam_text(refs, recs))
    lay = small_blocks(sam, os.path.join(d, "genome.bam"))
    return lay, gu.expected_reads(refs, recs, xms).soa(), [(len(g["contig"]), g["contig"])], bool(recs[0][2] & 1)


@pytest.mark.parametrize("staged_form", ["0", "1"], ids=["direct", "xm-staged"])
def test_cut_plans_with_calls_from_the_genome(eng, genome_case, monkeypatch, staged_form):
    lay, want, contigs, paired = genome_case
    monkeypatch.setenv("METHEOR_GENOME_STAGED", staged_form)
    assert lay.n_blocks >= 30 and len(want["cpg_pos"]) > 20000
    eng.tag_set_genome(contigs)
    eng.decode_set_genome(True, is_paired_end=paired)
    for staged in (False, True):
        plan = U.plan_every(lay.n_blocks, 1)
        run_plan(eng, lay, plan, staged)
        same(eng.decoded_fetch(), want, (staged_form, staged))
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (lay.n_blocks - 1, lay.n_blocks + 1, 0), st


@pytest.fixture(scope="module")
def modtags_case(d):
    from tests import modtags_util as M
    g = M.generate(1, 3000, long_reads=False)
    f, fp = os.path.join(d, "mm_f.sam"), os.path.join(d, "mm_fp.sam")
    M.write_pair(g["refs"], g["recs"], 128, f, fp)
    return small_blocks(f, os.path.join(d, "mm_f.bam")), small_blocks(fp, os.path.join(d, "mm_fp.bam"))


@pytest.mark.parametrize("staged_form", ["0", "1"], ids=["direct", "x-staged"])
def test_cut_plans_with_calls_from_modtags(eng, modtags_case, monkeypatch, staged_form):
    """F (MM / ML tags) in many calls == the single-call decode of F' (the same records with the XM string the tags stand for)"""
    lay, lay_p = modtags_case
    monkeypatch.setenv("METHEOR_MM_STAGED", staged_form)
    assert lay.n_blocks >= 30
    eng.decode_set_modtags(False)
    eng.bgzf_decode(*lay_p.call(0, lay_p.n_blocks))
    want = eng.decoded_fetch()
    assert len(want["cpg_pos"]) > 3000
    eng.decode_set_modtags(True, 128)
    for staged in (False, True):
        run_plan(eng, lay, U.plan_every(lay.n_blocks, 1), staged)
        same(eng.decoded_fetch(), want, (staged_form, staged))
    st = eng.load_stats()
    assert (st["staged_calls"], st["inline_calls"], st["stage_misses"]) == (lay.n_blocks - 1, lay.n_blocks + 2, 0), st


# ---- the pieced copy (METHEOR_COPY_PIECE_MB is read once per process: one child process) -------------------------------------------------
def test_pieced_copy():
    """every table inflated by a pieced call in a child process: the bytes (SHA-256 against the payloads the tables were made from),
    and the call and launch counts against the piece rule restated in chunked_load_util.piece_plan"""
    tables = U.pieced_tables()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chunked_load_child.py")], capture_output=True, text=True, cwd=ROOT, timeout=120,
                       env=dict(os.environ, METHEOR_COPY_PIECE_MB="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(got) == set(tables)
    for name, (fb, coff, csize, isize, payloads) in tables.items():
        pieces, launches = U.piece_plan(len(fb), coff, csize)
        g = got[name]
        print(name, len(fb), pieces, launches, g)
        assert U.is_pieced(len(fb), len(coff)) and len(pieces) >= 2
        assert g["sha256"] == hashlib.sha256(b"".join(payloads)).hexdigest(), name
        assert (g["pieced_calls"], g["inline_calls"], g["staged_calls"]) == (1, 0, 0), (name, g)
        assert g["pieced_launches"] == len(launches), (name, g, launches)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^\[metheor load\] chunk (\d+) of (\d+): (\d+) blocks, (\d+) file bytes, (staged|in line|pieced|header only), (?:not loaded|(\d+) piece launches, (\d+) records so far)$", re.M)
TAIL = re.compile(r"^\[metheor load\] (\d+) reallocations of the decoded arrays, (\d+) staged copies not taken$", re.M)


def run(env, *args):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=300,
                          env=dict(os.environ, METHEOR_TIMING="1", METHEOR_SEED="2", **{k: str(v) for k, v in (env or {}).items()}))


def chunk_lines(stderr):
    return [dict(i=int(m[0]), n=int(m[1]), blocks=int(m[2]), nbytes=int(m[3]), how=m[4], launches=int(m[5] or 0), reads=int(m[6] or 0)) for m in LINE.findall(stderr)]


def check_lines(stderr, lay, env, n_reads=None, last_pass=False):
    """the run's per-chunk lines against the planner and the path rules restated in chunked_load_util (last_pass: the lines of the
    run's last pass over the file -- the straddle route comes after an attempt on the aligned one)"""
    chunks = U.plan_chunks(lay.coff, lay.csize, lay.isize, env)
    hows = U.chunk_paths(chunks, lay.hbytes, env, int(env.get("METHEOR_COPY_PIECE_MB", 0)))
    got = chunk_lines(stderr)
    if last_pass:
        got = got[-len(chunks):]
    assert [g["i"] for g in got] == list(range(1, len(chunks) + 1)) and all(g["n"] == len(chunks) for g in got), stderr
    assert [(g["blocks"], g["nbytes"]) for g in got] == [(c["b1"] - c["b0"], c["nbytes"]) for c in chunks]
    assert [g["how"] for g in got] == hows, (got, hows)
    for g, c, how in zip(got, chunks, hows):
        want = 0
        if how == "pieced":
            rel = lay.coff[c["b0"]:c["b1"]] - lay.coff[c["b0"]]
            want = len(U.piece_plan(c["nbytes"], rel, lay.csize[c["b0"]:c["b1"]])[1])
            assert want >= 2
        assert g["launches"] == want, (g, want)
    loaded = [g for g in got if g["how"] != "header only"]
    assert all(a["reads"] <= b["reads"] for a, b in zip(loaded, loaded[1:]))
    if n_reads is not None:
        assert loaded[-1]["reads"] == n_reads
    tail = TAIL.findall(stderr)
    assert len(tail) == 1 and int(tail[0][1]) == 0, stderr
    return chunks, hows, int(tail[0][0]), got


@pytest.fixture(scope="module")
def cli(d):
    """the CLI's file and the oracle's text for pdr (-d 2 -p 1), lpmd (with the pairs table) and me (-d 2)"""
    p = os.path.join(d, "cli.bam")
    U.cli_bam(p)
    rec = bamio.read_bam(p)
    reads = pyoracle.Reads.decode(rec)
    names = [n for n, _ in rec.refs]
    want = {"pdr": util.oracle_text(reads, names, "pdr", min_depth=2, min_cpgs=1)[0], "me": util.oracle_text(reads, names, "me", min_depth=2)[0]}
    want["lpmd"], want["pairs"] = util.oracle_text(reads, names, "lpmd", input_name=p)
    assert len(want["pdr"]) > 100_000 and len(want["me"]) > 100_000 and want["pairs"].count("\n") > 1000
    return dict(path=p, lay=U.Layout(p), want=want, reads=reads, names=names, n=len(rec))


FLAGS = {"pdr": ["-d", "2", "-p", "1"], "lpmd": [], "me": ["-d", "2"]}


def check_outputs(sub, out, pairs, want):
    util.assert_tsv_equals_oracle(sub, out, want[sub])
    if sub == "lpmd":
        assert pairs == want["pairs"]


@pytest.mark.parametrize("setting", list(U.CLI_SETTINGS))
def test_cli_chunk_settings(cli, tmp_path, setting):
    env = U.CLI_SETTINGS[setting]
    lay = cli["lay"]
    for sub in ("pdr", "lpmd", "me", "all"):
        o = {k: tmp_path / ("%s.%s" % (sub, k)) for k in ("pdr", "lpmd", "me", "pairs")}
        if sub == "all":
            r = run(env, "all", "-i", cli["path"], "-d2", "-p1", "--pdr", o["pdr"], "--lpmd", o["lpmd"], "--me", o["me"], "--lpmd-pairs", o["pairs"])
        else:
            r = run(env, sub, "-i", cli["path"], "-o", o[sub], *FLAGS[sub], *(["--pairs", o["pairs"]] if sub == "lpmd" else []))
        assert r.returncode == 0, (setting, sub, r.stderr[-3000:])
        assert DEVICE in r.stderr and STRADDLE not in r.stderr and "host decode" not in r.stderr, r.stderr
        for k in (("pdr", "lpmd", "me") if sub == "all" else (sub,)):
            check_outputs(k, o[k].read_text(), o["pairs"].read_text() if k == "lpmd" else None, cli["want"])
        chunks, hows, reallocs, _ = check_lines(r.stderr, lay, env, cli["n"])
        # what the setting is about
        if setting == "default":
            assert hows == ["in line"] and reallocs == 8
        elif setting == "chunk1":
            assert len(chunks) >= 4 and hows == ["in line"] + ["staged"] * (len(chunks) - 1)
        elif setting == "chunk1-nostage":
            assert len(chunks) >= 4 and hows == ["in line"] * len(chunks)
        elif setting == "first1":
            assert len(chunks) == 2 and hows == ["in line", "staged"]
        elif setting == "first1-growth2":
            assert [c["lim"] for c in chunks] == [U.MIB, 2 * U.MIB, 4 * U.MIB][:len(chunks)] and len(chunks) == 3 and chunks[1]["nbytes"] > U.MIB
        else:
            # every chunk of two pieces or more goes up in pieces (the rule of inflate_blocks); the file's last sliver is below that
            assert hows[0] == "pieced" and "staged" not in hows and all((h == "pieced") == (c["nbytes"] >= 2 * U.MIB) for h, c in zip(hows, chunks))
        if len(chunks) > 1:
            # the arrays are sized once from the first chunk's yield: on this uniform file the +3 % hold, nothing grows after the reserve
            assert 8 <= reallocs <= 16, reallocs


def owned(text, name, b, e):
    return "".join(l for l in text.splitlines(True) if l.split("\t")[0] == name and b <= int(l.split("\t")[1]) < e)


def test_cli_region_starts_after_block_0(cli, tmp_path):
    """--region over the .bai: the plan starts at a later block with a non-zero first_byte, and is more than one chunk long"""
    if not os.path.exists(cli["path"] + ".bai"):
        bamio.write_bai(cli["path"])
    b, e = 150_000, 400_000
    for sub in ("pdr", "me"):
        o = tmp_path / (sub + ".tsv")
        r = run({"METHEOR_DEVICE_CHUNK_MB": "1"}, sub, "-i", cli["path"], "-o", o, *FLAGS[sub], "--region", "chrL:%d-%d" % (b + 1, e))
        assert r.returncode == 0, r.stderr[-3000:]
        want = owned(cli["want"][sub], "chrL", b, e)
        assert len(want) > 50_000
        util.assert_tsv_equals_oracle(sub, o.read_text(), want)
        got = chunk_lines(r.stderr)
        assert len(got) >= 2 and got[0]["how"] == "in line" and all(g["how"] == "staged" for g in got[1:]), r.stderr
        assert sum(g["blocks"] for g in got) < cli["lay"].n_blocks and got[-1]["reads"] < cli["n"]


def test_cli_two_shards_start_after_block_0(cli, tmp_path):
    """--gpus 2: the second shard's plan starts in the middle of the file; both shards load more than one chunk"""
    env = {"METHEOR_DEVICE_CHUNK_MB": "1", "METHEOR_SHARD_HALO": "4000"}
    for sub in ("pdr", "lpmd"):
        o, pf = tmp_path / (sub + ".tsv"), tmp_path / "pairs.tsv"
        r = run(env, sub, "-i", cli["path"], "-o", o, *FLAGS[sub], *(["--pairs", pf] if sub == "lpmd" else []), "--gpus", "2")
        assert r.returncode == 0, r.stderr[-3000:]
        check_outputs(sub, o.read_text(), pf.read_text() if sub == "lpmd" else None, cli["want"])
        got = chunk_lines(r.stderr)
        firsts = [g for g in got if g["i"] == 1]
        assert len(firsts) == 2 and all(g["n"] >= 2 for g in firsts) and len(got) == sum(g["n"] for g in firsts), r.stderr
        assert sorted(g["how"] for g in got).count("in line") == 2 and all(g["how"] in ("in line", "staged") for g in got)


def test_cli_file_order_replay(cli, d, tmp_path):
    """the same records in runs of 250 moved around: pdr replays the file order, over a load of several chunks"""
    p = U.shuffled_runs(cli["path"], os.path.join(d, "shuffled.bam"))
    rec = bamio.read_bam(p)
    want, _ = util.oracle_text(pyoracle.Reads.decode(rec), cli["names"], "pdr", min_depth=1, min_cpgs=1)
    o = tmp_path / "pdr.tsv"
    env = {"METHEOR_DEVICE_CHUNK_MB": "1"}
    r = run(env, "pdr", "-i", p, "-o", o, "-d", "1", "-p", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    assert "file-order replay" in r.stderr and DEVICE in r.stderr, r.stderr
    assert o.read_text() == want and len(want) > 100_000
    chunks, hows, _, _ = check_lines(r.stderr, U.Layout(p), env, len(rec))
    assert len(chunks) >= 3 and hows == ["in line"] + ["staged"] * (len(chunks) - 1)


@pytest.fixture(scope="module")
def huge(d):
    out = {}
    for case in U.HUGE:
        p, rec = U.huge_header_bam(d, case)
        reads, names = pyoracle.Reads.decode(rec), [n for n, _ in rec.refs]
        want = {"pdr": util.oracle_text(reads, names, "pdr", min_depth=2, min_cpgs=1)[0]}
        want["lpmd"], want["pairs"] = util.oracle_text(reads, names, "lpmd", input_name=p)
        out[case] = dict(path=p, lay=U.Layout(p), want=want, n=len(rec))
    return out


HUGE_HOWS = {"a": ["header only", "in line"], "b": ["in line", "staged"], "c": ["header only", "header only", "in line"], "b-cut": ["in line", "staged"]}


@pytest.mark.parametrize("case", list(U.HUGE))
def test_cli_huge_header(huge, tmp_path, case):
    """a header of thousands of @SQ lines under METHEOR_DEVICE_CHUNK_MB=1: (a) it ends inside chunk 1 -- chunk 0 is header only and is
    not loaded --, (b) it ends with chunk 0's last byte -- that call is given first_byte == total and yields no record --, (c) it
    covers two whole chunks; (b-cut) is b with records that straddle the blocks, through METHEOR_DEVICE_STRADDLE=1: the aligned
    route gives up at chunk 1, the straddle route runs the same loop"""
    h = huge[case]
    straddle = case == "b-cut"
    env = {"METHEOR_DEVICE_CHUNK_MB": "1"}
    if straddle:
        env["METHEOR_DEVICE_STRADDLE"] = "1"
    for sub in ("pdr", "lpmd"):
        o, pf = tmp_path / (sub + ".tsv"), tmp_path / "pairs.tsv"
        r = run(env, sub, "-i", h["path"], "-o", o, *FLAGS[sub], *(["--pairs", pf] if sub == "lpmd" else []))
        assert r.returncode == 0, r.stderr[-3000:]
        assert (STRADDLE if straddle else DEVICE) in r.stderr and "host decode" not in r.stderr, r.stderr
        assert len(h["want"]["pdr"]) > 10_000
        check_outputs(sub, o.read_text(), pf.read_text() if sub == "lpmd" else None, h["want"])
        chunks, hows, _, got = check_lines(r.stderr, h["lay"], env, h["n"], last_pass=straddle)
        assert hows == HUGE_HOWS[case], hows
        if case.startswith("b"):
            assert got[0]["reads"] == 0 and chunks[0]["ubytes"] == h["lay"].hbytes
