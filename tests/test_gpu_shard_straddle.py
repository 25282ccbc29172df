"""GPU: --gpus N over BAMs whose records straddle BGZF blocks (METHEOR_SHARD_STRADDLE=1).  The library: a file scanned as 2, 5 and 9
runs (mth_bgzf_straddle_scan from a guess, chain verification, mth_bgzf_straddle_rescan) gives the record table of the true offsets,
on run cuts that hold the cases (a) to (e) of tests/shard_straddle_util.py at each cut size; the shards' plans from that table
(mth_host_plan_shard_straddle) decode to the oracle's SoA, every read once.  The CLI: all seven measures and the pairs table under
--gpus 2, 5 and 8 on the file cut every 4 093 bytes against the single-GPU run of the same file and --gpus N on its block-aligned
copy; more shards than data blocks; records that cover whole blocks; pdr -g.  tests/test_shard_straddle_inputs.py checks the inputs
and the planner on the CPU."""
import os
import re

import pytest

from oracle import pyoracle
from tests import shard_straddle_util as X
from tests import straddle_util as S
from tests.test_gpu_irregular_paths import MEASURES
from tests.test_gpu_straddle import DEVICE, STRADDLE, STREAM, outputs, run
from tests.test_host_decode import same_soa

pytestmark = pytest.mark.gpu
ON = {"METHEOR_SHARD_STRADDLE": "1"}
SCAN_LINE = re.compile(r"^\[metheor straddle\] shard scan: (\d+) runs, (\d+) scanned again, (\d+) rounds$", re.M)


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shard_straddle"))


_made = {}


def made(d, case, cut):
    if (case, cut) not in _made:
        _made[case, cut] = X.make(d, case, cut)
    return _made[case, cut]


# ---- the library ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", S.CUTS)
@pytest.mark.parametrize("case", X.CASES)
def test_scanned_runs_give_the_true_table(eng, d, case, cut):
    rec, lay, edge, blk = made(d, case, cut)
    want = X.truth_table(lay)
    for n in X.N_RUNS:
        e = X.case_edges(lay, case, edge, blk, n)
        if e is None:                        # (d) in two runs: tests/test_shard_straddle_inputs.py says why
            assert case == "d" and n == 2
            continue
        table, rescans, infos = X.scan_file(eng, lay, e)
        X.same_table(table, want)
        assert all(i["rounds"] < S.MAX_ROUNDS for i in infos), infos
        if case == "e":
            assert rescans >= 1, (n, infos)


def test_a_lookalike_first_guess_is_scanned_again(eng, d):
    """case (f): the first block of a run guesses 4 bytes before a record start and its walk leaves more blocks on than there are
    rounds, inside the stream; the guessed scan settles all the same (the chain breaks behind that block) and is scanned again"""
    lay, blk = X.make_lookalike(d)
    want = X.truth_table(lay)
    for n in X.N_RUNS:
        table, rescans, infos = X.scan_file(eng, lay, X.lookalike_edges(n, blk))
        X.same_table(table, want)
        assert rescans >= 1 and all(i["rounds"] < S.MAX_ROUNDS for i in infos), (n, infos)


def test_a_rescan_needs_a_scan(eng, d):
    from metheor_amd import MthError
    rec, lay, _, _ = made(d, "c", 4093)
    eng.bgzf_straddle_scan(*X.run_call(lay, 0, 4), entry=lay.hbytes)
    lay.call(eng, 0, len(lay.coff), lay.hbytes, last=True)          # another load call: the run is gone
    with pytest.raises(MthError) as e:
        eng.bgzf_straddle_rescan(lay.hbytes)
    assert e.value.status == -1
    eng.reset()


@pytest.mark.parametrize("case,cut", [("c", 4093), ("d", 4093), ("e", 700)])
def test_shard_plans_decode_to_the_oracle(eng, d, case, cut):
    """the runs of mth_host_plan_straddle_run, scanned and verified; every shard's plan decoded as --region loads such a file
    (first_byte at a record, the tail dropped); the reads each shard owns by start, in shard order == the oracle's SoA"""
    from metheor_amd import hostapi
    rec, lay, _, _ = made(d, case, cut)
    want = pyoracle.Reads.decode(rec).soa()
    f = hostapi.BamFile(lay.path)
    for world, halo in ((2, 65536), (5, 300), (9, 300)):
        runs = [f.plan_straddle_run(r, world) for r in range(world)]
        assert all(q["ahead_end"] == X.ahead_end(lay, q["block_end"]) for q in runs)
        table, _, _ = X.scan_file(eng, lay, [q["block_beg"] for q in runs])
        X.same_table(table, X.truth_table(lay))
        parts = []
        for r in range(world):
            p = f.plan_shard_straddle(table, r, world, halo)
            if p["block_beg"] == p["block_end"]:
                continue
            lay.call(eng, p["block_beg"], p["block_end"], p["first_byte"], drop_tail=True)
            got = eng.decoded_fetch()
            parts.append(X.soa_take(got, X.owned(got, p["beg"], p["end"])))
        same_soa(X.soa_concat(parts), want)
    f.close()


# ---- the CLI --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def region(d):
    rd = os.path.join(d, "region")
    os.mkdir(rd)
    return S.region_inputs(rd)


def sharded(tmp_path, tag, sub, flags, bam, n, *more):
    """--gpus n on the new route: the straddle phase line on every shard, one scan line, no host decode"""
    r, out, pairs = outputs(tmp_path, tag, ON, sub, flags, bam, "--gpus", n, *more)
    assert r.stderr.count(STRADDLE) == n and STREAM not in r.stderr and "host decode" not in r.stderr, r.stderr
    assert len(SCAN_LINE.findall(r.stderr)) == 1, r.stderr
    return r, out, pairs


_one = {}


def single(tmp_path, key, sub, flags, bam):
    """the single-GPU run of a file, once per module"""
    if (key, sub) not in _one:
        _, out, pairs = outputs(tmp_path, "one", {}, sub, flags, bam)
        assert len(out) > (10 if sub == "lpmd" else 1000)
        _one[key, sub] = (out, pairs)
    return _one[key, sub]


@pytest.mark.parametrize("n", [2, 5, 8])
@pytest.mark.parametrize("sub,flags", MEASURES, ids=[m[0] for m in MEASURES])
def test_gpus_n_on_a_straddling_file(region, tmp_path, sub, flags, n):
    rec, names, cut, ali = region
    one, pairs_one = single(tmp_path, "region", sub, flags, cut)
    ra, out_a, pairs_a = outputs(tmp_path, "a%d" % n, ON, sub, flags, ali, "--gpus", n)
    assert DEVICE in ra.stderr and STRADDLE not in ra.stderr, ra.stderr          # the aligned route still takes an aligned file
    rc, out_c, pairs_c = sharded(tmp_path, "c%d" % n, sub, flags, cut, n)
    assert out_c == one and out_c == out_a and pairs_c == pairs_one and pairs_c == pairs_a, (sub, n)


def test_the_switch_alone_selects_the_route(region, tmp_path):
    """METHEOR_DEVICE_STRADDLE does not: the refusal, its message and its exit status stay"""
    rec, names, cut, ali = region
    for env in ({}, {"METHEOR_DEVICE_STRADDLE": "1"}, {"METHEOR_SHARD_STRADDLE": "0"}):
        r = run(env, "pdr", "-i", cut, "-o", tmp_path / "o.tsv", "--gpus", 2)
        assert r.returncode == 101 and "need the device load path" in r.stderr, r.stderr
    r = run(ON, "pdr", "-i", cut, "-o", tmp_path / "o.tsv", "--gpus", 2, "--region", names[0])
    assert r.returncode == 2 and "cannot be used with" in r.stderr, r.stderr


def test_more_shards_than_data_blocks(tmp_path):
    from oracle import bamio
    from tests import irregular_util
    rec = irregular_util.forced_records()[0].subset(range(500))
    raw, cut = str(tmp_path / "raw.bam"), str(tmp_path / "few.bam")
    bamio.write_bam(raw, rec)
    S.reblock(raw, cut, 60000)
    lay = S.Layout(cut)
    n = len(lay.b0) + 2
    assert 2 <= len(lay.b0) <= 5 and lay.blocks_cut_inside_a_record() == 1.0
    for sub, flags in (MEASURES[0], MEASURES[1], MEASURES[3]):
        _, one, pairs_one = outputs(tmp_path, "one", {}, sub, flags, cut)
        r, out, pairs = sharded(tmp_path, "n", sub, flags, cut, n)
        assert out == one and pairs == pairs_one and len(one) > (10 if sub == "lpmd" else 1000), sub


@pytest.fixture(scope="module")
def giants(d):
    return S.write_cut(os.path.join(d, "giants.bam"), S.chunked_records(), S.CHUNKED_CUT, realistic=True)


@pytest.mark.parametrize("sub,flags", MEASURES, ids=[m[0] for m in MEASURES])
def test_gpus_n_on_a_file_with_giants(giants, tmp_path, sub, flags):
    """records of 150 000 bytes in 20 000-byte blocks: runs that begin inside one, shard halos that end inside one (no block-aligned
    copy of such a file exists: the single-GPU run is the reference)"""
    one, pairs_one = single(tmp_path, "giants", sub, flags, giants)
    for n in (2, 5):
        r, out, pairs = sharded(tmp_path, "g%d" % n, sub, flags, giants, n)
        assert out == one and pairs == pairs_one and len(one) > (10 if sub == "lpmd" else 1000), (sub, n)


def test_genome_calls_on_the_new_route(tmp_path):
    """pdr -g under --gpus N on an untagged file cut every 4 093 bytes == the single-GPU run of its block-aligned copy and --gpus N on
    that copy.  The records of straddle_util.genome_files in the order of their first aligned base (shard_straddle_util.
    genome_files_sorted): as generated, sorted by pos, 198 of the 5 948 start behind their successor's first aligned base, and a
    shard plan refuses that as unsorted input -- on the block-aligned file as on the cut one, with the message that stays."""
    ali, cut, fa = X.genome_files_sorted(str(tmp_path))
    assert S.Layout(cut).blocks_cut_inside_a_record() >= 0.9
    flags = ["-d", "1", "-p", "1", "-g", fa]
    _, out_a, _ = outputs(tmp_path, "a", {}, "pdr", flags, ali)
    for n in (2, 5):
        _, out_an, _ = outputs(tmp_path, "a%d" % n, ON, "pdr", flags, ali, "--gpus", n)
        _, out_c, _ = sharded(tmp_path, "c%d" % n, "pdr", flags, cut, n)
        assert out_c == out_a and out_c == out_an and out_a.count(b"\n") >= 500
    # genome_files as generated: the refusal of unsorted input, the same on both files
    ali0, cut0, fa0 = S.genome_files(str(tmp_path))
    for bam in (ali0, cut0):
        r = run(ON, "pdr", "-i", bam, "-o", tmp_path / "o.tsv", "-d", 1, "-p", 1, "-g", fa0, "--gpus", 2)
        assert r.returncode == 101 and "need the device load path (coordinate-sorted input, contigs grouped" in r.stderr, r.stderr
