"""The inputs and run cuts of tests/test_gpu_shard_straddle.py on the CPU (tests/shard_straddle_util.py): every (case, cut size, number
of runs) that the GPU test scans holds the case it is named for -- a run is not used unless it does -- and the shard planner
(mth_host_plan_shard_straddle, mth_host_plan_straddle_run) on a record table built from the true offsets gives contiguous owned
intervals, first bytes that are record starts, and blocks that hold every record a shard needs, whole."""
import numpy as np
import pytest

from tests import shard_straddle_util as X
from tests import straddle_util as S

I32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shard_straddle_inputs"))


_made = {}


def made(d, case, cut):
    if (case, cut) not in _made:
        _made[case, cut] = X.make(d, case, cut)
    return _made[case, cut]


def case_edges(lay, case, edge, blk, n_runs):
    return X.case_edges(lay, case, edge, blk, n_runs)


@pytest.mark.parametrize("cut", S.CUTS)
@pytest.mark.parametrize("case", X.CASES)
def test_the_runs_hold_their_case(d, case, cut):
    rec, lay, edge, blk = made(d, case, cut)
    assert len(lay.b0) >= 10 and lay.blocks_cut_inside_a_record() >= (0.5 if case == "d" else 0.9)
    assert X.holds(lay, case, blk), (case, cut, blk)
    for n in X.N_RUNS:
        e = case_edges(lay, case, edge, blk, n)
        if case == "d" and n == 2:
            assert e is None              # two runs: the second ends with the file, neither lies inside one record
            continue
        assert e[0] == 0 and len(e) == n and e == sorted(set(e))
        if case == "a":                   # the run before blk ends inside the block_size field; its look-ahead holds the rest of the key
            assert blk in e and X.ahead_end(lay, blk) > blk
        elif case == "b":                 # inside a run: the key is read across a block's end from the run's own stream
            assert blk not in e and 0 < blk
        elif case == "c":
            assert blk in e and lay.b0[blk] in lay.starts
        elif case == "d":                 # the run [blk, blk + 1): no start in it, none at its first byte, none at the next block's
            assert blk in e and blk + 1 in e and lay.first_start_in()[blk] < 0
        else:                             # the guess of a stream that starts at blk and ends with the run's look-ahead
            nxt = (e + [len(lay.b0)])[e.index(blk) + 1]
            g = X.guess_from(lay, blk, X.ahead_end(lay, nxt))
            assert blk in e and g >= 0 and g != lay.first_start_in()[blk]


def test_a_lookalike_guess_leads_far_inside_the_stream(d):
    """case (f): the run that starts at the block guesses 4 bytes before a record start, and walking from there leaves dozens of
    blocks on, still inside the stream -- an exit that, believed, would cost a round per block it passes"""
    lay, blk = X.make_lookalike(d)
    assert blk is not None and len(lay.b0) >= 100 and lay.blocks_cut_inside_a_record() >= 0.9
    assert X.holds(lay, "f", blk)
    g = X.guess_from(lay, blk, len(lay.b0))
    to = g + 4 + int(np.frombuffer(lay.raw[g:g + 4], np.int32)[0])
    assert g + 4 in lay.starts and int(np.searchsorted(lay.b1, to)) - blk > S.MAX_ROUNDS
    for n in X.N_RUNS:                    # the run from blk ends with the file for every number of runs: the guess above is its guess
        e = X.lookalike_edges(n, blk)
        assert e[0] == 0 and e[-1] == blk and e == sorted(set(e)) and len(e) == n
        assert X.guess_from(lay, blk, X.ahead_end(lay, len(lay.b0))) == g


def test_the_truth_table_is_the_serial_chain(d):
    """every block enters where its predecessor leaves: the table restated from the offsets is a chain"""
    for case, cut in (("c", 4093), ("d", 4093), ("e", 700)):
        rec, lay, _, _ = made(d, case, cut)
        t = X.truth_table(lay)
        entry = lay.hbytes
        for b in range(len(lay.b0)):
            n = int(lay.isize[b])
            assert (int(t[b]["start"]) == entry) if entry < n else (t[b]["start"] == X.NO_START), b
            entry = int(t[b]["exit"])
        assert entry == 0


def keys_of(lay):
    k = np.array([np.frombuffer(lay.raw[s + 4:s + 12], np.int32) for s in lay.starts], np.int64)
    return np.where(k[:, 0] < 0, I32_MAX, k[:, 0]), k[:, 1]


@pytest.mark.parametrize("halo", [300, 65536])
@pytest.mark.parametrize("case,cut", [("c", 4093), ("d", 4093), ("d", 60000), ("e", 700), ("a", 60000)])
def test_planner_on_the_true_table(d, case, cut, halo):
    from metheor_amd import hostapi
    rec, lay, _, _ = made(d, case, cut)
    table = X.truth_table(lay)
    f = hostapi.BamFile(lay.path)
    tid, pos = keys_of(lay)
    key = tid << 32 | pos
    for world in (2, 5, 8, len(lay.b0) + 3):
        plans = [f.plan_shard_straddle(table, r, world, halo) for r in range(world)]
        assert plans[0]["beg"] == (-1, 0) and plans[-1]["end"][0] == I32_MAX
        loaded = 0
        for r, p in enumerate(plans):
            if r:
                assert p["beg"] == plans[r - 1]["end"], (world, r)            # contiguous: the key space is covered once
            if p["block_beg"] == p["block_end"]:
                assert p["beg"] == p["end"] or world > len(lay.b0), (world, r, p)
                continue
            loaded += 1
            first = int(lay.b0[p["block_beg"]]) + p["first_byte"]
            assert first in lay.starts, (world, r, p)
            last = int(lay.b1[p["block_end"] - 1])
            (tb, pb), (te, pe) = p["beg"], p["end"]
            lo, hi = (tb << 32 | pb) if tb >= 0 else -1, te << 32 | pe
            need = ((key >= lo) | ((tid == tb) & (pos >= pb - halo))) & (key <= hi)       # its interval, its halo, and exactly its end
            assert need.any()
            assert (lay.starts[need] >= first).all() and (lay.ends[need] <= last).all(), (world, r, p)
        assert loaded >= min(world, 2)
    # the runs the shards scan: block 0 to the last block, the header's end for run 0, a guess for the others, 36 bytes of look-ahead
    for world in (2, 5, len(lay.b0) + 3):
        runs = [f.plan_straddle_run(r, world) for r in range(world)]
        assert runs[0]["block_beg"] == 0 and runs[0]["entry"] == lay.hbytes and runs[-1]["block_end"] == len(lay.b0)
        for r, q in enumerate(runs):
            assert q["block_beg"] <= q["block_end"] <= q["ahead_end"] <= len(lay.b0)
            if r:
                assert q["entry"] is None and (q["block_beg"] == runs[r - 1]["block_end"] or q["block_beg"] == q["block_end"])
            ahead = int(lay.isize[q["block_end"]:q["ahead_end"]].sum())
            assert ahead >= X.LOOKAHEAD or q["ahead_end"] == len(lay.b0)
    f.close()


def test_planner_refuses_a_table_that_is_no_chain(d):
    from metheor_amd import hostapi
    rec, lay, _, _ = made(d, "c", 4093)
    table = X.truth_table(lay)
    table[len(table) // 2]["exit"] = X.EXIT_BAD
    f = hostapi.BamFile(lay.path)
    with pytest.raises(hostapi.HostError):
        f.plan_shard_straddle(table, 0, 2)
    f.close()
