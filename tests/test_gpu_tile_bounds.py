"""The dense tile kernel's own index (k_build_index<2>, mth_pdr_lpmd.hip): two families with one entry per 4096-bp tile, decided per
wave of 256 consecutive reads from the element before the wave and the wave's last read.  Every case runs the dense form
(MTH_PDR_WIDE=0) with min_depth = min_cpgs = 0, with and without the batch pipeline, and compares the PDR rows and the four LPMD
counters three ways: against the oracle, against the same call on the fine index (MTH_COARSE_INDEX=0, the path this kernel is not
part of), and bit for bit between the two.

150-bp reads on contigs of 20 000 to 400 000 bp; the cases put read counts, gaps, equal starts and unsorted neighbours on the
kernel's own seams (a lane's group of four, a wave, a workgroup; the constants are read from the source)."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

W = 4096                  # tile width of the dense form
RL = 150                  # read length = max_span
LPMD_KEYS = ("n_concordant", "n_discordant", "n_read", "n_valid_read")
ROW_KEYS = ("tid", "pos", "n_concordant", "n_discordant", "pdr")


def _constants():
    """the seams of the index kernel, from its source: reads per wave, threads per workgroup"""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "metheor_amd", "csrc")
    src = open(os.path.join(csrc, "mth_pdr_lpmd.hip")).read() + open(os.path.join(csrc, "mth_common.h")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    return get("IDX2_WAVE_READS"), get("BLOCK")


WAVE_READS, BLOCK = _constants()
BLOCK_READS = WAVE_READS * (BLOCK // 64)                   # reads one workgroup decides on


def contig(starts, length, seed, tail_calls=None):
    """150-bp reads at the given (sorted) starts with 0..7 calls each; tail_calls: the call counts of the last reads"""
    rng = np.random.default_rng(seed)
    starts = np.asarray(starts, np.int32)
    n = len(starts)
    ncall = rng.integers(0, 8, size=n)
    if tail_calls is not None:
        ncall[n - len(tail_calls):] = tail_calls
    off = np.zeros(n + 1, np.int64)
    np.cumsum(ncall, out=off[1:])
    rel = np.concatenate([np.sort(rng.choice(RL, size=int(k), replace=False)) for k in ncall] + [np.zeros(0, np.int64)]).astype(np.int64)
    meth = (rng.random(len(rel)) < 0.5).astype(np.uint32)
    pos = (np.repeat(starts.astype(np.int64), ncall) + rel).astype(np.uint32) | (meth << np.uint32(31))
    return dict(tid=0, length=int(length), read_start=starts, read_end=(starts + RL - 1).astype(np.int32),
                read_mapq=np.where(rng.random(n) < 0.1, 3, 40).astype(np.uint8), read_fwd=np.ones(n, np.uint8),
                cpg_off=off.astype(np.uint32), cpg_pos=pos, cpg_rel=rel.astype(np.uint8))


def random_starts(n, length, seed):
    return np.sort(np.random.default_rng(seed).integers(0, length - RL - 2, size=n)).astype(np.int32)


_oracle = {}


def oracle(name, c):
    """the oracle's rows and LPMD counters of the whole contig (computed once per case, shared by the pipeline modes)"""
    if name not in _oracle:
        from metheor_amd import synth
        reads = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
        _oracle[name] = (reads.pdr(min_depth=0, min_cpgs=0), reads.lpmd())
    return _oracle[name]


@pytest.fixture(scope="module")
def engines():
    """one context per pipeline mode (MTH_PIPELINE is read at a context's first PDR + LPMD call: a small batch latches it)"""
    import metheor_amd
    from metheor_amd import PdrLpmdParams
    from tests import util
    old = os.environ.get("MTH_PIPELINE")
    out = {}
    seed = contig(random_starts(50, 20_000, 1), 20_000, 1)
    try:
        for pipe in (True, False):
            os.environ["MTH_PIPELINE"] = "1" if pipe else "0"
            e = metheor_amd.Engine(0)
            e.pdr_lpmd_accumulate(util.device_batch(seed, device="cuda:0"), PdrLpmdParams(min_depth=0, min_cpgs=0))
            e.pdr_fetch()
            e.reset()
            out[pipe] = e
    finally:
        if old is None:
            os.environ.pop("MTH_PIPELINE", None)
        else:
            os.environ["MTH_PIPELINE"] = old
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(autouse=True)
def dense_form(monkeypatch):
    monkeypatch.setenv("MTH_PDR_WIDE", "0")
    monkeypatch.delenv("MTH_TILE_RUNS", raising=False)
    monkeypatch.delenv("MTH_COARSE_INDEX", raising=False)


def device(eng, batches):
    """one job of device batches -> (rows, LPMD counters)"""
    from metheor_amd import PdrLpmdParams
    eng.reset()
    for bt in batches:
        eng.pdr_lpmd_accumulate(bt, PdrLpmdParams(min_depth=0, min_cpgs=0))
    return eng.pdr_fetch(), eng.lpmd_global()


def three_ways(eng, monkeypatch, name, c, batches):
    o, ol = oracle(name, c)
    got = {}
    for coarse in (True, False):
        if coarse:
            monkeypatch.delenv("MTH_COARSE_INDEX", raising=False)
        else:
            monkeypatch.setenv("MTH_COARSE_INDEX", "0")
        d, l = device(eng, batches)
        assert len(d["pos"]) == len(o), (name, coarse, len(d["pos"]), len(o))
        assert (d["pos"] == o.pos[:, 0]).all() and (d["tid"] == o.tid).all(), (name, coarse)
        assert (d["n_concordant"] == o.cnt[:, 0]).all() and (d["n_discordant"] == o.cnt[:, 1]).all(), (name, coarse)
        assert (d["pdr"].view(np.uint32) == o.val.view(np.uint32)).all(), (name, coarse)
        assert tuple(int(l[k]) for k in LPMD_KEYS) == tuple(int(ol[k]) for k in LPMD_KEYS), (name, coarse, l, ol)
        got[coarse] = (d, l)
    (d1, l1), (d0, l0) = got[True], got[False]
    assert all(d1[k].tobytes() == d0[k].tobytes() for k in ROW_KEYS), name
    assert all(int(l1[k]) == int(l0[k]) for k in LPMD_KEYS), name


def whole(c):
    from tests import util
    return [util.device_batch(c, region=(0, c["length"]), device="cuda:0")]


def tiles_with_candidates(c, beg, end):
    """per tile of [beg, end): does any read start in [T0 - RL + 1, T0 + W]"""
    s = c["read_start"].astype(np.int64)
    t0 = np.arange(beg, end, W, dtype=np.int64)
    return np.searchsorted(s, t0 + W, side="right") > np.searchsorted(s, t0 - RL + 1, side="left")


PIPE = pytest.mark.parametrize("pipe", [True, False], ids=["pipelined", "serial"])


@PIPE
@pytest.mark.parametrize("n_reads", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_read_counts(engines, monkeypatch, pipe, n_reads):
    c = contig(random_starts(n_reads, 60_000, 1000 + n_reads), 60_000, n_reads)
    if n_reads >= 255:
        assert len(np.unique(c["read_start"] // W)) >= 10         # every wave crosses boundaries
    three_ways(engines[pipe], monkeypatch, "count%d" % n_reads, c, whole(c))


@PIPE
def test_reads_in_three_tiles_only(engines, monkeypatch, pipe):
    """reads in tiles 0, 7 and 90 of a 400 000-bp contig: between two adjacent reads more than 64 entries of both families"""
    rng = np.random.default_rng(5)
    starts = np.sort(np.concatenate([t * W + rng.integers(200, W - 400, size=k) for t, k in ((0, 100), (7, 130), (90, 90))])).astype(np.int32)
    c = contig(starts, 400_000, 5)
    cand = tiles_with_candidates(c, 0, c["length"])
    assert (np.diff(starts // W) > 64).any() and (~cand).sum() > 80 and cand.sum() >= 3
    three_ways(engines[pipe], monkeypatch, "three_tiles", c, whole(c))


JUMPS = sorted({2, 4, WAVE_READS - 4, WAVE_READS, WAVE_READS * 2 + 2, WAVE_READS * (BLOCK // 64), BLOCK_READS, BLOCK_READS + WAVE_READS})


@PIPE
@pytest.mark.parametrize("at", JUMPS)
def test_jump_placement(engines, monkeypatch, pipe, at):
    """reads 0..at-1 in tile 0, the others 70 tiles on: the jump inside a lane's group of four (at % 4 != 0), between two lanes,
    between two waves and between two workgroups"""
    assert {a % 4 != 0 for a in JUMPS} == {True, False} and any(a % WAVE_READS == 0 for a in JUMPS) and BLOCK_READS in JUMPS
    rng = np.random.default_rng(at)
    lo = np.sort(rng.integers(0, 3000, size=at))
    hi = np.sort(rng.integers(70 * W + 10, 72 * W, size=300))
    c = contig(np.concatenate([lo, hi]), 300_000, at)
    s = c["read_start"]
    assert s[at] // W - s[at - 1] // W > 64 and not tiles_with_candidates(c, 0, c["length"])[2:69].any()
    three_ways(engines[pipe], monkeypatch, "jump%d" % at, c, whole(c))


@PIPE
def test_equal_starts_on_the_boundaries(engines, monkeypatch, pipe):
    """300 reads each starting at b - 1, b and b + 1 for b a boundary of either family (T0 - max_span + 1 and T0 + 1): runs of
    equal starts longer than a wave across a boundary; nothing may raise (the batch is sorted)"""
    T0 = 2 * W
    bs = (T0 - RL + 1, T0 + 1, 5 * W - RL + 1, 5 * W + 1)
    starts = np.sort(np.concatenate([np.full(300, b + d) for b in bs for d in (-1, 0, 1)] + [random_starts(37, 40_000, 9)])).astype(np.int32)
    c = contig(starts, 40_000, 9)
    s = c["read_start"]
    edges = np.arange(WAVE_READS, len(s), WAVE_READS)
    inside_run = s[edges] == s[edges - 1]                       # a wave ends inside a run of equal starts ...
    assert inside_run.sum() >= 4
    for b in bs:                                                # ... and the runs sit on both sides of every boundary
        assert (s == b - 1).sum() >= 300 and (s == b).sum() >= 300 and (s == b + 1).sum() >= 300
    three_ways(engines[pipe], monkeypatch, "equal_starts", c, whole(c))


@PIPE
def test_regions(engines, monkeypatch, pipe):
    """regions from plan_regions / slice_region: region_beg off the tile grid, halo reads starting below region_beg - max_span,
    reads past region_end, an empty last tile"""
    from metheor_amd import shard
    from tests import util
    c = contig(random_starts(4000, 190_000, 21), 200_000, 21)
    regs = shard.plan_regions(c, 3)
    assert all(b % W != 0 for b, _ in regs[1:])
    batches = []
    for (b, e) in regs:
        sub = shard.slice_region(c, b, min(e + 700, c["length"]), halo=400)
        s = sub["read_start"]
        if b > 0:
            assert (s < b - RL).any()
        if e < c["length"]:
            assert (s > e).any()
        batches.append(util.device_batch(sub, region=(b, e), device="cuda:0"))
    b, e = regs[-1]
    last_t0 = b + ((e - b - 1) // W) * W
    assert not (c["read_start"] >= last_t0 - RL).any()           # the last tile has no candidate
    three_ways(engines[pipe], monkeypatch, "regions", c, batches)


@PIPE
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_read_start_off_the_16_byte_grid(engines, monkeypatch, pipe, offset):
    import torch
    from metheor_amd import Batch
    from tests import util
    c = contig(random_starts(1025, 50_000, 31), 50_000, 31)
    bt = util.device_batch(c, region=(0, c["length"]), device="cuda:0")
    big = torch.zeros(len(c["read_start"]) + 8, dtype=torch.int32, device="cuda:0")
    view = big[offset:offset + len(c["read_start"])]
    view.copy_(torch.from_numpy(c["read_start"]).to("cuda:0"))
    assert big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    k = bt.keep                                                  # read_start, read_end, read_mapq, cpg_off, cpg_pos, cpg_rel
    b2 = Batch(0, 0, c["length"], view, k[1], k[2], k[3], k[4], k[5], max_span=RL)
    three_ways(engines[pipe], monkeypatch, "offgrid", c, [b2])


@PIPE
def test_batch_ends_in_short_reads(engines, monkeypatch, pipe):
    """the last reads have 1..3 calls: their 8-slot windows end past the call arrays (safe_hi, the clamped-load tile)"""
    c = contig(random_starts(700, 30_000, 41), 30_000, 41, tail_calls=(2, 3, 1, 1, 2, 3))
    off = c["cpg_off"].astype(np.int64)
    assert off[-1] - off[-7] < 8 * 6 and (np.diff(off)[-6:] <= 3).all() and (np.diff(off)[-6:] >= 1).all()
    three_ways(engines[pipe], monkeypatch, "short_tail", c, whole(c))


@PIPE
def test_unsorted_neighbours_raise(engines, monkeypatch, pipe):
    """start[i] > start[i + 1] at every seam of the kernel: the getter raises; after a reset a clean batch gives the oracle's rows"""
    import metheor_amd
    from tests import util
    eng = engines[pipe]
    c = contig(random_starts(1400, 60_000, 51), 60_000, 51)
    n = len(c["read_start"])
    for i in (0, 1, 3, 4, 255, 256, 257, 1023, 1024, n - 2):
        bad = dict(c)
        rs = c["read_start"].copy()
        rs[i] = rs[i + 1] + 7
        bad["read_start"] = rs
        assert rs[i] > rs[i + 1] and (np.diff(rs.astype(np.int64)) < 0).sum() <= 2
        with pytest.raises(metheor_amd.MthError):
            device(eng, [util.device_batch(bad, region=(0, c["length"]), device="cuda:0")])
        eng.reset()
    three_ways(eng, monkeypatch, "clean1400", c, whole(c))
