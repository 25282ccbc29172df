"""The dense PDR + LPMD tile kernel with two waves per workgroup (k_pdr_lpmd_tile<4096, 128, ..>, mth_pdr_lpmd.hip): a wave takes two
chunks of 64 reads per loop trip on two register sets, and a thread compacts 32 positions.  Every case runs the dense form
(MTH_PDR_WIDE=0) with MTH_TILE_B=128 and with MTH_TILE_B=256, with and without the batch pipeline, under min_depth = min_cpgs = 0
and under the command line's defaults, and compares the PDR rows and the four LPMD counters against the oracle and bit for bit
between the two forms.

150-bp reads (max_span 150) on contigs of a few tiles.  A tile's candidate reads are cut into chunks of 64: with 128 threads wave w
takes the chunks 2 m + w ... of the first register set and 2 m + 2 + w ... of the second; the cases put read counts, long reads,
the batch's last reads, sites and region ends on those seams.  A tile that holds the batch's last reads takes the clamped loads
(one chunk per trip), so the cases that are about the two-chunk loop end in a tile of filler reads."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.test_gpu_tile_bounds import LPMD_KEYS, RL, ROW_KEYS, W, contig, engines, random_starts  # noqa: F401  (engines: the fixture)

pytestmark = pytest.mark.gpu

FORMS = (128, 256)
ZERO = dict(min_depth=0, min_cpgs=0)
CLI = dict()                                   # the reference's command-line defaults: min_depth 10, min_cpgs 4
PIPE = pytest.mark.parametrize("pipe", [True, False], ids=["pipelined", "serial"])


@pytest.fixture(autouse=True)
def dense_form(monkeypatch):
    monkeypatch.setenv("MTH_PDR_WIDE", "0")
    for k in ("MTH_TILE_RUNS", "MTH_COARSE_INDEX", "MTH_TILE_B", "MTH_TILE_NO_MARGIN"):
        monkeypatch.delenv(k, raising=False)


def reads(starts, ncall, length, seed, pos=None):
    """the builder of test_gpu_tile_bounds with the call count of every read given (contig() draws them).  pos: {read: positions}
    puts a read's calls on the given reference positions (ascending, in [start - 1, start + RL - 1]) instead of random ones"""
    rng = np.random.default_rng(seed)
    starts = np.asarray(starts, np.int32)
    ncall = np.asarray(ncall, np.int64)
    n = len(starts)
    assert (np.diff(starts.astype(np.int64)) >= 0).all() and len(ncall) == n
    off = np.zeros(n + 1, np.int64)
    np.cumsum(ncall, out=off[1:])
    rel = np.concatenate([np.sort(rng.choice(RL, size=int(k), replace=False)) for k in ncall] + [np.zeros(0, np.int64)]).astype(np.int64)
    p = np.repeat(starts.astype(np.int64), ncall) + rel
    for r, where in (pos or {}).items():
        where = np.asarray(where, np.int64)
        assert len(where) == ncall[r] and (np.diff(where) > 0).all() and where[0] >= starts[r] - 1 and where[-1] <= starts[r] + RL - 1
        p[off[r]:off[r + 1]] = where
        rel[off[r]:off[r + 1]] = np.maximum(where - starts[r], 0)
    meth = (rng.random(len(rel)) < 0.5).astype(np.uint32)
    return dict(tid=0, length=int(length), read_start=starts, read_end=(starts + RL - 1).astype(np.int32),
                read_mapq=np.where(rng.random(n) < 0.1, 3, 40).astype(np.uint8), read_fwd=np.ones(n, np.uint8),
                cpg_off=off.astype(np.uint32), cpg_pos=p.astype(np.uint32) | (meth << np.uint32(31)), cpg_rel=rel.astype(np.uint8))


def in_tile(t, k, seed, lo=200, hi=W - 400):
    """k sorted starts inside tile t, away from its neighbours' halos: exactly the tile's candidates"""
    return np.sort(np.random.default_rng(seed).integers(t * W + lo, t * W + hi, size=k)).astype(np.int32)


def filler(t, seed, k=40):
    """reads of a later tile with eight calls each: the tiles before it do not hold the batch's last reads"""
    return in_tile(t, k, seed), np.full(k, 8)


_oracle = {}


def oracle(name, c, params):
    key = (name, tuple(sorted(params.items())))
    if key not in _oracle:
        from metheor_amd import synth
        if name not in _oracle:
            _oracle[name] = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
        _oracle[key] = (_oracle[name].pdr(**params), _oracle[name].lpmd())
    return _oracle[key]


def device(eng, batches, params):
    from metheor_amd import PdrLpmdParams
    eng.reset()
    for bt in batches:
        eng.pdr_lpmd_accumulate(bt, PdrLpmdParams(**params))
    return eng.pdr_fetch(), eng.lpmd_global()


def both_forms(eng, monkeypatch, name, c, batches=None, param_sets=(ZERO, CLI)):
    from tests import util
    if batches is None:
        batches = [util.device_batch(c, region=(0, c["length"]), device="cuda:0")]
    for params in param_sets:
        o, ol = oracle(name, c, params)
        got = {}
        for form in FORMS:
            monkeypatch.setenv("MTH_TILE_B", str(form))
            d, l = device(eng, batches, params)
            tag = (name, form, params)
            assert len(d["pos"]) == len(o), (tag, len(d["pos"]), len(o))
            assert (d["pos"] == o.pos[:, 0]).all() and (d["tid"] == o.tid).all(), tag
            assert (d["n_concordant"] == o.cnt[:, 0]).all() and (d["n_discordant"] == o.cnt[:, 1]).all(), tag
            assert (d["pdr"].view(np.uint32) == o.val.view(np.uint32)).all(), tag
            assert tuple(int(l[k]) for k in LPMD_KEYS) == tuple(int(ol[k]) for k in LPMD_KEYS), (tag, l, ol)
            got[form] = (d, l)
        (d1, l1), (d0, l0) = got[128], got[256]
        assert all(d1[k].tobytes() == d0[k].tobytes() for k in ROW_KEYS), (name, params)
        assert all(int(l1[k]) == int(l0[k]) for k in LPMD_KEYS), (name, params)


def candidates(c, t):
    s = c["read_start"].astype(np.int64)
    return int(np.searchsorted(s, t * W + W, side="right") - np.searchsorted(s, t * W - RL + 1, side="left"))


@PIPE
@pytest.mark.parametrize("k", [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385])
def test_candidates_per_tile(engines, monkeypatch, pipe, k):
    """k candidate reads in tile 1 (none in tiles 0, 2, 3): every fill state of the first and the second chunk of both waves -- no second
    chunk, a second chunk of one lane, an odd number of chunks"""
    fs, fn = filler(4, k)
    rng = np.random.default_rng(k)
    c = reads(np.concatenate([in_tile(1, k, 100 + k), fs]), np.concatenate([rng.integers(0, 8, size=k), fn]), 6 * W, k)
    assert candidates(c, 1) == k and candidates(c, 0) == 0 and candidates(c, 2) == 0 and candidates(c, 4) == len(fs)
    both_forms(engines[pipe], monkeypatch, "cand%d" % k, c)


@PIPE
def test_long_reads_in_either_register_set(engines, monkeypatch, pipe):
    """reads with 9, 12 and 20 calls (the tail beyond eight comes from memory) in the first chunk, the second chunk and the last,
    partially filled chunk of a tile: tile 1 has 300 candidates (its last chunk, 44 reads, is a first chunk of wave 0), tile 3 has 230
    (its last chunk, 38 reads, is the second chunk of wave 1)"""
    rng = np.random.default_rng(7)
    n1, n3 = 300, 230
    nc1, nc3 = rng.integers(0, 8, size=n1), rng.integers(0, 8, size=n3)
    # chunk = index // 64: with 128 threads chunks 0, 1 are the first set of waves 0, 1 and chunks 2, 3 the second; chunk 4 starts the next trip
    for i, k in ((5, 9), (70, 12), (100, 20), (130, 9), (140, 20), (200, 12), (250, 20), (270, 9), (290, 12), (299, 20)):
        nc1[i] = k
    for i, k in ((0, 20), (63, 9), (64, 12), (127, 20), (128, 12), (191, 9), (192, 20), (210, 12), (229, 9)):
        nc3[i] = k
    fs, fn = filler(5, 3)
    c = reads(np.concatenate([in_tile(1, n1, 11), in_tile(3, n3, 13), fs]), np.concatenate([nc1, nc3, fn]), 7 * W, 7)
    assert candidates(c, 1) == n1 and candidates(c, 3) == n3
    both_forms(engines[pipe], monkeypatch, "long_reads", c)


@PIPE
@pytest.mark.parametrize("clamp", [True, False], ids=["clamped", "plain"])
def test_last_reads_of_the_batch(engines, monkeypatch, pipe, clamp):
    """the last reads of tile 1 have 1..3 calls.  clamped: they are the batch's last reads, their 8-slot windows end past the call arrays
    and the tile takes the clamped loads; plain: a tile of filler reads follows and the same tile takes the two-chunk loop"""
    rng = np.random.default_rng(17)
    n1 = 200
    nc = rng.integers(0, 8, size=n1)
    nc[-6:] = (2, 3, 1, 1, 2, 3)
    starts = in_tile(1, n1, 19)
    if not clamp:
        fs, fn = filler(3, 21)
        starts, nc = np.concatenate([starts, fs]), np.concatenate([nc, fn])
    c = reads(starts, nc, 5 * W, 17)
    off = c["cpg_off"].astype(np.int64)
    assert (off[n1] + 8 > off[-1]) == clamp                    # the last read of tile 1: does its window run past the arrays
    both_forms(engines[pipe], monkeypatch, "last_reads_%d" % clamp, c)


_deep = {}


def deep_contig():
    """70 000 candidate reads in tile 1 (more than a 16-bit counter counts: two half-tile passes with 32-bit counters, clamped loads),
    an ordinary tile on each side"""
    if not _deep:
        rng = np.random.default_rng(23)
        starts = np.concatenate([in_tile(0, 150, 25, lo=100, hi=W - 600), in_tile(1, 70_000, 27), in_tile(2, 150, 29, lo=600, hi=W - 100)])
        _deep["c"] = reads(starts, rng.integers(0, 5, size=len(starts)), 4 * W, 23)
    return _deep["c"]


@PIPE
def test_deep_tile_two_passes(engines, monkeypatch, pipe):
    c = deep_contig()
    assert candidates(c, 1) == 70_000 and candidates(c, 0) == 150 and candidates(c, 2) == 150
    both_forms(engines[pipe], monkeypatch, "deep", c)


@PIPE
@pytest.mark.parametrize("short", [1, 31, 32, 33, 4095])
def test_short_last_tile(engines, monkeypatch, pipe, short):
    """a region off the tile grid whose last tile has 1, 31, 32, 33 or 4095 positions (the edge mask of the compaction at 32 positions
    per thread), with sites on the first and the last position of threads' runs of 32 (and of 16), on positions 0 and Wp - 1 of both
    tiles, and calls just past the region's end that must not come out of this region's batch.  The regions before and behind it
    complete the contig, so the oracle's rows of the whole contig are what the three batches give."""
    from tests import util
    beg = W + 1234
    end = beg + W + short
    length = 4 * W
    at = {beg + x for x in (0, 15, 16, 31, 32, 63, 64, 2047, 2048, W - 33, W - 32, W - 1)}
    at |= {beg + W + x for x in (0, 15, 16, 30, 31, 32, 33, 63, 64, short - 2, short - 1, short, short + 1, short + 31) if 0 <= x}
    at = sorted(p for p in at if p + 3 < length)
    rng = np.random.default_rng(short)
    base = random_starts(900, length, 31 + short)
    extra = np.repeat(np.asarray([max(p - 70, 0) for p in at], np.int32), 3)        # three reads over every chosen position
    starts = np.sort(np.concatenate([base, extra])).astype(np.int32)
    ncall = rng.integers(0, 8, size=len(starts))
    pos = {}
    used = set()
    for p in at:
        for r in np.flatnonzero(starts == max(p - 70, 0)):
            if int(r) in used or len([x for x in pos.values() if x[0] == p]) == 3:
                continue
            used.add(int(r))
            pos[int(r)] = [p]
            ncall[r] = 1
    assert all(len([x for x in pos.values() if x[0] == p]) == 3 for p in at)
    c = reads(starts, ncall, length, short, pos=pos)
    regs = [(0, beg), (beg, end), (end, length)]
    batches = [util.device_batch(c, region=r, device="cuda:0") for r in regs]
    both_forms(engines[pipe], monkeypatch, "short%d" % short, c, batches)
    assert {beg, beg + W - 1, beg + W, end - 1, end} <= set(int(x) for x in oracle("short%d" % short, c, ZERO)[0].pos[:, 0])


@PIPE
def test_sites_at_the_ends_of_both_margins(engines, monkeypatch, pipe):
    """tile 2 (T0 = 2 W): reads starting at T0 - max_span + 1, the first start that can call the tile, with a call on T0 (their other
    calls fill the low margin); reads starting at T0 + W, the last such start, with a call on T0 + W - 1 = start - 1 (their other calls
    fill the high margin up to its last word that a read of this span reaches); reads one position outside either bound"""
    T0 = 2 * W
    rng = np.random.default_rng(37)
    special = []                                                # (start, positions)
    for rep in range(12):
        lo_s, hi_s = T0 - RL + 1, T0 + W
        special.append((lo_s, sorted({lo_s - 1, lo_s, *rng.integers(lo_s + 1, T0 - 1, size=3).tolist(), T0 - 1, T0})))
        special.append((hi_s, sorted({hi_s - 1, hi_s, *rng.integers(hi_s + 1, hi_s + RL - 2, size=3).tolist(), hi_s + RL - 1})))
        special.append((lo_s - 1, sorted({lo_s - 2, T0 - 2, T0 - 1})))            # cannot reach the tile
        special.append((hi_s + 1, sorted({hi_s, hi_s + RL})))                     # its first call is the next tile's first position
    base = in_tile(2, 400, 39, lo=0, hi=W)
    fs, fn = filler(4, 41)
    starts = np.concatenate([base, np.asarray([s for s, _ in special], np.int32), fs])
    ncall = np.concatenate([rng.integers(0, 8, size=len(base)), [len(p) for _, p in special], fn])
    order = np.argsort(starts, kind="stable")
    starts, ncall = starts[order], ncall[order]
    pos = {int(np.flatnonzero(order == len(base) + j)[0]): p for j, (_, p) in enumerate(special)}
    c = reads(starts, ncall, 6 * W, 37, pos=pos)
    both_forms(engines[pipe], monkeypatch, "margins", c)
    assert {T0, T0 + W - 1} <= set(int(x) for x in oracle("margins", c, ZERO)[0].pos[:, 0])


@PIPE
def test_rows_per_lane_and_wave(engines, monkeypatch, pipe):
    """about 600 sites in tile 1 in clusters (a thread's 32 positions hold up to six of them, both halves of the tile hold some: both
    waves' totals are non-zero) under 3000 reads, with min_depth 1 and 10; tile 3 has reads and no row (no calls), tile 2 no read"""
    rng = np.random.default_rng(43)
    T0 = W
    centres = np.sort(rng.choice(np.arange(T0 + 32, T0 + W - 32, 32), size=100, replace=False)) + 1      # inside one thread's run of 32
    sites = np.unique(np.concatenate([cc + np.sort(rng.choice(30, size=6, replace=False)) for cc in centres]))
    assert len(sites) == 600 and (sites < T0 + W // 2).sum() > 100 and (sites >= T0 + W // 2).sum() > 100
    per_run = np.bincount((sites - T0) // 32, minlength=W // 32)
    assert per_run.max() == 6
    starts = np.concatenate([in_tile(1, 3000, 47, lo=0, hi=W - RL), in_tile(3, 200, 49)])
    pos, ncall = {}, np.zeros(len(starts), np.int64)
    for r in range(3000):
        mine = sites[(sites >= starts[r]) & (sites < starts[r] + RL)]
        mine = mine[rng.random(len(mine)) < 0.3]
        if len(mine):
            pos[r], ncall[r] = mine.tolist(), len(mine)
    assert (ncall > 8).any() and (ncall == 0).any()
    fs, fn = filler(5, 51)
    c = reads(np.concatenate([starts, fs]), np.concatenate([ncall, fn]), 7 * W, 43, pos=pos)
    sets = (ZERO, CLI, dict(min_depth=1, min_cpgs=0), dict(min_depth=10, min_cpgs=0))
    both_forms(engines[pipe], monkeypatch, "rows", c, param_sets=sets)
    rows = oracle("rows", c, sets[-1])[0].pos[:, 0]
    assert ((rows >= T0) & (rows < T0 + W)).sum() > 500 and not ((rows >= 2 * W) & (rows < 4 * W)).any()


@PIPE
def test_span_violator_and_unsorted_neighbour_raise(engines, monkeypatch, pipe):
    """a call beyond start + max_span - 1 (in the first and in the second register set) and start[i] > start[i + 1]: the getter raises
    under both forms; after a reset a clean batch gives the oracle's rows"""
    import metheor_amd
    from tests import util
    eng = engines[pipe]
    fs, fn = filler(3, 53)
    rng = np.random.default_rng(53)
    n1 = 260
    c = reads(np.concatenate([in_tile(1, n1, 55), fs]), np.concatenate([rng.integers(1, 8, size=n1), fn]), 5 * W, 53)
    off = c["cpg_off"].astype(np.int64)
    for form in FORMS:
        monkeypatch.setenv("MTH_TILE_B", str(form))
        for r in (10, 150, 259):                                # first set, second set, the last chunk
            bad = dict(c)
            p = c["cpg_pos"].copy()
            last = off[r + 1] - 1
            p[last] = (p[last] & np.uint32(0x80000000)) | np.uint32(int(c["read_start"][r]) + RL + 40)
            bad["cpg_pos"] = p
            with pytest.raises(metheor_amd.MthError):
                device(eng, [util.device_batch(bad, region=(0, c["length"]), device="cuda:0")], ZERO)
            eng.reset()
        for i in (0, 130, n1 - 2):
            bad = dict(c)
            rs = c["read_start"].copy()
            rs[i] = rs[i + 1] + 7
            bad["read_start"] = rs
            assert rs[i] > rs[i + 1]
            with pytest.raises(metheor_amd.MthError):
                device(eng, [util.device_batch(bad, region=(0, c["length"]), device="cuda:0")], ZERO)
            eng.reset()
    both_forms(eng, monkeypatch, "clean260", c)
