"""The tail of the dense PDR + LPMD tile kernel (k_pdr_lpmd_tile, mth_pdr_lpmd.hip): the compaction that turns a tile's packed counters
(coverage and discordant reads, 16 bits each) into a mask of the positions with coverage >= min_depth and then into rows.  With two
waves per workgroup a thread compacts 32 positions, reading its eight 16-byte chunks in an order rotated by lane bits and turning the
mask back by one rotate.

Everything goes through the C ABI (metheor_amd.Engine), the dense form (MTH_PDR_WIDE=0) under MTH_TILE_B=128 and 256, with and without
the batch pipeline; the PDR rows and the four LPMD counters are compared against the oracle and bit for bit between the two forms.
The cases put coverages on either side of min_depth (up to 40 000), candidate counts on either side of 2^15 and of the packed path's
capacity of 65 535 with one half of the counter word at its maximum, sites on every position of the runs of 32, on tile and region
ends, 16-bit relative positions and reads of more than eight calls whose later calls decide a site."""
import numpy as np
import pytest

from tests.test_gpu_tile_bounds import RL, W, engines  # noqa: F401  (engines: the fixture)
from tests.test_gpu_tile_two_waves import both_forms, candidates, oracle

pytestmark = pytest.mark.gpu

PIPE = pytest.mark.parametrize("pipe", [True, False], ids=["pipelined", "serial"])
HALF = 32767                                         # a 16-bit count's sign bit stays clear up to here
PACKED_MAX = 65535                                   # candidate reads of a tile on the packed path; beyond: two passes, 32-bit counters


def depth(d, min_cpgs=0):
    return dict(min_depth=d, min_cpgs=min_cpgs)


@pytest.fixture(autouse=True)
def dense_form(monkeypatch):
    monkeypatch.setenv("MTH_PDR_WIDE", "0")
    for k in ("MTH_TILE_RUNS", "MTH_COARSE_INDEX", "MTH_TILE_B", "MTH_TILE_NO_MARGIN"):
        monkeypatch.delenv(k, raising=False)


class Contig:
    """reads given block by block: starts (n), the reference positions of their calls (n x k, ascending in a row, inside
    [start - 1, start + rl - 1]), the calls' states (n x k of 0 / 1; None: random) and the reads' mapq"""

    def __init__(self, length, seed, rl=RL):
        self.length, self.rl, self.rng, self.blocks = int(length), int(rl), np.random.default_rng(seed), []

    def add(self, starts, pos, meth=None, mapq=40):
        starts = np.atleast_1d(np.asarray(starts, np.int64))
        pos = np.asarray(pos, np.int64)
        pos = pos.reshape(len(starts), pos.size // max(len(starts), 1))
        if meth is None:
            meth = self.rng.random(pos.shape) < 0.5
        meth = np.broadcast_to(np.asarray(meth, np.int64), pos.shape)
        if pos.shape[1]:
            assert (np.diff(pos, axis=1) > 0).all() and (pos[:, 0] >= starts - 1).all() and (pos[:, -1] <= starts + self.rl - 1).all()
            assert pos.min() >= 0 and pos.max() + 2 < self.length
        self.blocks.append((starts, pos, meth, np.broadcast_to(np.asarray(mapq, np.uint8), starts.shape)))
        return self

    def site(self, p, cov, back=70, meth=None, mapq=40):
        """cov reads of one call each on position p"""
        return self.add(np.full(cov, max(p - back, 0)), np.full((cov, 1), p), meth, mapq)

    def random(self, starts, kmax=7, low_mapq=0.1):
        """reads with 0..kmax calls on random positions, a tenth of them below every min_qual"""
        starts = np.asarray(starts, np.int64)
        k = self.rng.integers(0, kmax + 1, size=len(starts))
        for kk in range(kmax + 1):
            s = starts[k == kk]
            rel = np.sort(np.argsort(self.rng.random((len(s), self.rl)), axis=1)[:, :kk], axis=1)
            self.add(s, s[:, None] + rel, None, np.where(self.rng.random(len(s)) < low_mapq, 3, 40))
        return self

    def build(self):
        starts = np.concatenate([b[0] for b in self.blocks])
        order = np.argsort(starts, kind="stable")
        ncall = np.concatenate([np.full(len(b[0]), b[1].shape[1]) for b in self.blocks])[order]
        rows = [(b[1][i], b[2][i]) for b in self.blocks for i in range(len(b[0]))]
        pos = np.concatenate([rows[i][0] for i in order] + [np.zeros(0, np.int64)])
        meth = np.concatenate([rows[i][1] for i in order] + [np.zeros(0, np.int64)]).astype(np.uint32)
        starts = starts[order]
        off = np.zeros(len(starts) + 1, np.int64)
        np.cumsum(ncall, out=off[1:])
        rel = np.maximum(pos - np.repeat(starts, ncall), 0)
        return dict(tid=0, length=self.length, read_start=starts.astype(np.int32), read_end=(starts + self.rl - 1).astype(np.int32),
                    read_mapq=np.concatenate([b[3] for b in self.blocks])[order].astype(np.uint8), read_fwd=np.ones(len(starts), np.uint8),
                    cpg_off=off.astype(np.uint32), cpg_pos=pos.astype(np.uint32) | (meth << np.uint32(31)),
                    cpg_rel=rel.astype(np.uint8 if self.rl <= 255 else np.uint16))


def starts_in(t, k, seed, lo=200, hi=W - 400):
    return np.sort(np.random.default_rng(seed).integers(t * W + lo, t * W + hi, size=k))


def rows_of(name, c, params):
    """the oracle's rows as {pos: (n_concordant, n_discordant)}"""
    o = oracle(name, c, params)[0]
    return {int(p): (int(a), int(b)) for p, (a, b) in zip(o.pos[:, 0], o.cnt)}


def filler(cg, t):
    """a last tile of ordinary reads: the tiles before it do not hold the batch's last reads (those take the clamped loads)"""
    s = starts_in(t, 40, 1000 + t)
    return cg.add(s, s[:, None] + np.arange(8)[None, :] * 9 + 3)


# ---- min_depth around the flag -------------------------------------------------------------------------------------------------------
DEPTHS = (0, 1, 2, 10, 255, 256, 32767, 32768, 40000)
_flag = {}


def flag_contig():
    """tile 1: sites covered by exactly 1, 2, 3, 9, 10, 11, 254, 255, 256 and 257 reads (d - 1, d, d + 1 of the small depths); tile 3:
    32 767 candidate reads, all calling site A and all but one calling site B (coverage 32 767 and 32 766: d and d - 1 of 32 767,
    d - 1 of 32 768); tile 5: the clamped loads of the batch's last reads see the same coverages"""
    if not _flag:
        cg = Contig(7 * W, 61)
        covs = (1, 2, 3, 9, 10, 11, 254, 255, 256, 257)
        for t in (1, 5):
            for j, cov in enumerate(covs):
                cg.site(t * W + 300 + 97 * j + (31 if j % 2 else 0), cov)
        a, b = 3 * W + 2000, 3 * W + 2031
        s = np.sort(np.random.default_rng(63).integers(b - RL + 1, a + 1, size=HALF))
        cg.add(s[:-1], np.tile([a, b], (HALF - 1, 1)))
        cg.add(s[-1:], [[a]])
        _flag.update(c=cg.build(), covs=covs, a=a, b=b)
    return _flag


@PIPE
@pytest.mark.parametrize("d", DEPTHS)
def test_min_depth_around_the_flag(engines, monkeypatch, pipe, d):
    f = flag_contig()
    c = f["c"]
    assert candidates(c, 3) == HALF
    both_forms(engines[pipe], monkeypatch, "flag", c, param_sets=(depth(d),))
    rows = rows_of("flag", c, depth(d))
    want = {t * W + 300 + 97 * j + (31 if j % 2 else 0) for t in (1, 5) for j, cov in enumerate(f["covs"]) if cov >= max(d, 1)}
    want |= {p for p, cov in ((f["a"], HALF), (f["b"], HALF - 1)) if cov >= max(d, 1)}
    assert set(rows) == want, d
    if d >= 32768:
        assert not rows                            # every tile's coverage stays below: nothing comes out
    if d == 32767:
        assert set(rows) == {f["a"]} and sum(rows[f["a"]]) == HALF


# ---- both sides of the capacity ------------------------------------------------------------------------------------------------------
_cap = {}


def capacity_contig(k, disc):
    """tile 1 has k candidate reads of four calls, every read calling the same four sites, all concordant or all discordant: the
    coverage half of the counter word, or both halves, reach k and must not carry.  k = 32 767 / 32 768: either side of a 16-bit
    count's top bit; 65 535 / 65 536: the most the packed path takes, and the first tile of the two-pass form, which must give the
    same rows.  Ordinary tiles on both sides"""
    if (k, disc) not in _cap:
        cg = Contig(5 * W, 71 + k + disc)
        cg.random(starts_in(0, 150, 73, lo=100, hi=W - 600))
        s0 = W + 1500
        s = np.sort(np.random.default_rng(75).integers(s0 - 60, s0 + 1, size=k))
        sites = s0 + np.asarray([10, 41, 42, 73])            # (42 = 10 + 32: neighbouring runs of the compaction; 41, 42: adjacent words)
        cg.add(s, np.tile(sites, (k, 1)), [0, 1, 0, 1] if disc else [1, 1, 1, 1])
        cg.random(starts_in(2, 150, 77, lo=600, hi=W - 100))
        filler(cg, 3)
        _cap[(k, disc)] = (cg.build(), sites)
    return _cap[(k, disc)]


@PIPE
@pytest.mark.parametrize("disc", [0, 1], ids=["concordant", "discordant"])
@pytest.mark.parametrize("k", [HALF, HALF + 1, PACKED_MAX, PACKED_MAX + 1])
def test_both_sides_of_the_capacity(engines, monkeypatch, pipe, k, disc):
    c, sites = capacity_contig(k, disc)
    assert candidates(c, 1) == k and candidates(c, 0) == 150 and candidates(c, 2) == 150
    name = "cap%d_%d" % (k, disc)
    both_forms(engines[pipe], monkeypatch, name, c, param_sets=(depth(0), depth(k), depth(k + 1), depth(10, 4)))
    rows = rows_of(name, c, depth(k))
    assert {p: rows[p] for p in sites.tolist()} == {p: ((0, k) if disc else (k, 0)) for p in sites.tolist()} and len(rows) == 4
    assert not rows_of(name, c, depth(k + 1))


# ---- positions and seams -------------------------------------------------------------------------------------------------------------
@PIPE
@pytest.mark.parametrize("short", [1, 31, 32, 33, 4095])
def test_short_last_tile_and_seams(engines, monkeypatch, pipe, short):
    """a region off the tile grid whose last tile has `short` positions.  Exactly four reads call each chosen position: the first and
    the last position of both tiles, the seams of the runs of 32 (and 16) positions a thread compacts, and positions at and past the
    region's end, whose adds land in the last tile's counters and must not come out of this region's batch (the next region's batch
    gives them).  Under min_depth 4 the chosen sites sit exactly on the flag, under 5 one below it"""
    from tests import util
    beg = W + 1234
    end = beg + W + short
    length = 4 * W
    at = {beg + x for x in (0, 15, 16, 31, 32, 63, 64, 2047, 2048, W - 33, W - 32, W - 1)}
    at |= {beg + W + x for x in (0, 15, 16, 30, 31, 32, 33, 63, 64, short - 2, short - 1, short, short + 1, short + 31) if x >= 0}
    at = sorted(p for p in at if p + 3 < length)
    cg = Contig(length, 81 + short)
    for p in at:
        cg.site(p, 4)
    c = cg.build()
    name = "seam%d" % short
    batches = [util.device_batch(c, region=r, device="cuda:0") for r in ((0, beg), (beg, end), (end, length))]
    both_forms(engines[pipe], monkeypatch, name, c, batches, param_sets=(depth(0), depth(4), depth(5)))
    assert set(rows_of(name, c, depth(4))) == set(at) and not rows_of(name, c, depth(5))
    # the middle batch alone: the rows of [beg, end) and nothing from the positions past its end
    from tests.test_gpu_tile_two_waves import FORMS, device
    for form in FORMS:
        monkeypatch.setenv("MTH_TILE_B", str(form))
        d, _ = device(engines[pipe], batches[1:2], depth(4))
        assert d["pos"].tolist() == [p for p in at if beg <= p < end], (short, form)


@PIPE
def test_sites_in_the_neighbouring_tiles_margins(engines, monkeypatch, pipe):
    """reads across both ends of tile 2 whose calls lie on the last two positions of one tile and the first two of the next: with counter
    margins (256 threads) the far calls land in margin words, without (128) in the trash words; ten reads each, min_depth 10 and 11"""
    cg = Contig(6 * W, 91)
    for edge in (2 * W, 3 * W):
        for s in (edge - RL + 2, edge - 75, edge - 1, edge):          # the first start that reaches the edge ... the last that reaches back over it
            cg.add(np.full(10, s), np.tile([edge - 2, edge - 1, edge, edge + 1], (10, 1))[:, [p >= s - 1 and p <= s + RL - 1 for p in (edge - 2, edge - 1, edge, edge + 1)]])
    cg.random(starts_in(2, 300, 93, lo=300, hi=W - 600))
    filler(cg, 4)
    c = cg.build()
    both_forms(engines[pipe], monkeypatch, "edges", c, param_sets=(depth(0), depth(10), depth(40), depth(41)))
    assert {2 * W - 2, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W - 2, 3 * W - 1, 3 * W, 3 * W + 1} <= set(rows_of("edges", c, depth(10)))


# ---- 16-bit relative positions -------------------------------------------------------------------------------------------------------
@PIPE
@pytest.mark.parametrize("rl", [300, 150], ids=["reads300", "reads150_rel16"])
def test_16_bit_relative_positions(engines, monkeypatch, pipe, rl):
    """reads of 300 bases (calls beyond offset 255: the u16 instantiation without margins) and 150-base reads handed over with 16-bit
    relative positions (the u16 instantiation with margins); sites of exactly 9, 10 and 11 reads under min_depth 10"""
    from tests import util
    cg = Contig(5 * W, 101 + rl, rl=rl)
    cg.random(np.sort(np.random.default_rng(103).integers(0, 4 * W, size=1500)))
    for j, cov in enumerate((9, 10, 11)):
        for p in (W + 500 + 32 * j, 2 * W - 1 - j, 2 * W + j):
            cg.site(p, cov, back=rl - 2)                       # the call sits at offset rl - 2 of its read
    c = cg.build()
    assert (c["cpg_rel"].max() > 255) == (rl == 300)
    batches = [util.device_batch(c, region=(0, c["length"]), device="cuda:0", rel16=True)]
    name = "rel16_%d" % rl
    both_forms(engines[pipe], monkeypatch, name, c, batches, param_sets=(depth(0), depth(10), depth(10, 4)))
    rows = set(rows_of(name, c, depth(10)))
    assert {W + 532, W + 564, 2 * W - 2, 2 * W - 3, 2 * W + 1, 2 * W + 2} <= rows


# ---- more than eight calls -----------------------------------------------------------------------------------------------------------
@PIPE
@pytest.mark.parametrize("where", ["first_chunk", "second_chunk"])
def test_ninth_and_later_calls_on_the_flag(engines, monkeypatch, pipe, where):
    """reads of 9, 12 and 20 calls: their ninth and later calls come from memory and add the same word as the eight in registers.  Site
    S0 gets the ninth call of all three and 7 single reads (coverage 10), S1 the 12th / 20th calls of two and 8 singles (10), S2 the
    11th / 16th of two and 7 singles (9): under min_depth 10 S0 and S1 sit exactly on the flag and S2 one below.  The long reads are
    among the tile's first 64 candidates or, with 200 reads before them, in the second register set of the two-wave loop"""
    T0 = W
    base = T0 + (300 if where == "first_chunk" else 2600)
    cg = Contig(4 * W, 111)
    if where == "second_chunk":
        cg.random(starts_in(1, 200, 113, lo=200, hi=1500))
    s = base
    own = lambda n, skip: [s + 2 + 3 * i for i in range(60) if s + 2 + 3 * i not in skip][:n]        # filler calls below the shared sites
    S0, S1, S2 = s + 100, s + 140, s + 120
    r9 = sorted(own(8, ()) + [S0])
    r12 = sorted(own(8, ()) + [S0, S2 - 1, S2, S1])                       # calls 9..12: S0, S2 - 1, S2 (11th), S1 (12th)
    r20 = sorted(own(8, ()) + [S0] + [S0 + 2 + 2 * i for i in range(6)] + [S2] + [S2 + 3, S2 + 6, S2 + 9] + [S1])      # S0 9th, S2 16th, S1 20th
    assert (len(r9), len(r12), len(r20)) == (9, 12, 20) and r9[8] == S0 and r12[8] == S0 and r12[10] == S2 and r12[11] == S1
    assert r20[8] == S0 and r20[15] == S2 and r20[19] == S1
    for r in (r9, r12, r20):
        cg.add([s], [r], mapq=40)
    cg.site(S0, 7).site(S1, 8).site(S2, 7)
    filler(cg, 2)
    c = cg.build()
    name = "long_" + where
    both_forms(engines[pipe], monkeypatch, name, c, param_sets=(depth(0), depth(9), depth(10), depth(11)))
    r10 = rows_of(name, c, depth(10))
    assert sum(r10[S0]) == 10 and sum(r10[S1]) == 10 and S2 not in r10
    assert sum(rows_of(name, c, depth(9))[S2]) == 9 and S0 not in rows_of(name, c, depth(11))


# ---- every position of a run of 32 ---------------------------------------------------------------------------------------------------
@PIPE
def test_every_position_of_the_runs(engines, monkeypatch, pipe):
    """a qualifying site at a position p with p % 32 = 0, 1, .. 31 in turn, in runs spread over the tile so that every 16-byte chunk of a
    thread's 32 counters, every lane pair and both waves hold some: the order of the rows and their counts.  Run r (of 128) has its
    sites at offsets r % 32, (r + 7) % 32 and (r + 18) % 32 with 2 + r % 3 reads each; min_depth 2, 3 and 4 drop the lighter ones"""
    T0 = W
    cg = Contig(4 * W, 121)
    want = {}
    for r in range(1, 127):                                 # (runs 0 and 127 lie in the neighbours' halos: left to the seam cases)
        for o in (r % 32, (r + 7) % 32, (r + 18) % 32):
            p = T0 + 32 * r + o
            want[p] = 2 + r % 3
            cg.site(p, want[p])
    filler(cg, 2)
    c = cg.build()
    both_forms(engines[pipe], monkeypatch, "runs32", c, param_sets=(depth(0), depth(2), depth(3), depth(4), depth(5)))
    assert {(p - T0) % 32 for p in want} == set(range(32))
    for d in (2, 3, 4, 5):
        got = rows_of("runs32", c, depth(d))
        assert sorted(p for p in got if p < 2 * W) == sorted(p for p, k in want.items() if k >= d), d


# ---- empty tiles ---------------------------------------------------------------------------------------------------------------------
@PIPE
def test_empty_tiles_between_full_ones(engines, monkeypatch, pipe):
    """tiles 1 and 4 give 600 rows each under min_depth 1 and 10.  Between them tile 2 has reads and no qualifying site under either
    (reads without calls, and reads below min_qual, whose adds go to the trash words) and tile 3 has sites of at most 9 reads: rows under
    min_depth 1, none under 10"""
    cg = Contig(7 * W, 131)
    rng = np.random.default_rng(133)
    for t in (1, 4):
        sites = t * W + 300 + 5 * np.sort(rng.choice(680, size=600, replace=False))
        for p in sites.tolist():
            cg.site(p, int(rng.integers(10, 14)), back=int(rng.integers(1, 140)))
    s2 = starts_in(2, 300, 135)
    cg.add(s2[:150], np.zeros((150, 0)))
    cg.add(s2[150:], s2[150:, None] + np.arange(6)[None, :] * 11 + 5, mapq=3)
    for j in range(40):
        cg.site(3 * W + 400 + 61 * j, 1 + j % 9)
    filler(cg, 5)
    c = cg.build()
    both_forms(engines[pipe], monkeypatch, "empty", c, param_sets=(depth(1), depth(10)))
    for d, in3 in ((1, 40), (10, 0)):
        pos = np.asarray(sorted(rows_of("empty", c, depth(d))))
        per_tile = np.bincount(pos // W, minlength=7)
        assert per_tile[1] == 600 and per_tile[4] == 600 and per_tile[2] == 0 and per_tile[3] == in3, (d, per_tile)
