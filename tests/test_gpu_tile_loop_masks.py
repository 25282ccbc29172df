"""The read loop of the PDR + LPMD tile kernels without its slot tables (mth_tile_dev.h, mth_lpmd_bytes.h): slot liveness and the LPMD
masks of a diagonal come from the live-byte mask LB(n) of the read's call count, in registers, and the diagonal walk goes on only where
some lane of the wave has two ADJACENT pairs within max_distance.

One batch of a few thousand 150-bp reads over six tiles, through the C ABI: the dense form under MTH_TILE_B=128 and 256, the run form
and the hashed-site form (which keeps the masks in LDS tables), pipelined and serial, in the windows 2/16, 0/0, 0/127, 1/1 (byte form),
2/200 and 0/130 (outside its domain: the launch counts on 16-bit fields with dtab; under 0/130 reads of 150 bases have pairs beyond
max, so that form's walk ends by its rule), with 8-bit and with 16-bit relative positions.  PDR rows and the four LPMD counters
against the oracle, and bit for bit between the forms.  PDR takes reads from mapq 5, LPMD from 10: reads of mapq 7 have live slots
for the span check and the scatter and none for the pair counts.

  tile 0   random reads of 0..8 calls
  tile 1   call counts 0..8, 9, 12 and 20 in turn over 300 reads: every count in the first chunk of 64, in the second register set of the
           two-wave loop and in the last, partial chunk; every third read at mapq 7
  tile 2   waves (64 consecutive candidates) of reads whose calls lie 30 apart -- no pair within 16, the walk ends on diagonal 1 for
           every lane -- with ONE read per wave built on an edge of the stop rule (tests/test_lpmd_exit_host.py has the same reads): that
           lane alone decides how far its wave walks
  tile 3   300 reads on one start with the same six calls (the scatter's atomics on six addresses), then ordinary reads: the tile's
           first chunk, and a chunk right behind heavy same-site scatter
  tile 4   waves of reads with two calls (one pair: nothing adjacent, the walk ends on diagonal 1 in every window) with ONE read per wave
           whose calls span more than 128 bases: under 0/130 its pair (0, g) lies beyond max and the pairs (1, 1 + g) and (2, 2 + g) within,
           the high field of one register of the 16-bit-field form and the low field of the next -- only that adjacency takes the wave
           to the diagonal that holds its last pair
  tile 5   filler, so that no tile above holds the batch's last reads (those take the clamped loads)"""
import numpy as np
import pytest

from oracle import pyoracle
from tests.test_gpu_tile_bounds import LPMD_KEYS, RL, ROW_KEYS, W, engines  # noqa: F401  (engines: the fixture)
from tests.test_gpu_tile_flagged import Contig, filler, starts_in

pytestmark = pytest.mark.gpu

PIPE = pytest.mark.parametrize("pipe", [True, False], ids=["pipelined", "serial"])
WINDOWS = ((2, 16), (0, 0), (0, 127), (1, 1), (2, 200), (0, 130))
FORMS = {"tile128": {"MTH_PDR_WIDE": "0", "MTH_TILE_B": "128"}, "tile256": {"MTH_PDR_WIDE": "0", "MTH_TILE_B": "256"},
         "runs": {"MTH_PDR_WIDE": "0", "MTH_TILE_RUNS": "1"}, "wide14": {"MTH_PDR_WIDE": "14"}}
KNOBS = ("MTH_PDR_WIDE", "MTH_TILE_RUNS", "MTH_TILE_B", "MTH_COARSE_INDEX", "MTH_TILE_NO_MARGIN")
PDR_QUAL, LPMD_QUAL, MID_MAPQ = 5, 10, 7
MAXD = 16                                              # the window the edge reads are built for

# relative positions of the edge reads (max_distance 16), and the diagonals their lane makes the wave evaluate in the window 2 / 16
EDGE_READS = (
    ([0, 17, 34, 35, 35 + 1, 50, 67, 84], 3),          # (a) one pair at exactly max on diagonal 3, (2, 5), nothing adjacent: stop there
    ([0, 17, 34, 35, 36, 50], 3),                      #     the same with nothing live behind the cluster
    ([0, 1, 15, 16], 3),                               # (b) (0, 2) and (1, 3) adjacent on diagonal 2, (0, 3) at exactly max
    ([0, 1, 16, 17], 3),                               #     ... and at max + 1: diagonal 3 runs and holds nothing
    ([0, 17, 34, 51, 52], 1),                          # (c) the pair (3, 4) in the last byte of word 0, slot 5 dead
    ([0, 17, 34, 51, 52, 53], 2),                      #     (3, 4) and (4, 5): adjacent across the two words
    ([0, 17, 34, 51, 52, 53, 54, 55], 4),              #     live slots beyond: slots 3..7 one apart, diagonals 1..4 hold pairs
    ([0, 17, 34, 51, 60, 61, 69, 70], 3),              #     (3, 5) = 10, (4, 6) = 9 adjacent across the words on diagonal 2; (3, 6) = 18
    ([10, 12, 14, 16, 18, 20, 22, 24], 7),             # (d) eight calls two apart: all seven diagonals
    ([5, 5 + 16], 1),                                  # one pair at exactly max, two calls
)


# reads for the 16-bit-field form under 0 / 130: (relative positions, diagonals walked, the pair only the last diagonal holds)
FIELD_READS = (
    ([0, 131, 140, 145], 2, (1, 3)),                   # diagonal 1: (0, 1) = 131 beyond; (1, 2), (2, 3) adjacent across registers 0 | 1
    ([0, 100, 132, 135, 140], 3, (1, 4)),              # diagonal 2: (0, 2) = 132 beyond; (1, 3), (2, 4) adjacent across registers 0 | 1
)


def model_walk(rel, maxd=MAXD):
    """the stop rule on one read: the number of diagonals its lane asks for"""
    n, g = len(rel), 1
    while g < 7 and any(rel[j + g] - rel[j] <= maxd and rel[j + g + 1] - rel[j + 1] <= maxd for j in range(n - g - 1)):
        g += 1
    return g


_case = {}


def the_contig():
    if not _case:
        cg = Contig(7 * W, 401)
        rng = np.random.default_rng(403)
        # tile 0
        cg.random(starts_in(0, 700, 405, lo=100, hi=W - 600), kmax=8)
        # tile 1: counts in turn, starts strictly ascending so that the order of the reads is the order below
        counts = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 20)
        for i in range(300):
            k, s = counts[i % len(counts)], W + 300 + 11 * i
            rel = np.sort(rng.choice(RL - 1, size=k, replace=False))
            cg.add([s], [s + rel], None, MID_MAPQ if i % 3 == 1 else 40)
        # tile 2: one edge read per wave of 64 candidates, at lane 17, 18, ..
        sparse = np.arange(5) * 30
        for i in range(64 * len(EDGE_READS)):
            s = 2 * W + 300 + 5 * i
            e, lane = divmod(i, 64)
            rel = np.asarray(EDGE_READS[e][0] if lane == 17 + e else sparse)
            cg.add([s], [s + rel], None, 40)
        # tile 3: 300 reads on one start, then ordinary ones
        s0 = 3 * W + 400
        cg.add(np.full(300, s0), np.tile(s0 + np.asarray([3, 4, 20, 21, 22, 90]), (300, 1)), None, 40)
        cg.random(starts_in(3, 200, 407, lo=700, hi=W - 600), kmax=8)
        # tile 4: two waves of two-call reads, one field read in each
        for i in range(64 * len(FIELD_READS)):
            s = 4 * W + 300 + 5 * i
            e, lane = divmod(i, 64)
            rel = np.asarray(FIELD_READS[e][0] if lane == 20 + e else [3, 53])
            cg.add([s], [s + rel], None, 40)
        filler(cg, 5)
        c = cg.build()
        for rel, want, (j, k) in FIELD_READS:
            # the walk the rule asks for, a pair on its last diagonal, and the first pair of the diagonal before it beyond max
            assert model_walk(rel, 130) == want and k - j == want and rel[k] - rel[j] <= 130 and rel[want - 1] - rel[0] > 130, rel
        assert model_walk([3, 53], 130) == 1
        for rel, want in EDGE_READS:
            assert model_walk(rel) == want, (rel, model_walk(rel), want)
        assert model_walk(list(sparse)) == 1
        n = np.diff(c["cpg_off"].astype(np.int64))
        mq = c["read_mapq"]
        assert set(counts) <= set(n.tolist()) and ((mq == MID_MAPQ) & (n > 1)).sum() > 50 and (mq == 3).sum() > 20
        _case.update(c=c, reads=None, want={})
    return _case


def oracle(window, depth):
    cs = the_contig()
    if cs["reads"] is None:
        from metheor_amd import synth
        cs["reads"] = pyoracle.Reads.from_soa(*synth.to_oracle_soa(cs["c"]))
    key = (window, depth)
    if key not in cs["want"]:
        pk, lk = ("pdr", depth), ("lpmd", window)
        if pk not in cs["want"]:
            cs["want"][pk] = cs["reads"].pdr(min_depth=depth[0], min_cpgs=depth[1], min_qual=PDR_QUAL)
        if lk not in cs["want"]:
            cs["want"][lk] = cs["reads"].lpmd(min_distance=window[0], max_distance=window[1], min_qual=LPMD_QUAL)
        cs["want"][key] = (cs["want"][pk], cs["want"][lk])
    return cs["want"][key]


def all_forms(eng, monkeypatch, window, depth, rel16):
    from metheor_amd import PdrLpmdParams
    from tests import util
    c = the_contig()["c"]
    o, ol = oracle(window, depth)
    bt = util.device_batch(c, region=(0, c["length"]), device="cuda:0", rel16=rel16)
    params = PdrLpmdParams(min_depth=depth[0], min_cpgs=depth[1], min_qual=PDR_QUAL, min_distance=window[0], max_distance=window[1],
                           lpmd_min_qual=LPMD_QUAL)
    got = {}
    for form, env in FORMS.items():
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng.reset()
        eng.pdr_lpmd_accumulate(bt, params)
        d, l = eng.pdr_fetch(), eng.lpmd_global()
        tag = (form, window, depth, rel16)
        assert len(d["pos"]) == len(o), (tag, len(d["pos"]), len(o))
        assert (d["pos"] == o.pos[:, 0]).all() and (d["tid"] == o.tid).all(), tag
        assert (d["n_concordant"] == o.cnt[:, 0]).all() and (d["n_discordant"] == o.cnt[:, 1]).all(), tag
        assert (d["pdr"].view(np.uint32) == o.val.view(np.uint32)).all(), tag
        assert tuple(int(l[k]) for k in LPMD_KEYS) == tuple(int(ol[k]) for k in LPMD_KEYS), (tag, l, [int(ol[k]) for k in LPMD_KEYS])
        got[form] = (d, l)
    d0, l0 = got["tile256"]
    for form, (d, l) in got.items():
        assert all(d[k].tobytes() == d0[k].tobytes() for k in ROW_KEYS), (form, window, depth, rel16)
        assert all(int(l[k]) == int(l0[k]) for k in LPMD_KEYS), (form, window, depth, rel16)


def test_the_batch_holds_what_it_says():
    """not vacuous: pairs in every window, more of them as it widens, and the mapq-7 reads count for PDR only"""
    tot = {w: oracle(w, (0, 0))[1] for w in WINDOWS}
    pairs = {w: int(t["n_concordant"]) + int(t["n_discordant"]) for w, t in tot.items()}
    assert pairs[(0, 0)] == 0 and 0 < pairs[(1, 1)] < pairs[(2, 16)] < pairs[(0, 127)] and pairs[(2, 200)] > pairs[(2, 16)]
    c = the_contig()["c"]
    assert int(tot[(2, 16)]["n_valid_read"]) == int((c["read_mapq"] >= LPMD_QUAL).sum()) < int(tot[(2, 16)]["n_read"])
    assert len(oracle((2, 16), (0, 0))[0]) > 2000


@PIPE
@pytest.mark.parametrize("rel16", [False, True], ids=["rel8", "rel16"])
@pytest.mark.parametrize("window", WINDOWS, ids=["%d_%d" % w for w in WINDOWS])
def test_every_form_in_every_window(engines, monkeypatch, pipe, window, rel16):
    all_forms(engines[pipe], monkeypatch, window, (0, 0), rel16)
    if window == (2, 16):
        all_forms(engines[pipe], monkeypatch, window, (10, 4), rel16)      # the command line's min_depth / min_cpgs
