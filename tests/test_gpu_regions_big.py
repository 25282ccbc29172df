"""The read x interval passes (`mhl-regions`, `pdr-regions`, `me-regions` / `pm-regions`) on slices whose searches take more than one
round of 64 probes (iv_upper_wave, mth_intervals_dev.h: a second round above 4096 entries of one length class, a third above 262 144),
and all four per-interval passes at the top of the coordinate range, where an interval may end at INT32_MAX -- the value that also
stands for "no eligible read" in a work item's span.  Against the restatements of the utility modules, at the per-pass modules' bars."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import lpmd_intervals_util as L
from tests import mhl_regions_util as M
from tests import pdr_regions_util as P
from tests import quartet_regions_util as Q
from tests import regions_fuzz_util as U
from tests import test_gpu_mhl_regions as T_mhl
from tests import test_gpu_pairs as T_pairs
from tests import test_gpu_pdr_regions as T_pdr
from tests import test_gpu_quartet_regions as T_quartet
from tests import util
from tests.test_gpu_regions_fuzz import arrays, check_lpmd, engine
from tests.test_gpu_regions_work_items import shared  # noqa: F401  (the fixture: the default records as a decoded stream)

pytestmark = pytest.mark.gpu

INT32_MAX = U.INT32_MAX


# ---- two rounds ----------------------------------------------------------------------------------------------------------------------------
def two_round_set():
    """contig ivA tiled at 40 bp (5000 windows, one length class) and 5000 copies of one of the windows inside the island: 10 000
    entries in a slice, with a run of equal starts longer than a step of the first round's probes (10 000 / 64)"""
    dup = (0, 66_960, 67_000, "dup")
    iv = [(0, b, b + 40, None) for b in range(0, L.REFS[0][1], 40)] + [dup] * 5000
    assert len(iv) == 10_000 and dup[:3] == iv[66_960 // 40][:3] and len(set(U.length_class(e - b) for _, b, e, _ in iv)) == 1
    return iv


@pytest.mark.parametrize("grid", [None, 1])
def test_two_search_rounds(shared, grid):
    iv = two_round_set()
    nar = U.Narrowed(M.default_calls())
    with engine(grid) as eng:
        eng.mhl_regions_begin(*arrays(iv))
        T_mhl.feed(eng, shared, "groups", min_cpgs=1, min_qual=10)
        want = U.restate_mhl(nar, iv, 10, min_cpgs=1, min_qual=10)
        assert np.isfinite(want[0]).sum() > 5000 + 500 and want[1][-1] > 100
        T_mhl.check(eng.mhl_regions_fetch(min_depth=10), want, "two rounds")
    with engine(grid) as eng:
        eng.pdr_regions_begin(*arrays(iv))
        T_pdr.feed(eng, shared, "groups", min_cpgs=1, min_qual=10)
        want = U.restate_pdr(nar, iv, 10, min_cpgs=1, min_qual=10)
        assert np.isfinite(want[0]).sum() > 5000 + 500 and want[3][-1] > 0
        T_pdr.check(eng.pdr_regions_fetch(min_depth=10), want, "two rounds")
    with engine(grid) as eng:
        eng.quartet_regions_begin(*arrays(iv))
        T_quartet.feed(eng, shared, "groups", min_qual=10)
        want = U.restate_quartet(nar, iv, 10, 10)
        assert np.isfinite(want[0]).sum() >= 5000 and want[3][-1] > 100       # (four calls within 40 bases: the island's windows)
        T_quartet.check(eng.quartet_regions_fetch(min_depth=10), want, "two rounds")
        T_quartet.check_counts(eng.quartet_regions_counts(), want, "two rounds")


# ---- three rounds ----------------------------------------------------------------------------------------------------------------------------
N_WIN, WIN = 262_145 + 64, 8


def three_round_contig():
    """at most 2000 reads of 100 bases on a contig of N_WIN adjacent 8-bp windows: over the first windows, over the last ones, around
    the windows the first round's probes fall on (index k x step - 1, k x step, k x step + 1 for step = ceil(N_WIN / 64)), and beyond
    the last window; one site in every window"""
    from metheor_amd import synth
    rng = np.random.default_rng(77)
    length = N_WIN * WIN + 5_000
    step = -(-N_WIN // 64)
    starts = [rng.integers(0, 1_500, 300), rng.integers(N_WIN * WIN - 1_600, N_WIN * WIN - 60, 300), rng.integers(N_WIN * WIN + 10, length - 200, 150)]
    for k in (1, 2, 3, 17, 32, 33, 62, 63):
        starts.append(rng.integers((k * step - 1) * WIN - 90, (k * step + 2) * WIN, 120))
    starts = np.sort(np.concatenate(starts)).astype(np.int32)
    assert len(starts) <= 2000 and starts.min() >= 0
    return synth.make_contig(0, length, None, None, rng, read_len=100, sites=np.arange(3, length - 8, WIN, dtype=np.int32), starts=starts), step


def test_three_search_rounds_pdr():
    from metheor_amd import synth
    c, step = three_round_contig()
    beg = np.arange(N_WIN, dtype=np.int64) * WIN
    t_, b_, e_ = np.zeros(N_WIN, np.int32), beg.astype(np.int32), (beg + WIN).astype(np.int32)
    calls = M.Calls.from_soa(*synth.to_oracle_soa(c))
    nar = U.Narrowed(calls)
    hit = np.unique(calls.pos // WIN)
    assert (calls.pos >= N_WIN * WIN).sum() > 100                            # calls beyond the last window
    hit = hit[hit < N_WIN]
    assert {0, N_WIN - 1} <= set(hit.tolist()) and all(k * step + d in hit for k in (1, 17, 63) for d in (-1, 0, 1)) and 500 < len(hit) < 5000
    iv = [(0, int(k) * WIN, int(k) * WIN + WIN, None) for k in hit]
    want = U.restate_pdr(nar, iv, 1, min_cpgs=1, min_qual=10)
    assert (want[1] + want[2] + want[3]).sum() > 5000
    with engine() as eng:
        eng.pdr_regions_begin(t_, b_, e_)
        b = util.device_batch(c)
        eng.pdr_regions_accumulate(b, min_cpgs=1, min_qual=10)
        got = eng.pdr_regions_fetch(min_depth=1)
    T_pdr.check({k: v[hit] for k, v in got.items()}, want, "three rounds")
    rest = np.ones(N_WIN, bool)
    rest[hit] = False
    assert np.isnan(got["pdr"][rest]).all() and not got["n_concordant"][rest].any() and not got["n_discordant"][rest].any()


# ---- high coordinates --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,top", [(3, 2 ** 31 - 1), (7, 2 ** 31 - 1), (11, 2 ** 30 + 5000)])
def test_high_coordinates(seed, top):
    """the contigs of tests/test_gpu_fuzz.py's test_high_coordinates as a region batch, with intervals that end at INT32_MAX, tile the
    last 3000 bases, hold the last base before INT32_MAX and hold the last called position alone"""
    from metheor_amd import synth
    from tests import test_gpu_fuzz as F
    _, cs, _, _ = F.scenario(seed)
    off = top - cs[0]["length"]
    hc = F.shift_contig(cs[0], off)
    region = (off - 1000, hc["length"])
    soa = synth.to_oracle_soa(hc)
    reads, calls = pyoracle.Reads.from_soa(*soa), M.Calls.from_soa(*soa)
    last = int(calls.pos.max())
    iv = [(0, top - 3000, INT32_MAX, "tail_open"), (0, 0, INT32_MAX, "open")] + [(0, b, b + 100, None) for b in range(top - 3000, top, 100)] + \
         [(0, 2 ** 31 - 2, INT32_MAX, "last_base"), (0, last, last + 1, "last_call")]
    assert last < INT32_MAX and all(e <= INT32_MAX for _, _, e, _ in iv)
    lk = dict(min_distance=1, max_distance=40, min_qual=10)
    kw = dict(min_cpgs=1, min_qual=10)
    with engine() as eng:
        T_pairs.run_device(eng, [hc], lk, regions=[[region]])
        want = L.reduce_table(U.pairs_table(reads, lk), iv)
        assert want[0][1] + want[1][1] > 0
        check_lpmd(eng.lpmd_intervals_fetch(*arrays(iv)), want)
    with engine() as eng:
        eng.mhl_regions_begin(*arrays(iv))
        eng.mhl_regions_accumulate(util.device_batch(hc, region=region), **kw)
        want = M.restate(calls, iv, min_depth=1, **kw)
        assert want[1][1] > 0 and (want[1][0] > 0 or seed == 11)            # (seed 11: no call in the last 3000 bases)
        T_mhl.check(eng.mhl_regions_fetch(min_depth=1), want, top)
    with engine() as eng:
        eng.pdr_regions_begin(*arrays(iv))
        b = util.device_batch(hc, region=region)
        eng.pdr_regions_accumulate(b, **kw)
        T_pdr.check(eng.pdr_regions_fetch(min_depth=1), P.restate(calls, iv, min_depth=1, **kw), top)
    with engine() as eng:
        eng.quartet_regions_begin(*arrays(iv))
        b = util.device_batch(hc, region=region)
        eng.quartet_regions_accumulate(b, min_qual=10)
        want = Q.restate(calls, iv, min_depth=1, min_qual=10)
        T_quartet.check(eng.quartet_regions_fetch(min_depth=1), want, top)
        T_quartet.check_counts(eng.quartet_regions_counts(), want, top)
