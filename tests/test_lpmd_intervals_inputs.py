"""The definition `lpmd --intervals` rests on, checked on the oracle alone (no device): for every interval of the test set,
`lpmd -c <all positions of the interval>` -- BismarkRead::filter_isin (readutil.rs:87-94), then the pairing of the calls that are left
(readutil.rs:166-224) -- counts exactly the rows of the unrestricted pairs table (lpmd.rs:70-87) with the interval's contig,
start <= cpg1 and cpg2 < end.  Also pins that the inputs of tests/test_gpu_lpmd_intervals.py hold the cases that can go wrong."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import lpmd_intervals_util as U


@pytest.fixture(scope="module")
def rec():
    return U.records()


@pytest.fixture(scope="module")
def per_tid(rec):
    """tid -> (record indices, their positions): the records of a contig, in file order"""
    return {t: (np.nonzero(rec.tid == t)[0], rec.pos[rec.tid == t]) for t in range(len(U.REFS))}


def by_cpg_set(rec, per_tid, t, b, e, **kw):
    """route 1: the reference's own restriction, on the records that can reach the interval (a record none of whose calls survives
    the filter adds to n_read only)"""
    idx, pos = per_tid[t]
    lo, hi = np.searchsorted(pos, b - 400, "left"), np.searchsorted(pos, e + 2, "right")
    e = min(e, U.REFS[t][1] + 2)
    if lo >= hi or b >= e:
        return 0, 0, U.lpmd_f32(0, 0)
    r = pyoracle.Reads.decode(rec.subset(idx[lo:hi]), cpg_set=[(t, p) for p in range(b, e)]).lpmd(**kw)
    return r["n_concordant"], r["n_discordant"], r["lpmd"]


@pytest.mark.parametrize("kw", [U.DEFAULT_KW, dict(min_distance=1, max_distance=3, min_qual=10), dict(min_distance=2, max_distance=16, min_qual=43)],
                         ids=["default", "m1_M3", "q43"])
def test_cpg_set_route_equals_the_summed_pairs_table(rec, per_tid, kw):
    iv = U.intervals()
    nc, nd = U.reduce_table(U.pairs_table(rec, **kw), iv)
    if kw is not U.DEFAULT_KW:
        iv_k = [x for k, x in enumerate(iv) if k % 9 == 0 or x[3] is not None and not x[3].startswith(("tile_", "slide_"))]
    else:
        iv_k = iv
    pick = {id(x): k for k, x in enumerate(iv)}
    for x in iv_k:
        k = pick[id(x)]
        c, d, v = by_cpg_set(rec, per_tid, x[0], x[1], x[2], **kw)
        assert (c, d) == (nc[k], nd[k]), (x, c, d, nc[k], nd[k])
        assert np.float32(v).view(np.uint32) == U.lpmd_f32(nc[k], nd[k]).view(np.uint32), x
    if kw["min_qual"] == 43:
        assert nc.sum() == 0 and nd.sum() == 0          # no read has such a mapq
    else:
        assert (nc + nd > 0).sum() > 200


def test_whole_file_is_the_global_counters(rec):
    """the rows of all contigs summed are LPMDResult's counters (lpmd.rs:11-12): the whole-contig intervals add up to them"""
    g = pyoracle.Reads.decode(rec).lpmd(**U.DEFAULT_KW)
    iv = [(t, 0, U.INT32_MAX, None) for t in range(3)]
    nc, nd = U.reduce_table(U.default_table(), iv)
    tid, p1, p2, c, d = U.default_table()
    minus = p1 < 0                                      # pairs whose first call lies at -1 belong to no interval
    assert minus.sum() >= 2
    assert nc.sum() + c[minus].sum() == g["n_concordant"] and nd.sum() + d[minus].sum() == g["n_discordant"]
    assert nc[2] == 0 and nd[2] == 0 and nc[0] > 100_000 and nc[1] > 10_000


def test_inputs_hold_the_cases_that_can_go_wrong(rec):
    tid, p1, p2, c, d = U.default_table()
    iv = U.intervals()
    nc, nd = U.reduce_table(U.default_table(), iv)
    named = {x[3]: k for k, x in enumerate(iv) if x[3]}
    assert 280 <= len(iv) <= 330
    rows = {(int(a), int(b)): int(x + y) for t, a, b, x, y in zip(tid, p1, p2, c, d) if t == 0}
    for tag, (q1, q2) in zip("sh", U.boundary_rows()):
        n_row = rows[(q1, q2)]
        assert n_row > 0
        k = named[tag + "_exact"]                       # start == cpg1 and end - 1 == cpg2: the row is in
        assert iv[k][1] == q1 and iv[k][2] - 1 == q2 and nc[k] + nd[k] >= n_row
        k = named[tag + "_end_on_cpg2"]                 # end == cpg2: cpg1 inside, cpg2 outside -- the row is out, others are in
        assert iv[k][2] == q2 and iv[k][1] <= q1 < iv[k][2]
        inside = sum(n for (a, b), n in rows.items() if iv[k][1] <= a and b < iv[k][2])
        straddling = sum(n for (a, b), n in rows.items() if iv[k][1] <= a < iv[k][2] <= b)
        assert nc[k] + nd[k] == inside > 0 and straddling >= n_row
        k = named[tag + "_start_past_cpg1"]
        assert iv[k][1] == q1 + 1 and nc[k] + nd[k] > 0
    # the island: more distinct pairs start in its 8192-bp tile than the pairs pass's LDS table holds (2048)
    assert ((tid == 0) & (p1 >= U.HOT_TILE[0]) & (p1 < U.HOT_TILE[1])).sum() > 2048
    assert ((tid == 0) & (p1 >= U.ISLAND[0]) & (p1 < U.ISLAND[1])).sum() > 2048        # (wherever a shifted contig's tiles are cut)
    assert nc[named["pairs_tile"]] > 0 and nc[named["nest_inner"]] > 0 and nc[named["nest_outer"]] > nc[named["nest_mid"]] > nc[named["nest_inner"]]
    assert nc[named["twin"]] > 0 and [x[3] for x in iv].count("twin") == 2
    assert nc[named["first_base"]] + nd[named["first_base"]] == 0 and nc[named["empty"]] + nd[named["empty"]] == 0
    # a reverse-strand read at position 0 calls at -1: its pairs (-1, 3) and (-1, 8) exist and lie in no interval, (3, 8) does
    assert rec.pos[0] == 0 and rec.flag[0] == 16
    assert rows[(-1, 3)] >= 12 and rows[(-1, 8)] >= 12 and rows[(3, 8)] >= 12
    k = named["after_minus_one"]
    assert nc[k] + nd[k] == sum(n for (a, b), n in rows.items() if 0 <= a and b < 9) >= 12
    assert nc[named["whole_a"]] + nd[named["whole_a"]] == sum(n for (a, b), n in rows.items() if a >= 0)
    # a deletion: the pair (+30, +50) is 15 query bases apart and 20 reference bases -- kept by relpos (readutil.rs:184-196), though
    # max_distance is 16; an insertion: (+48, +57) is 12 query bases apart
    assert rows[(U.INDEL_AT + 30, U.INDEL_AT + 50)] >= 10 and rows[(U.INS_AT + 48, U.INS_AT + 57)] >= 10
    assert (U.INDEL_AT + 30, U.INDEL_AT + 57) not in rows           # 22 query bases
    k = named["deletion_pair"]
    assert nc[k] + nd[k] >= 10 and nc[named["insertion"]] + nd[named["insertion"]] >= 10
