"""The inputs of tests/test_gpu_irregular_paths.py on the CPU: on small shuffled irregular instances the oracle, streaming the
records in file order, equals the transliteration of the reference (tools/gen_golden_unpinned.py) -- which pins the GPU tests'
reference on exactly this input -- and every input holds what its GPU test exists for: an order that changes the order-dependent
measures, flush traps that change rows, shard cuts and region edges at a read that starts at p and calls p - 1, and shard /
region plans that load every read of what they own."""
import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import irregular_util as I
from tests import test_irregular_inputs as T_in
from tests import unpinned_util as U
from tests import util

SHARD_N = (2, 5)
HALO = 4000


def _pin(rec):
    """test_oracle_equals_the_transliteration's bars for the order-dependent measures, on `rec` in its own (file) order"""
    G = T_in._translit()
    recs, rd = I.to_translit(rec), pyoracle.Reads.decode(rec)
    for p in (dict(min_depth=0, min_cpgs=0, min_qual=10), dict(min_depth=1, min_cpgs=2, min_qual=10)):
        t, want = rd.pdr(**p), G.pdr(recs, **p)
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [list(k) for k in want], p
        assert t.cnt.tolist() == [[v[1], v[2]] for v in want.values()]
        assert U.same_f32(t.val, [v[0] for v in want.values()])
    for p in (dict(min_depth=0, min_cpgs=1, min_qual=10), dict(min_depth=1, min_cpgs=2, min_qual=10)):
        t, want = rd.mhl(**p), G.mhl(recs, **p)
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [list(k) for k in want], p
        assert U.same_f32(t.val, list(want.values()), tol=1e-6)
    frec = I.fdrp_safe(rec)
    frecs, frd = I.to_translit(frec), pyoracle.Reads.decode(frec)
    for p in (dict(min_qual=10, min_depth=0, max_depth=100_000, min_overlap=0), dict(min_qual=10, min_depth=1, max_depth=100_000, min_overlap=35)):
        f, q, want = frd.fdrp(**p), frd.qfdrp(**p), G.fdrp_qfdrp(frecs, **p)
        keys = [list(k) for k in want]
        assert [[int(a), int(b)] for a, b in zip(f.tid, f.pos[:, 0])] == keys == [[int(a), int(b)] for a, b in zip(q.tid, q.pos[:, 0])], p
        assert f.cnt[:, 0].tolist() == [v[2] for v in want.values()]
        assert U.same_f32(f.val, [v[0] for v in want.values()]) and U.same_f32(q.val, [v[1] for v in want.values()]), p
    l, want = rd.lpmd(pairs=True, min_distance=1, max_distance=40, min_qual=10), G.lpmd(recs, min_distance=1, max_distance=40, min_qual=10)
    assert [l[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")] == \
        [want[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")]


@pytest.mark.parametrize("kind", I.ORDERS)
def test_oracle_equals_the_transliteration_in_file_order(kind):
    rec, _ = I.make_records(80 + I.ORDERS.index(kind), n_contigs=2, length=2_400, n_reads=130, density=0.05, unaligned=True)
    sh, _ = I.shuffle(rec, kind, np.random.default_rng(3))
    _pin(sh)


def _rows(rd, sub, **kw):
    t = getattr(rd, sub)(**kw)
    return {(int(a), int(b)): (int(np.float32(v).view(np.uint32)), tuple(int(x) for x in c)) for a, b, v, c in zip(t.tid, t.pos[:, 0], t.val, t.cnt)}


def _measures(rec):
    rd, frd = pyoracle.Reads.decode(rec), pyoracle.Reads.decode(I.fdrp_safe(rec))
    return dict(pdr=_rows(rd, "pdr", min_depth=1, min_cpgs=1, min_qual=10), mhl=_rows(rd, "mhl", min_depth=1, min_cpgs=1, min_qual=10),
                fdrp=_rows(frd, "fdrp", min_depth=1, max_depth=100_000, min_overlap=0, min_qual=10))


def _n_diff(a, b):
    return sum(1 for k in set(a) | set(b) if a.get(k) != b.get(k))


@pytest.mark.parametrize("seed", [0, 1])
def test_file_order_changes_the_order_dependent_measures(seed):
    """the unsorted GPU inputs (unsorted_records) in every order: the file-order oracle differs from the sorted one on >= 20 sites
    of each of PDR, MHL and FDRP"""
    rec = unsorted_records(seed)
    ref = _measures(rec)
    for kind in I.ORDERS:
        sh, _ = I.shuffle(rec, kind, np.random.default_rng(seed))
        got = _measures(sh)
        for m in ref:
            assert _n_diff(ref[m], got[m]) >= 20, (kind, m, _n_diff(ref[m], got[m]))


def unsorted_records(seed):
    """the input of the unsorted GPU tests: two contigs, every irregular class, records without an aligned base or a call"""
    rec, _ = I.make_records(900 + seed, n_contigs=2, length=8_000, n_reads=1_200, density=0.03, unaligned=True)
    return rec


def test_each_flush_trap_changes_rows():
    """flush_traps, one kind at a time, moved into the sorted order: far and other_contig records change PDR, MHL and FDRP rows at
    the trapped sites; low_mapq records change MHL's there and leave PDR and FDRP exactly as sorted (they flush MHL only); records
    without a call change nothing -- though each starts > 150 bp past its site, where a start-keyed flush would cut"""
    rec = unsorted_records(0)
    ref = _measures(rec)
    soa = pyoracle.Reads.decode(rec).soa()
    for kind in I.TRAPS:
        perm, traps = I.flush_traps(rec, np.random.default_rng(1), kinds=(kind,))
        assert len(traps) == 12, (kind, len(traps))
        got = _measures(rec.subset(perm))
        at = [(t, s) for _, t, s, _ in traps]
        n_at = {m: sum(1 for k in at if ref[m].get(k) != got[m].get(k)) for m in ref}
        if kind in ("far", "other_contig"):
            assert all(n_at[m] >= 3 for m in ref), (kind, n_at)
        elif kind == "low_mapq":
            assert n_at["mhl"] >= 3 and got["pdr"] == ref["pdr"] and got["fdrp"] == ref["fdrp"], (kind, n_at)
        else:
            assert got == ref
            assert all(int(soa["start"][x]) > s + 150 for _, _, s, x in traps)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    """the forced-boundary BAM of the shard and region tests: a block opens only before a read whose first call is at start - 1
    (and where the next record would not fit)"""
    rec, names, at = I.forced_records()
    d = tmp_path_factory.mktemp("forced")
    raw, bam = str(d / "raw.bam"), str(d / "f.bam")
    bamio.write_bam(raw, rec)
    targets = set(I.shifted_starts(rec).tolist())
    firsts = util.reblock_aligned(raw, bam, cut_before=targets)
    bamio.write_bai(bam)
    return rec, names, at, bam, targets, firsts


def region_edges(rec):
    """(tid, beg, end) of the region test: end = REGION_END; beg = a called site whose left neighbour is called too"""
    sites = I.called_sites(pyoracle.Reads.decode(rec)) & 0xffffffff
    sites = sites[(sites >= 4000) & (sites < 12000)]
    x = int(sites[1:][np.diff(sites) == 1][0])
    return 0, x, I.REGION_END


def test_shard_cuts_land_on_shifted_reads(forced):
    """--gpus N for N in SHARD_N: every interior cut (tid, p) opens at a record that starts at p and calls p - 1; one cut lies
    under the pile (reads starting at p fill several blocks: the right halo has to take them all), one inside a CG island"""
    from metheor_amd import hostapi
    rec, _, _, bam, targets, firsts = forced
    soa, n, first = I.read_calls(rec)
    sites = I.called_sites(pyoracle.Reads.decode(rec))
    f = hostapi.BamFile(bam)
    where = set()
    for N in SHARD_N:
        for r in range(N - 1):
            t, p = f.plan_shard(r, N, HALO)["end"]
            b1 = [j for j in firsts if (int(rec.tid[j]), int(rec.pos[j])) == (t, p)]
            assert b1 and b1[0] in targets, (N, r, t, p)
            assert int(soa["start"][b1[0]]) == p and int(first[b1[0]]) == p - 1
            if t == 0 and p == I.PILE_AT:
                where.add("pile")
            near = sites[(sites >> 32) == t] & 0xffffffff
            if ((near >= p - 10) & (near < p + 10)).sum() >= 8:
                where.add("island")
    assert where == {"pile", "island"}, where
    assert sum(1 for j in firsts if int(rec.tid[j]) == 0 and int(rec.pos[j]) == I.PILE_AT) >= 10


def test_shard_plans_load_every_reader(forced):
    """each shard's blocks hold every record that reports a call at a site the shard owns or starts inside it (mth_host_plan_shard:
    left halo, right halo of the reads that start exactly at the cut)"""
    from metheor_amd import hostapi
    rec, _, _, bam, _, _ = forced
    kb = I.record_blocks(bam)
    f = hostapi.BamFile(bam)
    for N in SHARD_N:
        for r in range(N):
            pl = f.plan_shard(r, N, HALO)
            need = I.readers(rec, pl["beg"], pl["end"])
            lo = 0 if pl["first_byte"] else pl["block_beg"]
            miss = need[(kb[need] < lo) | (kb[need] >= pl["block_end"])]
            assert len(miss) == 0, (N, r, pl, [(int(rec.pos[i]), int(rec.flag[i])) for i in miss[:5]])


def test_region_edges_and_plan(forced):
    """the region tid:beg+1-end: a read starting at end that reports end - 1, right after a block boundary, in a .bai bin that a
    query for [.., end) does not touch; sites beg - 1 and beg both called; the plan's blocks hold every reader of [beg, end)"""
    from metheor_amd import hostapi
    rec, _, at, bam, _, firsts = forced
    t, b, e = region_edges(rec)
    soa, n, first = I.read_calls(rec)
    assert int(soa["start"][at]) == e and int(first[at]) == e - 1 and at in firsts
    sites = I.called_sites(pyoracle.Reads.decode(rec))
    assert ((t << 32) | (b - 1)) in sites and ((t << 32) | b) in sites
    refs = bamio.read_bai(bam + ".bai")
    lo_hi = bamio.bai_query(refs, t, 0, e)
    kb = I.record_blocks(bam)
    assert lo_hi is not None and (lo_hi[1] >> 16) < (bamio.bam_record_offsets(bam)[0][at][3] >> 16)    # [.., end) stops before it
    f = hostapi.BamFile(bam)
    pl = f.plan_region(t, b, e)
    need = I.readers(rec, (t, b), (t, e))
    assert at in set(need.tolist())
    lo = 0 if pl["first_byte"] else pl["block_beg"]
    miss = need[(kb[need] < lo) | (kb[need] >= pl["block_end"])]
    assert len(miss) == 0, [(int(rec.pos[i]), int(rec.flag[i])) for i in miss[:5]]
