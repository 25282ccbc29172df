"""The inputs of tests/test_gpu_contig_start.py on the CPU, on the oracle alone: the two call_at_minus_one cases of
tests/golden/unpinned_cases.json.gz hold what the GPU tests exist for -- a row or key at position -1 on both contigs in every
measure, the pair (-1, 1), an unsorted order whose tables differ from those the engine's old ordering of the word gives (position
-1 read as 2^31 - 1: the last key of its contig, a first-CpG that flushes every open site of it), and a host decode that carries
the word -- so that a later edit cannot quietly make them trivial.  And the oracle reads its own SoA back with -1 intact."""
import importlib.util
import os

import numpy as np
import pytest

from metheor_amd import hostapi
from oracle import bamio, pyoracle
from tests import contig_start_util as S
from tests import irregular_util as I
from tests import unpinned_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[S.SORTED, S.UNSORTED])
def loaded(request):
    rec = S.records(request.param)
    return request.param, rec, S.decode(rec)


def test_shape_of_the_cases(loaded):
    name, rec, _ = loaded
    assert len(rec.refs) == 2 and len(rec) < 100
    for tid in (0, 1):
        at0 = [i for i in S.minus_one_records(rec) if rec.tid[i] == tid]
        assert {16, 1024, 83} <= {int(rec.flag[i]) for i in at0}
        assert any(rec.xms[i].startswith(b"Z.Z.z") and rec.flag[i] == 1024 for i in at0)            # calls -1, 1, 3
        assert any(sum(c in b"zZ" for c in rec.xms[i]) >= 4 for i in at0)                           # a quartet that starts at -1
        assert any(rec.mapq[i] < 10 for i in at0)
        assert any(len(rec.xms[i]) == 201 for i in at0)                                             # site -1's FDRP window ends at 200
        assert any(rec.pos[i] == 0 and rec.flag[i] == 0 for i in range(len(rec)) if rec.tid[i] == tid)
    order = list(zip(rec.tid.tolist(), rec.pos.tolist()))
    assert (order == sorted(order)) == (name == S.SORTED)
    if name == S.UNSORTED:
        # position-0 reads behind later reads of their contig, and behind reads of the other contig
        for i in S.minus_one_records(rec):
            assert any(rec.tid[j] == rec.tid[i] and rec.pos[j] > 0 for j in range(i))
        assert any(rec.tid[i] == 0 and (rec.tid[:i] == 1).any() for i in S.minus_one_records(rec))
        s = S.records(S.SORTED)
        key = lambda r: sorted(zip(r.tid.tolist(), r.pos.tolist(), r.flag.tolist(), r.mapq.tolist(), r.xms))
        assert key(rec) == key(s)                                                                   # the same records


def test_every_measure_has_minus_one_on_both_contigs(loaded):
    _, _, rd = loaded
    tabs, _ = S.seven_tables(rd)
    for k, t in tabs.items():
        for tid in (0, 1):
            rows = t.pos[t.tid == tid]
            assert len(rows) and (rows[:, 0] == -1).any(), (k, tid)
            if k not in ("me", "pm"):                                    # (HashMap order there)
                assert rows[0, 0] == -1, (k, tid)                        # the first row of its contig
    p = tabs["pairs"]
    for tid in (0, 1):
        assert any(t == tid and a == -1 and b == 1 for t, (a, b) in zip(p.tid.tolist(), p.pos.tolist())), tid


def test_from_soa_reads_the_word_back_as_minus_one(loaded):
    """Reads.from_soa(*decode(rec).soa()) gives the seven tables of Reads.decode(rec)"""
    _, _, rd = loaded
    soa = rd.soa()
    assert ((soa["cpg_pos"] & S.WORD) == S.WORD).sum() >= 10
    back = pyoracle.Reads.from_soa(**soa)
    a, ga = S.seven_tables(rd)
    b, gb = S.seven_tables(back)
    assert ga == gb
    for k in a:
        assert len(a[k]) and S.same_table(a[k], b[k]), k
    assert (back.soa()["cpg_pos"] == soa["cpg_pos"]).all()


@pytest.mark.parametrize("which", ["sorted", "one_contig", "reservoir_unsorted"])
def test_reservoir_draw_at_minus_one_matters(which):
    """under -d 3 -D 3 site -1 of every contig takes more arrivals than slots, and its row changes with the draw: over the seeds of
    the GPU runs the rows at -1 take at least three different values per contig, so a draw keyed by another site or contig
    (orc_sample_j is keyed by (seed, tid, position, arrivals)) cannot give all of them"""
    rec = S.records(S.SORTED)
    rec = {"sorted": rec, "one_contig": S.one_contig(rec, 1), "reservoir_unsorted": S.reservoir_unsorted(rec)}[which]
    if which == "reservoir_unsorted":
        order = list(zip(rec.tid.tolist(), rec.pos.tolist()))
        assert order != sorted(order) and rec.tid.tolist() == sorted(rec.tid.tolist())
    rd = S.decode(rec)
    per_seed = [S.rows_at_minus_one(rd, seed) for seed in S.RES_SEEDS]
    for tid in sorted(set(rec.tid.tolist())):
        rows = [r for rs in per_seed for r in rs if r[0] == tid]
        assert len(rows) == len(S.RES_SEEDS) and all(r[3] == 3 for r in rows), (tid, rows)
        assert len({r[1:3] for r in rows}) >= 3, (tid, rows)
        # the draws themselves: the fourth arrival's slot differs between the seeds, and from the draw of the same site on the other tid
        js = [pyoracle.sample_j(seed, tid, -1, 4) for seed in S.RES_SEEDS]
        assert len(set(js)) >= 3, js
    assert any(pyoracle.sample_j(seed, 0, -1, 4) != pyoracle.sample_j(seed, 1, -1, 4) for seed in S.RES_SEEDS)


def _translit():
    spec = importlib.util.spec_from_file_location("gen_golden_unpinned", os.path.join(ROOT, "tools", "gen_golden_unpinned.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_unsorted_tables_differ_from_the_old_ordering():
    """the same records with every call at -1 moved to 2147483647 -- how the engine ordered the word 0x7fffffff -- then relabelled
    back: other rows than the reference's in PDR and MHL (FDRP / qFDRP share MHL's flush rule; their 403-slot window has no place for a
    call 2^31 positions away, so the restatement cannot state the old ordering for them)"""
    G = _translit()
    c = S.case(S.UNSORTED)
    recs = I.to_translit(U.records_of(c))
    true_read = G.bismark_read

    def old(r):
        br = true_read(r)
        for cpg in br["cpgs"]:
            if cpg["abspos"][1] == -1:
                cpg["abspos"] = (cpg["abspos"][0], 2147483647)
        return br

    def relabel(res):
        return sorted(((k[0], -1 if k[1] == 2147483647 else k[1]), tuple(np.float32(x).view(np.uint32) if isinstance(x, np.float32) else x for x in (v if isinstance(v, tuple) else (v,))))
                      for k, v in res.items())

    p = dict(min_depth=1, min_qual=10)
    want = dict(pdr=relabel(G.pdr(recs, min_cpgs=0, **p)), mhl=relabel(G.mhl(recs, min_cpgs=1, **p)))
    G.bismark_read = old
    try:
        got = dict(pdr=relabel(G.pdr(recs, min_cpgs=0, **p)), mhl=relabel(G.mhl(recs, min_cpgs=1, **p)))
    finally:
        G.bismark_read = true_read
    for k in want:
        assert len(want[k]) > 50 and got[k] != want[k], k
    # ... and the reference's rows are the fixture's
    e = next(x for x in c["expect"]["pdr"] if x["params"] == dict(min_depth=1, min_cpgs=0, min_qual=10))
    assert [(k[0], k[1]) for k, _ in want["pdr"]] == [(r[0], r[1]) for r in e["rows"]]


def test_host_decode_carries_the_word(loaded, tmp_path):
    _, rec, rd = loaded
    bam = str(tmp_path / "in.bam")
    bamio.write_bam(bam, rec)
    f = hostapi.BamFile(bam)
    try:
        soa = f.decode()
    finally:
        f.close()
    want = rd.soa()
    for k in ("tid", "start", "end", "mapq", "cpg_off", "cpg_pos", "cpg_rel"):
        assert (soa[k] == want[k]).all(), k
    at0 = S.minus_one_records(rec)
    assert len(at0) >= 12
    for i in at0:
        assert soa["start"][i] == 0 and (int(soa["cpg_pos"][int(soa["cpg_off"][i])]) & S.WORD) == S.WORD, i
