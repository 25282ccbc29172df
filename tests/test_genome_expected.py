"""The expectations the `--genome` tests compare the device with, pinned on the CPU (no GPU, passes without the feature):
the generator's conditions, the plain-record rule of k_decode_genome restated in Python against the oracle chain
(pyoracle.tag_xm, then the decode's walk), and the chain on the reference's own fixture."""
import os

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import genome_util as gu
from tests import tag_util


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_generated_inputs_are_worth_comparing(seed):
    gen = gu.generate(seed)
    assert len(gen["recs"]) == 6000 and gen["paired"] == (seed >= 3)
    recs, xms = gu.runnable(gen)                                  # asserts that at most 1 % of the records panic
    n_empty = sum(1 for x in xms if not x)
    assert any(any((c & 15) not in (0, 4, 5) for c in r[4]) for r in recs) and 0 < n_empty < len(recs) // 20
    rd = gu.expected_reads([(gen["name"], len(gen["contig"]))], recs, xms)
    soa = rd.soa()
    print("seed %d: %d records kept, %d empty XM, %d calls" % (seed, len(recs), n_empty, len(soa["cpg_pos"])))
    assert len(soa["cpg_pos"]) > 30000
    # the oracle's decode is the walk restated in genome_util (used per record by the plain-rule test below)
    k = 0
    for i, (r, x) in enumerate(zip(recs, xms)):
        for q, p, meth in gu.decode_walk(r[1], r[2], r[4], x):
            assert (int(soa["cpg_rel"][k]), int(soa["cpg_pos"][k] & 0x7fffffff), bool(soa["cpg_pos"][k] >> 31)) == (q, p, meth), (i, k)
            k += 1
        assert k == int(soa["cpg_off"][i + 1])
    rows = dict(pdr=len(rd.pdr()), mhl=len(rd.mhl()), me=len(rd.me()), pm=len(rd.pm()), fdrp=len(rd.fdrp()))
    lp = rd.lpmd()
    print("seed %d rows: %s, lpmd %d / %d" % (seed, rows, lp["n_concordant"], lp["n_discordant"]))
    assert rows["pdr"] >= 500 and rows["mhl"] >= 500 and rows["fdrp"] >= 500 and rows["me"] >= 100 and rows["pm"] >= 100
    assert lp["n_concordant"] > 1000 and lp["n_discordant"] > 1000


def test_plain_record_rule_equals_the_chain():
    n_calls = n_panic = n_rec = 0
    for seed in (101, 102, 103):
        for pos, flag, cig, seq, contig, paired in gu.random_plain_records(seed, 8000):
            xm = pyoracle.tag_xm(pos, flag, cig, seq, contig, is_paired_end=paired)
            want = None if xm is None else gu.decode_walk(pos, flag, cig, xm)
            got = gu.plain_rule(pos, flag, cig, seq, contig, paired)
            assert got == want, (pos, flag, cig, seq, contig, paired, xm)
            n_rec += 1
            n_panic += want is None
            n_calls += len(want or [])
    print("%d plain records, %d calls, %d panics" % (n_rec, n_calls, n_panic))
    assert n_rec >= 20000 and n_calls > 20000 and n_panic > 100


def test_chain_reproduces_the_reference_fixture(golden_dir):
    hdr, reads, _, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    contig = bytes(contig)
    rec = bamio.read_sam(os.path.join(golden_dir, "test.chr19.XM.sam"))
    xms = [pyoracle.tag_xm(r.pos, r.flag, r.cigar, r.seq.encode(), contig, is_paired_end=bool(reads[0].flag & 1)) for r in reads]
    assert len(xms) == 1000 and [x.decode() for x in xms] == [r.xm for r in reads]
    want = pyoracle.Reads.decode(rec).soa()
    got = pyoracle.Reads.decode(bamio.Records(rec.refs, rec.tid, rec.pos, rec.flag, rec.mapq, rec.cigars, xms)).soa()
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    assert len(want["cpg_pos"]) > 500
