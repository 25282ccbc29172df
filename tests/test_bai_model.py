"""The index model of tests/bai_util.py, checked without a device: it reproduces the six samtools-made fixtures byte for byte,
the hand-made record set holds every case the GPU tests are meant to exercise, and mth_host_bai_write frames the model's tables
into the same bytes as the model's own framing."""
import os

import numpy as np
import pytest

from tests import bai_util as U


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_model_reproduces_the_samtools_fixture(golden_dir, k):
    bam = os.path.join(golden_dir, "test%d.bam" % k)
    assert U.bai_bytes(bam) == open(bam + ".bai", "rb").read()


def hand_index(limit=300):
    raw, off = U.pack(U.HAND)
    cuts = U.cuts_at_record_ends(off, limit)
    coffs = [(1 << 32) + 4242 + 131 * b for b in range(len(cuts) - 1)]
    return raw, off, cuts, coffs, U.index_rows(U.HAND, cuts, coffs, U.HAND_REF_LEN)


def test_hand_made_set_holds_what_it_must():
    H, LN = U.HAND, U.HAND_REF_LEN
    assert U.first_refusal(H, LN) is None
    placed = [r for r in H if r.ref >= 0]
    bins = [U.reg2bin(r.pos, U.end_of(r)) for r in placed]
    level = lambda b: sum(b >= s for s in (1, 9, 73, 585, 4681))
    assert {level(b) for b in bins} == {0, 1, 2, 3, 4, 5}                       # one record in each of the six bin levels
    for shift in (14, 17, 20, 23, 26):                                        # ... by a span that crosses each boundary
        assert any(r.pos >> shift != (U.end_of(r) - 1) >> shift and any(o == "N" for _, o in r.cigar) for r in placed)
    zero = [r for r in placed if U.reflen(r) == 0]
    assert any(r.cigar and all(o in "SI" for _, o in r.cigar) for r in zero) and any(not r.cigar for r in zero)
    assert any(r.flag & 4 for r in placed)                                    # placed-unmapped
    assert any(r.pos == 0 for r in placed)
    assert any(U.end_of(r) == LN[r.ref] for r in placed if r.ref == 0)
    assert LN[2] == 1 << 29 and any(r.ref == 2 and U.end_of(r) == 1 << 29 for r in placed)
    assert len(LN) == 3 and {r.ref for r in placed} == {0, 2}                 # the middle contig has no record
    assert [r.ref for r in H[-2:]] == [-1, -1] and all(r.ref >= 0 for r in H[:-2])
    # two runs of one bin separated by a record of its parent bin
    found = False
    for i in range(len(placed) - 2):
        a, p, b = bins[i], bins[i + 1], bins[i + 2]
        if a == b and a >= 4681 and p == 585 + ((a - 4681) >> 3) and placed[i].ref == placed[i + 1].ref == placed[i + 2].ref:
            found = True
    assert found


def test_hand_made_index_has_the_shape_the_cases_imply():
    raw, off, cuts, coffs, t = hand_index()
    assert isinstance(t, dict)
    sizes = np.diff(off.astype(np.int64))
    assert max(np.diff(cuts)) <= 300 and len(cuts) > 8
    ends = set(int(x) for x in off[1:])
    assert sum(1 for c in cuts[1:] if c in ends) >= 5                          # many records end exactly at a block's end
    spans = [np.searchsorted(cuts, int(off[k + 1]), "left") - (np.searchsorted(cuts, int(off[k]), "right") - 1) for k in range(len(sizes))]
    assert max(spans) >= 3                                                    # one record covers three blocks
    assert min(coffs) > 1 << 32
    assert list(t["ref_n_bins"]) == [int((t["bin_ref"] == 0).sum()), 0, int((t["bin_ref"] == 2).sum())] and t["ref_n_bins"][0] >= 6
    twice = [int(n) for r, b, n in zip(t["bin_ref"], t["bin_id"], t["bin_n_chunks"]) if b == 4681 + 512 and r == 0]
    assert twice == [2]                                                       # the bin the parent's record splits
    assert t["n_no_coor"] == 2 and list(t["ref_n_intv"]) == [(70_000_000 - 1 >> 14) + 1, 0, 1 << 15]
    assert int(t["meta"][0, 3]) == 1 and int(t["meta"][0, 2]) == sum(1 for r in U.HAND if r.ref == 0) - 1
    # a record that ends at a block's end keeps that block: its end offset's in-block part is the block's length, never 0
    vo = U.voffsets(off, cuts, coffs)
    at_end = [ve for (vb, ve), k in zip(vo, range(len(vo))) if int(off[k + 1]) in cuts]
    assert at_end and all(ve & 0xffff for ve in at_end)


@pytest.mark.parametrize("change,status,ordinal", [
    (lambda h: h[:4] + [h[5], h[4]] + h[6:], U.MTH_ERR_UNSORTED, 5),                          # pos descending inside a reference
    (lambda h: h[:17] + [U.rec(1, 10, "5M")] + [U.rec(0, 69999990, "5M")] + h[17:], U.MTH_ERR_UNSORTED, 18),      # refID descending
    (lambda h: h + [U.rec(2, 5, "5M")], U.MTH_ERR_UNSORTED, len(U.HAND)),                      # placed after unplaced
    (lambda h: h[:18] + [U.rec(2, (1 << 29) - 10, "40M")] + h[19:], U.MTH_ERR_RANGE, 18),      # ends beyond 2^29
    (lambda h: [U.rec(0, -1, "5M")] + h, U.MTH_ERR_RANGE, 0),                                  # pos < 0
    (lambda h: h[:17] + [U.rec(1, 4990, "20M")] + h[17:], U.MTH_ERR_RANGE, 17),                # ends beyond LN
    (lambda h: h[:19] + [U.rec(3, 5, "5M")] + h[19:], U.MTH_ERR_RANGE, 19),                    # refID >= n_ref
])
def test_model_refusals(change, status, ordinal):
    assert U.first_refusal(change(list(U.HAND)), U.HAND_REF_LEN) == (status, ordinal)
    assert U.first_refusal([U.rec(0, 5, "5M"), U.rec(0, 5, "7M")], U.HAND_REF_LEN) is None     # equal positions are fine


def test_host_writer_frames_the_tables(tmp_path):
    from metheor_amd import build, hostapi
    build.build_host()
    for t in (hand_index()[4], U.index_rows([], [0], [], [100, 200]), U.index_rows([], [0], [], [])):
        p = tmp_path / "x.bam.bai"
        p.write_bytes(b"stale")
        hostapi.bai_write(str(p), t)
        assert p.read_bytes() == U.frame(t)
        assert os.listdir(tmp_path) == ["x.bam.bai"]                          # the temporary name is gone
    # the framing is the one oracle.bamio reads back: bins, chunks and linear index of the hand-made set
    from oracle import bamio
    t = hand_index()[4]
    hostapi.bai_write(str(tmp_path / "h.bai"), t)
    refs = bamio.read_bai(str(tmp_path / "h.bai"))
    assert len(refs) == 3 and refs[1] == dict(bins={}, ioffset=[]) and len(refs[0]["bins"]) == int(t["ref_n_bins"][0])
    assert len(refs[0]["bins"][4681 + 512]) == 2
    # tables that do not add up are refused and nothing is written
    bad = dict(t); bad["bin_n_chunks"] = t["bin_n_chunks"].copy(); bad["bin_n_chunks"][0] += 1
    with pytest.raises(hostapi.HostError):
        hostapi.bai_write(str(tmp_path / "bad.bai"), bad)
    assert not (tmp_path / "bad.bai").exists()
