"""mth_bai_begin / mth_bai_add_records / mth_bai_finish against the model of tests/bai_util.py: the hand-made record set (every
bin level, zero-length and placed-unmapped records, contig ends, an empty contig, trailing records without a contig, a bin
split by its parent's record) on 300-byte blocks whose file offsets start above 2^32, the same set under every window split,
70 000 generated records as one window and as three, every refusal, and determinism."""
import numpy as np
import pytest

from tests import bai_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


def layout(records, limit, coff0=(1 << 32) + 4242):
    raw, off = U.pack(records)
    cuts = U.cuts_at_record_ends(off, limit)
    coffs = [coff0 + 131 * b for b in range(len(cuts) - 1)]
    return raw, off, cuts, coffs


def feed(eng, raw, off, cuts, coffs, ref_len, splits):
    """the records as windows [splits[k], splits[k + 1]): every window gets its own stream (offsets from 0) and the cuts that fall
    inside it -- the splits lie on cuts -- with the blocks' file offsets"""
    eng.bai_begin(ref_len)
    cuts = [int(c) for c in cuts]
    for a, b in zip(splits[:-1], splits[1:]):
        o0, o1 = int(off[a]), int(off[b])
        assert o0 in cuts and o1 in cuts
        k0, k1 = cuts.index(o0), cuts.index(o1)
        eng.bai_add_records(raw[o0:o1], off[a:b + 1] - off[a], [c - o0 for c in cuts[k0:k1 + 1]], coffs[k0:k1])
    return eng.bai_finish()


@pytest.fixture(scope="module")
def hand():
    raw, off, cuts, coffs = layout(U.HAND, 300)
    return dict(raw=raw, off=off, cuts=cuts, coffs=coffs, want=U.index_rows(U.HAND, cuts, coffs, U.HAND_REF_LEN))


def test_hand_made_set_equals_the_model(eng, hand):
    got = feed(eng, hand["raw"], hand["off"], hand["cuts"], hand["coffs"], U.HAND_REF_LEN, [0, len(U.HAND)])
    assert U.same_tables(got, hand["want"]) == []
    assert got["n_records"] == len(U.HAND) and int(got["chunk_beg"].min()) >> 16 > 1 << 32
    assert U.frame(got) == U.frame(hand["want"])


def one_record_cuts(records):
    """every record a block of its own (records longer than 300 bytes fill several): any record boundary is a cut"""
    raw, off = U.pack(records)
    cuts = [0]
    for k in range(len(records)):
        while int(off[k + 1]) - cuts[-1] > 300:
            cuts.append(cuts[-1] + 300)
        cuts.append(int(off[k + 1]))
    return raw, off, cuts, [(1 << 32) + 99 + 77 * b for b in range(len(cuts) - 1)]


@pytest.mark.parametrize("name,splits", [
    ("one window", None),
    ("one-record windows", "each"),
    ("inside a run of one bin", [0, 12]),          # records 11 and 12 share bin 4681 + 512
    ("at a run boundary", [0, 13]),
    ("at a contig change", [0, 17]),
    ("before the first record without a contig", [0, 19]),
    ("all of them", [0, 12, 13, 17, 19]),
])
def test_window_splits_do_not_change_the_index(eng, name, splits):
    raw, off, cuts, coffs = one_record_cuts(U.HAND)
    want = U.index_rows(U.HAND, cuts, coffs, U.HAND_REF_LEN)
    n = len(U.HAND)
    sp = [0, n] if splits is None else list(range(n + 1)) if splits == "each" else splits + [n]
    got = feed(eng, raw, off, cuts, coffs, U.HAND_REF_LEN, sp)
    assert U.same_tables(got, want) == [], name
    assert U.frame(got) == U.frame(want)


@pytest.fixture(scope="module")
def gen():
    records, ref_len = U.generated()
    raw, off = U.pack(records)
    limit = int(off[-1]) // 1000
    assert limit < 0xff00
    cuts = U.cuts_at_record_ends(off, limit)
    coffs = [(5 << 32) + 40_000 * b for b in range(len(cuts) - 1)]
    return dict(records=records, ref_len=ref_len, raw=raw, off=off, cuts=cuts, coffs=coffs, want=U.index_rows(records, cuts, coffs, ref_len))


def test_generated_records_one_window_and_three(eng, gen):
    n = len(gen["records"])
    assert n == 70_000 and 900 <= len(gen["cuts"]) - 1 <= 1200 and max(gen["ref_len"]) > 1 << 26
    assert len(gen["want"]["chunk_beg"]) > 10_000
    got1 = feed(eng, gen["raw"], gen["off"], gen["cuts"], gen["coffs"], gen["ref_len"], [0, n])
    assert U.same_tables(got1, gen["want"]) == []
    # three windows, split at the record ends that are cuts nearest to the thirds
    ends = {int(gen["off"][k]): k for k in range(n + 1)}
    at = [ends[c] for c in gen["cuts"] if c in ends]
    sp = [0] + [min(at, key=lambda k: abs(k - n * j // 3)) for j in (1, 2)] + [n]
    got3 = feed(eng, gen["raw"], gen["off"], gen["cuts"], gen["coffs"], gen["ref_len"], sp)
    assert U.same_tables(got3, gen["want"]) == []
    assert U.frame(got1) == U.frame(got3) == U.frame(gen["want"])
    # determinism: a second run of the same input is byte-identical
    again = feed(eng, gen["raw"], gen["off"], gen["cuts"], gen["coffs"], gen["ref_len"], [0, n])
    assert U.frame(again) == U.frame(got1)
    for k in ("chunk_beg", "chunk_end", "bin_id", "bin_n_chunks", "lin", "meta"):
        assert np.array_equal(again[k], got1[k]), k


H = U.HAND
REFUSALS = [
    ("pos descending", H[:4] + [H[5], H[4]] + H[6:]),
    ("refID descending", H[:17] + [U.rec(1, 10, "5M"), U.rec(0, 69999990, "5M")] + H[17:]),
    ("placed after unplaced", H + [U.rec(2, 5, "5M")]),
    ("ends beyond 2^29", H[:18] + [U.rec(2, (1 << 29) - 10, "40M")] + H[19:]),
    ("pos < 0", [U.rec(0, -1, "5M")] + H),
    ("ends beyond LN", H[:17] + [U.rec(1, 4990, "20M")] + H[17:]),
    ("refID >= n_ref", H[:19] + [U.rec(3, 5, "5M")] + H[19:]),
    ("two offenders: the lower one is reported", H[:4] + [H[5], H[4]] + H[6:17] + [U.rec(1, 4990, "20M")] + H[17:]),
]


@pytest.mark.parametrize("name,records", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, hand, name, records):
    import metheor_amd
    raw, off, cuts, coffs = one_record_cuts(records)
    want = U.index_rows(records, cuts, coffs, U.HAND_REF_LEN)
    assert want[0] == "error"
    _, status, ordinal = want
    n = len(records)
    # inside one window; with the offending record first in a window of its own (its predecessor in the window before)
    for sp in ([0, n], [0, ordinal, n] if 0 < ordinal else [0, 1, n]):
        with pytest.raises(metheor_amd.MthError) as e:
            feed(eng, raw, off, cuts, coffs, U.HAND_REF_LEN, sp)
        assert e.value.status == status, (name, sp)
        assert "record %d " % ordinal in str(e.value), (name, sp, str(e.value))
        if "2^29" in name:
            assert ".csi" in str(e.value)
        # finish returns the same error and no tables, and ends the index
        with pytest.raises(metheor_amd.MthError) as e:
            eng.bai_finish()
        assert e.value.status == status and "record %d " % ordinal in str(e.value)
        with pytest.raises(metheor_amd.MthError) as e:
            eng.bai_finish()
        assert e.value.status == -9                                # MTH_ERR_STATE: no index in progress
    # the context is as good as new
    got = feed(eng, hand["raw"], hand["off"], hand["cuts"], hand["coffs"], U.HAND_REF_LEN, [0, len(U.HAND)])
    assert U.same_tables(got, hand["want"]) == []


def test_an_empty_block_behind_the_last_record_is_its_end(eng):
    """the EOF block: bgzf_tell after the file's last record names the block that follows, which oracle.bamio's rule gives for an
    empty block -- in one call, or announced by a call without records"""
    recs = [r for r in U.HAND if r.ref >= 0]
    raw, off, cuts, coffs = layout(recs, 300)
    eof = coffs[-1] + 500
    want = U.index_rows(recs, cuts + [cuts[-1]], coffs + [eof], U.HAND_REF_LEN)
    assert int(want["meta"][2, 1]) == eof << 16
    eng.bai_begin(U.HAND_REF_LEN)
    eng.bai_add_records(raw, off, cuts + [cuts[-1]], coffs + [eof])
    assert U.same_tables(eng.bai_finish(), want) == []
    eng.bai_begin(U.HAND_REF_LEN)
    eng.bai_add_records(raw, off, cuts, coffs)
    eng.bai_add_records(b"", [0], [0, 0], [eof])
    assert U.same_tables(eng.bai_finish(), want) == []
    # nothing to index: every reference empty
    eng.bai_begin([100, 200])
    got = eng.bai_finish()
    assert U.same_tables(got, U.index_rows([], [0], [], [100, 200])) == [] and got["n_records"] == 0
