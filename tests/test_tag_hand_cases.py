"""`tag`'s context rule (tag.rs:130-384) pinned without a device: the hand-worked table tests/golden/tag_hand_cases.json against
the oracle (oracle/tag_oracle.cpp), and the enumeration of tests/tag_cases_util.py, whose size, panic share and class counts
are asserted so that tests/test_gpu_tag_cases.py is known to reach every branch it is meant to reach.

The table's `expect` strings were worked out by reading tag.rs, not by running anything that restates it."""
import collections
import hashlib
import time

import pytest

from tests import genome_util as gu
from tests import tag_cases_util as U

CASES = U.hand_cases()
SMALL_SIZE = 229488            # 286 CIGAR shapes x every pos 0 .. LN - reflen + 2 on the 41-base contig x 3 SEQ variants x 7 flags
PLAIN_SIZE = 29106             # 9 M lengths x with / without 1S x every pos on the 100-base contig x 3 x 7
MAX_PANIC_SHARE = 0.06         # the issue's bound; every pos with end > LN panics (tag.rs:168, 171), two of about forty positions


@pytest.fixture(scope="module")
def enumerated():
    small, plain = U.enumerate_small(), U.enumerate_plain()
    t0 = time.perf_counter()
    xs = [U.oracle_xm(r, U.SHORT) for r in small]
    xp = [U.oracle_xm(r, U.LONG) for r in plain]
    return dict(small=small, plain=plain, xs=xs, xp=xp, oracle_seconds=time.perf_counter() - t0)


def test_the_table_is_as_large_as_asked_and_named_once():
    assert len(CASES) >= 60
    assert len({c["name"] for c in CASES}) == len(CASES)
    for c in CASES:
        assert set(c) >= {"name", "contig", "pos", "flag", "paired", "cigar", "seq", "expect", "why"} and "tag.rs" in c["why"], c["name"]
        assert U.cigar_text(c["cig"]) == c["cigar"], c["name"]
        assert "ln" not in c or c["ln"] != len(c["contig"]), c["name"]
        assert "l_seq" not in c or c["l_seq"] < len(c["seq"]), c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_gives_the_hand_worked_string(case):
    assert U.oracle_xm(case["rec"], case["contig_b"], case["ln_v"]) == case["want"], case["why"]


def test_the_table_has_not_been_altered():
    """every expectation of the table, in order: a changed `expect` fails here even where the oracle were changed to follow it"""
    h = hashlib.sha256("\n".join("%s\t%s" % (c["name"], c["expect"]) for c in CASES).encode()).hexdigest()
    assert h == EXPECT_SHA256, h


def test_plain_rule_gives_the_calls_of_the_hand_worked_string():
    n = n_calls = 0
    for c in CASES:
        pos, flag, paired, cig, seq, _ = c["rec"]
        if not all((x & 15) in (0, 4, 5) for x in cig) or len(seq) < sum(x >> 4 for x in cig if (x & 15) == 0):
            continue
        got = gu.plain_rule(pos, flag, cig, seq, c["contig_b"][:c["ln_v"]], paired)
        want = None if c["want"] is None else gu.decode_walk(pos, flag, cig, c["want"])
        assert got == want, (c["name"], got, want)
        n += 1
        n_calls += len(want or ())
    assert n >= 40 and n_calls >= 20


def test_every_class_holds_hand_cases():
    cnt = collections.Counter(k for c in CASES for k, f in U.CLASSES.items() if f(c["rec"], c["contig_b"], c["ln_v"]))
    assert all(cnt[k] >= 2 for k in U.CLASSES), cnt
    # both orientations in every class that has both, and a panic where the class has one
    for k, f in U.CLASSES.items():
        rcs = {gu.is_rc(c["flag"], c["paired"]) for c in CASES if f(c["rec"], c["contig_b"], c["ln_v"])}
        assert rcs == {False, True} or k == "orientation", (k, rcs)
    for k in ("lookahead_runs_out", "complement_panic", "short_seq"):
        assert any(c["want"] is None for c in CASES if U.CLASSES[k](c["rec"], c["contig_b"], c["ln_v"])), k
    shorter = [c for c in CASES if c["want"] is not None and U.p_no_letter(c["rec"], c["contig_b"]) and len(c["want"]) < len(c["seq_b"])]
    assert len(shorter) >= 2


def test_enumeration_size_panic_share_and_classes(enumerated):
    """The enumeration is the issue's: 286 shapes on the 41-base contig (229 488 records) and 18 plain shapes on the 100-base
    one (29 106).  5.25 % of the first and 2.60 % of the second panic: exactly the records ending past the contig (pos =
    LN - reflen + 1 and + 2), 12 054 and 756 of them.

    The oracle's pass over all 258 594 records, timed here once: 2.2 s on one CPU core; packing them into BAM
    bytes takes another 0.9 s.  That is what tests/test_gpu_tag_cases.py spends on the CPU side before its first kernel."""
    small, plain, xs, xp = (enumerated[k] for k in ("small", "plain", "xs", "xp"))
    assert len(U.shapes()) == 286 and len(set(U.shapes())) == 286
    assert len(small) == SMALL_SIZE and len(plain) == PLAIN_SIZE
    print("oracle over %d records: %.2f s" % (len(small) + len(plain), enumerated["oracle_seconds"]))
    for recs, xms, contig in ((small, xs, U.SHORT), (plain, xp, U.LONG)):
        panics = [r for r, x in zip(recs, xms) if x is None]
        print("panic share %.4f (%d of %d)" % (len(panics) / len(recs), len(panics), len(recs)))
        assert 0 < len(panics) <= MAX_PANIC_SHARE * len(recs)
        assert all(r[0] + (U.ref_len(r[3]) or 1) > len(contig) for r in panics)                     # tag.rs:168-171 and nothing else
        assert sum(1 for r in recs if r[0] + (U.ref_len(r[3]) or 1) > len(contig)) == len(panics)
    assert (sum(x is None for x in xs), sum(x is None for x in xp)) == (12054, 756)
    # every class, counted by the predicates (inputs only) over every fifth record: 5 is coprime to the 3 variants and 7 flags
    cnt = collections.Counter(k for r in small[::5] for k, f in U.CLASSES.items() if f(r, U.SHORT))
    print(dict(cnt))
    for k in U.CLASSES:
        if k in U.NOT_ENUMERATED:
            assert cnt[k] == 0, k                                  # SEQ is written from the contig and as long as the CIGAR says
        else:
            assert cnt[k] >= 200, (k, cnt[k])
    # the look-ahead that runs out and the letter that is not pushed are reached on both strands
    for f in (U.p_runs_out, U.p_no_letter):
        assert {gu.is_rc(r[1], r[2]) for r in small[::5] if f(r, U.SHORT)} == {False, True}
    # plain records among them: the ones the genome decode's fast path must hand to the column walk
    assert sum(1 for r in plain[::5] if U.p_no_letter(r, U.LONG)) >= 200
    # the plain set meets the vector loop's edges: a CG at every offset of the read mod 16, on both strands
    up = U.LONG.upper()
    seen = {(gu.is_rc(r[1], r[2]), t % 16) for r in plain for t in range(U.ref_len(r[3])) if up[r[0] + t:r[0] + t + 2] == b"CG"}
    assert len(seen) == 32


EXPECT_SHA256 = "19a23b3335159b68d29b1ffd9116c8f676724dbe63904136d248a160ea5f9a8e"
