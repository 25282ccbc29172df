"""`tag`'s context rule on the MI355X, on every route that restates it: Engine.tag_records (mth_tag_dev.h's column walk),
Engine.tag_records_bam, the `--genome` decode in its direct form (mth_decode_genome.hip: gen_plain for plain records, the
walk and gen_walk_letters for the rest) and in its staged form, and the command line -- for the hand-worked table
tests/golden/tag_hand_cases.json against its `expect`, and for the enumeration of tests/tag_cases_util.py (229 488 short
records of 286 CIGAR shapes at every position of a 41-base contig, 29 106 plain records of 14 - 46 bases at every position of
a 100-base one) against the oracle.  tests/test_tag_hand_cases.py pins the table to the oracle and counts what the
enumeration reaches, without a device."""
import numpy as np
import pytest

from tests import bgzf_util as B
from tests import genome_util as gu
from tests import tag_cases_util as U
from tests import test_gpu_genome as G               # its run / measure / assert_same (imported, not edited)
from tests.test_gpu_tag_bam import expected_stream

pytestmark = pytest.mark.gpu
KEYS = G.KEYS
GROUPS = ("single", "paired")
MAPQ = 30


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


def _group(recs, paired):
    """records [(tid, pos, flag, paired, cig, seq, cigar text, want)] of one pairedness -> what every route needs"""
    sel = [r for r in recs if r[3] == paired]
    raw, off = U.window([(r[0], r[1], r[2], r[4], r[5]) for r in sel])
    return dict(paired=paired, raw=raw, off=off, want=[r[7] for r in sel],
                recs=[(r[0], r[1], r[2], MAPQ, r[4], r[5], r[6]) for r in sel])


@pytest.fixture(scope="module")
def hand():
    """the table: one contig per distinct (LN, bases), the cases that run through split by pairedness, the panics apart"""
    cases = U.hand_cases()
    keys = sorted({(c["ln_v"], c["contig_b"]) for c in cases})
    rows = [(keys.index((c["ln_v"], c["contig_b"])),) + c["rec"] + (c["want"],) for c in cases]
    ok = [r for r in rows if r[7] is not None]
    out = dict(contigs=keys, refs=[("h%d" % k, ln) for k, (ln, _) in enumerate(keys)], cases=cases, rows=rows,
               panics=[(r, c["name"]) for r, c in zip(rows, cases) if r[7] is None])
    for name, paired in zip(GROUPS, (False, True)):
        out[name] = _group(ok, paired)
    assert len(out["single"]["want"]) >= 50 and len(out["paired"]["want"]) >= 10 and len(out["panics"]) >= 8
    return out


@pytest.fixture(scope="module")
def enum():
    """the enumeration: tid 0 the 41-base contig with the short records, tid 1 the 100-base one with the plain records"""
    rows = []
    for tid, recs, contig in ((0, U.enumerate_small(), U.SHORT), (1, U.enumerate_plain(), U.LONG)):
        rows += [(tid,) + r + (U.oracle_xm(r, contig),) for r in recs]
    ok = [r for r in rows if r[7] is not None]
    bad = [r for r in rows if r[7] is None]
    out = dict(contigs=[(len(U.SHORT), U.SHORT), (len(U.LONG), U.LONG)], refs=[("e0", len(U.SHORT)), ("e1", len(U.LONG))],
               panics=[(r, "enumerated %d" % k) for k, r in list(enumerate(bad))[::len(bad) // 64][:64]])
    assert len(rows) == 258594 and len(bad) == 12810 and len(out["panics"]) == 64
    for name, paired in zip(GROUPS, (False, True)):
        out[name] = _group(ok, paired)
    return out


@pytest.fixture(scope="module", params=["hand", "enum"])
def data(request):
    return request.getfixturevalue(request.param)


def first_difference(got, want, recs):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return k, recs[k][:3], recs[k][6], recs[k][5], w, g
    return None


# ---- tag ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_tag_records_give_the_expected_strings(eng, data, group):
    g = data[group]
    eng.tag_set_genome(data["contigs"])
    got = eng.tag_records(g["raw"], g["off"], is_paired_end=g["paired"])
    assert len(got) == len(g["want"])
    assert got == g["want"], first_difference(got, g["want"], g["recs"])


# ---- tag -O bam -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_tag_records_bam_appends_the_expected_field(eng, data, group):
    g = data[group]
    eng.tag_set_genome(data["contigs"])
    blob, stream_bytes, n_blocks = eng.tag_records_bam(g["raw"], g["off"], is_paired_end=g["paired"])
    bl = B.blocks(blob, keep_eof=True)
    stream = b"".join(b.raw for b in bl)
    want = expected_stream(g["raw"], g["off"], g["want"])
    assert stream_bytes == len(stream) == sum(len(r) for r in want) and n_blocks == len(bl)
    if stream != b"".join(want):
        p, got = 0, []
        for w in want:
            got.append(stream[p:p + len(w)])
            p += len(w)
        assert False, first_difference(got, want, g["recs"])


# ---- --genome, direct and staged --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
@pytest.mark.parametrize("group", GROUPS)
def test_genome_decode_gives_the_calls_of_the_expected_strings(eng, data, group, staged, monkeypatch):
    g = data[group]
    monkeypatch.setenv("METHEOR_GENOME_STAGED", "1" if staged else "0")
    eng.tag_set_genome(data["contigs"])
    want_all = gu.expected_reads(data["refs"], g["recs"], g["want"]).soa()
    sites = sorted({(int(t), int(p & 0x7fffffff)) for t, a, b in zip(want_all["tid"], want_all["cpg_off"][:-1], want_all["cpg_off"][1:])
                    for p in want_all["cpg_pos"][int(a):int(b)]})
    assert len(want_all["tid"]) == len(g["recs"]) and len(sites) >= 2
    try:
        for filt in (None, sites[::2]):
            want = want_all if filt is None else gu.expected_reads(data["refs"], g["recs"], g["want"], cpg_set=filt).soa()
            assert 0 < len(want["cpg_pos"]) and (filt is None or len(want["cpg_pos"]) < len(want_all["cpg_pos"]))
            eng.decode_set_cpg_filter(filt)
            eng.decode_set_genome(True, is_paired_end=g["paired"])
            eng.decode_records(g["raw"], g["off"])
            got = eng.decoded_fetch()
            for k in KEYS:
                if not np.array_equal(got[k], want[k]):
                    at = int(np.flatnonzero(got[k][:len(want[k])] != want[k][:len(got[k])])[0]) if len(got[k]) and len(want[k]) else -1
                    rec = at - 1 if k == "cpg_off" else int(np.searchsorted(want["cpg_off"], at, side="right")) - 1 if k.startswith("cpg_") else at
                    assert False, (k, filt is not None, len(got[k]), len(want[k]), at, g["recs"][rec][:3] + g["recs"][rec][5:], g["want"][rec])
    finally:
        eng.decode_set_genome(False)
        eng.decode_set_cpg_filter(None)


@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
def test_a_letter_that_is_not_pushed_moves_the_calls_behind_it(eng, hand, staged, monkeypatch):
    """noletter_fwd_c_then_iupac: C R A gets no letter, so the Z of the CpG at offset 5 (position 7) is letter 4 and the
    decode, which reads letter q at query offset q, calls position 6"""
    monkeypatch.setenv("METHEOR_GENOME_STAGED", "1" if staged else "0")
    k, = [i for i, c in enumerate(hand["cases"]) if c["name"] == "noletter_fwd_c_then_iupac"]
    r = hand["rows"][k]
    assert r[7] == b"....Z." and len(r[5]) == 7
    raw, off = U.window([(r[0], r[1], r[2], r[4], r[5])])
    eng.tag_set_genome(hand["contigs"])
    try:
        eng.decode_set_genome(True)
        eng.decode_records(raw, off)
        got = eng.decoded_fetch()
    finally:
        eng.decode_set_genome(False)
    assert list(got["cpg_rel"]) == [4] and list(got["cpg_pos"]) == [(r[1] + 4) | 0x80000000]


# ---- panics -----------------------------------------------------------------------------------------------------------------
def test_panicking_records_are_errors_on_every_route(eng, data, monkeypatch):
    import metheor_amd
    assert len(data["panics"]) >= 8
    for row, name in data["panics"]:
        g = data["paired" if row[3] else "single"]
        # three good records of the same pairedness around it: two before, one behind
        ks = [(7 * len(name) + j * 13) % len(g["recs"]) for j in range(3)]
        good = [(g["recs"][k][0], g["recs"][k][1], g["recs"][k][2], g["recs"][k][4], g["recs"][k][5]) for k in ks]
        bad = (row[0], row[1], row[2], row[4], row[5])
        raw, off = U.window(good[:2] + [bad] + good[2:])
        graw, goff = U.window(good)
        eng.tag_set_genome(data["contigs"])
        with pytest.raises(metheor_amd.MthError) as e:
            eng.tag_records(raw, off, is_paired_end=row[3])
        assert "tag" in str(e.value), name
        eng.reset()
        eng.tag_set_genome(data["contigs"])
        assert eng.tag_records(graw, goff, is_paired_end=row[3]) == [g["want"][k] for k in ks], name
        for staged in ("0", "1"):
            monkeypatch.setenv("METHEOR_GENOME_STAGED", staged)
            try:
                eng.decode_set_genome(True, is_paired_end=row[3])
                with pytest.raises(metheor_amd.MthError) as e:
                    eng.decode_records(raw, off)
                assert "tag" in str(e.value), (name, staged)
                eng.reset()
                eng.tag_set_genome(data["contigs"])
                eng.decode_set_genome(True, is_paired_end=row[3])
                assert eng.decode_records(graw, goff)[0] == 3, (name, staged)
            finally:
                eng.decode_set_genome(False)


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _sam_and_fasta(hand, rows, d, stem):
    fa = d / (stem + ".fa")
    fa.write_bytes(b"".join(b">h%d\n%s\n" % (k, bases) for k, (ln, bases) in enumerate(hand["contigs"])))
    sam = d / (stem + ".sam")
    sam.write_text(gu.sam_text(hand["refs"], [(r[0], r[1], r[2], MAPQ, r[4], r[5], r[6]) for r in rows], so="unsorted"))
    return str(sam), str(fa)


def test_command_line_tags_the_table_and_genome_equals_the_tagged_file(hand, tmp_path):
    # SAM text cannot say a SEQ shorter than its CIGAR: those cases are BAM only
    full = {c["name"] for c in hand["cases"] if "l_seq" not in c}
    rows = [r for r, c in zip(hand["rows"], hand["cases"]) if c["name"] in full and not r[3] and r[7] is not None]
    assert len(rows) >= 45
    sam, fa = _sam_and_fasta(hand, rows, tmp_path, "table")
    tagged = tmp_path / "tagged.sam"
    r = G.run("tag", "-i", sam, "-o", tagged, "-g", fa)
    assert r.returncode == 0, r.stderr
    lines = [l for l in tagged.read_text().splitlines() if not l.startswith("@")]
    assert len(lines) == len(rows)
    for l, row in zip(lines, rows):
        assert l.endswith("\tXM:Z:" + row[7].decode()), (l, row[7])
    a = G.measure("pdr", sam, tmp_path, "g", ["-d", "1", "-p", "1"], genome=fa)
    b = G.measure("pdr", str(tagged), tmp_path, "two", ["-d", "1", "-p", "1"])
    outs = G.assert_same(a, b, "pdr -g on the table against pdr on the tagged table")
    assert outs["out"].count(b"\n") >= 5
    # one panicking case appended: both commands leave with the panic status
    bad = [r for r, c in zip(hand["rows"], hand["cases"]) if c["name"] == "runout_fwd_one_character_panics"]
    sam2, _ = _sam_and_fasta(hand, rows + bad, tmp_path, "with_panic")
    r = G.run("tag", "-i", sam2, "-o", tmp_path / "t2.sam", "-g", fa)
    assert r.returncode == 101, (r.returncode, r.stderr)
    r = G.run("pdr", "-d", "1", "-p", "1", "-i", sam2, "-o", tmp_path / "o2.tsv", "-g", fa)
    assert r.returncode == 101 and "tag" in r.stderr, (r.returncode, r.stderr)
