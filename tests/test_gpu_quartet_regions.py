"""GPU parity of ME / PM per interval (`metheor me-regions`, `pm-regions`, `all --me-intervals / --pm-intervals`,
mth_quartet_regions_*; mth_quartet_regions.hip) against the CPU restatement of the definition (tests/quartet_regions_util.py, which
tests/test_quartet_regions_definition.py ties to the oracle's pinned code): the sixteen bins and the reads exactly, PM bit for bit, ME
within 1e-6 (device and host log2f may differ in the last ulp); through the library on every kind of batch and in every form of the
kernel (packed summary, carried row, LDS rows, direct adds), and through the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import pdr_regions_util as P
from tests import quartet_regions_util as U
from tests import lpmd_intervals_util as L
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
KNOBS = ("MTH_QUARTET_REGIONS_LDS_CAP", "MTH_QUARTET_REGIONS_SUMMARY", "MTH_QUARTET_REGIONS_CARRY")


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=120, env=e)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the synthetic records as a BAM whose blocks hold whole records, the BED, and what the restatement expects"""
    assert os.path.exists(EXE)
    d = tmp_path_factory.mktemp("quartet_regions")
    rec = U.records()
    raw_bam, bam, bed = str(d / "raw.bam"), str(d / "iv.bam"), d / "iv.bed"
    bamio.write_bam(raw_bam, rec)
    util.reblock_aligned(raw_bam, bam)
    bed.write_text(U.bed_text())
    iv = U.intervals()
    want = U.default_expected()
    body, offs = L.record_stream(bam)
    me_text, pm_text = U.expected_texts(iv, want)
    return dict(dir=d, rec=rec, bam=bam, bed=str(bed), iv=iv, want=want, me_text=me_text, pm_text=pm_text, body=body, offs=offs)


def arrays(iv):
    return tuple(np.array([x[k] for x in iv], np.int32) for k in range(3))


def check_counts(c, want, what=""):
    assert (c["bins"].astype(np.int64) == want[4]).all(), what
    assert (c["reads"].astype(np.int64) == want[3]).all(), what


def check(got, want, what=""):
    me, pm, n_patterns, n_reads = want[:4]
    assert (got["n_patterns"].astype(np.int64) == n_patterns).all(), what
    assert (got["n_reads"].astype(np.int64) == n_reads).all(), what
    assert U.same_bits(got["pm"], pm), what
    nan = np.isnan(me)
    assert (np.isnan(got["me"]) == nan).all() and (np.abs(got["me"][~nan].astype(np.float64) - me[~nan].astype(np.float64)) <= 1e-6).all(), what
    assert (np.signbit(got["me"][~nan]) == np.signbit(me[~nan])).all(), what


def feed(eng, files, route, **kw):
    """the decoded stream into the engine's declared intervals, batched as `route` says (as tests/test_gpu_pdr_regions.py feeds it)"""
    eng.decode_records(files["body"], files["offs"])
    tids, rb, re_, fl = eng.decoded_contigs()
    assert tids.tolist() == [0, 1]
    groups = eng.decoded_group(tids, rb, re_, each=route != "groups")
    assert [g[0] <= -2 for g in groups] == ([True] if route == "groups" else [True, False])      # (the contig with a call at -1 is always shifted)
    for bt, r0, r1, _ in groups:
        if route == "prepared":
            db = eng.decoded_batch(r0, r1, bt, 0, -1)
            db.n_reads, db.n_cpgs, db.tid = db.c.n_reads, db.c.n_cpgs, db.c.tid
            pb = eng.batch_prepare(db)
            eng.quartet_regions_accumulate(pb, **kw)
            pb.release()
        elif route == "two_calls" and bt >= 0:
            # the contig's reads twice, each call owning the reads that start in its half: every read counts once
            eng.quartet_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, 30_000), **kw)
            eng.quartet_regions_accumulate(eng.decoded_batch(r0, r1, bt, 30_000, -1), **kw)
        else:
            eng.quartet_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **kw)


def counted(iv, files, min_qual=10):
    """one engine, the intervals, the whole stream as one group batch -> (the fetch at depth 10, the counts)"""
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin(*arrays(iv))
        feed(eng, files, "groups", min_qual=min_qual)
        return eng.quartet_regions_fetch(min_depth=10), eng.quartet_regions_counts()
    finally:
        eng.close()


# ---- 1. the library --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["groups", "one_contig_per_batch", "prepared", "two_calls"])
def test_library(files, route):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin(*arrays(files["iv"]))
        feed(eng, files, route, min_qual=10)
        check(eng.quartet_regions_fetch(min_depth=10), files["want"], route)
        assert np.isfinite(files["want"][0]).sum() == 295
        check(eng.quartet_regions_fetch(min_depth=10), files["want"], "a second fetch")
        check_counts(eng.quartet_regions_counts(), files["want"], route)
        # another depth is the finaliser's business alone: no new pass; mth_reset forgets the sums and keeps the intervals
        want2000 = U.restate(U.default_calls(), files["iv"], min_depth=2000, min_qual=10)
        assert 0 < np.isfinite(want2000[0]).sum() < 295
        check(eng.quartet_regions_fetch(min_depth=2000), want2000, "depth 2000")
        eng.reset()
        zero = eng.quartet_regions_fetch(min_depth=1)
        assert np.isnan(zero["me"]).all() and np.isnan(zero["pm"]).all() and not zero["n_patterns"].any() and not zero["n_reads"].any() and len(zero["me"]) == 307
        feed(eng, files, route, min_qual=10)                                # ... the same intervals take the reads again
        check(eng.quartet_regions_fetch(min_depth=10), files["want"], "after reset")
    finally:
        eng.close()


@pytest.mark.parametrize("min_qual", [0, 10, 43])
def test_parameters(files, min_qual):
    want = U.restate(U.default_calls(), files["iv"], min_depth=3, min_qual=min_qual)
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin(*arrays(files["iv"]))
        feed(eng, files, "groups", min_qual=min_qual)
        check(eng.quartet_regions_fetch(min_depth=3), want, min_qual)
        check_counts(eng.quartet_regions_counts(), want, min_qual)
        assert (want[2].sum() == 0) == (min_qual == 43)
    finally:
        eng.close()


def host_batch(s, tid, words=None):
    """contig `tid` of a decoded SoA as a host batch (its calls replaced by `words`, if given)"""
    from metheor_amd import capi
    m = s["tid"] == tid
    off = s["cpg_off"].astype(np.int64)
    lo, hi = off[:-1][m].min(), off[1:][m].max()
    w = s["cpg_pos"] if words is None else words
    return capi.Batch(tid, 0, int(s["end"][m].max()) + 2, s["start"][m], s["end"][m], s["mapq"][m], (off[np.r_[m, False] | np.r_[False, m]] - lo).astype(np.uint32),
                      w[lo:hi], s["cpg_rel"][lo:hi])


def test_host_batch_and_a_cpg_set(files):
    """contig ivB as a host batch made from the oracle's decode under a -c set (every second called position): the library sees the
    filtered calls, as the reference's filter_isin leaves them"""
    import metheor_amd
    c = U.default_calls()
    sites = [(1, int(p)) for p in np.unique(c.pos[c.by_tid[1]])[::2]]
    fc = U.Calls(files["rec"], cpg_set=sites)
    iv = [x for x in files["iv"] if x[0] == 1]
    want = U.restate(fc, iv, **U.DEFAULT_KW)
    b = host_batch(pyoracle.Reads.decode(files["rec"], cpg_set=sites).soa(), 1)
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin(*arrays(iv))
        eng.quartet_regions_accumulate(b, min_qual=10)
        check(eng.quartet_regions_fetch(min_depth=10), want, "host batch")
        check_counts(eng.quartet_regions_counts(), want, "host batch")
        full = files["want"][2][[i for i, x in enumerate(files["iv"]) if x[0] == 1]].sum()
        assert 0 < want[2].sum() < full
    finally:
        eng.close()


def test_calls_in_descending_order(files):
    """the calls of every read of contig ivB reversed within the read: the windows follow the call order (other patterns than the
    ascending reads give), the extremes come from min / max (the same reads contribute)"""
    import metheor_amd
    s = pyoracle.Reads.decode(files["rec"]).soa()
    off = s["cpg_off"].astype(np.int64)
    words = s["cpg_pos"].copy()
    for a, b in zip(off[:-1], off[1:]):
        words[a:b] = words[a:b][::-1]
    c = U.default_calls()
    rc = U.Calls.__new__(U.Calls)
    rc.__dict__.update(c.__dict__)
    p = (words & 0x7fffffff).astype(np.int64)
    rc.pos, rc.meth = np.where(p == 0x7fffffff, -1, p), (words >> 31).astype(bool)
    iv = [x for x in files["iv"] if x[0] == 1]
    want, asc = U.restate(rc, iv, **U.DEFAULT_KW), U.restate(c, iv, **U.DEFAULT_KW)
    assert (want[4] != asc[4]).any() and (want[3] == asc[3]).all() and (want[2] == asc[2]).all()
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin(*arrays(iv))
        eng.quartet_regions_accumulate(host_batch(s, 1, words), min_qual=10)
        check(eng.quartet_regions_fetch(min_depth=10), want, "descending")
        check_counts(eng.quartet_regions_counts(), want, "descending")
    finally:
        eng.close()


# ---- 2. the routes ---------------------------------------------------------------------------------------------------------------------
def lds_cap():
    """the cap the kernel actually runs with: the knob's default (mth_knobs.h)"""
    text = open(os.path.join(ROOT, "metheor_amd", "csrc", "mth_knobs.h")).read()
    return int(re.search(r"constexpr int QUARTET_REGIONS_LDS_CAP = (\d+);", text).group(1))


@pytest.mark.parametrize("among", [False, True], ids=["alone", "among_1kbp_windows"])
def test_a_whole_contig_interval(files, among):
    """the interval every workgroup meets in every work item: its row is carried in LDS, alone (its class is the only one) and among
    tiling windows (a class of its own)"""
    iv = [(0, 0, L.REFS[0][1], "whole")] + ([(0, b, b + 1000, None) for b in range(0, L.REFS[0][1], 1000)] if among else [])
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert want[3][0] > 40 * 256 and (want[4][0] > 0).all()               # dozens of work items (256 reads each) add to the one row
    got, counts = counted(iv, files)
    check(got, want, "whole contig")
    check_counts(counts, want, "whole contig")


def test_nesting_deeper_than_the_lds_cap(files):
    """1.45 times as many 3 kbp windows, 2 bp apart over the island, as a workgroup sums in LDS (348 for the cap of 240): those add
    to memory directly -- depth costs time, never a wrong value"""
    cap = lds_cap()
    iv = P.deep_nesting(cap)
    assert len(iv) > cap and iv[-1][1] < iv[0][2]                          # every window holds the bases before the first one's end: all are candidates there
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert np.isfinite(want[0]).all()
    got, counts = counted(iv, files)
    check(got, want, "deep nesting")
    check_counts(counts, want, "deep nesting")


FORMS = dict(default={}, cap_4={"MTH_QUARTET_REGIONS_LDS_CAP": "4"}, cap_0={"MTH_QUARTET_REGIONS_LDS_CAP": "0"}, summary_off={"MTH_QUARTET_REGIONS_SUMMARY": "0"},
             carry_off={"MTH_QUARTET_REGIONS_CARRY": "0"}, all_off={"MTH_QUARTET_REGIONS_LDS_CAP": "4", "MTH_QUARTET_REGIONS_SUMMARY": "0", "MTH_QUARTET_REGIONS_CARRY": "0"})


@pytest.mark.parametrize("form", list(FORMS))
def test_the_forms_agree(files, form, monkeypatch):
    """the full set in the kernel's differential forms (read once per context): with a cap of 4 most classes add to memory directly,
    with a cap of 0 all do; without the packed summary every pair walks its calls; without the carried row a single candidate is
    flushed once per work item"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    got, counts = counted(files["iv"], files)
    check(got, files["want"], form)
    check_counts(counts, files["want"], form)


def test_call_order(files):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(files["body"], files["offs"])
        tids, rb, re_, fl = eng.decoded_contigs()
        with pytest.raises(metheor_amd.MthError):
            eng.quartet_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))       # no intervals declared
        with pytest.raises(metheor_amd.MthError):
            eng.quartet_regions_begin([0], [10], [9])
        with pytest.raises(metheor_amd.MthError):
            eng.quartet_regions_begin([-1], [0], [9])
        eng.quartet_regions_begin([], [], [])
        eng.quartet_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))
        assert len(eng.quartet_regions_fetch()["me"]) == 0
    finally:
        eng.close()


def test_a_data_error_surfaces_at_the_fetch():
    """a batch whose read of five calls carries the word of position -1 (as its second call, where the host's look at the batch does
    not see it): the accumulate queues the pass and returns, the fetch reports MTH_ERR_RANGE"""
    import metheor_amd
    from metheor_amd import capi
    words = np.array([10, 0x7fffffff, 14 | 1 << 31, 16, 18], np.uint32)
    b = capi.Batch(0, 0, 100, np.array([5], np.int32), np.array([30], np.int32), np.array([40], np.uint8), np.array([0, 5], np.uint32), words, np.zeros(5, np.uint8))
    eng = metheor_amd.Engine(0)
    try:
        eng.quartet_regions_begin([0], [0], [100])
        eng.quartet_regions_accumulate(b, min_qual=10)
        with pytest.raises(metheor_amd.MthError) as e:
            eng.quartet_regions_fetch()
        assert e.value.status == -7                                          # MTH_ERR_RANGE
    finally:
        eng.close()


# ---- 3. the command line ----------------------------------------------------------------------------------------------------------------
def cli(files, sub, tag, *extra, env=None, bam=None, bed=None):
    o = files["dir"] / ("%s_%s.tsv" % (sub, tag))
    r = run(sub, "-i", bam or files["bam"], "--intervals", bed or files["bed"], "-o", o, *extra, env=env)
    assert r.returncode == 0, r.stderr
    return o.read_text()


def both(files, tag, *extra, want=None, **kw):
    """both commands on the same input: the PM table byte for byte, the ME table by the ME rule"""
    me_text, pm_text = want or (files["me_text"], files["pm_text"])
    assert cli(files, "pm-regions", tag, *extra, **kw) == pm_text
    got = cli(files, "me-regions", tag, *extra, **kw)
    U.assert_me_text(got, me_text)
    return got


@pytest.mark.parametrize("group", ["1", "0"])
def test_cli_bytes(files, group):
    text = both(files, "g" + group, env={"METHEOR_GROUP": group})
    row = [l for l in text.splitlines() if "\tempty\t" in l]
    assert len(row) == 1 and row[0].split("\t")[4:] == ["NaN", "0", "0"]                  # a zero-length interval
    assert text.splitlines()[0] + "\n" == U.HEADER_ME


def test_cli_parameters_and_cpg_set(files):
    c = U.default_calls()
    both(files, "par", "-d", "2", "-q", "0", want=U.expected_texts(files["iv"], U.restate(c, files["iv"], min_depth=2, min_qual=0)))
    key = np.unique((c.tid << 32) | np.where(c.pos < 0, 0x7fffffff, c.pos))
    sites = [(int(k >> 32), int(k & 0xffffffff)) for k in key[(key & 0xffffffff) != 0x7fffffff][::2]]
    bed = files["dir"] / "sites.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % (U.NAMES[t], p, p + 2) for t, p in sites))
    want = U.restate(U.Calls(files["rec"], cpg_set=sites), files["iv"], **U.DEFAULT_KW)
    both(files, "set", "-c", bed, want=U.expected_texts(files["iv"], want))
    assert 0 < want[2].sum() < files["want"][2].sum()


def test_cli_shuffled_records_and_sam_text(files):
    rec = files["rec"]
    perm = np.random.default_rng(5).permutation(len(rec))
    raw, bam = str(files["dir"] / "shuf_raw.bam"), str(files["dir"] / "shuf.bam")
    bamio.write_bam(raw, rec.subset(perm))
    util.reblock_aligned(raw, bam)
    both(files, "shuf", bam=bam)
    sam = files["dir"] / "iv.sam"
    sam.write_text(U.sam_text(rec))
    both(files, "sam", bam=sam)


def test_cli_two_shards_on_one_device(files):
    """--gpus 2: a read is owned by the shard that holds its start, every shard counts its reads for all the intervals, main() adds
    the seventeen arrays and finalises once; the whole-contig interval and the windows around a cut straddle it"""
    env = {"METHEOR_SHARD_HALO": "4000", "METHEOR_DEVICES": "1"}
    both(files, "sh2", "--gpus", "2", env=env)


def test_all_forms(files):
    d = files["dir"]
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--me-intervals", d / "all_me.tsv", "--pm-intervals", d / "all_pm.tsv")
    assert r.returncode == 0, r.stderr
    one_me, one_pm = cli(files, "me-regions", "one"), cli(files, "pm-regions", "one")
    assert (d / "all_me.tsv").read_text() == one_me and (d / "all_pm.tsv").read_text() == one_pm and one_pm == files["pm_text"]
    # either table alone
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--pm-intervals", d / "all_pm_alone.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_pm_alone.tsv").read_text() == one_pm
    # beside the per-quartet table, the per-CpG PDR table and the other per-interval tables, on the same BED
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--me-intervals", d / "all_me2.tsv", "--pm-intervals", d / "all_pm2.tsv", "--me", d / "all_q.tsv",
            "--pdr", d / "all_pdr.tsv", "--pdr-intervals", d / "all_pr.tsv", "--mhl-intervals", d / "all_mr.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_me2.tsv").read_text() == one_me and (d / "all_pm2.tsv").read_text() == one_pm
    for sub, one, got in (("me", "one_q.tsv", "all_q.tsv"), ("pdr", "one_pdr.tsv", "all_pdr.tsv")):
        r = run(sub, "-i", files["bam"], "-o", d / one)
        assert r.returncode == 0, r.stderr
        assert (d / got).read_bytes() == (d / one).read_bytes() and (d / one).stat().st_size > 0
    for sub, one, got in (("pdr-regions", "one_pr.tsv", "all_pr.tsv"), ("mhl-regions", "one_mr.tsv", "all_mr.tsv")):
        r = run(sub, "-i", files["bam"], "--intervals", files["bed"], "-o", d / one)
        assert r.returncode == 0, r.stderr
        assert (d / got).read_bytes() == (d / one).read_bytes()


def _tiling(rec, step):
    return [(t, b, b + step, None) for t, (_, ln) in enumerate(rec.refs) for b in range(0, ln, step)] + \
           [(t, 0, U.INT32_MAX, "all_%d" % t) for t in range(len(rec.refs))]


def _write_bed(path, rec, iv):
    path.write_text("".join("%s\t%d\t%d%s\n" % (rec.refs[t][0], b, e, "\t" + n if n else "") for t, b, e, n in iv))


def _routes(tmp_path, rec, iv, inputs, *flags, **kw):
    """both commands on each (tag, input, extra options): the first input's tables are the restatement's, the others' equal them"""
    names = [n for n, _ in rec.refs]
    want = U.restate(U.Calls(rec), iv, min_qual=10, **kw)
    me_text, pm_text = U.expected_texts(iv, want, names=names)
    out = {}
    for tag, inp, extra in inputs:
        for sub in ("me-regions", "pm-regions"):
            o = tmp_path / ("%s_%s.tsv" % (tag, sub))
            r = run(sub, "-i", inp, "--intervals", tmp_path / "i.bed", "-o", o, *flags, *extra)
            assert r.returncode == 0, r.stderr
            out[tag, sub] = o.read_text()
    first = inputs[0][0]
    assert out[first, "pm-regions"] == pm_text
    U.assert_me_text(out[first, "me-regions"], me_text)
    for tag, _, _ in inputs[1:]:
        assert out[tag, "pm-regions"] == pm_text and out[tag, "me-regions"] == out[first, "me-regions"]
    return want


def test_genome_route(golden_dir, tmp_path):
    """--genome on the untagged records gives the files of the tagged ones, which are the restatement's"""
    from tests import tag_util
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    noxm, fa, xm = tmp_path / "noxm.sam", tmp_path / "chr19.fa", os.path.join(golden_dir, "test.chr19.XM.sam")
    noxm.write_text(noxm_text)
    tag_util.write_fasta(str(fa), "chr19", contig)
    rec = bamio.read_sam(xm)
    pos = rec.pos[rec.pos >= 0]
    lo, hi = int(pos.min()), int(pos.max())
    iv = [(0, b, b + 2000, None) for b in range(max(lo - 1000, 0), hi + 1000, 2000)] + [(0, 0, U.INT32_MAX, "all"), (0, lo, lo + 150, "head")]
    _write_bed(tmp_path / "i.bed", rec, iv)
    want = _routes(tmp_path, rec, iv, [("tagged", xm, []), ("genome", noxm, ["--genome", fa])], "-d", "2", min_depth=2)
    assert want[2].sum() > 0


def test_mm_tags_route(tmp_path):
    """--mm-tags on MM / ML records gives the files of the equivalent XM records, which are the restatement's"""
    from tests import modtags_util as M
    g = M.generate(1, 1500, long_reads=False)
    f, fp = tmp_path / "f.sam", tmp_path / "fp.sam"
    M.write_pair(g["refs"], g["recs"], 128, f, fp)
    rec = bamio.read_sam(str(fp))
    rec.xms = [x if x else b"." for x in rec.xms]                      # a record without SEQ has an empty XM:Z: no call (the oracle wants a byte)
    iv = _tiling(rec, 1000)
    _write_bed(tmp_path / "i.bed", rec, iv)
    want = _routes(tmp_path, rec, iv, [("xm", fp, []), ("mm", f, ["--mm-tags"])], "-d", "3", min_depth=3)
    assert np.isfinite(want[0]).sum() > 10


def test_reference_fixtures(golden_dir, tmp_path):
    """tests/golden/test1.bam ... test6.bam, a whole-contig interval, -d 0: the values the unit tests of me.rs and pm.rs assert for
    the fixture's single quartet (tests 1-3), no pattern at all (test 5), and the restatement's for the rest"""
    literal = {1: ("1", "0.9375", "16"), 2: ("0.25", "0.5", None), 3: ("0.25", "0.5", None), 5: ("NaN", "NaN", "0")}
    for k in range(1, 7):
        p = os.path.join(golden_dir, "test%d.bam" % k)
        rec = bamio.read_bam(p)
        name = rec.refs[0][0]
        iv = [(0, 0, U.INT32_MAX, "whole")]
        bed = tmp_path / ("i%d.bed" % k)
        bed.write_text("%s\t0\t%d\twhole\n" % (name, U.INT32_MAX))
        want = U.restate(U.Calls(rec), iv, min_depth=0, min_qual=10)
        me_text, pm_text = U.expected_texts(iv, want, names=[n for n, _ in rec.refs])
        got = {}
        for sub in ("me-regions", "pm-regions"):
            r = run(sub, "-i", p, "--intervals", bed, "-o", tmp_path / ("%s%d.tsv" % (sub, k)), "-d", "0")
            assert r.returncode == 0, r.stderr
            got[sub] = (tmp_path / ("%s%d.tsv" % (sub, k))).read_text()
        assert got["pm-regions"] == pm_text, k
        U.assert_me_text(got["me-regions"], me_text)
        if k in literal:
            me, pm, n = literal[k]
            fm, fp_ = got["me-regions"].splitlines()[1].split("\t"), got["pm-regions"].splitlines()[1].split("\t")
            assert fm[:5] == [name, "0", str(U.INT32_MAX), "whole", me] and fp_[4] == pm and (n is None or (fm[5] == n and fp_[5] == n)), (k, fm, fp_)
