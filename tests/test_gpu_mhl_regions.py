"""GPU parity of MHL per interval (`metheor mhl-regions`, `all --mhl-intervals`, mth_mhl_regions_*; mth_mhl_regions.hip) against the CPU
restatement of the definition (tests/mhl_regions_util.py, which tests/test_mhl_regions_definition.py ties to the oracle's pinned code):
mhl bit for bit, n_reads and max_cpgs exactly; through the library on every kind of batch, and through the command line byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import mhl_regions_util as U
from tests import lpmd_intervals_util as L
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=120, env=e)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the synthetic records as a BAM whose blocks hold whole records, the BED, and what the restatement expects"""
    assert os.path.exists(EXE)
    d = tmp_path_factory.mktemp("mhl_regions")
    rec = U.records()
    raw_bam, bam, bed = str(d / "raw.bam"), str(d / "iv.bam"), d / "iv.bed"
    bamio.write_bam(raw_bam, rec)
    util.reblock_aligned(raw_bam, bam)
    bed.write_text(U.bed_text())
    iv = U.intervals()
    mhl, n_reads, max_cpgs = U.default_expected()
    body, offs = L.record_stream(bam)
    return dict(dir=d, rec=rec, bam=bam, bed=str(bed), iv=iv, want=(mhl, n_reads, max_cpgs), text=U.table_text(iv, mhl, n_reads, max_cpgs),
                body=body, offs=offs)


def arrays(iv):
    return tuple(np.array([x[k] for x in iv], np.int32) for k in range(3))


def check(got, want, what=""):
    mhl, n_reads, max_cpgs = want
    assert (got["n_reads"].astype(np.int64) == n_reads).all(), what
    assert (got["max_cpgs"].astype(np.int64) == max_cpgs).all(), what
    assert U.same_bits(got["mhl"], mhl), what


def feed(eng, files, route, **kw):
    """the decoded stream into the engine's declared intervals, batched as `route` says"""
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
            eng.mhl_regions_accumulate(pb, **kw)
            pb.release()
        elif route == "two_calls" and bt >= 0:
            # the contig's reads twice, each call owning the reads that start in its half: every read counts once
            eng.mhl_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, 30_000), **kw)
            eng.mhl_regions_accumulate(eng.decoded_batch(r0, r1, bt, 30_000, -1), **kw)
        else:
            eng.mhl_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **kw)


# ---- 1. the library --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["groups", "one_contig_per_batch", "prepared", "two_calls"])
def test_library(files, route):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(files["iv"]))
        feed(eng, files, route, min_cpgs=4, min_qual=10)
        got = eng.mhl_regions_fetch(min_depth=10)
        check(got, files["want"], route)
        assert np.isfinite(files["want"][0]).sum() > 250
        check(eng.mhl_regions_fetch(min_depth=10), files["want"], "a second fetch")
        # the long reads put lengths above the dense rows' 64 into the overflow list: 100 and 70 kept calls, a run of 70
        st = eng.mhl_regions_stats()
        assert st[0] >= 7 and st[1] == 0 and st[2] == (1 if route == "groups" else 3 if route == "two_calls" else 2), st
        rows = eng.mhl_regions_counts()
        k = [n for _, _, _, n in files["iv"]].index("long_run_70")
        mine = rows["interval"] == k
        assert rows["length"][mine].max() == 70 and rows["runs"][mine][rows["length"][mine] == 70].tolist() == [1]
        assert rows["reads"][mine][rows["length"][mine] == 70].tolist() == [2]
        key = rows["interval"].astype(np.int64) << 32 | rows["length"]
        assert (np.diff(key) > 0).all()                                  # sorted by (interval, length), no row twice
        # another depth is the finaliser's business alone; mth_reset forgets the sums and keeps the intervals
        c = U.default_calls()
        check(eng.mhl_regions_fetch(min_depth=200), U.restate(c, files["iv"], min_depth=200, min_cpgs=4, min_qual=10), "depth 200")
        eng.reset()
        zero = eng.mhl_regions_fetch(min_depth=1)
        assert np.isnan(zero["mhl"]).all() and not zero["n_reads"].any() and len(eng.mhl_regions_counts()["interval"]) == 0
    finally:
        eng.close()


@pytest.mark.parametrize("kw", [dict(min_cpgs=1, min_qual=0), dict(min_cpgs=1, min_qual=10), dict(min_cpgs=4, min_qual=0), dict(min_cpgs=9, min_qual=43)],
                         ids=["p1_q0", "p1_q10", "p4_q0", "p9_q43"])
def test_parameters(files, kw):
    import metheor_amd
    want = U.restate(U.default_calls(), files["iv"], min_depth=3, **kw)
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(files["iv"]))
        feed(eng, files, "groups", **kw)
        check(eng.mhl_regions_fetch(min_depth=3), want, str(kw))
        assert (want[1].sum() == 0) == (kw["min_qual"] == 43)
    finally:
        eng.close()


def test_host_batch_and_a_cpg_set(files):
    """contig ivB as a host batch made from the oracle's decode under a -c set (every second called position): the library sees the
    filtered calls, as the reference's filter_isin leaves them"""
    import metheor_amd
    from metheor_amd import capi
    c = U.default_calls()
    sites = [(1, int(p)) for p in np.unique(c.pos[c.by_tid[1]])[::2]]
    fc = U.Calls(files["rec"], cpg_set=sites)
    iv = [x for x in files["iv"] if x[0] == 1]
    want = U.restate(fc, iv, **U.DEFAULT_KW)
    s = pyoracle.Reads.decode(files["rec"], cpg_set=sites).soa()
    m = s["tid"] == 1
    off = s["cpg_off"].astype(np.int64)
    lo, hi = off[:-1][m].min(), off[1:][m].max()
    b = capi.Batch(1, 0, int(s["end"][m].max()) + 2, s["start"][m], s["end"][m], s["mapq"][m], (off[np.r_[m, False] | np.r_[False, m]] - lo).astype(np.uint32),
                   s["cpg_pos"][lo:hi], s["cpg_rel"][lo:hi])
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(iv))
        eng.mhl_regions_accumulate(b, min_cpgs=4, min_qual=10)
        check(eng.mhl_regions_fetch(min_depth=10), want, "host batch")
        assert 0 < want[1].sum() < files["want"][1][[k for k, x in enumerate(files["iv"]) if x[0] == 1]].sum()
    finally:
        eng.close()


def test_overflow_list_too_short_runs_the_batch_again(files, monkeypatch):
    """a list of two entries: the batch that holds the long reads counts what it could not write and is run again, appending only"""
    import metheor_amd
    monkeypatch.setenv("MTH_MHL_REGIONS_LIST", "2")
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(files["iv"]))
        feed(eng, files, "one_contig_per_batch", min_cpgs=4, min_qual=10)
        check(eng.mhl_regions_fetch(min_depth=10), files["want"], "short list")
        st = eng.mhl_regions_stats()
        assert st[0] >= 7 and st[1] == 1, st
    finally:
        eng.close()


@pytest.mark.parametrize("among", [False, True], ids=["alone", "among_1kbp_windows"])
def test_a_whole_contig_interval(files, among):
    """the interval every read of the contig adds to: alone (its class is the only one), and among tiling windows (a class of its own)"""
    import metheor_amd
    iv = [(0, 0, L.REFS[0][1], "whole")] + ([(0, b, b + 1000, None) for b in range(0, L.REFS[0][1], 1000)] if among else [])
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert want[1][0] > 40 * 256                                      # dozens of workgroups (256 reads each) add to the one row
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(iv))
        feed(eng, files, "groups", min_cpgs=4, min_qual=10)
        check(eng.mhl_regions_fetch(min_depth=10), want, "whole contig")
    finally:
        eng.close()


def test_nesting_deeper_than_the_lds_rows(files):
    """400 windows of 3 kbp ten bases apart over the island and 300 nested ones: more entries of a class under one workgroup than it
    sums in LDS -- those add to memory directly: depth costs time, never a wrong value"""
    import metheor_amd
    iv = [(0, 63_000 + 10 * k, 66_000 + 10 * k, None) for k in range(400)] + [(0, 66_000 - k, 68_000 + k, None) for k in range(300)]
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert np.isfinite(want[0]).all()
    eng = metheor_amd.Engine(0)
    try:
        eng.mhl_regions_begin(*arrays(iv))
        feed(eng, files, "groups", min_cpgs=4, min_qual=10)
        check(eng.mhl_regions_fetch(min_depth=10), want, "deep nesting")
    finally:
        eng.close()


def test_call_order(files):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(files["body"], files["offs"])
        tids, rb, re_, fl = eng.decoded_contigs()
        with pytest.raises(metheor_amd.MthError):
            eng.mhl_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))       # no intervals declared
        with pytest.raises(metheor_amd.MthError):
            eng.mhl_regions_begin([0], [10], [9])
        eng.mhl_regions_begin([], [], [])
        eng.mhl_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))
        assert len(eng.mhl_regions_fetch()["mhl"]) == 0
    finally:
        eng.close()


# ---- 2. the command line ----------------------------------------------------------------------------------------------------------------
def cli(files, tag, *extra, env=None, bam=None, bed=None):
    o = files["dir"] / (tag + ".tsv")
    r = run("mhl-regions", "-i", bam or files["bam"], "--intervals", bed or files["bed"], "-o", o, *extra, env=env)
    assert r.returncode == 0, r.stderr
    return o.read_text()


@pytest.mark.parametrize("group", ["1", "0"])
def test_cli_bytes(files, group):
    assert cli(files, "g" + group, env={"METHEOR_GROUP": group}) == files["text"]


def test_cli_parameters_and_cpg_set(files):
    c = U.default_calls()
    kw = dict(min_depth=2, min_cpgs=1, min_qual=0)
    assert cli(files, "par", "-d", "2", "-p", "1", "-q", "0") == U.table_text(files["iv"], *U.restate(c, files["iv"], **kw))
    key = np.unique((c.tid << 32) | np.where(c.pos < 0, 0x7fffffff, c.pos))
    sites = [(int(k >> 32), int(k & 0xffffffff)) for k in key[(key & 0xffffffff) != 0x7fffffff][::2]]
    bed = files["dir"] / "sites.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % (U.NAMES[t], p, p + 2) for t, p in sites))
    want = U.restate(U.Calls(files["rec"], cpg_set=sites), files["iv"], **U.DEFAULT_KW)
    assert cli(files, "set", "-c", bed) == U.table_text(files["iv"], *want)
    assert 0 < want[1].sum() < files["want"][1].sum()


def test_cli_shuffled_records_and_sam_text(files):
    rec = files["rec"]
    perm = np.random.default_rng(5).permutation(len(rec))
    raw, bam = str(files["dir"] / "shuf_raw.bam"), str(files["dir"] / "shuf.bam")
    bamio.write_bam(raw, rec.subset(perm))
    util.reblock_aligned(raw, bam)
    assert cli(files, "shuf", bam=bam) == files["text"]
    sam = files["dir"] / "iv.sam"
    sam.write_text(U.sam_text(rec))
    assert cli(files, "sam", bam=sam) == files["text"]


def test_cli_two_shards_on_one_device(files):
    """--gpus 2 and 3: a read is owned by the shard that holds its start, every shard counts its reads for all the intervals, main()
    adds the histograms and finalises once; the whole-contig interval and the windows around a cut straddle it"""
    env = {"METHEOR_SHARD_HALO": "4000", "METHEOR_DEVICES": "1"}
    assert cli(files, "sh2", "--gpus", "2", env=env) == files["text"]
    assert cli(files, "sh3", "--gpus", "3", env=env) == files["text"]


def test_all_forms(files):
    d = files["dir"]
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--mhl-intervals", d / "all_alone.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_alone.tsv").read_text() == files["text"]
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--mhl-intervals", d / "all_mr.tsv", "--lpmd", d / "all_lpmd.tsv",
            "--lpmd-intervals", d / "all_li.tsv", "--mhl", d / "all_mhl.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_mr.tsv").read_text() == files["text"]
    # the other tables are what the single commands write
    r = run("mhl", "-i", files["bam"], "-o", d / "one_mhl.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_mhl.tsv").read_bytes() == (d / "one_mhl.tsv").read_bytes()
    r = run("lpmd", "-i", files["bam"], "-o", d / "one_lpmd.tsv", "--intervals", files["bed"], "--intervals-output", d / "one_li.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_li.tsv").read_bytes() == (d / "one_li.tsv").read_bytes()


def _tiling(rec, step):
    return [(t, b, b + step, None) for t, (_, ln) in enumerate(rec.refs) for b in range(0, ln, step)] + \
           [(t, 0, U.INT32_MAX, "all_%d" % t) for t in range(len(rec.refs))]


def _write_bed(path, rec, iv):
    path.write_text("".join("%s\t%d\t%d%s\n" % (rec.refs[t][0], b, e, "\t" + n if n else "") for t, b, e, n in iv))


def test_genome_route(golden_dir, tmp_path):
    """--genome on the untagged records gives the file of the tagged ones, which is the restatement's"""
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
    out = {}
    for tag, inp, extra in (("genome", noxm, ["--genome", fa]), ("tagged", xm, [])):
        r = run("mhl-regions", "-i", inp, "--intervals", tmp_path / "i.bed", "-o", tmp_path / (tag + ".tsv"), "-d", "2", "-p", "2", *extra)
        assert r.returncode == 0, r.stderr
        out[tag] = (tmp_path / (tag + ".tsv")).read_text()
    want = U.restate(U.Calls(rec), iv, min_depth=2, min_cpgs=2, min_qual=10)
    assert out["tagged"] == U.table_text(iv, *want, names=[n for n, _ in rec.refs])
    assert out["genome"] == out["tagged"] and want[1].sum() > 0


def test_mm_tags_route(tmp_path):
    """--mm-tags on MM / ML records gives the file of the equivalent XM records, which is the restatement's"""
    from tests import modtags_util as M
    g = M.generate(1, 1500, long_reads=False)
    f, fp = tmp_path / "f.sam", tmp_path / "fp.sam"
    M.write_pair(g["refs"], g["recs"], 128, f, fp)
    rec = bamio.read_sam(str(fp))
    rec.xms = [x if x else b"." for x in rec.xms]                      # a record without SEQ has an empty XM:Z: no call (the oracle wants a byte)
    iv = _tiling(rec, 1000)
    _write_bed(tmp_path / "i.bed", rec, iv)
    out = {}
    for tag, inp, extra in (("mm", f, ["--mm-tags"]), ("xm", fp, [])):
        r = run("mhl-regions", "-i", inp, "--intervals", tmp_path / "i.bed", "-o", tmp_path / (tag + ".tsv"), "-d", "3", "-p", "2", *extra)
        assert r.returncode == 0, r.stderr
        out[tag] = (tmp_path / (tag + ".tsv")).read_text()
    want = U.restate(U.Calls(rec), iv, min_depth=3, min_cpgs=2, min_qual=10)
    assert out["xm"] == U.table_text(iv, *want, names=[n for n, _ in rec.refs])
    assert out["mm"] == out["xm"] and np.isfinite(want[0]).sum() > 10


def test_reference_fixtures(golden_dir, tmp_path):
    """tests/golden/test1.bam ... test6.bam, a whole-contig interval, -p 1 -d 1: the answers mhl.rs's unit tests assert for every CpG"""
    want = ["0.1625", "0.5", "0.5", "0.1625", "NaN", "0.5"]
    for k in range(1, 7):
        p = os.path.join(golden_dir, "test%d.bam" % k)
        name = bamio.read_bam(p).refs[0][0]
        bed = tmp_path / ("i%d.bed" % k)
        bed.write_text("%s\t0\t%d\twhole\n" % (name, U.INT32_MAX))
        r = run("mhl-regions", "-i", p, "--intervals", bed, "-o", tmp_path / ("o%d.tsv" % k), "-p", "1", "-d", "1")
        assert r.returncode == 0, r.stderr
        lines = (tmp_path / ("o%d.tsv" % k)).read_text().splitlines()
        assert lines[0] + "\n" == U.HEADER and len(lines) == 2 and lines[1].split("\t")[:5] == [name, "0", str(U.INT32_MAX), "whole", want[k - 1]], lines
