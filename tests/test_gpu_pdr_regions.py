"""GPU parity of PDR per interval (`metheor pdr-regions`, `all --pdr-intervals`, mth_pdr_regions_*; mth_pdr_regions.hip) against the CPU
restatement of the definition (tests/pdr_regions_util.py, which tests/test_pdr_regions_definition.py ties to the oracle's pinned code):
the three counters exactly, pdr bit for bit; through the library on every kind of batch and in every form of the kernel (span route,
LDS rows, direct adds), and through the command line byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import pdr_regions_util as U
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
    d = tmp_path_factory.mktemp("pdr_regions")
    rec = U.records()
    raw_bam, bam, bed = str(d / "raw.bam"), str(d / "iv.bam"), d / "iv.bed"
    bamio.write_bam(raw_bam, rec)
    util.reblock_aligned(raw_bam, bam)
    bed.write_text(U.bed_text())
    iv = U.intervals()
    want = U.default_expected()
    body, offs = L.record_stream(bam)
    return dict(dir=d, rec=rec, bam=bam, bed=str(bed), iv=iv, want=want, text=U.table_text(iv, *want), body=body, offs=offs)


def arrays(iv):
    return tuple(np.array([x[k] for x in iv], np.int32) for k in range(3))


def check(got, want, what=""):
    pdr, m, u, d = want
    assert (got["n_methylated"].astype(np.int64) == m).all(), what
    assert (got["n_concordant"].astype(np.int64) == m + u).all(), what
    assert (got["n_discordant"].astype(np.int64) == d).all(), what
    assert U.same_bits(got["pdr"], pdr), what


def feed(eng, files, route, **kw):
    """the decoded stream into the engine's declared intervals, batched as `route` says (as tests/test_gpu_mhl_regions.py feeds it)"""
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
            eng.pdr_regions_accumulate(pb, **kw)
            pb.release()
        elif route == "two_calls" and bt >= 0:
            # the contig's reads twice, each call owning the reads that start in its half: every read counts once
            eng.pdr_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, 30_000), **kw)
            eng.pdr_regions_accumulate(eng.decoded_batch(r0, r1, bt, 30_000, -1), **kw)
        else:
            eng.pdr_regions_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **kw)


def counted(iv, files, **kw):
    """one engine, the intervals, the whole stream as one group batch -> the fetch at depth 10"""
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.pdr_regions_begin(*arrays(iv))
        feed(eng, files, "groups", **(kw or dict(min_cpgs=4, min_qual=10)))
        return eng.pdr_regions_fetch(min_depth=10)
    finally:
        eng.close()


# ---- 1. the library --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["groups", "one_contig_per_batch", "prepared", "two_calls"])
def test_library(files, route):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.pdr_regions_begin(*arrays(files["iv"]))
        feed(eng, files, route, min_cpgs=4, min_qual=10)
        check(eng.pdr_regions_fetch(min_depth=10), files["want"], route)
        assert np.isfinite(files["want"][0]).sum() == 295
        check(eng.pdr_regions_fetch(min_depth=10), files["want"], "a second fetch")
        c = eng.pdr_regions_counts()
        _, m, u, d = files["want"]
        assert (c["methylated"] == m).all() and (c["unmethylated"] == u).all() and (c["discordant"] == d).all()
        # another depth is the finaliser's business alone: no new pass; mth_reset forgets the sums and keeps the intervals
        calls = U.default_calls()
        want200 = U.restate(calls, files["iv"], min_depth=200, min_cpgs=4, min_qual=10)
        assert 0 < np.isfinite(want200[0]).sum() < 295
        check(eng.pdr_regions_fetch(min_depth=200), want200, "depth 200")
        eng.reset()
        zero = eng.pdr_regions_fetch(min_depth=1)
        assert np.isnan(zero["pdr"]).all() and not zero["n_concordant"].any() and not zero["n_discordant"].any() and len(zero["pdr"]) == 307
        feed(eng, files, route, min_cpgs=4, min_qual=10)                   # ... the same intervals take the reads again
        check(eng.pdr_regions_fetch(min_depth=10), files["want"], "after reset")
    finally:
        eng.close()


@pytest.mark.parametrize("kw", [dict(min_cpgs=1, min_qual=0), dict(min_cpgs=1, min_qual=10), dict(min_cpgs=4, min_qual=0), dict(min_cpgs=9, min_qual=43)],
                         ids=["p1_q0", "p1_q10", "p4_q0", "p9_q43"])
def test_parameters(files, kw):
    import metheor_amd
    want = U.restate(U.default_calls(), files["iv"], min_depth=3, **kw)
    eng = metheor_amd.Engine(0)
    try:
        eng.pdr_regions_begin(*arrays(files["iv"]))
        feed(eng, files, "groups", **kw)
        check(eng.pdr_regions_fetch(min_depth=3), want, str(kw))
        assert ((want[1] + want[2] + want[3]).sum() == 0) == (kw["min_qual"] == 43)
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
        eng.pdr_regions_begin(*arrays(iv))
        eng.pdr_regions_accumulate(b, min_cpgs=4, min_qual=10)
        check(eng.pdr_regions_fetch(min_depth=10), want, "host batch")
        full = sum(files["want"][k][[i for i, x in enumerate(files["iv"]) if x[0] == 1]].sum() for k in (1, 2, 3))
        assert 0 < (want[1] + want[2] + want[3]).sum() < full
    finally:
        eng.close()


# ---- 2. the three routes -----------------------------------------------------------------------------------------------------------------
def lds_cap():
    """the cap the kernel actually runs with: the knob's default (mth_knobs.h)"""
    text = open(os.path.join(ROOT, "metheor_amd", "csrc", "mth_knobs.h")).read()
    return int(re.search(r"constexpr int PDR_REGIONS_LDS_CAP = (\d+);", text).group(1))


@pytest.mark.parametrize("among", [False, True], ids=["alone", "among_1kbp_windows"])
def test_a_whole_contig_interval(files, among):
    """the interval that holds every workgroup's span: counted by the span route, alone (its class is the only one) and among tiling
    windows (a class of its own)"""
    iv = [(0, 0, L.REFS[0][1], "whole")] + ([(0, b, b + 1000, None) for b in range(0, L.REFS[0][1], 1000)] if among else [])
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert want[1][0] + want[2][0] + want[3][0] > 40 * 256                # dozens of workgroups (256 reads each) add to the one row
    assert min(want[1][0], want[2][0], want[3][0]) > 0
    check(counted(iv, files), want, "whole contig")


def test_nesting_deeper_than_the_lds_cap(files):
    """1.45 times as many 3 kbp windows, 2 bp apart over the island, as a workgroup sums in LDS (1484 for the cap of 1024): those add
    to memory directly -- depth costs time, never a wrong value"""
    cap = lds_cap()
    iv = U.deep_nesting(cap)
    assert len(iv) > cap and iv[-1][1] < iv[0][2]                          # every window holds the bases before the first one's end: all are candidates there
    want = U.restate(U.default_calls(), iv, **U.DEFAULT_KW)
    assert np.isfinite(want[0]).all()
    check(counted(iv, files), want, "deep nesting")


@pytest.mark.parametrize("form", ["default", "span_off", "cap_4", "cap_0"])
def test_the_forms_agree(files, form, monkeypatch):
    """the full set in the kernel's differential forms (read once per context): without the span route every interval is counted read
    by read, with a cap of 4 most classes add to memory directly, with a cap of 0 all do"""
    env = dict(default={}, span_off={"MTH_PDR_REGIONS_SPAN": "0"}, cap_4={"MTH_PDR_REGIONS_LDS_CAP": "4"}, cap_0={"MTH_PDR_REGIONS_LDS_CAP": "0"})[form]
    for k in ("MTH_PDR_REGIONS_SPAN", "MTH_PDR_REGIONS_LDS_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check(counted(files["iv"], files), files["want"], form)


def test_call_order(files):
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(files["body"], files["offs"])
        tids, rb, re_, fl = eng.decoded_contigs()
        with pytest.raises(metheor_amd.MthError):
            eng.pdr_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))       # no intervals declared
        with pytest.raises(metheor_amd.MthError):
            eng.pdr_regions_begin([0], [10], [9])
        with pytest.raises(metheor_amd.MthError):
            eng.pdr_regions_begin([-1], [0], [9])
        eng.pdr_regions_begin([], [], [])
        eng.pdr_regions_accumulate(eng.decoded_batch(rb[1], re_[1], 1, 0, -1))
        assert len(eng.pdr_regions_fetch()["pdr"]) == 0
    finally:
        eng.close()


def test_a_data_error_surfaces_at_the_fetch(files):
    """contig ivA as a plain contig carries the word of position -1: the accumulate queues the pass and returns, the fetch reports it"""
    import metheor_amd
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(files["body"], files["offs"])
        tids, rb, re_, fl = eng.decoded_contigs()
        eng.pdr_regions_begin(*arrays(files["iv"]))
        eng.pdr_regions_accumulate(eng.decoded_batch(rb[0], re_[0], 0, 0, -1), min_cpgs=1, min_qual=0)
        with pytest.raises(metheor_amd.MthError):
            eng.pdr_regions_fetch()
    finally:
        eng.close()


# ---- 3. the command line ----------------------------------------------------------------------------------------------------------------
def cli(files, tag, *extra, env=None, bam=None, bed=None):
    o = files["dir"] / (tag + ".tsv")
    r = run("pdr-regions", "-i", bam or files["bam"], "--intervals", bed or files["bed"], "-o", o, *extra, env=env)
    assert r.returncode == 0, r.stderr
    return o.read_text()


@pytest.mark.parametrize("group", ["1", "0"])
def test_cli_bytes(files, group):
    text = cli(files, "g" + group, env={"METHEOR_GROUP": group})
    assert text == files["text"]
    row = [l for l in text.splitlines() if "\tempty\t" in l]
    assert len(row) == 1 and row[0].split("\t")[4:] == ["NaN", "0", "0", "0"]             # a zero-length interval


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
    assert 0 < sum(want[k].sum() for k in (1, 2, 3)) < sum(files["want"][k].sum() for k in (1, 2, 3))


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
    adds the three arrays and finalises once; the whole-contig interval and the windows around a cut straddle it"""
    env = {"METHEOR_SHARD_HALO": "4000", "METHEOR_DEVICES": "1"}
    assert cli(files, "sh2", "--gpus", "2", env=env) == files["text"]
    assert cli(files, "sh3", "--gpus", "3", env=env) == files["text"]


def test_all_forms(files):
    d = files["dir"]
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--pdr-intervals", d / "all_alone.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_alone.tsv").read_text() == files["text"]
    # beside the per-CpG table
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--pdr-intervals", d / "all_pr.tsv", "--pdr", d / "all_pdr.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_pr.tsv").read_text() == files["text"]
    r = run("pdr", "-i", files["bam"], "-o", d / "one_pdr.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_pdr.tsv").read_bytes() == (d / "one_pdr.tsv").read_bytes() and (d / "one_pdr.tsv").stat().st_size > 0
    # beside the other two per-interval tables, on the same BED
    r = run("all", "-i", files["bam"], "--intervals", files["bed"], "--pdr-intervals", d / "all_pr2.tsv", "--mhl-intervals", d / "all_mr.tsv",
            "--lpmd", d / "all_lpmd.tsv", "--lpmd-intervals", d / "all_li.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_pr2.tsv").read_text() == files["text"]
    r = run("mhl-regions", "-i", files["bam"], "--intervals", files["bed"], "-o", d / "one_mr.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_mr.tsv").read_bytes() == (d / "one_mr.tsv").read_bytes()
    r = run("lpmd", "-i", files["bam"], "-o", d / "one_lpmd.tsv", "--intervals", files["bed"], "--intervals-output", d / "one_li.tsv")
    assert r.returncode == 0, r.stderr
    assert (d / "all_li.tsv").read_bytes() == (d / "one_li.tsv").read_bytes() and (d / "all_lpmd.tsv").read_bytes() == (d / "one_lpmd.tsv").read_bytes()


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
        r = run("pdr-regions", "-i", inp, "--intervals", tmp_path / "i.bed", "-o", tmp_path / (tag + ".tsv"), "-d", "2", "-p", "2", *extra)
        assert r.returncode == 0, r.stderr
        out[tag] = (tmp_path / (tag + ".tsv")).read_text()
    want = U.restate(U.Calls(rec), iv, min_depth=2, min_cpgs=2, min_qual=10)
    assert out["tagged"] == U.table_text(iv, *want, names=[n for n, _ in rec.refs])
    assert out["genome"] == out["tagged"] and want[3].sum() > 0


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
        r = run("pdr-regions", "-i", inp, "--intervals", tmp_path / "i.bed", "-o", tmp_path / (tag + ".tsv"), "-d", "3", "-p", "2", *extra)
        assert r.returncode == 0, r.stderr
        out[tag] = (tmp_path / (tag + ".tsv")).read_text()
    want = U.restate(U.Calls(rec), iv, min_depth=3, min_cpgs=2, min_qual=10)
    assert out["xm"] == U.table_text(iv, *want, names=[n for n, _ in rec.refs])
    assert out["mm"] == out["xm"] and np.isfinite(want[0]).sum() > 10


def test_reference_fixtures(golden_dir, tmp_path):
    """tests/golden/test1.bam ... test6.bam, a whole-contig interval, -d 0: the counters pdr.rs's unit tests assert for every CpG
    (tests 4 and 6: tests/test_pdr_regions_definition.py derives them)"""
    want = {1: ("0.875", 2, 14), 2: ("0", 16, 0), 3: ("0", 2, 0), 4: ("0.875", 4, 28), 5: ("NaN", 0, 0), 6: ("0", 32, 0), 7: ("NaN", 0, 0)}
    for k in range(1, 8):
        p = os.path.join(golden_dir, "test%d.bam" % min(k, 6))        # 7: test 6's file under -p 2, where no read passes
        name = bamio.read_bam(p).refs[0][0]
        bed = tmp_path / ("i%d.bed" % k)
        bed.write_text("%s\t0\t%d\twhole\n" % (name, U.INT32_MAX))
        r = run("pdr-regions", "-i", p, "--intervals", bed, "-o", tmp_path / ("o%d.tsv" % k), "-p", {6: "1", 7: "2"}.get(k, "0"), "-d", "0")
        assert r.returncode == 0, r.stderr
        lines = (tmp_path / ("o%d.tsv" % k)).read_text().splitlines()
        v, c, d = want[k]
        assert lines[0] + "\n" == U.HEADER and len(lines) == 2, lines
        assert lines[1].split("\t")[:7] == [name, "0", str(U.INT32_MAX), "whole", v, str(c), str(d)], (k, lines)
