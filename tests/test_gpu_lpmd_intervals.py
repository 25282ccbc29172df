"""GPU parity of the per-interval LPMD (`lpmd --intervals`, mth_lpmd_intervals_fetch; mth_intervals.hip) against the CPU oracle: for
every interval the exact counters of the oracle's pairs table summed under the invariant (same contig, start <= cpg1, cpg2 < end) --
which tests/test_lpmd_intervals_inputs.py shows to be what `lpmd -c` counts for the interval's positions -- and the f32 lpmd bit for
bit; through the library with and without contig groups, and through the command line byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import lpmd_intervals_util as U
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
    """the synthetic records as a BAM whose blocks hold whole records (+ .bai), the BED, and what the oracle expects"""
    assert os.path.exists(EXE)
    d = tmp_path_factory.mktemp("lpmd_intervals")
    rec = U.records()
    raw_bam, bam, bed = str(d / "raw.bam"), str(d / "iv.bam"), d / "iv.bed"
    bamio.write_bam(raw_bam, rec)
    util.reblock_aligned(raw_bam, bam)
    bamio.write_bai(bam)
    bed.write_text(U.bed_text())
    iv = U.intervals()
    nc, nd = U.reduce_table(U.default_table(), iv)
    return dict(dir=d, rec=rec, bam=bam, bed=str(bed), iv=iv, nc=nc, nd=nd, text=U.table_text(iv, nc, nd),
                pairs_text=util.oracle_text(pyoracle.Reads.decode(rec), U.NAMES, "lpmd", input_name=bam, **U.DEFAULT_KW)[1])


def cli(files, tag, *extra, sub="lpmd", env=None, bam=None, bed=None, pairs=False):
    """one run -> (the interval table's bytes as text, the pairs table's or None)"""
    d = files["dir"]
    o, ivo, po = d / (tag + ".lpmd.tsv"), d / (tag + ".iv.tsv"), d / (tag + ".pairs.tsv")
    if sub == "lpmd":
        a = ["lpmd", "-i", bam or files["bam"], "-o", o, "--intervals", bed or files["bed"], "--intervals-output", ivo] + (["--pairs", po] if pairs else [])
    else:
        a = ["all", "-i", bam or files["bam"], "--lpmd", o, "--intervals", bed or files["bed"], "--lpmd-intervals", ivo] + (["--lpmd-pairs", po] if pairs else [])
    r = run(*a, *extra, env=env)
    assert r.returncode == 0, r.stderr
    return ivo.read_text(), (po.read_text() if pairs else None)


def same_bits(got, want):
    """f32 bit for bit; an interval without pairs is 0 / 0, a NaN whose sign and payload are the dividing unit's business"""
    nan = np.isnan(want)
    return (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["groups", "no_groups", "global_path"])
def test_library(files, monkeypatch, route):
    """the decoded stream as contig groups (one batch, virtual coordinates), as one batch per contig (the contig that holds a call at
    -1 still shifted, a group of one), and with every tile's rows on the pairs pass's global path (all rows unsorted)"""
    import metheor_amd
    body, offs = U.record_stream(files["bam"])
    iv = files["iv"]
    t_, b_, e_ = (np.array([x[k] for x in iv], np.int32) for k in range(3))
    if route == "global_path":
        monkeypatch.setenv("MTH_PAIRS_FORCE_GLOBAL", "1")
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(body, offs)
        tids, rb, re_, fl = eng.decoded_contigs()
        assert tids.tolist() == [0, 1]
        groups = eng.decoded_group(tids, rb, re_, each=route == "no_groups")
        assert [g[0] <= -2 for g in groups] == ([True, False] if route == "no_groups" else [True])
        for bt, r0, r1, _ in groups:
            eng.lpmd_pairs_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **U.DEFAULT_KW)
        first = eng.lpmd_intervals_fetch(t_, b_, e_)
        again = eng.lpmd_intervals_fetch(t_, b_, e_)                     # the reduction leaves the table as it was
        for got in (first, again):
            assert (got["n_concordant"] == files["nc"]).all() and (got["n_discordant"] == files["nd"]).all()
            assert same_bits(got["lpmd"], np.array([U.lpmd_f32(c, d) for c, d in zip(files["nc"], files["nd"])], np.float32))
        assert (files["nc"] + files["nd"] > 0).sum() > 250
        d = eng.lpmd_pairs_fetch()
        tid, p1, p2, c, dd = U.default_table()
        assert len(d["tid"]) == len(tid) and (d["tid"] == tid).all() and (d["pos1"] == p1).all() and (d["pos2"] == p2).all()
        assert (d["n_concordant"] == c).all() and (d["n_discordant"] == dd).all()
        # a subset in another order, an interval on a contig no batch has, and none at all
        sub = eng.lpmd_intervals_fetch(t_[::-3], b_[::-3], e_[::-3])
        assert (sub["n_concordant"] == files["nc"][::-3]).all() and (sub["n_discordant"] == files["nd"][::-3]).all()
        far = eng.lpmd_intervals_fetch([7], [0], [1000])
        assert far["n_concordant"].tolist() == [0] and far["n_discordant"].tolist() == [0]
        assert len(eng.lpmd_intervals_fetch([], [], [])["lpmd"]) == 0
        with pytest.raises(metheor_amd.MthError):
            eng.lpmd_intervals_fetch([0], [10], [9])
    finally:
        eng.close()


@pytest.mark.parametrize("force_global", [False, True], ids=["tiles", "global_path"])
def test_overlap_deeper_than_the_kernel_sums_in_lds(files, monkeypatch, force_global):
    """3000 windows of 3 kbp one base apart over the island, and 2500 nested ones: one length class each, deeper than the 1024
    intervals a workgroup sums in LDS (its rows add to memory directly) and with more starts inside a tile than the 2048 it stages
    (they are searched in memory) -- depth costs time, never a wrong sum or a capacity error"""
    import metheor_amd
    iv = [(0, 64_000 + k, 67_000 + k, None) for k in range(3000)] + [(0, 66_000 - k, 68_000 + k, None) for k in range(2500)]
    iv += [(1, 10_000 + k, 12_000 + k, None) for k in range(0, 1500, 3)]
    nc, nd = U.reduce_table(U.default_table(), iv)
    assert (nc > 0).all() and nc[3000:5500].min() > nc[:3000].max() // 2
    if force_global:
        monkeypatch.setenv("MTH_PAIRS_FORCE_GLOBAL", "1")
    body, offs = U.record_stream(files["bam"])
    eng = metheor_amd.Engine(0)
    try:
        eng.decode_records(body, offs)
        tids, rb, re_, fl = eng.decoded_contigs()
        for bt, r0, r1, _ in eng.decoded_group(tids, rb, re_):
            eng.lpmd_pairs_accumulate(eng.decoded_batch(r0, r1, bt, 0, -1), **U.DEFAULT_KW)
        got = eng.lpmd_intervals_fetch(*[[x[k] for x in iv] for k in range(3)])
        assert (got["n_concordant"] == nc).all() and (got["n_discordant"] == nd).all()
    finally:
        eng.close()


# ---- 2. the command line ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["1", "0"])
def test_cli_bytes_and_the_pairs_file_is_untouched(files, group):
    env = {"METHEOR_GROUP": group}
    got, pairs = cli(files, "g" + group, env=env, pairs=True)
    assert got == files["text"]
    assert pairs == files["pairs_text"]
    alone, _ = cli(files, "alone" + group, env=env)                      # without --pairs the table is never fetched
    assert alone == files["text"]
    d = files["dir"]
    r = run("lpmd", "-i", files["bam"], "-o", d / "plain.tsv", "--pairs", d / "plain.pairs.tsv", env=env)
    assert r.returncode == 0, r.stderr
    assert (d / "plain.pairs.tsv").read_text() == pairs and (d / "plain.tsv").read_bytes() == (d / ("g%s.lpmd.tsv" % group)).read_bytes()


def test_all_form_is_byte_equal(files):
    got, pairs = cli(files, "all", sub="all", pairs=True)
    assert got == files["text"] and pairs == files["pairs_text"]
    assert cli(files, "all_alone", sub="all")[0] == files["text"]


@pytest.mark.parametrize("flags", [["-m", "1", "-M", "3"], ["-q", "43"]], ids=["m1_M3", "q43"])
def test_parameters(files, flags):
    kw = dict(U.DEFAULT_KW, **util.oracle_kwargs("lpmd", flags))
    nc, nd = U.reduce_table(U.pairs_table(files["rec"], **kw), files["iv"])
    assert cli(files, "par" + flags[1], *flags)[0] == U.table_text(files["iv"], nc, nd)
    assert (nc.sum() == 0) == (flags[0] == "-q")


def test_cpg_set_gives_the_intersection(files):
    soa = pyoracle.Reads.decode(files["rec"]).soa()
    pos = (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    key = (np.repeat(soa["tid"].astype(np.int64), np.diff(soa["cpg_off"].astype(np.int64))) << 32) | pos
    keep = np.unique(key[pos < 0x7fffffff])[::2]
    sites = [(int(k >> 32), int(k & 0xffffffff)) for k in keep]
    bed = files["dir"] / "sites.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % (U.NAMES[t], p, p + 2) for t, p in sites))
    nc, nd = U.reduce_table(U.pairs_table(files["rec"], cpg_set=sites, **U.DEFAULT_KW), files["iv"])
    assert cli(files, "set", "-c", bed)[0] == U.table_text(files["iv"], nc, nd)
    assert 0 < nc.sum() < files["nc"].sum()


def test_unsorted_input(files):
    rec = files["rec"]
    perm = np.random.default_rng(5).permutation(len(rec))
    raw, bam = str(files["dir"] / "shuf_raw.bam"), str(files["dir"] / "shuf.bam")
    bamio.write_bam(raw, rec.subset(perm))
    util.reblock_aligned(raw, bam)
    assert cli(files, "shuf", bam=bam)[0] == files["text"]


def test_region_against_the_invariant(files):
    """--region over the middle third of the first contig: the pairs table holds the rows whose cpg1 lies in the region, and the
    interval table is that table summed"""
    b, e = 66_666, 133_333
    tid, p1, p2, c, d = U.default_table()
    m = (tid == 0) & (p1 >= b) & (p1 < e)
    nc, nd = U.reduce_table(tuple(x[m] for x in (tid, p1, p2, c, d)), files["iv"])
    got, pairs = cli(files, "reg", "--region", "ivA:%d-%d" % (b + 1, e), pairs=True)
    assert got == U.table_text(files["iv"], nc, nd)
    own = U.reduce_table(U.parse_pairs_file(pairs, U.NAMES), files["iv"])
    assert (own[0] == nc).all() and (own[1] == nd).all() and 0 < nc.sum() < files["nc"].sum()


def test_two_shards_on_one_device(files):
    """--gpus 2: every shard reduces its own rows for all the intervals, the sums are added once; intervals that straddle the cut
    (the whole contig, and the windows around it) are counted once"""
    env = {"METHEOR_SHARD_HALO": "4000", "METHEOR_DEVICES": "1"}
    got, pairs = cli(files, "sh2", "--gpus", "2", env=env, pairs=True)
    assert got == files["text"] and pairs == files["pairs_text"]
    # the cut lies inside the first contig: both shards own rows of the whole-contig interval
    r = run("lpmd", "-i", files["bam"], "-o", files["dir"] / "x.tsv", "--intervals", files["bed"], "--intervals-output", files["dir"] / "sh3.tsv",
            "--gpus", "3", env=env)
    assert r.returncode == 0, r.stderr
    assert (files["dir"] / "sh3.tsv").read_text() == files["text"]


def _own_pairs_route(tmp, inp, flags):
    """intervals cut from a run's own --pairs file; the interval table of the same command line must be that file summed"""
    r = run("lpmd", "-i", inp, "-o", tmp / "o.tsv", "--pairs", tmp / "p.tsv", *flags)
    assert r.returncode == 0, r.stderr
    text = (tmp / "p.tsv").read_text()
    names = sorted(set(l.split("\t")[0] for l in text.splitlines()[1:]))
    table = U.parse_pairs_file(text, names)
    assert len(table[0]) > 100
    iv = []
    for t in range(len(names)):
        p = table[1][table[0] == t]
        lo, hi = int(p.min()), int(p.max())
        step = max((hi - lo) // 20, 50)
        iv += [(t, b, b + step, None) for b in range(max(lo - 10, 0), hi, step)] + [(t, 0, U.INT32_MAX, "all"), (t, lo, hi, "inner"), (t, max(lo - 10, 0), lo + 2 * step + 7, "head")]
    (tmp / "i.bed").write_text("".join("%s\t%d\t%d%s\n" % (names[t], b, e, "\t" + n if n else "") for t, b, e, n in iv))
    r = run("lpmd", "-i", inp, "-o", tmp / "o2.tsv", "--pairs", tmp / "p2.tsv", "--intervals", tmp / "i.bed", "--intervals-output", tmp / "iv.tsv", *flags)
    assert r.returncode == 0, r.stderr
    assert (tmp / "p2.tsv").read_text() == text
    nc, nd = U.reduce_table(table, iv)
    assert (tmp / "iv.tsv").read_text() == U.table_text(iv, nc, nd, names) and (nc + nd > 0).sum() > 5


def test_genome_route(golden_dir, tmp_path):
    from tests import tag_util
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    noxm, fa = tmp_path / "noxm.sam", tmp_path / "chr19.fa"
    noxm.write_text(noxm_text)
    tag_util.write_fasta(str(fa), "chr19", contig)
    _own_pairs_route(tmp_path, noxm, ["--genome", fa])


def test_mm_tags_route(tmp_path):
    from tests import modtags_util as M
    g = M.generate(1, 1500, long_reads=False)
    f, fp = tmp_path / "f.sam", tmp_path / "fp.sam"
    M.write_pair(g["refs"], g["recs"], 128, f, fp)
    _own_pairs_route(tmp_path, f, ["--mm-tags", "-m", "1", "-M", "30"])


def test_reference_fixtures(golden_dir, tmp_path):
    """tests/golden/test1.bam: the interval [0, 8) holds every pair of z.z.z.z. -- 48 / 48 and 0.5 (lpmd.rs:219); test5.bam: no pair"""
    p1 = os.path.join(golden_dir, "test1.bam")
    rec = bamio.read_bam(p1)
    name = rec.refs[0][0]
    iv = [(0, 0, 8, "all"), (0, 0, 6, "three"), (0, 2, 8, None), (0, 0, U.INT32_MAX, "open")]
    nc, nd = U.reduce_table(U.pairs_table(rec, **U.DEFAULT_KW), iv)
    assert (nc[0], nd[0]) == (48, 48) and 0 < nc[1] + nd[1] < 96
    bed = tmp_path / "i.bed"
    bed.write_text("".join("%s\t%d\t%d%s\n" % (name, b, e, "\t" + n if n else "") for _, b, e, n in iv))
    r = run("lpmd", "-i", p1, "-o", tmp_path / "o.tsv", "--intervals", bed, "--intervals-output", tmp_path / "iv.tsv")
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "iv.tsv").read_text()
    assert text == U.table_text(iv, nc, nd, [name])
    assert text.splitlines()[1] == "%s\t0\t8\tall\t0.5\t48\t48" % name
    p5 = os.path.join(golden_dir, "test5.bam")
    name5 = bamio.read_bam(p5).refs[0][0]
    bed.write_text("%s\t0\t1000\n" % name5)
    r = run("lpmd", "-i", p5, "-o", tmp_path / "o5.tsv", "--intervals", bed, "--intervals-output", tmp_path / "iv5.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "iv5.tsv").read_text() == U.HEADER + "%s\t0\t1000\t.\tNaN\t0\t0\n" % name5
    bed.write_text("")                                                   # an empty BED: the header alone
    r = run("lpmd", "-i", p1, "-o", tmp_path / "o.tsv", "--intervals", bed, "--intervals-output", tmp_path / "iv0.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "iv0.tsv").read_text() == U.HEADER
