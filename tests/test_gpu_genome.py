"""`--genome` on the MI355X: `metheor M -i in -g genome.fa` == `metheor tag -i in -o tagged.sam -g genome.fa`, then
`metheor M -i tagged.sam`, byte for byte -- the library entry (mth_decode_set_genome) in both of its forms against the CPU
chain and against the two existing device steps, the command line on the reference's fixture and on generated records."""
import os
import re
import subprocess

import numpy as np
import pytest

from metheor_amd import hostapi
from oracle import bamio
from tests import genome_util as gu
from tests import tag_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
KEYS = ("tid", "start", "end", "mapq", "fwd", "cpg_off", "cpg_pos", "cpg_rel")
SINGLE = ["pdr", "mhl", "me", "pm", "fdrp", "qfdrp", "lpmd"]
LOW = {"pdr": ["-d", "1", "-p", "1"], "mhl": ["-d", "1", "-p", "1"], "me": ["-d", "1"], "pm": ["-d", "1"], "fdrp": ["-d", "1"],
       "qfdrp": ["-d", "1"], "lpmd": ["-m", "1", "-M", "30"]}


def run(*args, env=None):
    e = dict(os.environ, METHEOR_SEED="5")
    e.update(env or {})
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=600, env=e)


def measure(sub, inp, outdir, tag, extra=(), genome=None, env=None, more=()):
    """one measure run -> (status, stderr, {output name: bytes with the input's path taken out of lpmd's row})"""
    outdir = outdir / tag
    outdir.mkdir(exist_ok=True)
    if sub == "all":
        names = ["pdr", "lpmd", "lpmd-pairs", "mhl", "me", "pm", "fdrp", "qfdrp"]
        args = ["all", "-i", inp] + [x for n in names for x in ("--" + n, outdir / (n + ".tsv"))]
    else:
        names = ["out"] + (["pairs"] if sub == "lpmd" else [])
        args = [sub, "-i", inp, "-o", outdir / "out.tsv"] + (["--pairs", outdir / "pairs.tsv"] if sub == "lpmd" else [])
    r = run(*args, *extra, *more, *(["-g", genome] if genome else []), env=env)
    outs = {n: (outdir / (n + ".tsv")).read_bytes().replace(str(inp).encode(), b"<input>") for n in names if (outdir / (n + ".tsv")).exists()}
    return r.returncode, r.stderr, outs


def assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0], a[1], b[1])
    assert a[0] == 0, (what, a[1])
    assert a[2].keys() == b[2].keys() and a[2], what
    for k in a[2]:
        assert a[2][k] == b[2][k], (what, k, len(a[2][k]), len(b[2][k]))
    return a[2]


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gens(tmp_path_factory):
    """seed -> the generated input without the records `tag` panics on: SAM text (XM-free), FASTA, the chain's strings"""
    d = tmp_path_factory.mktemp("genome_gen")
    out = {}
    for seed in (1, 2, 3, 4):
        g = gu.generate(seed)
        recs, xms = gu.runnable(g)
        refs = [(g["name"], len(g["contig"]))]
        sam, fa = str(d / ("in%d.sam" % seed)), str(d / ("g%d.fa" % seed))
        open(sam, "w").write(gu.sam_text(refs, recs))
        tag_util.write_fasta(fa, g["name"], g["contig"])
        out[seed] = dict(g, recs=recs, xms=xms, refs=refs, sam=sam, fa=fa, dir=d)
    return out


@pytest.fixture(scope="module")
def chr19(golden_dir, tmp_path_factory):
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    d = tmp_path_factory.mktemp("genome_chr19")
    noxm, fa = str(d / "test.chr19.noXM.sam"), str(d / "chr19.rebuilt.fa")
    open(noxm, "w").write(noxm_text)
    tag_util.write_fasta(fa, "chr19", contig)
    xm = os.path.join(golden_dir, "test.chr19.XM.sam")
    bams = {}
    for name, p in (("noxm", noxm), ("xm", xm)):                 # the BAM forms: mth_bgzf_decode is the path taken
        f = hostapi.BamFile(p)
        bams[name] = str(d / (name + ".bam"))
        open(bams[name], "wb").write(open(f.staged_path(), "rb").read())
        f.close()
    return dict(noxm=noxm, xm=xm, fa=fa, noxm_bam=bams["noxm"], xm_bam=bams["xm"], dir=d)


# ---- 1. the library ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_library_soa_equals_the_chain_and_the_two_device_steps(eng, gens, tmp_path, monkeypatch, seed, staged):
    g = gens[seed]
    monkeypatch.setenv("METHEOR_GENOME_STAGED", "1" if staged else "0")
    f = hostapi.BamFile(g["sam"])
    (raw, off), = f.windows()
    n = len(off) - 1
    assert n == len(g["recs"]) and f.first_flag() == g["recs"][0][2]
    paired = bool(g["recs"][0][2] & 1)
    assert paired == g["paired"]
    contigs = [(len(g["contig"]), g["contig"])]
    # the second expectation: the records carrying the strings mth_tag_records returns, decoded with the mode off
    eng.tag_set_genome(contigs)
    dev_xm = eng.tag_records(raw, off, is_paired_end=paired)
    assert dev_xm == g["xms"]
    tagged = tmp_path / "tagged.sam"
    with open(tagged, "wb") as fh:
        fh.write(f.header_text())
        for k in range(n):
            fh.write(f.sam_line(raw, int(off[k]), int(off[k + 1]), dev_xm[k]))
    assert sum(1 for l in open(tagged, "rb") if l.endswith(b"\tXM:Z:\n")) == sum(1 for x in dev_xm if not x) > 0      # an empty tag stays a present tag
    ft = hostapi.BamFile(str(tagged))
    (raw_t, off_t), = ft.windows()
    want_all = gu.expected_reads(g["refs"], g["recs"], g["xms"]).soa()
    half = sorted({(0, int(p & 0x7fffffff)) for p in want_all["cpg_pos"]})[::2]
    try:
        for filt in (None, half):
            want = want_all if filt is None else gu.expected_reads(g["refs"], g["recs"], g["xms"], cpg_set=filt).soa()
            assert len(want["cpg_pos"]) > (20000 if filt is None else 8000)
            eng.decode_set_cpg_filter(filt)
            eng.decode_set_genome(False)
            eng.decode_records(raw_t, off_t)
            two_step = eng.decoded_fetch()
            eng.decode_set_genome(True, is_paired_end=paired)
            eng.decode_records(raw, off)
            one = eng.decoded_fetch()
            cuts = [0, n // 3, n // 3 + 1, 2 * n // 3, n]           # the same appended in several windows
            for a, b in zip(cuts[:-1], cuts[1:]):
                eng.decode_records(raw[int(off[a]):int(off[b])], off[a:b + 1] - off[a], append=a > 0)
            several = eng.decoded_fetch()
            for k in KEYS:
                assert np.array_equal(one[k], want[k]), (k, "chain", filt is not None)
                assert np.array_equal(one[k], two_step[k]), (k, "two device steps", filt is not None)
                assert np.array_equal(one[k], several[k]), (k, "appended windows", filt is not None)
    finally:
        eng.decode_set_genome(False)
        eng.decode_set_cpg_filter(None)


def test_set_genome_before_a_genome_is_a_state_error():
    import metheor_amd
    e = metheor_amd.Engine(0)
    try:
        with pytest.raises(metheor_amd.MthError) as err:
            e.decode_set_genome(True)
        assert err.value.status == -9                              # MTH_ERR_STATE
        e.decode_set_genome(False)                                 # switching it off needs no genome
    finally:
        e.close()


# ---- 2. the reference's data ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sam", "bam"])
@pytest.mark.parametrize("low", [False, True], ids=["defaults", "d1p1"])
def test_reference_fixture_with_genome_equals_its_tagged_file(chr19, tmp_path, form, low):
    noxm, xm = (chr19["noxm"], chr19["xm"]) if form == "sam" else (chr19["noxm_bam"], chr19["xm_bam"])
    rows = {}
    for sub in SINGLE + ["all"]:
        extra = (LOW[sub] if sub != "all" else ["-d", "1", "-p", "1"]) if low else []
        a = measure(sub, noxm, tmp_path, sub + "_g", extra, genome=chr19["fa"])
        b = measure(sub, xm, tmp_path, sub + "_xm", extra)
        outs = assert_same(a, b, (sub, form, low))
        for k, v in outs.items():
            rows[(sub, k)] = v.count(b"\n")
    if not low:       # the oracle's row counts at the defaults
        assert rows[("pdr", "out")] == 62 and rows[("mhl", "out")] == 62 and rows[("me", "out")] == 22 and rows[("pm", "out")] == 22
        assert rows[("fdrp", "out")] == 77 and rows[("qfdrp", "out")] == 77
        assert (rows[("all", "pdr")], rows[("all", "mhl")], rows[("all", "me")], rows[("all", "pm")], rows[("all", "fdrp")]) == (62, 62, 22, 22, 77)


# ---- 3. generated input against the two-step run ------------------------------------------------------------------------
def two_step_input(g, tmp_path, sam=None, name="tagged.sam"):
    tagged = tmp_path / name
    r = run("tag", "-i", sam or g["sam"], "-o", tagged, "-g", g["fa"])
    assert r.returncode == 0, r.stderr
    return str(tagged)


@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
@pytest.mark.parametrize("seed", [1, 3])
def test_generated_input_equals_the_two_step_run(gens, tmp_path, seed, staged):
    g = gens[seed]
    tagged = two_step_input(g, tmp_path)
    env = {"METHEOR_GENOME_STAGED": "1"} if staged else {}
    for sub in SINGLE + ["all"]:
        a = measure(sub, g["sam"], tmp_path, sub + "_g", genome=g["fa"], env=env)
        b = measure(sub, tagged, tmp_path, sub + "_two")
        outs = assert_same(a, b, (sub, seed, staged))
        n = {k: v.count(b"\n") for k, v in outs.items()}
        if sub in ("pdr", "mhl", "fdrp", "qfdrp"):
            assert n["out"] >= 500, (sub, n)
        if sub in ("me", "pm"):
            assert n["out"] >= 100, (sub, n)
        if sub == "lpmd":
            assert n["pairs"] > 1000
        if sub == "all":
            assert min(n["pdr"], n["mhl"], n["fdrp"], n["qfdrp"]) >= 500 and min(n["me"], n["pm"]) >= 100, n


def aligned_start(rec):
    """first reference position an M / = / X run covers: what --region and --gpus N want the records sorted by"""
    r = rec[1]
    for c in rec[4]:
        if (c & 15) in (0, 7, 8) and (c >> 4):
            return r
        if (c & 15) in (2, 3):
            r += c >> 4
    return -1


def sorted_by_start(g, recs, path):
    """the records in the order of their first aligned base (a leading D / N moves it past the next record's), as SAM text"""
    order = sorted(range(len(recs)), key=lambda k: (aligned_start(recs[k]), k))
    open(path, "w").write(gu.sam_text(g["refs"], [recs[k] for k in order]))
    return dict(g, sam=str(path), recs=[recs[k] for k in order])


def as_bam(sam, path):
    f = hostapi.BamFile(sam)
    open(path, "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    return str(path)


@pytest.mark.parametrize("seed", [2, 4])
def test_shuffled_copy_file_order_replay_and_device_sort(gens, tmp_path, seed):
    g = gens[seed]
    lines = open(g["sam"]).read().splitlines()
    head, body = [l for l in lines if l.startswith("@")], [l for l in lines if not l.startswith("@")]
    rng = np.random.default_rng(seed)
    # blocks of records moved around: the first record stays first (the paired flag is the same on all of them anyway)
    blocks = [body[k:k + 500] for k in range(0, len(body), 500)]
    order = [0] + list(1 + rng.permutation(len(blocks) - 1))
    shuffled = tmp_path / "shuffled.sam"
    shuffled.write_text("\n".join([head[0].replace("coordinate", "unsorted")] + head[1:] + [l for k in order for l in blocks[k]]) + "\n")
    tagged = two_step_input(g, tmp_path, sam=str(shuffled))
    for sub in SINGLE:
        a = measure(sub, str(shuffled), tmp_path, sub + "_g", LOW[sub] if sub in ("me", "pm") else [], genome=g["fa"])
        b = measure(sub, tagged, tmp_path, sub + "_two", LOW[sub] if sub in ("me", "pm") else [])
        outs = assert_same(a, b, (sub, seed))
        assert outs["out"].count(b"\n") >= (2 if sub == "lpmd" else 100), sub


def test_region_gpus_and_cpg_set(gens, tmp_path):
    g = sorted_by_start(gens[3], gens[3]["recs"], tmp_path / "in.sam")
    xms = gu.chain_xm(g["recs"], [g["contig"]], g["paired"])
    bam = as_bam(g["sam"], tmp_path / "in.bam")
    tagged_bam = as_bam(two_step_input(g, tmp_path), tmp_path / "tagged.bam")
    bamio.write_bai(bam)
    bamio.write_bai(tagged_bam)
    region = "%s:9001-21000" % g["name"]
    env = {"METHEOR_SHARD_HALO": "4000"}
    for sub in SINGLE:
        extra = ["-d", "3"] if sub not in ("lpmd",) else []
        a = measure(sub, bam, tmp_path, sub + "_rg", extra, genome=g["fa"], more=["--region", region], env=env)
        b = measure(sub, tagged_bam, tmp_path, sub + "_r2", extra, more=["--region", region], env=env)
        outs = assert_same(a, b, (sub, "region"))
        assert outs["out"].count(b"\n") >= (2 if sub == "lpmd" else 50), sub
        a = measure(sub, bam, tmp_path, sub + "_sg", extra, genome=g["fa"], more=["--gpus", "2"], env=env)
        b = measure(sub, tagged_bam, tmp_path, sub + "_s2", extra, env=env)
        assert_same(a, b, (sub, "gpus 2"))
    # -c: a BED of half the CpGs the chain calls
    want = gu.expected_reads(g["refs"], g["recs"], xms).soa()
    sites = sorted({int(p & 0x7fffffff) for p in want["cpg_pos"]})[::2]
    bed = tmp_path / "half.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % (g["name"], p, p + 2) for p in sites))
    for sub in ("pdr", "lpmd", "fdrp", "all"):
        extra = ["-d", "3", "-p", "2"] if sub in ("pdr", "all") else (["-d", "3"] if sub == "fdrp" else [])
        a = measure(sub, bam, tmp_path, sub + "_cg", extra, genome=g["fa"], more=["-c", bed])
        b = measure(sub, tagged_bam, tmp_path, sub + "_c2", extra, more=["-c", bed])
        outs = assert_same(a, b, (sub, "cpg-set"))
        assert all(v.count(b"\n") >= 2 for v in outs.values()), sub


def test_the_paired_flag_is_the_files_first_record_also_under_region(gens, tmp_path):
    """first record unpaired, every later record carries 0x1: `tag` treats them all as single-end (bamutil.rs:27-37), and so
    must a --region run that never decodes the first record"""
    g = gens[4]
    lines = open(g["sam"]).read().splitlines()
    head, body = [l for l in lines if l.startswith("@")], [l for l in lines if not l.startswith("@")]
    first = body[0].split("\t")
    first[1] = "0"
    recs = []
    for x in [first] + [l.split("\t") for l in body[1:]]:
        cig = [(int(n) << 4) | gu.OPS.index(o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", x[5])]
        recs.append((0, int(x[3]) - 1, int(x[1]), int(x[4]), cig, x[9].encode(), x[5]))
    # single-end rules on paired flags: drop the records `tag` panics on under THAT rule, as the generator does under its own
    xms = gu.chain_xm(recs, [g["contig"]], paired=False)
    keep = [k for k, x in enumerate(xms) if x is not None]
    assert keep[0] == 0 and len(keep) > 0.99 * len(recs)
    mixed = tmp_path / "mixed.sam"
    kept = [recs[0]] + sorted_by_start(g, [recs[k] for k in keep[1:]], mixed)["recs"]
    assert aligned_start(kept[0]) <= aligned_start(kept[1])
    mixed.write_text(gu.sam_text(g["refs"], kept))
    f = hostapi.BamFile(str(mixed))
    assert f.first_flag() == 0
    f.close()
    g2 = dict(g, sam=str(mixed))
    bam = as_bam(str(mixed), tmp_path / "mixed.bam")
    tagged_bam = as_bam(two_step_input(g2, tmp_path), tmp_path / "mixed_tagged.bam")
    bamio.write_bai(bam)
    bamio.write_bai(tagged_bam)
    region = "%s:15001-25000" % g["name"]
    for sub in ("pdr", "me"):
        a = measure(sub, bam, tmp_path, sub + "_g", ["-d", "3"], genome=g["fa"], more=["--region", region])
        b = measure(sub, tagged_bam, tmp_path, sub + "_2", ["-d", "3"], more=["--region", region])
        outs = assert_same(a, b, (sub, "mixed flags, region"))
        assert outs["out"].count(b"\n") >= 30
    # and the flag matters: the same records read as paired give another table
    xs, xp = gu.chain_xm(kept, [g["contig"]], paired=False), gu.chain_xm(kept, [g["contig"]], paired=True)
    assert sum(1 for a_, b_ in zip(xp, xs) if a_ != b_) > 100


# ---- 4. errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line,why", [
    ("r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*", "an unplaced record: tid2size[&tid] panics (tag.rs:155)"),
    ("r\t0\tc0\t398\t30\t10M\t*\t0\t0\tACGTACGTAC\t*", "the alignment ends more than two bases past the contig (tag.rs:170)"),
    ("r\t16\tc0\t10\t3\t2M1I2M\t*\t0\t0\tAC=GT\t*", "'=' has no complement (tag.rs:24); mapq below lpmd's --min-qual"),
    ("r\t16\tc0\t10\t3\t5M\t*\t0\t0\tAC=GT\t*", "the same on a plain record"),
])
@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
def test_a_record_tag_panics_on_ends_the_run_with_101(tmp_path, line, why, staged):
    contig = b"ACGT" * 100
    p = tmp_path / "p.sam"
    p.write_text("@HD\tVN:1.6\n@SQ\tSN:c0\tLN:400\nok\t0\tc0\t21\t30\t8M\t*\t0\t0\tACGTACGT\t*\n" + line + "\n")
    fa = str(tmp_path / "g.fa")
    tag_util.write_fasta(fa, "c0", contig)
    env = {"METHEOR_GENOME_STAGED": "1"} if staged else {}
    r = run("tag", "-i", p, "-o", tmp_path / "t.sam", "-g", fa)
    assert r.returncode == 101, why
    for sub in ("pdr", "lpmd"):
        r = run(sub, "-i", p, "-o", tmp_path / "o.tsv", "-g", fa, env=env)
        assert r.returncode == 101, (sub, why, r.stderr)
        assert "tag" in r.stderr, (sub, why, r.stderr)


def test_fasta_errors_are_tags_and_leave_no_output(tmp_path):
    p = tmp_path / "two.sam"
    p.write_text("@HD\tVN:1.6\n@SQ\tSN:c0\tLN:8\n@SQ\tSN:other\tLN:8\nr\t0\tc0\t1\t30\t4M\t*\t0\t0\tACGT\t*\n")
    fa = str(tmp_path / "g.fa")
    tag_util.write_fasta(fa, "c0", b"ACGTACGT", with_fai=False)
    for sub in ("pdr", "all"):
        out = tmp_path / ("o_%s.tsv" % sub)
        o = ["--pdr", out] if sub == "all" else ["-o", out]
        r = run(sub, "-i", p, *o, "-g", tmp_path / "no_such.fa")
        assert r.returncode == 101 and "Error opening reference genome file" in r.stderr and "no_such.fa" in r.stderr
        assert not out.exists() and r.stdout == ""
        r = run(sub, "-i", p, *o, "-g", fa)
        assert r.returncode == 101 and "Error fetching reference genome sequence" in r.stderr
        assert not out.exists() and r.stdout == ""


def test_without_genome_a_record_without_xm_still_fails(chr19, tmp_path):
    r = run("pdr", "-i", chr19["noxm"], "-o", tmp_path / "o.tsv")
    assert r.returncode == 101 and "Error reading XM tag in BAM record" in r.stderr


def test_host_decoder_has_no_genome_form(chr19, tmp_path):
    out = tmp_path / "o.tsv"
    r = run("pdr", "-i", chr19["noxm"], "-o", out, "-g", chr19["fa"], env={"METHEOR_HOST_DECODE": "1"})
    assert r.returncode == 101 and "--genome needs the device record decode" in r.stderr and not out.exists()


# ---- 5. XM:Z already in the input is ignored -----------------------------------------------------------------------------
def test_an_xm_tag_in_the_input_is_ignored_with_genome(chr19, tmp_path):
    # spoil the tags: the z / Z letters of every read alternate, so every read with two calls becomes discordant.  Without -g
    # that changes the PDR table; with -g it does not
    def spoil(xm):
        out, k = [], 0
        for ch in xm:
            if ch in "zZ":
                ch = "Zz"[k & 1]
                k += 1
            out.append(ch)
        return "".join(out)
    spoiled = tmp_path / "spoiled.sam"
    n_changed = 0
    with open(spoiled, "w") as fh:
        for l in open(chr19["xm"]):
            f = l.rstrip("\n").split("\t")
            if not l.startswith("@"):
                g = ["XM:Z:" + spoil(x[5:]) if x.startswith("XM:Z:") else x for x in f]
                n_changed += g != f
                f = g
            fh.write("\t".join(f) + "\n")
    assert n_changed > 100
    a = measure("pdr", chr19["noxm"], tmp_path, "noxm", ["-d", "1", "-p", "1"], genome=chr19["fa"])
    b = measure("pdr", str(spoiled), tmp_path, "spoiled_g", ["-d", "1", "-p", "1"], genome=chr19["fa"])
    c = measure("pdr", chr19["xm"], tmp_path, "xm_g", ["-d", "1", "-p", "1"], genome=chr19["fa"])
    d = measure("pdr", str(spoiled), tmp_path, "spoiled", ["-d", "1", "-p", "1"])
    assert_same(a, b, "spoiled XM with -g")
    assert_same(a, c, "golden XM with -g")
    assert d[0] == 0 and d[2]["out"] != a[2]["out"]
