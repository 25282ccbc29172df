"""`metheor me-regions / pm-regions -i IN --intervals BED -o OUT` and `all --intervals BED --me-intervals OUT --pm-intervals OUT` (an
MI355X extension: ME and PM per interval, counted on the device): options, `requires` rules, the BED's errors.  All of it happens
before any device is needed or any output is created: runs on CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
T1 = os.path.join(ROOT, "tests", "golden", "test1.bam")        # one contig, "chr1"
HEADER = {"me-regions": "chrom\tstart\tend\tname\tme\tn_patterns\tn_reads\n", "pm-regions": "chrom\tstart\tend\tname\tpm\tn_patterns\tn_reads\n"}
SUBS = ["me-regions", "pm-regions"]
TABLE = {"me-regions": "--me-intervals", "pm-regions": "--pm-intervals"}


def run(*args):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=120)


@pytest.fixture(scope="module", autouse=True)
def built():
    from metheor_amd import build
    build.build()
    assert os.path.exists(EXE)


@pytest.fixture(scope="module")
def contig():
    from oracle import bamio
    return bamio.read_bam(T1).refs[0][0]


@pytest.mark.parametrize("sub", SUBS)
def test_help_lists_the_options(sub):
    h = run(sub, "--help")
    assert h.returncode == 0, h.stderr
    assert "Usage: metheor %s [OPTIONS] --input <INPUT> --output <OUTPUT> --intervals <INTERVALS>" % sub in h.stdout
    for o, d in (("-d, --min-depth <MIN_DEPTH>", "10"), ("-q, --min-qual <MIN_QUAL>", "10"), ("-G, --gpus <GPUS>", "1")):      # me's defaults
        line = [l for l in h.stdout.splitlines() if o in l]
        assert len(line) == 1 and line[0].endswith("[default: %s]" % d), (o, line)
    options = h.stdout[h.stdout.index("Options:"):].splitlines()          # (the usage line names the required ones too)
    for o in ("--intervals <INTERVALS>", "-c, --cpg-set <CPG_SET>", "-g, --genome <GENOME>", "--mm-tags ", "--mm-threshold <MM_THRESHOLD>", "-o, --output <OUTPUT>"):
        assert len([l for l in options if o in l]) == 1, o
    assert "--region" not in h.stdout and "--bai" not in h.stdout and "--min-cpgs" not in h.stdout      # no -p, as on me / pm
    line = [l for l in run("--help").stdout.splitlines() if l.strip().startswith(sub + " ")]
    assert len(line) == 1 and "(MI355X extension)" in line[0]


def test_all_help_and_the_single_commands():
    h = run("all", "--help")
    assert h.returncode == 0, h.stderr
    for o in ("--me-intervals <ME_INTERVALS>", "--pm-intervals <PM_INTERVALS>", "--pdr-intervals <PDR_INTERVALS>", "--intervals <INTERVALS>", "--me <ME>", "--pm <PM>"):
        assert len([l for l in h.stdout.splitlines() if o in l]) == 1, o
    assert "--intervals" not in run("me", "--help").stdout and "--intervals" not in run("pm", "--help").stdout
    r = run("me-regions", "-i", T1, "-o", "x", "--intervals", "y", "-p", "4")
    assert r.returncode == 2 and "unexpected argument '-p' found" in r.stderr


@pytest.mark.parametrize("sub", SUBS)
def test_required_arguments(tmp_path, sub):
    bed, out = tmp_path / "i.bed", tmp_path / "o.tsv"
    bed.write_text("")
    r = run(sub, "-i", T1, "-o", out)
    assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr and "Usage: metheor " + sub in r.stderr
    r = run(sub, "-i", T1, "--intervals", bed)
    assert r.returncode == 2 and "--output <OUTPUT>" in r.stderr
    r = run(sub, "-o", out, "--intervals", bed)
    assert r.returncode == 2 and "--input <INPUT>" in r.stderr
    assert not out.exists()


def test_region_is_refused(tmp_path):
    bed, out, lp = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "l.tsv"
    bed.write_text("")
    for sub in SUBS:
        r = run(sub, "-i", T1, "-o", out, "--intervals", bed, "--region", "chr1")
        assert r.returncode == 2 and "unexpected argument '--region' found" in r.stderr
        r = run(sub, "-i", T1, "-o", out, "--intervals", bed, "--bai", "x.bai")
        assert r.returncode == 2 and "unexpected argument '--bai' found" in r.stderr
    r = run("all", "-i", T1, "--intervals", bed, "--me-intervals", out, "--region", "chr1")
    assert r.returncode == 2 and "'--me-intervals <ME_INTERVALS>' cannot be used with '--region <REGION>'" in r.stderr and "Usage: metheor all" in r.stderr
    r = run("all", "-i", T1, "--intervals", bed, "--pm-intervals", out, "--region", "chr1")
    assert r.returncode == 2 and "'--pm-intervals <PM_INTERVALS>' cannot be used with '--region <REGION>'" in r.stderr and "Usage: metheor all" in r.stderr
    r = run("all", "-i", T1, "--lpmd", lp, "--intervals", bed, "--lpmd-intervals", tmp_path / "li.tsv", "--me-intervals", out, "--region", "chr1")
    assert r.returncode == 2 and "--me-intervals" in r.stderr
    r = run("all", "-i", T1, "--me", lp, "--region", "chr1", "--bai", tmp_path / "none.bai")      # --me itself still takes a region
    assert "cannot be used with" not in r.stderr
    assert not out.exists()


def test_all_requires(tmp_path):
    bed, out, out2, li, me = (tmp_path / n for n in ("i.bed", "o.tsv", "o2.tsv", "li.tsv", "me.tsv"))
    bed.write_text("")
    for opt in ("--me-intervals", "--pm-intervals"):
        r = run("all", "-i", T1, opt, out)                                          # the table needs the BED
        assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr and "Usage: metheor all" in r.stderr
        r = run("all", "-i", T1, "--me", me, opt, out)                              # ... also beside the per-quartet table
        assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr
        r = run("all", "-i", T1, opt, out, "--intervals", bed, "--lpmd-intervals", li)      # the LPMD table is still LPMD's
        assert r.returncode == 2 and "--lpmd <LPMD>" in r.stderr
    r = run("all", "-i", T1, "--me", me, "--intervals", bed)                        # the BED needs one of its tables
    assert r.returncode == 2 and all(o in r.stderr for o in ("--lpmd-intervals <LPMD_INTERVALS>", "--mhl-intervals <MHL_INTERVALS>", "--pdr-intervals <PDR_INTERVALS>",
                                                               "--me-intervals <ME_INTERVALS>", "--pm-intervals <PM_INTERVALS>"))
    r = run("all", "-i", T1)                                                        # either table is an output of its own
    assert r.returncode == 2 and "--me-intervals <ME_INTERVALS>" in r.stderr and "--pm-intervals <PM_INTERVALS>" in r.stderr and "--pdr <PDR>|--lpmd <LPMD>" in r.stderr
    assert not any(p.exists() for p in (out, out2, li, me))


def test_the_tables_need_no_me_or_pm_and_serve_the_bed(tmp_path):
    """either table alone, and both, pass the argument rules: what stops the run, if anything, is the device"""
    bed, out, out2 = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "o2.tsv"
    bed.write_text("# nothing\n")
    for extra in (["--me-intervals", out], ["--pm-intervals", out], ["--me-intervals", out, "--pm-intervals", out2]):
        r = run("all", "-i", T1, "--intervals", bed, *extra)
        assert r.returncode in (0, 101) and "Usage:" not in r.stderr, r.stderr
        if r.returncode == 101:
            assert "no CPU fallback" in r.stderr


BAD = [
    ("{c}\t0\t10\n{c}\t5\n", 2, "fewer than 3"),
    ("{c}\t0\t10\n{c}\tten\t20\n", 2, "start 'ten'"),
    ("{c}\t0\t2147483648\n", 1, "end '2147483648'"),
    ("track name=x\n{c}\t0\t10\tn\n{c}\t11\t10\n", 3, "beyond end"),
    ("{c}\t0\t10\nbrowser position x\nchrNope\t0\t10\n", 3, "no reference named 'chrNope'"),
]


@pytest.mark.parametrize("text,line,what", BAD, ids=[b[2].replace(" ", "_").replace("'", "") for b in BAD])
@pytest.mark.parametrize("sub", SUBS + ["all"])
def test_bed_errors_name_the_line_and_create_nothing(tmp_path, contig, sub, text, line, what):
    bed, out, out2, me = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "o2.tsv", tmp_path / "me.tsv"
    bed.write_text(text.format(c=contig))
    if sub == "all":
        r = run("all", "-i", T1, "--me", me, "--intervals", bed, "--me-intervals", out, "--pm-intervals", out2)
    else:
        r = run(sub, "-i", T1, "-o", out, "--intervals", bed)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert "line %d:" % line in r.stderr and what in r.stderr and str(bed) in r.stderr, r.stderr
    assert not out.exists() and not out2.exists() and not me.exists()


def test_missing_bed_or_input(tmp_path):
    out = tmp_path / "o.tsv"
    for sub in SUBS:
        r = run(sub, "-i", T1, "-o", out, "--intervals", tmp_path / "none.bed")
        assert r.returncode == 101 and "none.bed" in r.stderr and not out.exists()
        r = run("all", "-i", T1, TABLE[sub], out, "--intervals", tmp_path / "none.bed")
        assert r.returncode == 101 and "none.bed" in r.stderr and not out.exists()
        r = run(sub, "-i", tmp_path / "missing.bam", "-o", out, "--intervals", tmp_path / "none.bed")
        assert r.returncode == 101 and "Error opening BAM file" in r.stderr and not out.exists()


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("through_all", [False, True], ids=["single", "all"])
def test_an_empty_bed_writes_the_header_alone(tmp_path, sub, through_all):
    """with a device the file is the header; without one the run gets as far as the device (the library's own refusal), the BED is not
    what it reports, and nothing was written"""
    bed, out = tmp_path / "i.bed", tmp_path / "o.tsv"
    bed.write_text("# nothing but comments\ntrack name=none\n\n")
    r = run("all", "-i", T1, "--intervals", bed, TABLE[sub], out) if through_all else run(sub, "-i", T1, "-o", out, "--intervals", bed)
    if r.returncode == 0:
        assert out.read_text() == HEADER[sub]
    else:
        assert r.returncode == 101 and "intervals file" not in r.stderr and "no CPU fallback" in r.stderr, r.stderr
        assert not out.exists()
