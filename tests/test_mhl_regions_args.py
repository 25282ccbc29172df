"""`metheor mhl-regions -i IN --intervals BED -o OUT` and `all --intervals BED --mhl-intervals OUT` (an MI355X extension: MHL per
interval, counted on the device): options, `requires` rules, the BED's errors.  All of it happens before any device is needed or any
output is created: runs on CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
T1 = os.path.join(ROOT, "tests", "golden", "test1.bam")        # one contig, "chr1"
HEADER = "chrom\tstart\tend\tname\tmhl\tn_reads\tmax_cpgs\n"


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


def test_help_lists_the_options():
    h = run("mhl-regions", "--help")
    assert h.returncode == 0, h.stderr
    assert "Usage: metheor mhl-regions [OPTIONS] --input <INPUT> --output <OUTPUT> --intervals <INTERVALS>" in h.stdout
    for o, d in (("-d, --min-depth <MIN_DEPTH>", "10"), ("-p, --min-cpgs <MIN_CPGS>", "4"), ("-q, --min-qual <MIN_QUAL>", "10"), ("-G, --gpus <GPUS>", "1")):
        line = [l for l in h.stdout.splitlines() if o in l]
        assert len(line) == 1 and line[0].endswith("[default: %s]" % d), (o, line)
    options = h.stdout[h.stdout.index("Options:"):].splitlines()          # (the usage line names the required ones too)
    for o in ("--intervals <INTERVALS>", "-c, --cpg-set <CPG_SET>", "-g, --genome <GENOME>", "--mm-tags ", "--mm-threshold <MM_THRESHOLD>", "-o, --output <OUTPUT>"):
        assert len([l for l in options if o in l]) == 1, o
    assert "--region" not in h.stdout and "--bai" not in h.stdout
    h = run("all", "--help")
    assert h.returncode == 0, h.stderr
    for o in ("--mhl-intervals <MHL_INTERVALS>", "--intervals <INTERVALS>", "--lpmd-intervals <LPMD_INTERVALS>", "--mhl <MHL>"):
        assert len([l for l in h.stdout.splitlines() if o in l]) == 1, o
    line = [l for l in run("--help").stdout.splitlines() if l.strip().startswith("mhl-regions ")]
    assert len(line) == 1 and "(MI355X extension)" in line[0]
    assert "--intervals" not in run("mhl", "--help").stdout


def test_required_arguments(tmp_path):
    bed, out = tmp_path / "i.bed", tmp_path / "o.tsv"
    bed.write_text("")
    r = run("mhl-regions", "-i", T1, "-o", out)
    assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr and "Usage: metheor mhl-regions" in r.stderr
    r = run("mhl-regions", "-i", T1, "--intervals", bed)
    assert r.returncode == 2 and "--output <OUTPUT>" in r.stderr
    assert not out.exists()


def test_region_is_refused(tmp_path):
    bed, out, lp = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "l.tsv"
    bed.write_text("")
    r = run("mhl-regions", "-i", T1, "-o", out, "--intervals", bed, "--region", "chr1")
    assert r.returncode == 2 and "unexpected argument '--region' found" in r.stderr
    r = run("all", "-i", T1, "--intervals", bed, "--mhl-intervals", out, "--region", "chr1")
    assert r.returncode == 2 and "'--mhl-intervals <MHL_INTERVALS>' cannot be used with '--region <REGION>'" in r.stderr and "Usage: metheor all" in r.stderr
    r = run("all", "-i", T1, "--lpmd", lp, "--intervals", bed, "--lpmd-intervals", tmp_path / "li.tsv", "--mhl-intervals", out, "--region", "chr1")
    assert r.returncode == 2 and "--mhl-intervals" in r.stderr
    assert not out.exists() and not lp.exists()


def test_all_requires(tmp_path):
    bed, out, lp, li, pdr = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "l.tsv", tmp_path / "li.tsv", tmp_path / "p.tsv"
    bed.write_text("")
    r = run("all", "-i", T1, "--mhl-intervals", out)                               # the table needs the BED
    assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr and "Usage: metheor all" in r.stderr
    r = run("all", "-i", T1, "--pdr", pdr, "--intervals", bed)                      # the BED needs one of its tables
    assert r.returncode == 2 and "--lpmd-intervals <LPMD_INTERVALS>" in r.stderr and "--mhl-intervals <MHL_INTERVALS>" in r.stderr
    r = run("all", "-i", T1, "--lpmd", lp, "--intervals", bed)                      # (pinned by the per-interval LPMD tests too)
    assert r.returncode == 2 and "--lpmd-intervals <LPMD_INTERVALS>" in r.stderr
    r = run("all", "-i", T1, "--pdr", pdr, "--intervals", bed, "--lpmd-intervals", li)
    assert r.returncode == 2 and "--lpmd <LPMD>" in r.stderr
    r = run("all", "-i", T1, "--mhl-intervals", out, "--intervals", bed, "--lpmd-intervals", li)     # ... also beside the MHL table
    assert r.returncode == 2 and "--lpmd <LPMD>" in r.stderr
    r = run("all", "-i", T1)                                                        # the MHL table is an output of its own
    assert r.returncode == 2 and "--mhl-intervals <MHL_INTERVALS>" in r.stderr and "--pdr <PDR>|--lpmd <LPMD>" in r.stderr
    assert not any(p.exists() for p in (out, lp, li, pdr))


BAD = [
    ("{c}\t0\t10\n{c}\t5\n", 2, "fewer than 3"),
    ("{c}\t0\t10\n{c}\tten\t20\n", 2, "start 'ten'"),
    ("{c}\t0\t2147483648\n", 1, "end '2147483648'"),
    ("track name=x\n{c}\t0\t10\tn\n{c}\t11\t10\n", 3, "beyond end"),
    ("{c}\t0\t10\nbrowser position x\nchrNope\t0\t10\n", 3, "no reference named 'chrNope'"),
]


@pytest.mark.parametrize("text,line,what", BAD, ids=[b[2].replace(" ", "_").replace("'", "") for b in BAD])
@pytest.mark.parametrize("sub", ["mhl-regions", "all"])
def test_bed_errors_name_the_line_and_create_nothing(tmp_path, contig, sub, text, line, what):
    bed, out, mhl = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "m.tsv"
    bed.write_text(text.format(c=contig))
    if sub == "all":
        r = run("all", "-i", T1, "--mhl", mhl, "--intervals", bed, "--mhl-intervals", out)
    else:
        r = run("mhl-regions", "-i", T1, "-o", out, "--intervals", bed)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert "line %d:" % line in r.stderr and what in r.stderr and str(bed) in r.stderr, r.stderr
    assert not out.exists() and not mhl.exists()


def test_missing_bed_or_input(tmp_path):
    out = tmp_path / "o.tsv"
    r = run("mhl-regions", "-i", T1, "-o", out, "--intervals", tmp_path / "none.bed")
    assert r.returncode == 101 and "none.bed" in r.stderr and not out.exists()
    r = run("mhl-regions", "-i", tmp_path / "missing.bam", "-o", out, "--intervals", tmp_path / "none.bed")
    assert r.returncode == 101 and "Error opening BAM file" in r.stderr


@pytest.mark.parametrize("sub", ["mhl-regions", "all"])
def test_an_empty_bed_writes_the_header_alone(tmp_path, sub):
    """with a device the file is the header; without one the run gets as far as the device (the library's own refusal), the BED is not
    what it reports, and nothing was written"""
    bed, out = tmp_path / "i.bed", tmp_path / "o.tsv"
    bed.write_text("# nothing but comments\ntrack name=none\n\n")
    r = run("mhl-regions", "-i", T1, "-o", out, "--intervals", bed) if sub == "mhl-regions" else run("all", "-i", T1, "--intervals", bed, "--mhl-intervals", out)
    if r.returncode == 0:
        assert out.read_text() == HEADER
    else:
        assert r.returncode == 101 and "intervals file" not in r.stderr and "no CPU fallback" in r.stderr, r.stderr
        assert not out.exists()
