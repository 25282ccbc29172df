"""`lpmd --intervals BED --intervals-output FILE` and `all --lpmd ... --intervals BED --lpmd-intervals FILE` (an MI355X extension:
LPMD per interval, reduced on the device): options, `requires` rules, and the BED's errors.  All of it happens before any device is
needed or any output is created: runs on CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
T1 = os.path.join(ROOT, "tests", "golden", "test1.bam")        # one contig, "chr1"
HEADER = "chrom\tstart\tend\tname\tlpmd\tn_concordant\tn_discordant\n"


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
    h = run("lpmd", "--help")
    assert h.returncode == 0, h.stderr
    for o in ("--intervals <INTERVALS>", "--intervals-output <INTERVALS_OUTPUT>", "-p, --pairs <PAIRS>"):
        assert len([l for l in h.stdout.splitlines() if o in l]) == 1, o
    h = run("all", "--help")
    assert h.returncode == 0, h.stderr
    for o in ("--intervals <INTERVALS>", "--lpmd-intervals <LPMD_INTERVALS>", "--lpmd-pairs <LPMD_PAIRS>"):
        assert len([l for l in h.stdout.splitlines() if o in l]) == 1, o
    for sub in ("pdr", "mhl", "me", "pm", "fdrp", "qfdrp", "tag"):
        assert "--intervals" not in run(sub, "--help").stdout, sub


def test_lpmd_requires_both(tmp_path):
    bed, out, iv = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "iv.tsv"
    bed.write_text("")
    r = run("lpmd", "-i", T1, "-o", out, "--intervals", bed)
    assert r.returncode == 2 and r.stderr.startswith("error: the following required arguments were not provided:")
    assert "--intervals-output <INTERVALS_OUTPUT>" in r.stderr and "Usage: metheor lpmd" in r.stderr
    r = run("lpmd", "-i", T1, "-o", out, "--intervals-output", iv)
    assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr and "Usage: metheor lpmd" in r.stderr
    # before any file is touched: a missing input or BED is not what is reported
    r = run("lpmd", "-i", tmp_path / "missing.bam", "-o", out, "--intervals", tmp_path / "missing.bed")
    assert r.returncode == 2 and "--intervals-output" in r.stderr
    assert not out.exists() and not iv.exists()


def test_all_requires_both_and_lpmd(tmp_path):
    bed, out, iv, pdr = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "iv.tsv", tmp_path / "p.tsv"
    bed.write_text("")
    r = run("all", "-i", T1, "--lpmd", out, "--intervals", bed)
    assert r.returncode == 2 and "--lpmd-intervals <LPMD_INTERVALS>" in r.stderr and "Usage: metheor all" in r.stderr
    r = run("all", "-i", T1, "--lpmd", out, "--lpmd-intervals", iv)
    assert r.returncode == 2 and "--intervals <INTERVALS>" in r.stderr
    r = run("all", "-i", T1, "--pdr", pdr, "--intervals", bed, "--lpmd-intervals", iv)      # the way --lpmd-pairs needs --lpmd
    assert r.returncode == 2 and "--lpmd <LPMD>" in r.stderr
    r = run("all", "-i", T1, "--lpmd", out, "--intervals-output", iv)                        # lpmd's name for it is not all's
    assert r.returncode == 2 and "unexpected argument '--intervals-output' found" in r.stderr
    assert not out.exists() and not iv.exists() and not pdr.exists()


BAD = [
    ("{c}\t0\t10\n{c}\t5\n", 2, "fewer than 3"),
    ("# a comment\n\n{c}\t0\t10\n{c} 3 9\n", 4, "fewer than 3"),                   # blanks are not separators
    ("{c}\t0\t10\n{c}\tten\t20\n", 2, "start 'ten'"),
    ("{c}\t0\t1e3\n", 1, "end '1e3'"),
    ("{c}\t-1\t10\n", 1, "start '-1'"),
    ("{c}\t0\t2147483648\n", 1, "end '2147483648'"),
    ("{c}\t0\t99999999999\n", 1, "end '99999999999'"),
    ("{c}\t\t5\n", 1, "start ''"),
    ("track name=x\n{c}\t0\t10\tn\n{c}\t11\t10\n", 3, "beyond end"),
    ("{c}\t0\t10\nbrowser position x\nchrNope\t0\t10\n", 3, "no reference named 'chrNope'"),
]


@pytest.mark.parametrize("text,line,what", BAD, ids=[b[2].replace(" ", "_").replace("'", "") + "_%d" % k for k, b in enumerate(BAD)])
@pytest.mark.parametrize("sub", ["lpmd", "all"])
def test_bed_errors_name_the_line_and_create_nothing(tmp_path, contig, sub, text, line, what):
    bed, out, iv, pairs = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "iv.tsv", tmp_path / "pairs.tsv"
    bed.write_text(text.format(c=contig))
    if sub == "lpmd":
        r = run("lpmd", "-i", T1, "-o", out, "--pairs", pairs, "--intervals", bed, "--intervals-output", iv)
    else:
        r = run("all", "-i", T1, "--lpmd", out, "--lpmd-pairs", pairs, "--intervals", bed, "--lpmd-intervals", iv)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert "line %d:" % line in r.stderr and what in r.stderr and str(bed) in r.stderr, r.stderr
    assert not out.exists() and not iv.exists() and not pairs.exists()


def test_missing_bed_or_input(tmp_path):
    out, iv = tmp_path / "o.tsv", tmp_path / "iv.tsv"
    r = run("lpmd", "-i", T1, "-o", out, "--intervals", tmp_path / "none.bed", "--intervals-output", iv)
    assert r.returncode == 101 and "none.bed" in r.stderr and not out.exists() and not iv.exists()
    r = run("lpmd", "-i", tmp_path / "missing.bam", "-o", out, "--intervals", tmp_path / "none.bed", "--intervals-output", iv)
    assert r.returncode == 101 and "Error opening BAM file" in r.stderr


def _accepted(r, iv, want_rows):
    """a BED that is read without complaint: with a device the run ends well and the table is as expected; without one the run gets as
    far as the device (the library's own refusal), the BED itself is not what it reports, and nothing was written"""
    if r.returncode == 0:
        assert iv.read_text().splitlines(True)[:1] == [HEADER] and [l.split("\t")[:4] for l in iv.read_text().splitlines()[1:]] == want_rows
    else:
        assert r.returncode == 101 and "intervals file" not in r.stderr and "no CPU fallback" in r.stderr, r.stderr
        assert not iv.exists()


def test_an_empty_bed_is_accepted(tmp_path):
    bed, out, iv = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "iv.tsv"
    bed.write_text("")
    _accepted(run("lpmd", "-i", T1, "-o", out, "--intervals", bed, "--intervals-output", iv), iv, [])
    bed.write_text("# nothing but comments\ntrack name=none\n\nbrowser hide all\n")
    _accepted(run("lpmd", "-i", T1, "-o", out, "--intervals", bed, "--intervals-output", iv), iv, [])


def test_comment_track_and_empty_lines_are_skipped(tmp_path, contig):
    """also: a name column, further columns ignored, no name -> '.', a zero-length interval, the largest end, a last line without a newline"""
    bed, out, iv = tmp_path / "i.bed", tmp_path / "o.tsv", tmp_path / "iv.tsv"
    bed.write_text("#c\ntrack name=t\n{c}\t0\t8\tfirst\t0\t+\n\nbrowser position\n{c}\t3\t3\n{c}\t0\t2147483647\tall\r\n{c}\t2\t6".format(c=contig))
    want = [[contig, "0", "8", "first"], [contig, "3", "3", "."], [contig, "0", "2147483647", "all"], [contig, "2", "6", "."]]
    _accepted(run("lpmd", "-i", T1, "-o", out, "--intervals", bed, "--intervals-output", iv), iv, want)
