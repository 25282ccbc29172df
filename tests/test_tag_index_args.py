"""`metheor tag -O bam --write-index`: what of its contract ends before the first kernel, so it runs without a device -- the flag's
parsing and help, and the early failures of `tag`, which keep their order and messages with the flag present."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
SAM = os.path.join(ROOT, "tests", "golden", "test.chr19.XM.sam")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


@pytest.fixture(scope="module", autouse=True)
def built():
    from metheor_amd import build
    build.build()
    assert os.path.exists(EXE)


@pytest.mark.parametrize("fmt", [(), ("-O", "sam"), ("--output-format=sam",)])
def test_write_index_needs_bam_output(tmp_path, fmt):
    out = tmp_path / "o.bam"
    (tmp_path / "o.bam.bai").write_bytes(b"someone else's")
    r = run("tag", "-i", SAM, "-o", str(out), "-g", "tests/no_such.fa", "--write-index", *fmt)
    assert r.returncode == 2
    assert r.stderr.startswith("error: ") and "--write-index" in r.stderr and "Usage: metheor tag" in r.stderr and "For more information, try '--help'." in r.stderr
    assert not out.exists()                                     # nothing is opened or created ...
    assert (tmp_path / "o.bam.bai").read_bytes() == b"someone else's"         # ... or removed


def test_the_flag_takes_no_value(tmp_path):
    r = run("tag", "-i", SAM, "-o", str(tmp_path / "o.bam"), "-g", "tests/no_such.fa", "-O", "bam", "--write-index=yes")
    assert r.returncode == 2 and "unexpected value 'yes'" in r.stderr and not (tmp_path / "o.bam").exists()
    # a token behind it is the next argument, not its value
    r = run("tag", "-i", SAM, "-o", str(tmp_path / "o.bam"), "-g", "tests/no_such.fa", "--write-index", "-O", "bam")
    assert r.returncode == 101 and "no_such.fa" in r.stderr
    r = run("tag", "-i", SAM, "-o", str(tmp_path / "o.bam"), "-g", "tests/no_such.fa", "-O", "bam", "--write-index", "stray")
    assert r.returncode == 2 and "unexpected argument 'stray'" in r.stderr
    # the other commands do not know it
    r = run("pdr", "-i", SAM, "-o", str(tmp_path / "o.tsv"), "--write-index")
    assert r.returncode == 2 and "unexpected argument '--write-index'" in r.stderr


def test_help_lists_the_flag_on_stderr():
    r = run("tag", "--help")
    assert r.returncode == 0
    assert "--write-index" not in r.stdout and "--output-format" not in r.stdout
    assert r.stdout == ("Add bismark XM tag to BAM file\n\nUsage: metheor tag [OPTIONS] --input <INPUT> --output <OUTPUT> --genome <GENOME>\n\nOptions:\n"
                        "  -i, --input <INPUT>              \n  -o, --output <OUTPUT>            \n  -g, --genome <GENOME>            \n"
                        "  -h, --help                       Print help\n")
    err = r.stderr.splitlines()
    assert len([x for x in err if "--output-format" in x]) == 1
    line = [x for x in err if "--write-index" in x]
    assert len(line) == 1 and "(MI355X extension)" in line[0] and "with -O bam" in line[0] and ".bai" in line[0]
    assert err.index(line[0]) == [i for i, x in enumerate(err) if "--output-format" in x][0] + 1 and "Extension:" in err


def test_early_failures_keep_their_order_with_the_flag(tmp_path):
    fmt = ("-O", "bam", "--write-index")
    r = run("tag", "-i", "tests/no_such_input.bam", "-o", "no_such_dir/out.bam", "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "file not found" in r.stderr and "no_such_input.bam" in r.stderr
    r = run("tag", "-i", SAM, "-o", "no_such_dir/out.bam", "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "No such directory for output alignment file: no_such_dir" in r.stderr and "no_such.fa" not in r.stderr
    out = tmp_path / "out.bam"
    (tmp_path / "out.bam.bai").write_bytes(b"stale")
    r = run("tag", "-i", SAM, "-o", str(out), "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "file not found" in r.stderr and "no_such.fa" in r.stderr and r.stdout == ""
    # the output holds the BAM header, as without the flag, and the run that failed leaves no index of some other file behind
    same = tmp_path / "plain.bam"
    r = run("tag", "-i", SAM, "-o", str(same), "-g", "tests/no_such.fa", "-O", "bam")
    assert r.returncode == 101 and out.read_bytes() == same.read_bytes() and len(out.read_bytes()) > 28
    assert not (tmp_path / "out.bam.bai").exists()
