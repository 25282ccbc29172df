"""`metheor all`'s command line (an MI355X extension: any subset of the seven measures from one decode of the input): options,
defaults, usage errors.  Argument parsing happens before any GPU work: runs on CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
T1 = os.path.join(ROOT, "tests", "golden", "test1.bam")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


@pytest.fixture(scope="module", autouse=True)
def built():
    from metheor_amd import build
    build.build()
    assert os.path.exists(EXE)


def test_main_help_lists_all():
    r = run("--help")
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.strip().startswith("all ")]
    assert len(line) == 1 and "(MI355X extension)" in line[0]


def test_all_help_lists_every_option_with_its_default():
    r = run("all", "--help")
    assert r.returncode == 0, r.stderr
    h = r.stdout
    assert "Usage: metheor all [OPTIONS] --input <INPUT>" in h
    for o in ("--pdr <PDR>", "--lpmd <LPMD>", "--lpmd-pairs <LPMD_PAIRS>", "--mhl <MHL>", "--me <ME>", "--pm <PM>", "--fdrp <FDRP>",
              "--qfdrp <QFDRP>", "-c, --cpg-set <CPG_SET>", "-r, --region <REGION>", "-b, --bai <BAI>"):
        assert o in h, o
    # the single commands' names and defaults (lib.rs)
    for o, d in (("-d, --min-depth <MIN_DEPTH>", "10"), ("-p, --min-cpgs <MIN_CPGS>", "4"), ("-q, --min-qual <MIN_QUAL>", "10"),
                 ("-m, --min-distance <MIN_DISTANCE>", "2"), ("-M, --max-distance <MAX_DISTANCE>", "16"),
                 ("-D, --max-depth <MAX_DEPTH>", "40"), ("-l, --min-overlap <MIN_OVERLAP>", "35")):
        line = [l for l in h.splitlines() if o in l]
        assert len(line) == 1 and line[0].endswith("[default: %s]" % d), (o, line)
    assert "--gpus" not in h


def test_no_output_is_a_usage_error():
    r = run("all", "-i", T1)
    assert r.returncode == 2
    assert r.stderr.startswith("error: the following required arguments were not provided:")
    assert "--pdr <PDR>|--lpmd <LPMD>" in r.stderr and "Usage: metheor all" in r.stderr


def test_gpus_is_not_an_option_of_all(tmp_path):
    r = run("all", "-i", T1, "--pdr", str(tmp_path / "p.tsv"), "--gpus", "2")
    assert r.returncode == 2 and "unexpected argument '--gpus' found" in r.stderr
    assert not (tmp_path / "p.tsv").exists()


def test_lpmd_pairs_needs_lpmd(tmp_path):
    """pinned: --lpmd-pairs is lpmd's --pairs table and is refused without --lpmd (clap's `requires`), also next to other outputs"""
    r = run("all", "-i", T1, "--pdr", str(tmp_path / "p.tsv"), "--lpmd-pairs", str(tmp_path / "pp.tsv"))
    assert r.returncode == 2 and "--lpmd <LPMD>" in r.stderr
    assert not (tmp_path / "p.tsv").exists()


def test_bad_values_and_missing_input(tmp_path):
    r = run("all", "-i", T1, "--pdr", str(tmp_path / "p.tsv"), "-q", "300")
    assert r.returncode == 2 and "300 is not in 0..=255" in r.stderr
    r = run("all", "--pdr", str(tmp_path / "p.tsv"))
    assert r.returncode == 2 and "--input <INPUT>" in r.stderr
    r = run("all", "-i", str(tmp_path / "missing.bam"), "--pdr", str(tmp_path / "p.tsv"))
    assert r.returncode == 101 and "Error opening BAM file" in r.stderr


def test_bai_without_region():
    r = run("all", "-i", T1, "--me", "/dev/null", "-b", T1 + ".bai")
    assert r.returncode == 2 and "needs '--region <REGION>'" in r.stderr
