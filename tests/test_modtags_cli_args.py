"""`--mm-tags` and `--mm-threshold <MM_THRESHOLD>` on the seven measure commands and on `all`: argument parsing only (no
device needed)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
COMMANDS = ["pdr", "pm", "me", "fdrp", "qfdrp", "mhl", "lpmd", "all"]


def run(*args, env=None):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, **(env or {})))


def out_args(sub, tmp_path):
    return ["--pdr", str(tmp_path / "o.tsv")] if sub == "all" else ["-o", str(tmp_path / "o.tsv")]


@pytest.fixture(scope="module", autouse=True)
def built():
    from metheor_amd import build
    build.build()
    assert os.path.exists(EXE)


@pytest.mark.parametrize("sub", COMMANDS)
def test_help_lists_the_two_options(sub):
    r = run(sub, "--help")
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    flag = [l for l in lines if l.startswith("      --mm-tags ")]
    thr = [l for l in lines if l.startswith("      --mm-threshold <MM_THRESHOLD>")]
    assert len(flag) == 1 and len(thr) == 1, r.stdout
    assert "<" not in flag[0].split("(MI355X extension)")[0]           # a flag: no value placeholder
    assert "(MI355X extension)" in flag[0] and "MM:Z / ML:B:C" in flag[0] and "XM:Z tags in the input are ignored" in flag[0]
    assert "(MI355X extension)" in thr[0] and "0..=255" in thr[0] and thr[0].endswith("[default: 128]")
    # tests/test_cli_args.py finds an option's line by "--name ": no other line may hold these, nor these lines another option's
    names = [l.split("--")[1].split()[0] for l in lines if l.startswith("  -") or l.startswith("      --")]
    assert "mm-tags" in names and "mm-threshold" in names and "input" in names
    for n in names:
        hits = [l for l in flag + thr if "--" + n + " " in l]
        assert len(hits) == (1 if n in ("mm-tags", "mm-threshold") else 0), (n, hits)
    assert [l for l in lines if "--mm-tags " in l] == flag and [l for l in lines if "--mm-threshold " in l] == thr


def test_tag_has_neither_and_its_help_is_unchanged():
    r = run("tag", "--help")
    assert r.returncode == 0
    assert r.stdout == ("Add bismark XM tag to BAM file\n\nUsage: metheor tag [OPTIONS] --input <INPUT> --output <OUTPUT> --genome <GENOME>\n\n"
                        "Options:\n"
                        "  -i, --input <INPUT>              \n  -o, --output <OUTPUT>            \n  -g, --genome <GENOME>            \n"
                        "  -h, --help                       Print help\n")
    assert "mm-t" not in r.stderr
    r = run("tag", "-i", "x", "-o", "y", "-g", "z", "--mm-tags")
    assert r.returncode == 2 and "unexpected argument '--mm-tags'" in r.stderr


@pytest.mark.parametrize("sub", COMMANDS)
def test_usage_errors_exit_2_before_the_input_is_opened(sub, tmp_path):
    o = out_args(sub, tmp_path)
    r = run(sub, "-i", "tests/no_such.bam", *o, "--mm-threshold", "100")
    assert r.returncode == 2 and "'--mm-threshold <MM_THRESHOLD>' cannot be used without '--mm-tags'" in r.stderr and "no_such.bam" not in r.stderr
    r = run(sub, "-i", "tests/no_such.bam", *o, "--mm-tags", "-g", "tests/no_such.fa")
    assert r.returncode == 2 and "'--mm-tags' cannot be used with '--genome <GENOME>'" in r.stderr and "no_such" not in r.stderr
    assert not (tmp_path / "o.tsv").exists()


def test_the_threshold_is_a_u8_and_the_flag_takes_no_value(tmp_path):
    o = out_args("pdr", tmp_path)
    r = run("pdr", "-i", "x", *o, "--mm-tags", "--mm-threshold", "256")
    assert r.returncode == 2 and "invalid value '256' for '--mm-threshold <MM_THRESHOLD>': 256 is not in 0..=255" in r.stderr
    r = run("pdr", "-i", "x", *o, "--mm-tags", "--mm-threshold")
    assert r.returncode == 2 and "a value is required for '--mm-threshold <MM_THRESHOLD>' but none was supplied" in r.stderr
    r = run("pdr", "-i", "x", *o, "--mm-tags=yes")
    assert r.returncode == 2 and "unexpected value 'yes' for '--mm-tags'" in r.stderr


@pytest.mark.parametrize("sub", COMMANDS)
def test_the_options_are_parsed_before_the_input_is_opened(sub, tmp_path):
    for extra in (["--mm-tags"], ["--mm-tags", "--mm-threshold", "0"], ["--mm-threshold=255", "--mm-tags"]):
        r = run(sub, "-i", "tests/no_such.bam", *out_args(sub, tmp_path), *extra)
        assert r.returncode == 101 and "unexpected argument" not in r.stderr
        assert "file not found" in r.stderr and "no_such.bam" in r.stderr


def test_the_host_decoder_has_no_form_of_it(tmp_path):
    r = run("pdr", "-i", "tests/no_such.bam", *out_args("pdr", tmp_path), "--mm-tags", env={"METHEOR_HOST_DECODE": "1"})
    assert r.returncode == 101 and "--mm-tags needs the device record decode" in r.stderr
