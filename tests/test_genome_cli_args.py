"""`-g, --genome <GENOME>` on the seven measure commands and on `all`: argument parsing only (no device needed)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
COMMANDS = ["pdr", "pm", "me", "fdrp", "qfdrp", "mhl", "lpmd", "all"]


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


@pytest.fixture(scope="module", autouse=True)
def built():
    from metheor_amd import build
    build.build()
    assert os.path.exists(EXE)


@pytest.mark.parametrize("sub", COMMANDS)
def test_help_lists_the_option(sub):
    r = run(sub, "--help")
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("  -g, --genome <GENOME>")]
    assert len(line) == 1, r.stdout
    assert "instead of XM:Z tags" in line[0] and "XM:Z tags in the input are ignored" in line[0]
    # -G stays --gpus where the command has it
    assert sub == "all" or any(l.startswith("  -G, --gpus <GPUS>") for l in r.stdout.splitlines())


def test_a_value_is_required():
    r = run("pdr", "-i", "x", "-o", "y", "-g")
    assert r.returncode == 2
    assert "a value is required for '--genome <GENOME>' but none was supplied" in r.stderr


@pytest.mark.parametrize("sub", COMMANDS)
def test_the_option_is_parsed_before_the_input_is_opened(sub, tmp_path):
    out = ["--pdr", str(tmp_path / "o.tsv")] if sub == "all" else ["-o", str(tmp_path / "o.tsv")]
    r = run(sub, "-i", "tests/no_such.bam", *out, "--genome", "tests/no_such.fa")
    assert r.returncode == 101 and "unexpected argument" not in r.stderr
    assert "file not found" in r.stderr and "no_such.bam" in r.stderr      # bamutil.rs:7-9 comes first, as in `tag`


def test_tag_help_unchanged():
    r = run("tag", "--help")
    assert r.returncode == 0
    assert r.stdout == ("Add bismark XM tag to BAM file\n\nUsage: metheor tag [OPTIONS] --input <INPUT> --output <OUTPUT> --genome <GENOME>\n\n"
                        "Options:\n"
                        "  -i, --input <INPUT>              \n  -o, --output <OUTPUT>            \n  -g, --genome <GENOME>            \n"
                        "  -h, --help                       Print help\n")
