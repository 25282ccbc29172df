"""`metheor tag --output-format`: the parts of its contract that end before the first kernel, so they run without a device -- the
option's parsing and help, and the three early failures of `tag` (tests/tag-cli.rs), which keep their order and messages under
`-O bam`; the file a missing FASTA leaves behind then holds the BAM header in BGZF blocks instead of the SAM header text."""
import os
import struct
import subprocess
import zlib

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


def bgzf_blocks(data):
    """[(inflated bytes, BTYPE of the first DEFLATE block)] of a BGZF stream, every field of the framing checked by hand"""
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04", "gzip magic / FEXTRA at %d" % p
        assert struct.unpack_from("<H", data, p + 10)[0] == 6 and data[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, p + 16)[0]
        assert p + bsize + 1 <= len(data)
        payload = data[p + 18:p + bsize + 1 - 8]
        d = zlib.decompressobj(-15)
        raw = d.decompress(payload)
        assert d.eof and not d.unused_data
        crc, isize = struct.unpack_from("<II", data, p + bsize + 1 - 8)
        assert isize == len(raw) <= 0xff00 and crc == zlib.crc32(raw)
        out.append((raw, (payload[0] >> 1) & 3))
        p += bsize + 1
    return out


def test_invalid_output_format_is_a_usage_error(tmp_path):
    for flag in ("-O", "--output-format"):
        r = run("tag", "-i", SAM, "-o", str(tmp_path / "o.bam"), "-g", "tests/hg38.chr19.fa", flag, "cram")
        assert r.returncode == 2
        assert "invalid value 'cram'" in r.stderr and "--output-format <OUTPUT_FORMAT>" in r.stderr and "Usage: metheor tag" in r.stderr
        assert not (tmp_path / "o.bam").exists()
    r = run("tag", "-i", SAM, "-o", str(tmp_path / "o.bam"), "-g", "tests/hg38.chr19.fa", "-O")
    assert r.returncode == 2 and "a value is required" in r.stderr


def test_help_names_the_option():
    """`tag --help` lists the option.  Its stdout stays the reference's text to the byte (tests/test_genome_cli_args.py pins all of
    it), so the extension is listed on stderr, after the help."""
    r = run("tag", "--help")
    assert r.returncode == 0
    assert "--output-format" not in r.stdout and "--genome" in r.stdout and "Add bismark XM tag" in r.stdout
    line = [x for x in r.stderr.splitlines() if "--output-format" in x]
    assert len(line) == 1 and "-O," in line[0] and "(MI355X extension)" in line[0] and "[default: sam]" in line[0]


@pytest.mark.parametrize("fmt", [("-O", "bam"), ("--output-format=bam",), ("-O", "sam"), ()])
def test_early_failures_keep_their_order(tmp_path, fmt):
    # 1. the input is opened first (tag-cli.rs:7-23) -- before the output directory is looked at
    r = run("tag", "-i", "tests/no_such_input.bam", "-o", "no_such_dir/out.bam", "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "file not found" in r.stderr and "no_such_input.bam" in r.stderr
    # 2. then the output directory (tag-cli.rs:24-40) -- before the FASTA
    r = run("tag", "-i", SAM, "-o", "no_such_dir/out.bam", "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "No such directory for output alignment file: no_such_dir" in r.stderr
    assert "no_such.fa" not in r.stderr
    # 3. then the FASTA (tag-cli.rs:41-58), with the output created and its header written
    out = tmp_path / "out.bam"
    r = run("tag", "-i", SAM, "-o", str(out), "-g", "tests/no_such.fa", *fmt)
    assert r.returncode == 101 and "file not found" in r.stderr and "no_such.fa" in r.stderr
    assert r.stdout == ""                                   # neither progress line yet
    data = out.read_bytes()
    text = b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr19\tLN:58617616\n"
    if "bam" not in "".join(fmt):
        assert data.startswith(text)
        return
    blocks = bgzf_blocks(data)                              # a valid BGZF stream ...
    hdr = b"".join(b for b, _ in blocks)                   # ... that holds the BAM header and nothing else
    assert hdr[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<I", hdr, 4)
    sam_hdr = b"".join(x for x in open(SAM, "rb").read().splitlines(True) if x.startswith(b"@"))
    assert hdr[8:8 + l_text] == sam_hdr and sam_hdr.startswith(text)
    p = 8 + l_text
    n_ref, l_name = struct.unpack_from("<II", hdr, p)
    assert n_ref == 1 and hdr[p + 8:p + 8 + l_name] == b"chr19\x00"
    assert struct.unpack_from("<I", hdr, p + 8 + l_name)[0] == 58617616 and len(hdr) == p + 12 + l_name
