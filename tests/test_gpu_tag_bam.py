"""`metheor tag --output-format bam` on the MI355X: the tagged record stream (mth_tag.hip: k_tag_sizes / k_tag_assemble) and its
BGZF blocks (mth_deflate.hip) through Engine.tag_records_bam and through the CLI.  Every block is inflated with Python's zlib and
its framing checked by hand (tests/bgzf_util.py); what the records must be is built here from the input records and the strings
Engine.tag_records returns for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

from metheor_amd import hostapi
from oracle import pyoracle
from tests import bgzf_util as B
from tests import tag_util
from tests import test_gpu_tag as T        # its record generator and its hand-made BAM record (imported, not edited)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
MAX = B.MAX_BLOCK

# Compressed size against zlib level 1 (the level the project's own staging writer uses) over the same uncompressed blocks, DEFLATE
# payload bytes against payload bytes: measured 1.0048 on the 1000-read fixture (profiles/tag_bam.md), rounded up to the next 0.05.
# The output is a function of the input, so there is no noise in the figure; the rounding leaves room for a change of tie-breaking.
ZLIB1_RATIO_BOUND = 1.05


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chr19(golden_dir, tmp_path_factory):
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    d = tmp_path_factory.mktemp("tag_bam")
    noxm = str(d / "test.chr19.noXM.sam")
    open(noxm, "w").write(noxm_text)
    fa = str(d / "chr19.rebuilt.fa")
    tag_util.write_fasta(fa, "chr19", contig)
    return dict(ln=ln, contig=bytes(contig), noxm=noxm, fa=fa, dir=d, want=open(os.path.join(golden_dir, "test.chr19.XM.sam"), "rb").read())


def run(*args, cwd=ROOT):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=cwd, timeout=600)


def expected_stream(raw, off, xms):
    """record by record: the input record with block_size + 4 + len(xm), then XMZ + xm + NUL"""
    out = []
    for i, xm in enumerate(xms):
        rec = raw[int(off[i]):int(off[i + 1])]
        bs, = struct.unpack_from("<I", rec, 0)
        assert bs == len(rec) - 4
        out.append(struct.pack("<I", bs + 4 + len(xm)) + rec[4:] + b"XMZ" + xm + b"\x00")
    return out


def check_window(eng, raw, off, paired=False):
    """tag_records_bam of one window against tag_records of the same window -> (blocks, the expected records)"""
    xms = eng.tag_records(raw, off, is_paired_end=paired)
    want = expected_stream(raw, off, xms)
    data, stream_bytes, n_blocks = eng.tag_records_bam(raw, off, is_paired_end=paired)
    bl = B.blocks(data, keep_eof=True)
    stream = b"".join(b.raw for b in bl)
    assert stream_bytes == len(stream) == sum(len(r) for r in want) and n_blocks == len(bl)
    assert stream == b"".join(want)
    # no block begins or ends inside a record that fits a block; a longer record starts a block and fills every block but its last
    edges = np.concatenate([[0], np.cumsum([len(r) for r in want])])
    cuts = np.concatenate([[0], np.cumsum([len(b.raw) for b in bl])])
    for c in np.setdiff1d(cuts, edges):
        k = int(np.searchsorted(edges, c)) - 1
        assert edges[k + 1] - edges[k] > MAX and edges[k] in cuts and (c - edges[k]) % MAX == 0
    return bl, want


def window_of(path):
    w = hostapi.BamFile(path).windows()
    assert len(w) == 1
    return w[0]


# ---- the API ---------------------------------------------------------------------------------------------------------------
def test_golden_fixture_records_and_cuts(eng, chr19):
    raw, off = window_of(chr19["noxm"])
    eng.tag_set_genome([(chr19["ln"], chr19["contig"])])
    bl, want = check_window(eng, raw, off)
    assert len(want) == 1000 and len(bl) >= 3
    # greedy cuts: every block but the last is as full as the records allow
    sizes = [len(r) for r in want]
    k = 0
    for b in bl[:-1]:
        n = 0
        while n < len(b.raw):
            n += sizes[k]; k += 1
        assert n == len(b.raw) and n + sizes[k] > MAX
    # compression: against zlib level 1 over the same blocks, against the stored form, and the block forms
    dev = sum(len(b.payload) for b in bl)
    z1 = sum(B.zlib1_size(b.raw) for b in bl)
    print("tag_records_bam, 1000-read fixture: %d payload bytes, zlib level 1 %d, ratio %.4f, stream %d bytes, forms %s"
          % (dev, z1, dev / z1, sum(sizes), [b.btype for b in bl]))
    assert dev <= z1 * ZLIB1_RATIO_BOUND
    assert sum(b.size for b in bl) < sum(sizes)
    assert sum(b.btype == 2 for b in bl) * 2 >= len(bl)
    # the same call again: the same bytes
    first = eng.tag_records_bam(raw, off)
    assert eng.tag_records_bam(raw, off) == first and B.blocks(first[0], keep_eof=True)[0].payload == bl[0].payload


def test_two_windows_give_the_stream_of_one(eng, chr19):
    raw, off = window_of(chr19["noxm"])
    eng.tag_set_genome([(chr19["ln"], chr19["contig"])])
    one = b"".join(b.raw for b in B.blocks(eng.tag_records_bam(raw, off)[0], keep_eof=True))
    k = 437
    cut = int(off[k])
    a, na, _ = eng.tag_records_bam(raw[:cut], off[:k + 1])
    b, nb, _ = eng.tag_records_bam(raw[cut:], off[k:] - off[k])
    ba, bb = B.blocks(a, keep_eof=True), B.blocks(b, keep_eof=True)
    assert b"".join(x.raw for x in ba) + b"".join(x.raw for x in bb) == one and na + nb == len(one)
    assert len(ba[-1].raw) < MAX - 400                      # the first window's last block was closed short, not carried over


@pytest.mark.parametrize("seed,paired", [(1, False), (3, True)])
def test_generated_records(eng, tmp_path, seed, paired):
    rng = np.random.default_rng(seed)
    contigs = [bytes(rng.choice(list(b"ACGT") * 8 + list(b"Nacgt"), size=ln).astype(np.uint8)) for ln in (400, 1500, 37)]
    text, recs = T.random_records(rng, contigs, 1500, paired)
    lines = text.splitlines()
    keep = lines[:4] + [line for line, (tid, pos, flag, cig, seq) in zip(lines[4:], recs)
                        if pyoracle.tag_xm(pos, flag, cig, seq, contigs[tid], is_paired_end=paired) is not None]
    assert len(keep) > 1300
    p = tmp_path / "gen.sam"
    p.write_text("\n".join(keep) + "\n")
    raw, off = window_of(str(p))
    eng.tag_set_genome([(len(c), c) for c in contigs])
    bl, want = check_window(eng, raw, off, paired)
    assert len(want) == len(keep) - 4 and len(bl) >= 2


@pytest.mark.parametrize("line", [
    "r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*",
    "r\t0\tc0\t398\t30\t10M\t*\t0\t0\tACGTACGTAC\t*",
    "r\t16\tc0\t10\t30\t2M1I2M\t*\t0\t0\tAC=GT\t*",
])
def test_panic_records_raise_and_return_nothing(eng, tmp_path, line):
    import metheor_amd
    contig = b"ACGT" * 100
    p = tmp_path / "p.sam"
    p.write_text("@HD\tVN:1.6\n@SQ\tSN:c0\tLN:400\nok\t0\tc0\t5\t30\t8M\t*\t0\t0\tACGTACGT\t*\n" + line + "\n")
    raw, off = window_of(str(p))
    eng.tag_set_genome([(400, contig)])
    got = None
    with pytest.raises(metheor_amd.MthError) as e:
        got = eng.tag_records_bam(raw, off)
    assert got is None and "tag" in str(e.value)
    eng.reset()
    fa = str(tmp_path / "g.fa")
    tag_util.write_fasta(fa, "c0", contig)
    r = run("tag", "-i", str(p), "-o", str(tmp_path / "o.bam"), "-g", fa, "-O", "bam")
    assert r.returncode == 101, (r.returncode, r.stderr)
    left = (tmp_path / "o.bam").read_bytes()                 # what was written is flushed: the header's blocks, readable
    assert b"".join(b.raw for b in B.blocks(left, keep_eof=True))[:4] == b"BAM\x01"


def test_seq_star_records_get_an_empty_field(eng, tmp_path):
    contig = b"ACGTCGCGAACCGGTTACGT" * 20
    p = tmp_path / "s.sam"
    p.write_text("@HD\tVN:1.6\n@SQ\tSN:c0\tLN:400\n"
                 "a\t0\tc0\t10\t30\t20M\t*\t0\t0\tCGCGAACCGGTTACGTACGT\t*\n"
                 "b\t256\tc0\t10\t30\t20M\t*\t0\t0\t*\t*\n"
                 "c\t272\tc0\t30\t30\t5M2D10M1I4M\t*\t0\t0\t*\t*\n")
    raw, off = window_of(str(p))
    eng.tag_set_genome([(400, contig)])
    bl, want = check_window(eng, raw, off)
    assert want[1].endswith(b"XMZ\x00") and want[2].endswith(b"XMZ\x00") and len(want[0]) - (int(off[1]) - int(off[0])) == 24
    assert len(bl) == 1


def test_a_record_longer_than_a_block(eng):
    rng = np.random.default_rng(6)
    contig = bytes(rng.choice(list(b"ACGT"), size=70100).astype(np.uint8))
    seq = bytes(rng.choice(list(b"ACGT"), size=70000).astype(np.uint8))
    small = T._bam_record(0, 10, 0, [(30 << 4)], seq[:30], name=b"small")
    big = T._bam_record(0, 50, 0, [(70000 << 4)], seq, name=b"big")
    raw = small + big + small
    off = np.array([0, len(small), len(small) + len(big), len(raw)], np.uint64)
    eng.tag_set_genome([(70100, contig)])
    bl, want = check_window(eng, raw, off)
    n_big = len(want[1])
    assert n_big == len(big) + 4 + 70000 and n_big > 2 * MAX
    tail = n_big - (n_big // MAX) * MAX
    # the first record alone; the long one starts a block and fills every block but its last, which the next record shares
    assert [len(b.raw) for b in bl] == [len(want[0])] + [MAX] * (n_big // MAX) + [tail + len(want[2])]
    assert b"".join(b.raw for b in bl[1:])[:n_big] == want[1]


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def parse_bam(data):
    """-> header text, [(name, length)], bytes of the header, [records with their block_size field], the blocks"""
    assert data.endswith(B.EOF_BLOCK)
    bl = B.blocks(data)
    s = b"".join(b.raw for b in bl)
    assert s[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<I", s, 4)
    text = s[8:8 + l_text]
    p = 8 + l_text
    n_ref, = struct.unpack_from("<I", s, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", s, p)
        name = s[p + 4:p + 4 + l_name]
        assert name.endswith(b"\x00")
        refs.append((name[:-1].decode(), struct.unpack_from("<I", s, p + 4 + l_name)[0]))
        p += 8 + l_name
    hdr_bytes, recs = p, []
    while p < len(s):
        bs, = struct.unpack_from("<I", s, p)
        recs.append(s[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(s)
    return text, refs, hdr_bytes, recs, bl


@pytest.fixture(scope="module")
def cli_bam(chr19):
    out = chr19["dir"] / "out.tagged.bam"
    r = run("tag", "-i", chr19["noxm"], "-o", str(out), "-g", chr19["fa"], "-O", "bam")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Parsing reference genome...\nDone!\n"
    return str(out), out.read_bytes()


def test_cli_bam_file_layout(chr19, cli_bam):
    path, data = cli_bam
    assert data[-28:] == B.EOF_BLOCK
    text, refs, hdr_bytes, recs, bl = parse_bam(data)
    want_lines = chr19["want"].splitlines(True)
    assert text == b"".join(x for x in want_lines if x.startswith(b"@"))          # the SAM route's header bytes
    assert refs == [("chr19", 58617616)] and len(recs) == 1000
    # the header has blocks of its own: the first record starts a block
    n, k = 0, 0
    while n < hdr_bytes:
        n += len(bl[k].raw); k += 1
    assert n == hdr_bytes and k >= 1 and len(bl) > k
    # every record back to SAM text through the host formatter: the golden file's lines
    f = hostapi.BamFile(chr19["noxm"])
    lines = [f.sam_line(r, 0, len(r)) for r in recs]
    assert lines == [x for x in want_lines if not x.startswith(b"@")]
    assert all(r.endswith(b"\x00") and b"XMZ" in r for r in recs)
    # compression of the record blocks
    rb = bl[k:]
    dev, z1 = sum(len(b.payload) for b in rb), sum(B.zlib1_size(b.raw) for b in rb)
    print("tag -O bam, 1000-read fixture: file %d bytes, record payloads %d, zlib level 1 %d, ratio %.4f" % (len(data), dev, z1, dev / z1))
    assert dev <= z1 * ZLIB1_RATIO_BOUND and sum(b.size for b in rb) < sum(len(b.raw) for b in rb)
    assert sum(b.btype == 2 for b in rb) * 2 >= len(rb)


def test_cli_bam_feeds_the_measures_through_the_device_decode(chr19, cli_bam, tmp_path):
    path, data = cli_bam
    # (lpmd's row names its input as given: both runs read a file called "aln", each in a directory of its own)
    da, db = tmp_path / "tagged", tmp_path / "genome"
    da.mkdir(); db.mkdir()
    (da / "aln").write_bytes(data)
    (db / "aln").write_bytes(open(chr19["noxm"], "rb").read())
    for cmd, extra in (("pdr", ["-d", "1", "-p", "1"]), ("lpmd", [])):
        a, b = tmp_path / (cmd + ".tagged.tsv"), tmp_path / (cmd + ".genome.tsv")
        r = run(cmd, "-i", "aln", "-o", str(a), *extra, cwd=str(da))
        assert r.returncode == 0, r.stderr
        r = run(cmd, "-i", "aln", "-o", str(b), "-g", chr19["fa"], *extra, cwd=str(db))
        assert r.returncode == 0, r.stderr
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > (100 if cmd == "pdr" else 20)
    w = hostapi.BamFile(path).windows()
    assert sum(len(off) - 1 for _, off in w) == 1000


def test_cli_bam_input_sam_route_and_determinism(chr19, cli_bam, tmp_path):
    path, data = cli_bam
    # BAM input gives the same output bytes as SAM input
    f = hostapi.BamFile(chr19["noxm"])
    bam_in = tmp_path / "noxm.bam"
    bam_in.write_bytes(open(f.staged_path(), "rb").read())
    out = tmp_path / "from_bam.bam"
    r = run("tag", "-i", str(bam_in), "-o", str(out), "-g", chr19["fa"], "--output-format", "bam")
    assert r.returncode == 0 and out.read_bytes() == data
    # twice: identical files
    out2 = tmp_path / "again.bam"
    r = run("tag", "-i", chr19["noxm"], "-o", str(out2), "-g", chr19["fa"], "--output-format=bam")
    assert r.returncode == 0 and out2.read_bytes() == data
    # -O sam, and no -O at all (also with a .bam name): the golden SAM bytes
    for k, extra in enumerate((["-O", "sam"], [])):
        o = tmp_path / ("sam_route_%d.bam" % k)
        r = run("tag", "-i", chr19["noxm"], "-o", str(o), "-g", chr19["fa"], *extra)
        assert r.returncode == 0 and r.stdout == "Parsing reference genome...\nDone!\n" and o.read_bytes() == chr19["want"]
