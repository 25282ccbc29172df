"""`metheor tag -O bam --write-index` end to end: the index written beside the BAM equals the model's index of that BAM
(tests/bai_util.py), the BAM's bytes do not depend on the flag, several decode windows give the index of one, `--region` runs
find and use the index, and unsorted input leaves a complete BAM and no index."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio
from oracle import pyoracle
from tests import bai_util as U
from tests import tag_util
from tests import test_gpu_tag as T        # its record generator (imported, not edited)
from tests import test_gpu_tag_bam as TB   # its BAM parser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")


def run(*args, env=None):
    return subprocess.run([EXE, *args], capture_output=True, text=True, cwd=ROOT, timeout=600, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def chr19(golden_dir, tmp_path_factory):
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    d = tmp_path_factory.mktemp("tag_index")
    noxm = str(d / "test.chr19.noXM.sam")
    open(noxm, "w").write(noxm_text)
    fa = str(d / "chr19.rebuilt.fa")
    tag_util.write_fasta(fa, "chr19", contig)
    return dict(noxm=noxm, noxm_text=noxm_text, fa=fa, dir=d)


@pytest.fixture(scope="module")
def indexed(chr19):
    """the 1000-read fixture tagged with and without the flag; a stale index was lying where the new one goes"""
    out, plain = chr19["dir"] / "out.bam", chr19["dir"] / "plain.bam"
    (chr19["dir"] / "out.bam.bai").write_bytes(b"the index of some other file")
    r = run("tag", "-i", chr19["noxm"], "-o", str(out), "-g", chr19["fa"], "-O", "bam", "--write-index")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Parsing reference genome...\nDone!\n"
    r = run("tag", "-i", chr19["noxm"], "-o", str(plain), "-g", chr19["fa"], "-O", "bam")
    assert r.returncode == 0, r.stderr
    return str(out), str(plain)


def test_fixture_index_equals_the_model(chr19, indexed):
    out, plain = indexed
    assert open(out, "rb").read() == open(plain, "rb").read()                 # the flag does not change the BAM
    assert not os.path.exists(plain + ".bai")
    got = open(out + ".bai", "rb").read()                                     # the stale file is replaced
    assert got == U.bai_bytes(out)
    refs = bamio.read_bai(out + ".bai")
    assert len(refs) == 1 and len(refs[0]["ioffset"]) >= 3 and len(refs[0]["bins"]) >= 3       # three 16-kbp windows hold reads
    assert sorted(os.listdir(chr19["dir"])).count("out.bam.bai") == 1 and not [x for x in os.listdir(chr19["dir"]) if ".tmp." in x]


@pytest.mark.parametrize("cmd,extra", [("pdr", ["-d", "1", "-p", "1"]), ("mhl", ["-d", "1", "-p", "1"])])
def test_region_runs_use_the_index(chr19, indexed, tmp_path, cmd, extra):
    out, _ = indexed
    other = str(tmp_path / "other.bai")
    bamio.write_bai(out, other)
    a, b = tmp_path / "own.tsv", tmp_path / "other.tsv"
    r = run(cmd, "-i", out, "-o", str(a), "-r", "chr19:58420000-58430000", *extra)            # finds out.bam.bai by itself
    assert r.returncode == 0, r.stderr
    r = run(cmd, "-i", out, "-o", str(b), "-r", "chr19:58420000-58430000", "-b", other, *extra)
    assert r.returncode == 0, r.stderr
    print("%s --region: %d bytes" % (cmd, len(a.read_bytes())))
    assert a.read_bytes() == b.read_bytes()


def test_several_decode_windows_give_the_index_of_one(tmp_path):
    """24 000 generated records over two contigs, positions sorted: the generator's records are about 90 bytes each, so this many
    make more than 2 MB of inflated input and at least three windows of METHEOR_DECODE_WINDOW_MB=1"""
    rng = np.random.default_rng(5)
    contigs = [bytes(rng.choice(list(b"ACGT") * 8 + list(b"Nacgt"), size=ln).astype(np.uint8)) for ln in (60_000, 45_000)]
    text, recs = T.random_records(rng, contigs, 24_000, False)
    lines = text.splitlines()
    body = [(tid, pos, line) for line, (tid, pos, flag, cig, seq) in zip(lines[3:], recs)
            if pyoracle.tag_xm(pos, flag, cig, seq, contigs[tid], is_paired_end=False) is not None]
    body.sort(key=lambda x: (x[0], x[1]))
    assert len(body) > 22_000
    sam, fa = tmp_path / "gen.sam", tmp_path / "gen.fa"
    sam.write_text("\n".join(["@HD\tVN:1.6\tSO:coordinate"] + lines[1:3] + [x[2] for x in body]) + "\n")
    with open(fa, "w") as fh:
        for t, c in enumerate(contigs):
            fh.write(">c%d\n" % t)
            for o in range(0, len(c), 60):
                fh.write(c[o:o + 60].decode() + "\n")
    one, many = tmp_path / "one.bam", tmp_path / "many.bam"
    r = run("tag", "-i", str(sam), "-o", str(one), "-g", str(fa), "-O", "bam", "--write-index")
    assert r.returncode == 0, r.stderr
    r = run("tag", "-i", str(sam), "-o", str(many), "-g", str(fa), "-O", "bam", "--write-index", env=dict(METHEOR_DECODE_WINDOW_MB="1", METHEOR_TIMING="1"))
    assert r.returncode == 0, r.stderr
    launches = [int(x.split(" in ")[1].split()[0]) for x in r.stderr.splitlines() if "tag/k_bai_keys" in x]
    assert launches and launches[0] >= 3, r.stderr
    assert open(str(many) + ".bai", "rb").read() == U.bai_bytes(str(many))
    assert open(str(one) + ".bai", "rb").read() == U.bai_bytes(str(one))
    # The writer closes a window's last block short (mth_tag_records_bam), so the two files hold the same records in different
    # blocks and their virtual offsets differ.  Everything else of the two indexes is the same: bins, chunks per bin, windows.
    a, b = TB.parse_bam(one.read_bytes()), TB.parse_bam(many.read_bytes())
    assert a[3] == b[3] and len(a[4]) < len(b[4])
    ra, rb = bamio.read_bai(str(one) + ".bai"), bamio.read_bai(str(many) + ".bai")
    assert len(ra) == len(rb) == 2 and all(len(r["bins"]) >= 3 for r in rb)
    for x, y in zip(ra, rb):
        assert {k: len(v) for k, v in x["bins"].items()} == {k: len(v) for k, v in y["bins"].items()}
        assert len(x["ioffset"]) == len(y["ioffset"])
    tail = lambda p: open(p, "rb").read()[-8:]
    assert tail(str(one) + ".bai") == tail(str(many) + ".bai")


def test_unsorted_input_leaves_a_complete_bam_and_no_index(chr19, tmp_path):
    lines = chr19["noxm_text"].splitlines()
    head = [x for x in lines if x.startswith("@")]
    body = [x for x in lines if not x.startswith("@")]
    pos = [int(x.split("\t")[3]) for x in body]
    k = next(i for i in range(len(body) - 1) if pos[i] < pos[i + 1])
    body[k], body[k + 1] = body[k + 1], body[k]                               # record k + 1 now comes before its predecessor
    sam = tmp_path / "swapped.sam"
    sam.write_text("\n".join(head + body) + "\n")
    out, plain = tmp_path / "out.bam", tmp_path / "plain.bam"
    for planted in (False, True):
        if planted:
            (tmp_path / "out.bam.bai").write_bytes(b"stale")
        r = run("tag", "-i", str(sam), "-o", str(out), "-g", chr19["fa"], "-O", "bam", "--write-index")
        assert r.returncode == 101, r.stderr
        msg = [x for x in r.stderr.splitlines() if "record %d " % (k + 1) in x]
        assert len(msg) == 1 and "not coordinate-sorted" in msg[0] and "no index" in msg[0], r.stderr
        assert not (tmp_path / "out.bam.bai").exists()
    r = run("tag", "-i", str(sam), "-o", str(plain), "-g", chr19["fa"], "-O", "bam")
    assert r.returncode == 0, r.stderr
    got, want = TB.parse_bam(out.read_bytes()), TB.parse_bam(plain.read_bytes())
    assert got[3] == want[3] and len(got[3]) == 1000 and got[:2] == want[:2]
    assert out.read_bytes() == plain.read_bytes()
