"""The --genome FASTA read on the MI355X (mth_tag_set_genome_fasta, k_fasta_pack): the packed genome equals the Python sequences
and what mth_tag_set_genome is given, byte for byte, from plain and from bgzip-compressed files; what cannot be read comes back
as a status and leaves the previous genome set; the command line gives the same files from g.fa.gz, g.fa and g.fa through the
device route.  Every comparison is byte equality."""
import gzip
import os
import struct
import subprocess

import pytest

from metheor_amd import hostapi
from oracle import bamio
from tests import fasta_util as fu
from tests import genome_util as gu
from tests import tag_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
CASES = fu.cases()
MTH_ERR_FORMAT = -10
ALL_NAMES = ["pdr", "lpmd", "lpmd-pairs", "mhl", "me", "pm", "fdrp", "qfdrp"]


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_fasta")
    return {k: fu.build(c, d, k) for k, c in CASES.items()}


def load(eng, path, header):
    """the genome of `header` from the FASTA at path through the library, rows and mapping from the host calls"""
    f = hostapi.Fasta(path)
    try:
        rows = [f.layout(nm, ln) for nm, ln in header]
        m = f.map()
        eng.tag_set_genome_fasta(m["file"], [ln for _, ln in header], rows, blocks=(m["coff"], m["csize"], m["isize"]) if m["compressed"] else None)
    finally:
        f.close()


def fetch_all(eng, want):
    return [eng.tag_genome_fetch(t, 0, len(w)) for t, w in enumerate(want)]


# ---- 1. pack parity through the library ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 777, 64], ids=["default_window", "chunk777", "chunk64"])
@pytest.mark.parametrize("route", ["plain", "bgzf"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_genome_equals_the_sequences_and_set_genome(eng, built, monkeypatch, name, route, chunk):
    c, b = CASES[name], built[name]
    seqs = {x[0]: x[1] for x in c["contigs"]}
    want = [fu.want_bases(seqs[nm], ln) for nm, ln in c["header"]]
    if chunk is None:
        monkeypatch.delenv("METHEOR_FASTA_CHUNK", raising=False)
    else:
        monkeypatch.setenv("METHEOR_FASTA_CHUNK", str(chunk))             # windows that end inside lines and inside contigs
    eng.tag_set_genome([(ln, w) for (_, ln), w in zip(c["header"], want)])
    by_copy = fetch_all(eng, want)
    eng.tag_set_genome([(5, b"NNNNN")])                                   # something else in between
    load(eng, b["gz"] if route == "bgzf" else b["fa"], c["header"])
    packed = fetch_all(eng, want)
    for t, (nm, _) in enumerate(c["header"]):
        assert packed[t] == want[t], (name, route, chunk, nm)
        assert packed[t] == by_copy[t], (name, route, chunk, nm)
        if len(want[t]) > 3:                                              # a slice from inside, and the contig's end is the end
            assert eng.tag_genome_fetch(t, 1, len(want[t]) - 2) == want[t][1:-1]
    import metheor_amd
    with pytest.raises(metheor_amd.MthError):
        eng.tag_genome_fetch(0, 0, len(want[0]) + 1)
    with pytest.raises(metheor_amd.MthError):
        eng.tag_genome_fetch(len(want), 0, 0)


def test_the_packed_genome_serves_the_tag_kernel(eng, tmp_path):
    """the state after the FASTA route is the state after mth_tag_set_genome: the same XM strings from either"""
    g = gu.generate(2)
    recs, xms = gu.runnable(g)
    sam = tmp_path / "in.sam"
    sam.write_text(gu.sam_text([(g["name"], len(g["contig"]))], recs))
    f = hostapi.BamFile(str(sam))
    (raw, off), = f.windows()
    paired = bool(recs[0][2] & 1)
    case = dict(contigs=[("decoy", b"ACGTN" * 41, 50), (g["name"], bytes(g["contig"]), 61)], eol=b"\n", final_newline=True, cuts=[5000, 3], kinds=("dynamic", "fixed"),
                empty_after=(2,))
    b = fu.build(case, tmp_path, "g")
    header = [(g["name"], len(g["contig"]))]
    for path in (b["fa"], b["gz"]):
        eng.tag_set_genome([(5, b"NNNNN")])
        load(eng, path, header)
        assert eng.tag_records(raw, off, is_paired_end=paired) == xms
    f.close()


# ---- 2. refusals: a status, and the previous genome stays ---------------------------------------------------------------------
PREV = [(8, b"ACGTACGT"), (3, b"gat")]


def refused(eng, call):
    import metheor_amd
    eng.tag_set_genome(PREV)
    with pytest.raises(metheor_amd.MthError) as e:
        call()
    assert e.value.status == MTH_ERR_FORMAT, str(e.value)
    assert [eng.tag_genome_fetch(t, 0, len(s)) for t, (_, s) in enumerate(PREV)] == [s for _, s in PREV]       # nothing half-set
    with pytest.raises(metheor_amd.MthError):
        eng.tag_genome_fetch(2, 0, 0)                                     # tag_n_refs kept its value
    return str(e.value)


def two_contigs(tmp_path, spoil_text=None, spoil_rows=None, spoil_blob=None, gz=False):
    import numpy as np
    rng = np.random.default_rng(4)
    contigs = [("c0", rng.choice(np.frombuffer(b"ACGT", np.uint8), size=5003).tobytes(), 60), ("c1", rng.choice(np.frombuffer(b"ACGT", np.uint8), size=7001).tobytes(), 60)]
    text, rows = fu.fasta_text(contigs)
    if spoil_text:
        text = spoil_text(text, rows)
    if spoil_rows:
        rows = spoil_rows(rows)
    p = tmp_path / ("g.fa.gz" if gz else "g.fa")
    blob = fu.bgzf_bytes(text, [3000], ("dynamic",))[0] if gz else text
    if spoil_blob:
        blob = spoil_blob(blob)
    p.write_bytes(blob)
    (tmp_path / (p.name + ".fai")).write_text(fu.fai_text(rows))
    return str(p), [("c0", 5003), ("c1", 7001)]


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "bgzf"])
@pytest.mark.parametrize("chunk", [None, 1000])
def test_line_bases_one_too_large_is_refused(eng, tmp_path, monkeypatch, gz, chunk):
    if chunk:
        monkeypatch.setenv("METHEOR_FASTA_CHUNK", str(chunk))
    path, header = two_contigs(tmp_path, spoil_rows=lambda rows: [rows[0], (rows[1][0], rows[1][1], rows[1][2], 61, 61)], gz=gz)
    msg = refused(eng, lambda: load(eng, path, header))
    assert "c1" in msg and "c0" not in msg, msg                          # the message names the contig


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "bgzf"])
def test_a_blank_inside_a_line_is_refused(eng, tmp_path, gz):
    def spoil(text, rows):
        at = rows[0][2] + 61 * 40 + 17                                    # a base of c0, mid-line
        assert text[at] in b"ACGT"
        return text[:at] + b" " + text[at + 1:]
    path, header = two_contigs(tmp_path, spoil_text=spoil, gz=gz)
    msg = refused(eng, lambda: load(eng, path, header))
    assert "c0" in msg and "c1" not in msg, msg


def test_a_flipped_payload_bit_is_refused(eng, tmp_path):
    def spoil(blob):
        coff, csize, _ = fu.bgzf_table(blob)
        at = int(coff[1]) + int(csize[1]) // 2
        return blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:]
    path, header = two_contigs(tmp_path, spoil_blob=spoil, gz=True)
    with pytest.raises(Exception):
        gzip.decompress(open(path, "rb").read())                          # zlib refuses it too
    refused(eng, lambda: load(eng, path, header))


def test_a_wrong_crc32_is_refused(eng, tmp_path):
    def spoil(blob):
        coff, csize, _ = fu.bgzf_table(blob)
        at = int(coff[2]) + int(csize[2])
        crc = struct.unpack_from("<I", blob, at)[0]
        return blob[:at] + struct.pack("<I", crc ^ 1) + blob[at + 4:]
    path, header = two_contigs(tmp_path, spoil_blob=spoil, gz=True)
    msg = refused(eng, lambda: load(eng, path, header))
    assert "CRC32" in msg


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "bgzf"])
def test_a_row_past_the_end_of_the_stream_is_a_status(eng, tmp_path, gz):
    """the library's own bounds test (the host layout call refuses such a row before: tests/test_fasta_inputs.py)"""
    path, header = two_contigs(tmp_path, gz=gz)
    f = hostapi.Fasta(path)
    rows = [f.layout(nm, ln) for nm, ln in header]
    m = f.map()
    lying = [rows[0], (rows[1].src_off, rows[1].n_bases + 50000, 60, 61, b"c1")]
    blocks = (m["coff"], m["csize"], m["isize"]) if gz else None
    msg = refused(eng, lambda: eng.tag_set_genome_fasta(m["file"], [5003, 57001], lying, blocks=blocks))
    assert "FASTA shorter than its index says" in msg
    far = [rows[0], ((1 << 62), 10, 60, 61, b"c1")]
    refused(eng, lambda: eng.tag_set_genome_fasta(m["file"], [5003, 10], far, blocks=blocks))
    f.close()


# ---- 3. the command line ----------------------------------------------------------------------------------------------------
def run(*args, env=None):
    e = dict(os.environ, METHEOR_SEED="5")
    e.pop("METHEOR_FASTA_CHUNK", None); e.pop("METHEOR_GENOME_DEVICE", None)
    e.update(env or {})
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=600, env=e)


def measure(sub, inp, outdir, tag, extra=(), genome=None, env=None, more=()):
    """one measure run -> (status, stderr, {output name: bytes with the input's path taken out of lpmd's row})"""
    outdir = outdir / tag
    outdir.mkdir(exist_ok=True)
    if sub == "all":
        names = ALL_NAMES
        args = ["all", "-i", inp] + [x for n in names for x in ("--" + n, outdir / (n + ".tsv"))]
    else:
        names = ["out"] + (["pairs"] if sub == "lpmd" else [])
        args = [sub, "-i", inp, "-o", outdir / "out.tsv"] + (["--pairs", outdir / "pairs.tsv"] if sub == "lpmd" else [])
    r = run(*args, *extra, *more, *(["-g", genome] if genome else []), env=env)
    outs = {n: (outdir / (n + ".tsv")).read_bytes().replace(str(inp).encode(), b"<input>") for n in names if (outdir / (n + ".tsv")).exists()}
    return r.returncode, r.stderr, outs


def assert_same(a, b, what):
    assert a[0] == b[0] == 0, (what, a[0], b[0], a[1], b[1])
    assert a[2].keys() == b[2].keys() and a[2], what
    for k in a[2]:
        assert a[2][k] == b[2][k], (what, k, len(a[2][k]), len(b[2][k]))
    return a[2]


def three_routes(sub, inp, tmp_path, fa, gz, extra=(), more=(), env=None):
    """M -g g.fa.gz, M -g g.fa, METHEOR_GENOME_DEVICE=1 M -g g.fa: identical files"""
    host = measure(sub, inp, tmp_path, sub + "_host", extra, genome=fa, more=more, env=env)
    comp = measure(sub, inp, tmp_path, sub + "_gz", extra, genome=gz, more=more, env=env)
    dev = measure(sub, inp, tmp_path, sub + "_dev", extra, genome=fa, more=more, env=dict(env or {}, METHEOR_GENOME_DEVICE="1", METHEOR_TIMING="1"))
    assert "genome FASTA -> device" in dev[1] and "refused" not in dev[1], dev[1]        # the device route ran, and kept its result
    assert_same(comp, host, (sub, "fa.gz against fa"))
    return assert_same(dev, host, (sub, "device route against host route"))


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    """generated records on one contig; the FASTA holds it between two contigs the header does not name, 61 bases a line"""
    d = tmp_path_factory.mktemp("gpu_fasta_cli")
    g = gu.generate(3)
    recs, xms = gu.runnable(g)
    refs = [(g["name"], len(g["contig"]))]
    sam = str(d / "in.sam")
    open(sam, "w").write(gu.sam_text(refs, recs))
    case = dict(contigs=[("decoy1", b"ACGTN" * 41, 61), (g["name"], bytes(g["contig"]), 61), ("decoy2", b"TTGCA" * 33, 61)], eol=b"\n", final_newline=True,
                cuts=[4001, 1, 6000], kinds=("dynamic", "stored", "fixed"), empty_after=(1,))
    b = fu.build(case, d, "g")
    return dict(g, recs=recs, refs=refs, sam=sam, fa=b["fa"], gz=b["gz"], dir=d)


@pytest.mark.parametrize("sub", ["pdr", "all"])
def test_generated_input_three_genome_routes_give_identical_files(gen, tmp_path, sub):
    outs = three_routes(sub, gen["sam"], tmp_path, gen["fa"], gen["gz"])
    assert set(outs) == (set(ALL_NAMES) if sub == "all" else {"out"})               # every table
    assert min(v.count(b"\n") for k, v in outs.items() if k != "lpmd") >= 100, {k: v.count(b"\n") for k, v in outs.items()}


@pytest.fixture(scope="module")
def chr19(golden_dir, tmp_path_factory):
    """the reference's XM-free chr19 fixture with the rebuilt contig, as .fa and .fa.gz"""
    hdr, reads, noxm_text, ln = tag_util.golden(golden_dir)
    contig, _, _, _ = tag_util.rebuild_contig(reads, ln)
    d = tmp_path_factory.mktemp("gpu_fasta_chr19")
    noxm = str(d / "test.chr19.noXM.sam")
    open(noxm, "w").write(noxm_text)
    case = dict(contigs=[("chr19", bytes(contig), 60)], eol=b"\n", final_newline=True, cuts=[65280], kinds=("dynamic",), empty_after=())
    b = fu.build(case, d, "chr19.rebuilt")
    return dict(noxm=noxm, fa=b["fa"], gz=b["gz"])


@pytest.mark.parametrize("sub", ["pdr", "all"])
def test_reference_fixture_three_genome_routes_give_identical_files(chr19, tmp_path, sub):
    outs = three_routes(sub, chr19["noxm"], tmp_path, chr19["fa"], chr19["gz"])
    assert outs["pdr" if sub == "all" else "out"].count(b"\n") == 62                    # the oracle's row count at the defaults


def test_tag_writes_the_same_sam_from_the_compressed_genome(gen, tmp_path):
    outs = {}
    for k, genome, env in (("fa", gen["fa"], None), ("gz", gen["gz"], None), ("dev", gen["fa"], {"METHEOR_GENOME_DEVICE": "1"})):
        r = run("tag", "-i", gen["sam"], "-o", tmp_path / (k + ".sam"), "-g", genome, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "Parsing reference genome...\nDone!\n"
        outs[k] = (tmp_path / (k + ".sam")).read_bytes()
    assert outs["gz"] == outs["fa"] == outs["dev"] and outs["fa"].count(b"XM:Z:") == len(gen["recs"])


def aligned_start(rec):
    r = rec[1]
    for c in rec[4]:
        if (c & 15) in (0, 7, 8) and (c >> 4):
            return r
        if (c & 15) in (2, 3):
            r += c >> 4
    return -1


def test_gpus_region_and_staged_with_the_compressed_genome(gen, tmp_path):
    recs = gen["recs"]
    order = sorted(range(len(recs)), key=lambda k: (aligned_start(recs[k]), k))
    sam = tmp_path / "sorted.sam"
    sam.write_text(gu.sam_text(gen["refs"], [recs[k] for k in order]))
    f = hostapi.BamFile(str(sam))
    bam = str(tmp_path / "in.bam")
    open(bam, "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    bamio.write_bai(bam)
    env = {"METHEOR_SHARD_HALO": "4000"}
    region = "%s:9001-21000" % gen["name"]
    for sub in ("pdr", "me"):
        for what, more, e in (("region", ["--region", region], env), ("gpus 2", ["--gpus", "2"], env), ("staged", [], dict(env, METHEOR_GENOME_STAGED="1"))):
            a = measure(sub, bam, tmp_path, "%s_%s_gz" % (sub, what[:3]), ["-d", "3"], genome=gen["gz"], more=more, env=e)
            b = measure(sub, bam, tmp_path, "%s_%s_fa" % (sub, what[:3]), ["-d", "3"], genome=gen["fa"], more=more, env=e)
            outs = assert_same(a, b, (sub, what))
            assert outs["out"].count(b"\n") >= 50, (sub, what)
    # --gpus 2 through the device route of the plain file: one open, one layout, every shard packs from the shared mapping
    a = measure("pdr", bam, tmp_path, "pdr_gpus_dev", ["-d", "3"], genome=gen["fa"], more=["--gpus", "2"], env=dict(env, METHEOR_GENOME_DEVICE="1"))
    b = measure("pdr", bam, tmp_path, "pdr_gpus_host", ["-d", "3"], genome=gen["fa"], more=["--gpus", "2"], env=env)
    assert_same(a, b, "gpus 2, device route")


# ---- 4. error runs ------------------------------------------------------------------------------------------------------------
SAM2 = "@HD\tVN:1.6\n@SQ\tSN:c0\tLN:8\n@SQ\tSN:other\tLN:8\nr\t0\tc0\t1\t30\t4M\t*\t0\t0\tACGT\t*\n"


def test_unreadable_compressed_genomes_end_with_101_and_no_output(tmp_path):
    p = tmp_path / "two.sam"
    p.write_text(SAM2)
    text, rows = fu.fasta_text([("c0", b"ACGTACGT")])
    plain_gz = tmp_path / "plain.fa.gz"
    plain_gz.write_bytes(gzip.compress(text))
    (tmp_path / "plain.fa.gz.fai").write_text(fu.fai_text(rows))
    no_fai = tmp_path / "nofai.fa.gz"
    no_fai.write_bytes(fu.bgzf_bytes(text, [100])[0])
    lacks = tmp_path / "lacks.fa.gz"                                                    # holds c0, the header also names `other`
    lacks.write_bytes(fu.bgzf_bytes(text, [100])[0])
    (tmp_path / "lacks.fa.gz.fai").write_text(fu.fai_text(rows))
    for sub in ("pdr", "all"):
        out = tmp_path / ("o_%s.tsv" % sub)
        o = ["--pdr", out] if sub == "all" else ["-o", out]
        for genome, texts in ((plain_gz, ("Error opening reference genome file: ", "bgzip")),
                              (no_fai, ("Error opening reference genome file: ", "nofai.fa.gz.fai", "samtools faidx")),
                              (lacks, ("Error fetching reference genome sequence.: sequence not in the FASTA: other",))):
            r = run(sub, "-i", p, *o, "-g", genome)
            assert r.returncode == 101, (sub, genome, r.stderr)
            for t in texts:
                assert t in r.stderr, (sub, genome, r.stderr)
            assert not out.exists() and r.stdout == ""
    # tag: the same texts, after its header went out
    r = run("tag", "-i", p, "-o", tmp_path / "t.sam", "-g", lacks)
    assert r.returncode == 101 and "Error fetching reference genome sequence.: sequence not in the FASTA: other" in r.stderr
    assert r.stdout == "Parsing reference genome...\n"


def test_device_route_falls_back_to_the_host_read_on_a_plain_file(tmp_path):
    g = gu.generate(1, n=800, length=6000)
    recs, _ = gu.runnable(g)
    sam = tmp_path / "in.sam"
    sam.write_text(gu.sam_text([(g["name"], len(g["contig"]))], recs))
    text, rows = fu.fasta_text([(g["name"], bytes(g["contig"]))])
    name, length, off, lb, lw = rows[0]
    dev_env = {"METHEOR_GENOME_DEVICE": "1", "METHEOR_TIMING": "1"}
    # a .fai that disagrees with the text, harmlessly for the host read (it keeps the first n isgraph bytes of a span that is
    # longer than needed): the device route refuses the layout, the fallback gives the host route's bytes
    fa = tmp_path / "wide.fa"
    fa.write_bytes(text + b"\n" * 400)
    (tmp_path / "wide.fa.fai").write_text(fu.fai_text([(name, length, off, lb, lw + 1)]))
    host = measure("pdr", sam, tmp_path, "wide_host", genome=str(fa))
    dev = measure("pdr", sam, tmp_path, "wide_dev", genome=str(fa), env=dev_env)
    outs = assert_same(dev, host, "a harmless lie in the .fai")
    assert outs["out"].count(b"\n") >= 50
    assert "refused" in dev[1] and "host read instead" in dev[1], dev[1]
    # a blank inside a line: today's error from either route, and no output file
    at = off + 61 * 20 + 7
    fa2 = tmp_path / "blank.fa"
    fa2.write_bytes(text[:at] + b" " + text[at + 1:])
    (tmp_path / "blank.fa.fai").write_text(fu.fai_text(rows))
    host = measure("pdr", sam, tmp_path, "blank_host", genome=str(fa2))
    dev = measure("pdr", sam, tmp_path, "blank_dev", genome=str(fa2), env={"METHEOR_GENOME_DEVICE": "1"})
    assert host[0] == dev[0] == 101 and not host[2] and not dev[2]
    line = "Error fetching reference genome sequence.: FASTA shorter than its index says: " + str(fa2)
    assert line in host[1] and line in dev[1], (host[1], dev[1])
    # the same blank in a compressed file ends the run with the fetch error text
    gz = tmp_path / "blank.fa.gz"
    gz.write_bytes(fu.bgzf_bytes(text[:at] + b" " + text[at + 1:], [5000])[0])
    (tmp_path / "blank.fa.gz.fai").write_text(fu.fai_text(rows))
    comp = measure("pdr", sam, tmp_path, "blank_gz", genome=str(gz))
    assert comp[0] == 101 and not comp[2] and "Error fetching reference genome sequence.: " in comp[1] and name in comp[1], comp[1]
