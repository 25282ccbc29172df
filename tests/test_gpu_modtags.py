"""`--mm-tags` on the MI355X: `metheor M --mm-tags -i F` == `metheor M -i F'`, byte for byte, where F' is F with every flag
reduced to flag & 0x10 and XM:Z:X(record, T) in place of any XM:Z field (tests/modtags_util.py writes it from the rule's
text) -- the library entry (mth_decode_set_modtags) in both of its forms, its errors and notes, the command line, and a
record longer than a BGZF block through the straddle route."""
import os
import struct
import subprocess

import numpy as np
import pytest

from metheor_amd import hostapi
from oracle import bamio
from tests import modtags_util as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
KEYS = ("tid", "start", "end", "mapq", "fwd", "cpg_off", "cpg_pos", "cpg_rel")
SINGLE = ["pdr", "mhl", "me", "pm", "fdrp", "qfdrp", "lpmd"]
LOW = {"pdr": ["-d", "1", "-p", "1"], "mhl": ["-d", "1", "-p", "1"], "me": ["-d", "1"], "pm": ["-d", "1"], "fdrp": ["-d", "1"],
       "qfdrp": ["-d", "1"], "lpmd": ["-m", "1", "-M", "30"]}
THRESHOLD = {1: 128, 2: 0, 3: 255, 4: 128}
ERR_INVALID, ERR_CAPACITY, ERR_STATE, ERR_FORMAT = -1, -8, -9, -10
FORMS = [False, True]
FORM_IDS = ["direct", "staged"]


def run(*args, env=None):
    e = dict(os.environ, METHEOR_SEED="5")
    e.update(env or {})
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=600, env=e)


def measure(sub, inp, outdir, tag, extra=(), env=None, more=()):
    """one measure run -> (status, stderr, {output name: bytes with the input's path taken out of lpmd's row})"""
    outdir = outdir / tag
    outdir.mkdir(exist_ok=True)
    if sub == "all":
        names = ["pdr", "lpmd", "lpmd-pairs", "mhl", "me", "pm", "fdrp", "qfdrp"]
        args = ["all", "-i", inp] + [x for n in names for x in ("--" + n, outdir / (n + ".tsv"))]
    else:
        names = ["out"] + (["pairs"] if sub == "lpmd" else [])
        args = [sub, "-i", inp, "-o", outdir / "out.tsv"] + (["--pairs", outdir / "pairs.tsv"] if sub == "lpmd" else [])
    r = run(*args, *extra, *more, env=env)
    outs = {n: (outdir / (n + ".tsv")).read_bytes().replace(str(inp).encode(), b"<input>") for n in names if (outdir / (n + ".tsv")).exists()}
    return r.returncode, r.stderr, outs


def mm(T):
    return ["--mm-tags"] + ([] if T == 128 else ["--mm-threshold", str(T)])


def assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0], a[1], b[1])
    assert a[0] == 0, (what, a[1])
    assert a[2].keys() == b[2].keys() and a[2], what
    for k in a[2]:
        assert a[2][k] == b[2][k], (what, k, len(a[2][k]), len(b[2][k]))
    return a[2]


def as_bam(sam, path):
    f = hostapi.BamFile(str(sam))
    open(path, "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    return str(path)


def blocks_of(path):
    f = hostapi.BamFile(str(path))
    t = f.bgzf_blocks()
    f.close()
    return open(path, "rb").read(), t["coff"], t["csize"], t["isize"], t["header_bytes"]


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gens(tmp_path_factory):
    """seed -> generated records, F and F' as SAM text and as BAM"""
    d = tmp_path_factory.mktemp("modtags_gen")
    out = {}
    for seed, T in THRESHOLD.items():
        g = M.generate(seed, 3000, long_reads=False)
        f, fp = d / ("f%d.sam" % seed), d / ("fp%d.sam" % seed)
        M.write_pair(g["refs"], g["recs"], T, f, fp)
        out[seed] = dict(g, T=T, f=str(f), fp=str(fp), f_bam=as_bam(f, d / ("f%d.bam" % seed)), fp_bam=as_bam(fp, d / ("fp%d.bam" % seed)), dir=d)
    return out


def windows(path):
    f = hostapi.BamFile(str(path))
    (raw, off), = f.windows()
    f.close()
    return raw, off


def same_soa(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- 1. the library ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_library_soa_of_f_equals_that_of_fprime(eng, gens, monkeypatch, seed, staged):
    g = gens[seed]
    monkeypatch.setenv("METHEOR_MM_STAGED", "1" if staged else "0")
    raw, off = windows(g["f"])
    raw_p, off_p = windows(g["fp"])
    n = len(off) - 1
    assert n == len(g["recs"]) == len(off_p) - 1
    try:
        eng.decode_set_modtags(False)
        eng.decode_records(raw_p, off_p)
        want = eng.decoded_fetch()
        assert len(want["cpg_pos"]) > (3000 if g["T"] != 0 else 20000) and 0 < want["fwd"].sum() < n
        assert (want["cpg_pos"] >> 31).sum() > (0 if g["T"] == 255 else 1000)
        eng.decode_set_modtags(True, g["T"])
        eng.decode_records(raw, off)
        same_soa(eng.decoded_fetch(), want, "records")
        cuts = [0, n // 3, n // 3 + 1, n]                                # the same appended in several windows
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.decode_records(raw[int(off[a]):int(off[b])], off[a:b + 1] - off[a], append=a > 0)
        same_soa(eng.decoded_fetch(), want, "appended windows")
        # the BAM form: inflate, record walk and decode on the device
        eng.bgzf_decode(*blocks_of(g["f_bam"]))
        same_soa(eng.decoded_fetch(), want, "bgzf")
        eng.decode_set_modtags(False)
        eng.bgzf_decode(*blocks_of(g["fp_bam"]))
        same_soa(eng.decoded_fetch(), want, "bgzf of F'")
        if seed == 1:                                                    # --cpg-set: half the sites
            half = sorted({(0, int(p & 0x7fffffff)) for p in want["cpg_pos"]})[::2]
            eng.decode_set_cpg_filter(half)
            eng.decode_records(raw_p, off_p)
            want_half = eng.decoded_fetch()
            assert 0 < len(want_half["cpg_pos"]) < len(want["cpg_pos"])
            eng.decode_set_modtags(True, g["T"])
            eng.decode_records(raw, off)
            same_soa(eng.decoded_fetch(), want_half, "cpg filter")
        assert eng.notes() & 2                                           # hard clips / MN mismatches were seen
    finally:
        eng.decode_set_modtags(False)
        eng.decode_set_cpg_filter(None)


@pytest.mark.parametrize("staged", FORMS, ids=FORM_IDS)
def test_three_long_records(eng, monkeypatch, staged):
    monkeypatch.setenv("METHEOR_MM_STAGED", "1" if staged else "0")
    g = M.generate(9, 3000, long_reads=True)
    recs = [r for r in g["recs"] if len(r.seq) > 2000 and "H" not in r.cigar][:3]
    assert len(recs) == 3
    raw, off = M.pack_stream(recs)
    raw_p, off_p = M.pack_stream([M.fprime(r, 128) for r in recs])
    try:
        eng.decode_set_modtags(False)
        eng.decode_records(raw_p, off_p)
        want = eng.decoded_fetch()
        assert len(want["cpg_pos"]) > 100
        eng.decode_set_modtags(True, 128)
        eng.decode_records(raw, off)
        same_soa(eng.decoded_fetch(), want, "long")
    finally:
        eng.decode_set_modtags(False)


# ---- 2. errors and notes ------------------------------------------------------------------------------------------------
OK = M.Rec("ok", 0, 50, 30, "10M", "ACGTCGCCGA", ["MM:Z:C+m?,1,1;", "ML:B:C,200,30"])


def fresh():
    import metheor_amd
    return metheor_amd.Engine(0)


@pytest.mark.parametrize("staged", FORMS, ids=FORM_IDS)
def test_every_error_case_is_a_format_error(monkeypatch, staged):
    import metheor_amd
    monkeypatch.setenv("METHEOR_MM_STAGED", "1" if staged else "0")
    e = fresh()
    try:
        e.decode_set_modtags(True, 128)
        crafted = [("aux count wraps the cursor", M.pack_record(OK, raw_aux=b"XBBI" + struct.pack("<I", 0x3ffffffe) + b"MMZC+m?,1;\0")),
                   ("Z without its NUL", M.pack_record(OK, raw_aux=b"MMZC+m?,1;"))]
        for what, raw_bad in [(w, M.pack_record(M.Rec(r.name, r.flag, r.pos, 0, r.cigar, r.seq, r.tags))) for w, r in M.error_recs()] + crafted:
            parts = [M.pack_record(OK), raw_bad, M.pack_record(OK)]        # mapq 0: raised whatever the mapq
            off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
            with pytest.raises(metheor_amd.MthError) as err:
                e.decode_records(b"".join(parts), off)
                e.decoded_fetch()
            assert err.value.status == ERR_FORMAT and "modtags:" in str(err.value), (what, str(err.value))
            e.reset()
        # and the context still decodes
        raw, off = M.pack_stream([OK])
        assert e.decode_records(raw, off) == (1, 2)
    finally:
        e.close()


@pytest.mark.parametrize("staged", FORMS, ids=FORM_IDS)
def test_capacity_notes_and_state(monkeypatch, staged):
    import metheor_amd
    monkeypatch.setenv("METHEOR_MM_STAGED", "1" if staged else "0")
    e = fresh()
    try:
        e.decode_set_modtags(True, 128)
        raw, off = M.pack_stream([OK])
        assert e.decode_records(raw, off) == (1, 2) and e.notes() == 0
        tags = ["MM:Z:C+m.,0;"]
        for r in (M.Rec("h", 0, 50, 30, "3H10M", OK.seq, tags), M.Rec("mn", 16, 50, 30, "10M", OK.seq, tags + ["MN:i:12"]),
                  M.Rec("noseq", 0, 50, 30, "10M", "*", tags)):
            e2 = fresh()
            try:
                e2.decode_set_modtags(True, 128)
                raw, off = M.pack_stream([r])
                assert e2.decode_records(raw, off) == (1, 0), r.name
                d = e2.decoded_fetch()
                assert (d["start"][0], d["end"][0], d["fwd"][0]) == (50, 59, 0 if r.flag & 16 else 1)
                assert e2.notes() == 2, r.name
            finally:
                e2.close()
        # l_seq = 65536: cpg_rel is 16 bits
        raw, off = M.pack_stream([M.Rec("long", 0, 50, 30, "65536M", "AC" * 32768, ["MM:Z:C+m?,0;"])])
        with pytest.raises(metheor_amd.MthError) as err:
            e.decode_records(raw, off)
            e.decoded_fetch()
        assert err.value.status == ERR_CAPACITY and "modtags:" in str(err.value)
        e.reset()
        raw, off = M.pack_stream([M.Rec("long", 16, 50, 30, "65535M", "CG" * 32767 + "C", ["MM:Z:C+m.;"])])
        assert e.decode_records(raw, off) == (1, 32767)
        # one source of calls; a threshold is an ML value
        for bad in (256, 1 << 20):
            with pytest.raises(metheor_amd.MthError) as err:
                e.decode_set_modtags(True, bad)
            assert err.value.status == ERR_INVALID
        with pytest.raises(metheor_amd.MthError) as err:
            e.tag_set_genome([(8, b"ACGTACGT")])
            e.decode_set_genome(True)
        assert err.value.status == ERR_STATE
        e.decode_set_modtags(False)
        e.decode_set_genome(True)
        with pytest.raises(metheor_amd.MthError) as err:
            e.decode_set_modtags(True, 128)
        assert err.value.status == ERR_STATE
        e.decode_set_genome(False)
        e.decode_set_modtags(True, 128)
    finally:
        e.close()


# ---- 3. the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub,staged", [(s, None) for s in SINGLE + ["all"]] + [("pdr", "0"), ("all", "0"), ("pdr", "1")],
                         ids=[s + "-default" for s in SINGLE + ["all"]] + ["pdr-direct", "all-direct", "pdr-staged"])
def test_measures_and_all_equal_the_run_on_fprime(gens, tmp_path, sub, staged):
    g = gens[1]
    env = {} if staged is None else {"METHEOR_MM_STAGED": staged}      # (unset: the default form, which is the staged one)
    extra = LOW[sub] if sub != "all" else ["-d", "1", "-p", "1"]
    a = measure(sub, g["f"], tmp_path, sub + "_mm", extra, more=mm(g["T"]), env=env)
    b = measure(sub, g["fp"], tmp_path, sub + "_fp", extra)
    outs = assert_same(a, b, (sub, staged))
    assert all(v.count(b"\n") >= 2 for v in outs.values()), sub
    if sub in ("pdr", "mhl", "fdrp"):
        assert outs["out"].count(b"\n") >= 1000, sub
    assert "--mm-tags: the input holds records" in a[1] and "--mm-tags" not in b[1]


@pytest.mark.parametrize("seed", [2, 3])
def test_thresholds_0_and_255_on_the_command_line(gens, tmp_path, seed):
    g = gens[seed]
    for sub in ("pdr", "lpmd"):
        a = measure(sub, g["f_bam"], tmp_path, sub + "_mm", LOW[sub], more=mm(g["T"]))
        b = measure(sub, g["fp_bam"], tmp_path, sub + "_fp", LOW[sub])
        assert_same(a, b, (sub, seed))
    if seed == 3:       # and the threshold matters
        c = measure("pdr", g["f_bam"], tmp_path, "pdr_128", LOW["pdr"], more=mm(128))
        assert c[0] == 0 and c[2]["out"] != a[2]["out"]


def test_region_and_gpus(gens, tmp_path):
    g = gens[4]
    bamio.write_bai(g["f_bam"])
    bamio.write_bai(g["fp_bam"])
    region = "c0:9001-21000"
    env = {"METHEOR_SHARD_HALO": "4000"}
    for sub in ("pdr", "lpmd"):
        extra = ["-d", "2"] if sub != "lpmd" else []
        a = measure(sub, g["f_bam"], tmp_path, sub + "_rm", extra, more=["--region", region] + mm(g["T"]), env=env)
        b = measure(sub, g["fp_bam"], tmp_path, sub + "_rp", extra, more=["--region", region], env=env)
        outs = assert_same(a, b, (sub, "region"))
        assert outs["out"].count(b"\n") >= (2 if sub == "lpmd" else 50), sub
    for sub in ("fdrp", "me"):                     # the mode is set on every shard's context
        a = measure(sub, g["f_bam"], tmp_path, sub + "_sm", ["-d", "2"], more=["--gpus", "2"] + mm(g["T"]), env=dict(env, METHEOR_MM_STAGED="0"))
        b = measure(sub, g["fp_bam"], tmp_path, sub + "_sp", ["-d", "2"], env=env)
        outs = assert_same(a, b, (sub, "gpus 2"))
        assert outs["out"].count(b"\n") >= 50, sub


def test_cpg_set_and_unsorted_input(gens, tmp_path):
    g = gens[4]
    # -c: a BED of half the CpGs F' calls
    f = hostapi.BamFile(g["fp"])
    sites = sorted({int(p & 0x7fffffff) for p in f.decode()["cpg_pos"]})[::2]
    f.close()
    bed = tmp_path / "half.bed"
    bed.write_text("".join("c0\t%d\t%d\n" % (p, p + 2) for p in sites))
    for sub in ("pdr", "all"):
        a = measure(sub, g["f_bam"], tmp_path, sub + "_cm", ["-d", "2", "-p", "2"], more=["-c", bed] + mm(g["T"]))
        b = measure(sub, g["fp_bam"], tmp_path, sub + "_cp", ["-d", "2", "-p", "2"], more=["-c", bed])
        outs = assert_same(a, b, (sub, "cpg-set"))
        assert all(v.count(b"\n") >= 2 for v in outs.values()), sub
    # not coordinate-sorted: blocks of records moved around (file-order replay for pdr, the device sort for lpmd)
    rng = np.random.default_rng(4)
    blocks = [g["recs"][k:k + 250] for k in range(0, len(g["recs"]), 250)]
    order = [0] + list(1 + rng.permutation(len(blocks) - 1))
    recs = [r for k in order for r in blocks[k]]
    uf, ufp = tmp_path / "u.sam", tmp_path / "up.sam"
    M.write_pair(g["refs"], recs, g["T"], uf, ufp, sorted_=False)
    for sub in ("pdr", "lpmd"):
        a = measure(sub, uf, tmp_path, sub + "_um", LOW[sub], more=mm(g["T"]))
        b = measure(sub, ufp, tmp_path, sub + "_up", LOW[sub])
        outs = assert_same(a, b, (sub, "unsorted"))
        assert outs["out"].count(b"\n") >= (2 if sub == "lpmd" else 100), sub


def test_a_malformed_file_exits_101(tmp_path):
    head = "@HD\tVN:1.6\n@SQ\tSN:c0\tLN:400\n"
    for k, (what, r) in enumerate(M.error_recs()[::9]):
        p = tmp_path / ("bad%d.sam" % k)
        p.write_text(head + OK.line([("c0", 400)]) + "\n" + M.Rec(r.name, r.flag, r.pos, 3, r.cigar, r.seq, r.tags).line([("c0", 400)]) + "\n")
        for sub, env in (("lpmd", {}), ("pdr", {"METHEOR_MM_STAGED": "0"})):
            out = tmp_path / "o.tsv"
            r2 = run(sub, "-i", p, "-o", out, "--mm-tags", env=env)
            assert r2.returncode == 101 and "modtags:" in r2.stderr, (what, sub, r2.stderr)
    # without --mm-tags the same file is a file without XM tags: 101 as ever
    r2 = run("pdr", "-i", p, "-o", tmp_path / "o2.tsv")
    assert r2.returncode == 101 and "Error reading XM tag in BAM record" in r2.stderr
    # and the host decoder has no form of the mode
    r2 = run("pdr", "-i", p, "-o", tmp_path / "o3.tsv", "--mm-tags", env={"METHEOR_HOST_DECODE": "1"})
    assert r2.returncode == 101 and "--mm-tags needs the device record decode" in r2.stderr


def test_fdrp_on_a_long_reverse_record_exits_as_the_run_on_fprime(tmp_path):
    """a reverse record of 203..403 reference bases calling at its start - 1 and 202 bp further: the reference's window index is
    -1 (fdrp.rs:70-72) and the run on F' ends with 101 -- so does the run on F"""
    seq = "CG" + "A" * 200 + "CG" + "A" * 97                          # the leading C is soft-clipped: the record starts on its G
    assert len(seq) == 301 and seq[202:204] == "CG"
    rng = np.random.default_rng(1)
    recs = [M.Rec("r%d" % k, 16, 1000, 30, "1S300M", seq, ["MM:Z:C+m.,0,0;", "ML:B:C,200,%d" % int(rng.integers(0, 256))]) for k in range(12)]
    x = M.x_string(recs[0], 128)[0]
    assert x[1] in "zZ" and x[203] == "Z" and x.count(".") == 299      # calls at start - 1 = 999 and at start + 201 = 1201
    f, fp = tmp_path / "f.sam", tmp_path / "fp.sam"
    M.write_pair([("c0", 40000)], recs, 128, f, fp)
    for sub in ("fdrp", "qfdrp"):
        a = run(sub, "-i", f, "-o", tmp_path / "a.tsv", "-d", "1", "--mm-tags")
        b = run(sub, "-i", fp, "-o", tmp_path / "b.tsv", "-d", "1")
        assert a.returncode == b.returncode == 101, (sub, a.stderr, b.stderr)
        assert "fdrp" in a.stderr and a.stderr.splitlines()[-1] == b.stderr.splitlines()[-1]
    a = measure("pdr", f, tmp_path, "pdr_mm", ["-d", "1", "-p", "1"], more=["--mm-tags"])
    b = measure("pdr", fp, tmp_path, "pdr_fp", ["-d", "1", "-p", "1"])
    assert_same(a, b, "pdr on the same file")


# ---- 4. a record longer than a BGZF block -----------------------------------------------------------------------------------
def write_straddling_bam(path, refs, recs, cut=0xff00):
    text = M.sam_text(refs, []).encode()
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    hbytes = len(raw)
    raw += M.pack_stream(recs)[0]
    with open(path, "wb") as fh:
        for o in range(0, len(raw), cut):
            fh.write(bamio._bgzf_block(raw[o:o + cut]))
        fh.write(bamio._bgzf_block(b""))
    return hbytes


@pytest.mark.parametrize("staged", FORMS, ids=FORM_IDS)
def test_a_record_longer_than_a_block_through_the_straddle_route(eng, tmp_path, monkeypatch, staged):
    from tests.test_gpu_inflate import block_table
    monkeypatch.setenv("METHEOR_MM_STAGED", "1" if staged else "0")
    rng = np.random.default_rng(3)
    g = M.generate(5, 300, long_reads=False)
    L = 60000
    seq = "".join(rng.choice(list("ACGT"), L, p=[0.2, 0.3, 0.3, 0.2]))
    n_c = seq.count("C")
    pick = sorted(rng.choice(n_c, n_c // 3, replace=False).tolist())
    big = M.Rec("big", 0, 20000, 40, "%dM" % L, seq, ["MM:Z:C+m?" + "".join(",%d" % x for x in M.skips_of(pick)) + ";",
                                                       "ML:B:C" + "".join(",%d" % x for x in rng.integers(0, 256, len(pick)))])
    big_r = M.Rec("bigr", 16, 20001, 40, big.cigar, seq, ["MM:Z:C+m." + "".join(",%d" % x for x in M.skips_of(sorted(rng.choice(seq.count("G"), 5000, replace=False).tolist()))) + ";"])
    k = next(i for i, r in enumerate(g["recs"]) if r.pos > 20001)
    recs = g["recs"][:k] + [big, big_r] + g["recs"][k:]
    assert len(M.pack_record(big)) > 0xff00
    refs = [("c0", 100000)]
    f, fp = str(tmp_path / "f.bam"), str(tmp_path / "fp.bam")
    write_straddling_bam(f, refs, recs)
    write_straddling_bam(fp, refs, [M.fprime(r, 128) for r in recs])
    try:
        eng.decode_set_modtags(False)
        fb, coff, csize, isize, hbytes, _ = block_table(fp)
        n, nc, _ = eng.bgzf_decode_straddle(fb, coff, csize, isize, hbytes, last=True)
        want = eng.decoded_fetch()
        assert n == len(recs) and nc > 5000
        eng.decode_set_modtags(True, 128)
        fb, coff, csize, isize, hbytes, _ = block_table(f)
        assert len(coff) >= 3
        eng.bgzf_decode_straddle(fb, coff, csize, isize, hbytes, last=True)
        same_soa(eng.decoded_fetch(), want, "straddle")
    finally:
        eng.decode_set_modtags(False)
    if not staged:      # and the command line's straddle route
        a = measure("pdr", f, tmp_path, "s_mm", ["-d", "1", "-p", "1"], more=["--mm-tags"], env={"METHEOR_DEVICE_STRADDLE": "1"})
        b = measure("pdr", fp, tmp_path, "s_fp", ["-d", "1", "-p", "1"], env={"METHEOR_DEVICE_STRADDLE": "1"})
        assert_same(a, b, "straddle, command line")
