"""The CLI's other routes from BAM to TSV on irregular reads (tests/irregular_util.py), each against the oracle's text and each
asserting from METHEOR_TIMING which route ran: the device BGZF load (block-aligned BAM), unsorted input replayed in file order
(mth_fileorder.hip) for pdr / mhl / fdrp / qfdrp in five orders -- flush traps among them -- through both load paths, unsorted
input through the device sort and the host sort for lpmd / me / pm, `metheor all` on unsorted input, --region at a read that
starts at its end and calls end - 1, and --gpus N with every cut at such a read.  Low -d throughout: one read missing or extra
changes a row.  tests/test_irregular_paths.py checks on the CPU that the inputs hold these cases."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import irregular_util as I
from tests import test_gpu_multi as T_multi
from tests import test_irregular_paths as P
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
STREAM, DEVICE = "  inflate + device record decode", "  device inflate + walk + decode"


def run(env, *args):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env=dict(os.environ, METHEOR_TIMING="1", **{k: str(v) for k, v in (env or {}).items()}))


def write(tmp_path, rec, name, aligned):
    """write_bam cuts blocks every 60 000 bytes (records straddle them: the host-inflate stream); aligned: whole records per block"""
    raw = str(tmp_path / (name + ".raw.bam"))
    bamio.write_bam(raw, rec)
    if not aligned:
        return raw
    bam = str(tmp_path / (name + ".bam"))
    util.reblock_aligned(raw, bam)
    return bam


def names_of(rec):
    return [n for n, _ in rec.refs]


def test_device_bgzf_whole_path(tmp_path):
    """irregular records (all-S and call-less ones too) in a flush-trap order, reblocked: mth_bgzf_decode's SoA == the oracle's"""
    import metheor_amd
    from tests.test_gpu_inflate import block_table, same_soa
    rec = P.unsorted_records(0)
    sh, _ = I.shuffle(rec, "flush_trap", np.random.default_rng(2))
    bam = write(tmp_path, sh, "u", True)
    fb, coff, csize, isize, hbytes, raw = block_table(bam)
    eng = metheor_amd.Engine(0)
    try:
        assert eng.bgzf_inflate(fb, coff, csize, isize).tobytes() == raw
        eng.bgzf_decode(fb, coff, csize, isize, hbytes)
        same_soa(eng.decoded_fetch(), pyoracle.Reads.decode(sh).soa())
    finally:
        eng.close()


CASES = [(o, p) for o in I.ORDERS for p in ("stream", "device")]


@pytest.mark.parametrize("order,path", CASES, ids=["%s-%s" % c for c in CASES])
def test_unsorted_order_dependent(tmp_path, order, path):
    """pdr, mhl and fdrp or qfdrp of the file-order replay against the oracle streaming the same file; device-path cases take
    --max-depth 8 (below the piles: the reservoir under METHEOR_SEED); the flush-trap stream case a BED that keeps one site of
    every adjacent pair; the shuffled stream case also keeps the records the reference panics on (exit 101, fdrp.rs:70-72)"""
    k = CASES.index((order, path))
    rng = np.random.default_rng(40 + k)
    rec = P.unsorted_records(k % 2)
    sh, _ = I.shuffle(rec, order, rng)
    names = names_of(sh)
    if order == "shuffled" and path == "stream":                  # + test_gpu_fileorder._panic_records' reads, spread over the file
        rows = I.rows_of(sh)
        xm = ["."] * 210
        xm[0], xm[100], xm[202] = "z", "z", "Z"
        for j, row in enumerate([(0, 3000, 16, 40, [("M", 210)], "".join(xm)), (0, 3005, 0, 40, [("M", 50)], "z" + "." * 48 + "Z"),
                                 (0, 3300, 0, 40, [("M", 32)], "Z" + "." * 30 + "z")]):
            rows.insert(len(rows) * (j + 1) // 4, row)
        bad = I.records_from_rows(sh.refs, rows)
        bam = write(tmp_path, bad, "panic", False)
        with pytest.raises(pyoracle.ReferencePanic):
            pyoracle.Reads.decode(bad).fdrp(min_depth=1, max_depth=40, min_overlap=0)
        r = run({}, "fdrp", "-i", bam, "-o", tmp_path / "x.tsv", "-d", 1, "-D", 40, "-l", 0)
        assert r.returncode == 101 and "fdrp.rs:70-72" in r.stderr, (r.returncode, r.stderr)
    sh = I.fdrp_safe(sh)
    bam = write(tmp_path, sh, "u", path == "device")
    extra, cpg_set = [], None
    if order == "flush_trap" and path == "stream":
        keys = I.called_sites(pyoracle.Reads.decode(sh), 0)
        keep = keys[np.concatenate([[True], np.diff(keys) != 1])]              # the right site of each adjacent pair goes
        assert len(keep) < len(keys) - 20
        cpg_set = [(int(x >> 32), int(x & 0xffffffff)) for x in keep]
        (tmp_path / "s.bed").write_text("".join("%s\t%d\t%d\n" % (names[t], p, p + 2) for t, p in cpg_set))
        extra = ["-c", tmp_path / "s.bed"]
    reads = pyoracle.Reads.decode(sh, cpg_set=cpg_set)
    D = 8 if path == "device" else 200
    fd = "fdrp" if k % 4 < 2 else "qfdrp"
    o = tmp_path / "o.tsv"
    for sub, flags in (("pdr", ["-d", k % 2, "-p", 1]), ("mhl", ["-d", 1, "-p", 1]), (fd, ["-d", 1, "-D", D, "-l", 0])):
        r = run({"METHEOR_SEED": 5}, sub, "-i", bam, "-o", o, *flags, *extra)
        assert r.returncode == 0, (sub, r.stderr)
        assert "file-order replay" in r.stderr and (STREAM if path == "stream" else DEVICE) in r.stderr, (sub, r.stderr)
        want, _ = util.oracle_text(reads, names, sub, seed=5, **util.oracle_kwargs(sub, [str(x) for x in flags]))
        assert len(want) > 2000
        util.assert_tsv_equals_oracle(sub, o.read_text(), want)


@pytest.mark.parametrize("order", ["shuffled", "flush_trap"])
def test_unsorted_order_free(tmp_path, order):
    """lpmd (+ pairs), me and pm through the device sort; lpmd again through the host decoder's sort, where pdr is refused"""
    rec, names = I.make_records(950, n_contigs=2, length=8_000, n_reads=1_200, density=0.03)
    sh, _ = I.shuffle(rec, order, np.random.default_rng(7))
    bam = write(tmp_path, sh, "u", order == "flush_trap")
    reads = pyoracle.Reads.decode(sh)
    o, pf = tmp_path / "o.tsv", tmp_path / "p.tsv"
    for env, route in (({}, "device sort by (tid, start)"), ({"METHEOR_HOST_DECODE": "1"}, "  sort by (tid, start)")):
        subs = (("lpmd", ["-m", "1", "-M", "40"]), ("me", ["-d", "1"]), ("pm", ["-d", "1"])) if not env else (("lpmd", ["-m", "1", "-M", "40"]),)
        for sub, flags in subs:
            r = run(env, sub, "-i", bam, "-o", o, *flags, *(["-p", pf] if sub == "lpmd" else []))
            assert r.returncode == 0, (sub, r.stderr)
            assert route in r.stderr and (env or "host decode" not in r.stderr), (sub, r.stderr)
            if env:
                assert "device sort" not in r.stderr
            want, want_pairs = util.oracle_text(reads, names, sub, input_name=bam, **util.oracle_kwargs(sub, flags))
            util.assert_tsv_equals_oracle(sub, o.read_text(), want)
            if sub == "lpmd":
                assert pf.read_text() == want_pairs and want_pairs.count("\n") > 1000
    r = run({"METHEOR_HOST_DECODE": "1"}, "pdr", "-i", bam, "-o", o)
    assert r.returncode == 101 and "not coordinate-sorted" in r.stderr, r.stderr


def test_all_on_unsorted_input(tmp_path):
    """`metheor all` on a flush-trap order with all-S and call-less records (its order-free measures then load the file again on
    the host) against the single commands, and every single command against the oracle"""
    rec = I.fdrp_safe(P.unsorted_records(1))
    sh, _ = I.shuffle(rec, "flush_trap", np.random.default_rng(9))
    bam = write(tmp_path, sh, "u", True)
    reads = pyoracle.Reads.decode(sh)
    params = {"d": 1, "p": 1, "q": 10, "m": 1, "M": 40, "D": 40, "l": 0}
    d = tmp_path / ("c%d" % len(list(tmp_path.iterdir())))
    ra = T_multi.check_all(tmp_path, bam, params, env={"METHEOR_SEED": "3", "METHEOR_TIMING": "1"})
    assert "file-order replay" in ra.stderr
    for sub in T_multi.OUT:
        flags = []
        for f, v in params.items():
            if f in T_multi.SINGLE_FLAGS[sub]:
                flags += ["-" + f, str(v)]
        want, want_pairs = util.oracle_text(reads, names_of(sh), sub, input_name=bam, seed=3, **util.oracle_kwargs(sub, flags))
        util.assert_tsv_equals_oracle(sub, (d / ("one." + sub)).read_text(), want)
        if sub == "lpmd":
            assert (d / "one.pairs").read_text() == want_pairs


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    d = tmp_path_factory.mktemp("forced")
    rec, names, at = I.forced_records()
    raw, bam = str(d / "raw.bam"), str(d / "f.bam")
    bamio.write_bam(raw, rec)
    util.reblock_aligned(raw, bam, cut_before=set(I.shifted_starts(rec).tolist()))
    bamio.write_bai(bam)
    return rec, names, bam, pyoracle.Reads.decode(rec)


MEASURES = (("pdr", ["-d", "1", "-p", "1"]), ("lpmd", ["-m", "1", "-M", "40"]), ("mhl", ["-d", "1", "-p", "1"]), ("me", ["-d", "1"]),
            ("pm", ["-d", "1"]), ("fdrp", ["-d", "1", "-D", "40", "-l", "0"]), ("qfdrp", ["-d", "1", "-D", "40", "-l", "0"]))


def test_region_at_adversarial_edges(forced, tmp_path):
    """--region chrI0:beg+1-REGION_END (test_irregular_paths.region_edges): rows == the whole-file oracle's rows the region owns
    (sites by position, quartets and pairs by their first CpG), LPMD == the oracle over the reads that start in it"""
    rec, names, bam, reads = forced
    t, b, e = P.region_edges(rec)
    region = "%s:%d-%d" % (names[t], b + 1, e)

    def owned(text):
        return "".join(l for l in text.splitlines(True) if l.split("\t")[0] == names[t] and b <= int(l.split("\t")[1]) < e)
    o, pf = tmp_path / "o.tsv", tmp_path / "p.tsv"
    for sub, flags in MEASURES:
        r = run({"METHEOR_SEED": "2"}, sub, "-i", bam, "-o", o, *flags, "--region", region, *(["-p", pf] if sub == "lpmd" else []))
        assert r.returncode == 0, (sub, r.stderr)
        assert DEVICE in r.stderr, r.stderr
        want, want_pairs = util.oracle_text(reads, names, sub, input_name=bam, seed=2, **util.oracle_kwargs(sub, flags))
        if sub == "lpmd":
            sel = np.nonzero((rec.tid == t) & (rec.pos >= b) & (rec.pos < e))[0]
            w, _ = util.oracle_text(pyoracle.Reads.decode(rec.subset(sel)), names, "lpmd", input_name=bam, **util.oracle_kwargs(sub, flags))
            assert o.read_text() == w
            head, body = want_pairs.split("\n", 1)
            assert pf.read_text() == head + "\n" + owned(body) and len(owned(body)) > 1000
        else:
            assert len(owned(want)) > 1000
            assert sub in ("me", "pm") or ("%s\t%d\t" % (names[t], e - 1)) in owned(want)
            util.assert_tsv_equals_oracle(sub, o.read_text(), owned(want))


def test_shards_with_forced_cuts(forced, tmp_path):
    """--gpus N, N in test_irregular_paths.SHARD_N (every cut at a read that starts at p and calls p - 1, one under a pile, one in
    a CG island): every measure byte-identical to the single run and equal to the oracle, the pairs table too; one -c run; a file
    with an all-S record is refused loudly"""
    rec, names, bam, reads = forced
    env = {"METHEOR_SEED": "4", "METHEOR_SHARD_HALO": str(P.HALO)}
    for sub, flags in MEASURES:
        o1 = tmp_path / ("one_" + sub)
        r = run(env, sub, "-i", bam, "-o", o1, *flags, *(["-p", tmp_path / "one_pairs"] if sub == "lpmd" else []))
        assert r.returncode == 0 and DEVICE in r.stderr, (sub, r.stderr)
        want, want_pairs = util.oracle_text(reads, names, sub, input_name=bam, seed=4, **util.oracle_kwargs(sub, flags))
        util.assert_tsv_equals_oracle(sub, o1.read_text(), want)
        if sub == "lpmd":
            assert (tmp_path / "one_pairs").read_text() == want_pairs
        for n in P.SHARD_N:
            oN = tmp_path / ("sh%d_%s" % (n, sub))
            r = run(env, sub, "-i", bam, "-o", oN, *flags, "--gpus", n, *(["-p", tmp_path / ("sh_pairs%d" % n)] if sub == "lpmd" else []))
            assert r.returncode == 0, (sub, n, r.stderr)
            assert oN.read_bytes() == o1.read_bytes(), (sub, n)
            if sub == "lpmd":
                assert (tmp_path / ("sh_pairs%d" % n)).read_bytes() == (tmp_path / "one_pairs").read_bytes()
    keys = I.called_sites(reads, 0)
    keep = keys[::2]
    (tmp_path / "s.bed").write_text("".join("%s\t%d\t%d\n" % (names[int(x >> 32)], int(x & 0xffffffff), int(x & 0xffffffff) + 2) for x in keep))
    r = run(env, "pdr", "-i", bam, "-o", tmp_path / "c.tsv", "-d", 1, "-p", 1, "-c", tmp_path / "s.bed", "--gpus", 5)
    assert r.returncode == 0, r.stderr
    cpg = [(int(x >> 32), int(x & 0xffffffff)) for x in keep]
    want, _ = util.oracle_text(pyoracle.Reads.decode(rec, cpg_set=cpg), names, "pdr", min_depth=1, min_cpgs=1)
    assert (tmp_path / "c.tsv").read_text() == want and len(want) > 1000
    # one record without an aligned base: the batches cannot hold it, and a shard must not quietly answer differently
    rows = I.rows_of(rec)
    rows.insert(len(rows) // 2, (rows[len(rows) // 2][0], rows[len(rows) // 2][1], 0, 42, [("S", 50)], "Z" * 50))
    ub = write(tmp_path, I.records_from_rows(rec.refs, rows), "unal", True)
    r = run(env, "pdr", "-i", ub, "-o", tmp_path / "u.tsv", "--gpus", 2)
    assert r.returncode != 0 and "need the device load path" in r.stderr, r.stderr
