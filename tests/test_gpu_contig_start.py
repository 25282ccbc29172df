"""CpG calls at position -1 -- a record at position 0 whose flag is outside {0, 99, 147} calling on its first aligned base
(readutil.rs:332-340); the reference keeps -1 as an ordinary i32 key, the first of its contig -- on every measure and every route
from file to TSV, byte for byte against the oracle's text built from Reads.decode (tests/contig_start_util.py: the two
call_at_minus_one cases of tests/golden/unpinned_cases.json.gz, a few dozen records on two contigs; tests/test_contig_start_inputs.py
checks on the CPU what they hold).  The engine keeps 31 bits of position: the decoders write -1 as the word 0x7fffffff, a contig
that holds one is run as a contig group shifted up (the call lies at voff - 1) and every fetch maps it back to -1; the file-order
replay orders the word before 0.  Integers and PDR / LPMD / PM / FDRP / qFDRP floats bit for bit, MHL and ME within 1e-6
(util.assert_tsv_equals_oracle)."""
import os
import subprocess

import numpy as np
import pytest

from metheor_amd import hostapi
from oracle import bamio, pyoracle
from tests import contig_start_util as S
from tests import test_gpu_multi as T_multi
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
PARAMS = {"d": 1, "p": 1, "q": 10, "m": 2, "M": 16, "D": 64, "l": 10}
SUBS = ("pdr", "mhl", "fdrp", "qfdrp", "me", "pm", "lpmd")
BASE = 4096                                                    # MTH_GROUP_MINUS_ONE_BASE


def run(env, *args):
    """one measure = one CLI process under a time limit; a process that died on a signal or ran into the limit ends the session --
    nothing more is started on a GPU that may have faulted"""
    try:
        r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=120,
                           env=dict(os.environ, METHEOR_TIMING="1", **(env or {})))
    except subprocess.TimeoutExpired:
        pytest.exit("metheor %s did not finish in 120 s" % " ".join(str(a) for a in args), returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:
        pytest.exit("metheor %s died (%d): %s" % (" ".join(str(a) for a in args), r.returncode, r.stderr[-2000:]), returncode=3)
    return r


def flags_of(sub):
    return [x for f, v in PARAMS.items() if f in T_multi.SINGLE_FLAGS[sub] for x in ("-" + f, str(v))]


def write_sam(bam, path, refs):
    f = hostapi.BamFile(bam)
    try:
        lines = [b"@HD\tVN:1.0\tSO:coordinate\n"] + [("@SQ\tSN:%s\tLN:%d\n" % r).encode() for r in refs]
        for raw, off in f.windows():
            lines += [f.sam_line(raw, int(off[k]), int(off[k + 1])) for k in range(len(off) - 1)]
    finally:
        f.close()
    with open(path, "wb") as fh:
        fh.write(b"".join(lines))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("contig_start")
    out = {}
    srt, uns = S.records(S.SORTED), S.records(S.UNSORTED)
    for key, rec in (("sorted", srt), ("unsorted", uns), ("one", S.one_contig(srt, 1)), ("res_unsorted", S.reservoir_unsorted(srt))):
        bam = str(d / (key + ".bam"))
        bamio.write_bam(bam, rec)
        out[key] = (bam, rec, pyoracle.Reads.decode(rec), [n for n, _ in rec.refs])
    bamio.write_bai(out["sorted"][0])
    sam = str(d / "sorted.sam")
    write_sam(out["sorted"][0], sam, srt.refs)
    out["sam"] = (sam,) + out["sorted"][1:]
    return out


def want_text(f, sub, inp):
    _, _, reads, names = f
    return util.oracle_text(reads, names, sub, input_name=inp, **util.oracle_kwargs(sub, flags_of(sub)))


def check_single(f, sub, env, tmp_path, inp=None):
    inp = inp or f[0]
    o, pf = tmp_path / "o.tsv", tmp_path / "pairs.tsv"
    r = run(env, sub, "-i", inp, "-o", o, *flags_of(sub), *(["-p", pf] if sub == "lpmd" else []))
    assert r.returncode == 0, (sub, env, r.stderr)
    want, want_pairs = want_text(f, sub, inp)
    got = o.read_text()
    if sub != "lpmd":
        assert "\t-1\t" in want and want.count("\n") > 20                   # (the expectation holds the rows at -1 ...)
        first = {}
        for l in got.splitlines():
            first.setdefault(l.split("\t")[0], l.split("\t")[1])
        if sub not in ("me", "pm"):
            assert set(first.values()) == {"-1"}, first                     # ... and they come first in their contig
    util.assert_tsv_equals_oracle(sub, got, want)
    if sub == "lpmd":
        assert "\t-1\t1\t" in want_pairs
        assert pf.read_text() == want_pairs
    return r


def check_all(f, env, tmp_path, inp=None):
    inp = inp or f[0]
    args = ["all", "-i", inp] + ["-%s%s" % kv for kv in PARAMS.items()]
    for m in T_multi.OUT:
        args += ["--" + m, tmp_path / ("all." + m)]
    args += ["--lpmd-pairs", tmp_path / "all.pairs"]
    r = run(env, *args)
    assert r.returncode == 0, (env, r.stderr)
    for m in T_multi.OUT:
        want, want_pairs = want_text(f, m, inp)
        util.assert_tsv_equals_oracle(m, (tmp_path / ("all." + m)).read_text(), want)
        if m == "lpmd":
            assert (tmp_path / "all.pairs").read_text() == want_pairs and "\t-1\t1\t" in want_pairs
    return r


# ---- every measure on every route of sorted input ---------------------------------------------------------------------------------------
ROUTES = {"default": ("sorted", {}), "group0": ("sorted", {"METHEOR_GROUP": "0"}), "group1": ("sorted", {"METHEOR_GROUP": "1"}),
          "host_decode": ("sorted", {"METHEOR_HOST_DECODE": "1"}), "sam": ("sam", {}), "one_contig": ("one", {}),
          "one_contig_host": ("one", {"METHEOR_HOST_DECODE": "1"})}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("sub", SUBS + ("all",))
def test_measure_on_route(files, tmp_path, sub, route):
    key, env = ROUTES[route]
    r = (check_all(files[key], env, tmp_path) if sub == "all" else check_single(files[key], sub, env, tmp_path))
    if route in ("default", "group1"):
        assert "contig groups" in r.stderr
    if route == "group0":
        assert "contig groups" not in r.stderr
    if "host" in route:
        assert "host decode" in r.stderr, r.stderr


# ---- the kernel forms the per-measure tests force ---------------------------------------------------------------------------------------
FORMS = [(s, e) for s in ("pdr", "lpmd") for e in ({"MTH_PDR_WIDE": "0"}, {"MTH_PDR_WIDE": "14"}, {"MTH_PDR_WIDE": "0", "MTH_TILE_NO_MARGIN": "1"})] + \
        [("mhl", e) for e in ({"MTH_MHL_WALK": "1"}, {"MTH_MHL_ROWCHK": "0"}, {"MTH_MHL_ROWCHK": "1"})] + \
        [(s, e) for s in ("fdrp", "qfdrp") for e in ({"METHEOR_FDRP_WTILE": "0"}, {"METHEOR_FDRP_WTILE": "1"})]


@pytest.mark.parametrize("sub,env", FORMS, ids=["%s-%s" % (s, "-".join("%s=%s" % kv for kv in e.items())) for s, e in FORMS])
def test_kernel_forms(files, tmp_path, sub, env):
    check_single(files["sorted"], sub, env, tmp_path)


# ---- unsorted input: the file-order replay, and `all` ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ("pdr", "mhl", "fdrp", "qfdrp", "all"))
def test_unsorted(files, tmp_path, sub):
    f = files["unsorted"]
    r = check_all(f, {}, tmp_path) if sub == "all" else check_single(f, sub, {}, tmp_path)
    assert "file-order replay" in r.stderr, r.stderr
    # the order matters: the sorted file's rows are other rows
    if sub != "all":
        assert want_text(f, sub, f[0])[0] != want_text(files["sorted"], sub, f[0])[0]


# ---- the reservoir at site -1: -D below the site's arrivals, the draw keyed by (seed, tid, -1, arrivals) -----------------------------------
RES_ROUTES = {"default": ("sorted", {}), "group0": ("sorted", {"METHEOR_GROUP": "0"}), "host_decode": ("sorted", {"METHEOR_HOST_DECODE": "1"}),
              "one_contig": ("one", {}), "file_order": ("res_unsorted", {})}


@pytest.mark.parametrize("route", list(RES_ROUTES))
@pytest.mark.parametrize("sub", ("fdrp", "qfdrp"))
def test_reservoir_at_minus_one(files, tmp_path, sub, route):
    """-d 3 -D 3: site -1 of every contig takes four arrivals, so its row depends on the draw (tests/test_contig_start_inputs.py: at least
    three different rows over these seeds).  A grouped batch must make the draw on the mapped-back site -- the second contig's -1 lies at
    voff - 1, below its own offset -- and the file-order replay on the key's position -1: the oracle's orc_sample_j takes (tid, -1)"""
    key, env = RES_ROUTES[route]
    inp, _, reads, names = files[key]
    o = tmp_path / "o.tsv"
    flags = ["-q", "10", "-d", "3", "-D", "3", "-l", "10"]
    for seed in S.RES_SEEDS:
        r = run(dict(env, METHEOR_SEED=str(seed)), sub, "-i", inp, "-o", o, *flags)
        assert r.returncode == 0, (sub, route, seed, r.stderr)
        assert ("file-order replay" in r.stderr) == (route == "file_order"), r.stderr
        want, _ = util.oracle_text(reads, names, sub, seed=seed, **util.oracle_kwargs(sub, flags))
        assert all(("%s\t-1\t" % n) in want for n in names)
        assert o.read_text() == want, (sub, route, seed)


# ---- --region from the contig's first base ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_region_from_the_first_base(files, tmp_path, sub):
    """--region ctg:1-LN (with a .bai) owns the site at -1: the whole-contig rows"""
    bam, rec, reads, names = files["sorted"]
    o, pf = tmp_path / "o.tsv", tmp_path / "p.tsv"
    want, want_pairs = want_text(files["sorted"], sub, bam)
    for t, name in enumerate(names):
        r = run({}, sub, "-i", bam, "-o", o, *flags_of(sub), "--region", "%s:1-%d" % (name, rec.refs[t][1]), *(["-p", pf] if sub == "lpmd" else []))
        assert r.returncode == 0, (sub, name, r.stderr)
        own = lambda text: "".join(l for l in text.splitlines(True) if l.split("\t")[0] == name)
        if sub == "lpmd":
            sel = np.nonzero(rec.tid == t)[0]
            w, _ = util.oracle_text(pyoracle.Reads.decode(rec.subset(sel)), names, "lpmd", input_name=bam, **util.oracle_kwargs(sub, flags_of(sub)))
            assert o.read_text() == w
            head, body = want_pairs.split("\n", 1)
            assert pf.read_text() == head + "\n" + own(body) and ("%s\t-1\t1\t" % name) in own(body)
        else:
            assert ("%s\t-1\t" % name) in own(want)
            util.assert_tsv_equals_oracle(sub, o.read_text(), own(want))


# ---- the C ABI: a single-contig group, and a plain batch -----------------------------------------------------------------------------------
def _contig(files, tid):
    """contig `tid` of the sorted case as the dict util.device_batch takes (positions as the oracle's SoA has them: -1 = 0x7fffffff)"""
    _, rec, reads, _ = files["sorted"]
    c = util.contig_from_oracle_soa(reads.soa(), tid, 1000)
    assert ((c["cpg_pos"] & S.WORD) == S.WORD).sum() >= 5
    return c, pyoracle.Reads.decode(rec.subset(np.nonzero(rec.tid == tid)[0]))


def _lifted(c, handle):
    g = dict(c, tid=handle, length=c["length"] + BASE)
    g["read_start"] = (c["read_start"] + BASE).astype(np.int32)
    g["read_end"] = (c["read_end"] + BASE).astype(np.int32)
    g["cpg_pos"] = (((c["cpg_pos"] + np.uint32(BASE)) & np.uint32(S.WORD)) | (c["cpg_pos"] & np.uint32(0x80000000))).astype(np.uint32)
    return g


def _fetch_all(e, bt, fused=None):
    """every measure's rows of one batch: through the single entry points, or through mth_multi_accumulate in form `fused`"""
    out = {}
    kw = dict(min_depth=1, min_cpgs=1)
    if fused is None:
        e.reset()
        import metheor_amd
        e.pdr_lpmd_accumulate(bt, metheor_amd.PdrLpmdParams(**kw)); out["pdr"] = e.pdr_fetch(); out["lpmd"] = e.lpmd_global()
        e.reset(); e.mhl_accumulate(bt, **kw); out["mhl"] = e.mhl_fetch()
        e.reset(); e.fdrp_accumulate(bt, min_depth=1, max_depth=64, min_overlap=10); out["fdrp"] = e.fdrp_fetch()
        e.reset(); e.quartet_accumulate(bt); out["quartet"] = e.quartet_fetch(min_depth=1)
        e.reset(); e.lpmd_pairs_accumulate(bt); out["pairs"] = e.lpmd_pairs_fetch()
    else:
        e.reset()
        e.multi_accumulate(bt, want=("pdr", "lpmd", "quartet", "mhl", "fdrp", "pairs"), form=fused, max_depth=64, min_overlap=10, **kw)
        out = dict(pdr=e.pdr_fetch(), lpmd=e.lpmd_global(), mhl=e.mhl_fetch(), fdrp=e.fdrp_fetch(), quartet=e.quartet_fetch(min_depth=1),
                   pairs=e.lpmd_pairs_fetch())
    return out


def _check_rows(d, ora, tid):
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    kw = dict(min_depth=1, min_cpgs=1)
    t = ora.pdr(**kw)
    assert d["pdr"]["pos"].dtype == np.int32 and d["pdr"]["pos"][0] == -1 and (d["pdr"]["tid"] == tid).all()
    assert (d["pdr"]["pos"] == t.pos[:, 0]).all() and (bits(d["pdr"]["pdr"]) == bits(t.val)).all()
    assert (d["pdr"]["n_concordant"] == t.cnt[:, 0]).all() and (d["pdr"]["n_discordant"] == t.cnt[:, 1]).all()
    l = ora.lpmd()
    assert all(d["lpmd"][k] == l[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read"))
    t = ora.mhl(**kw)
    assert d["mhl"]["pos"].dtype == np.int32 and d["mhl"]["pos"][0] == -1 and (d["mhl"]["tid"] == tid).all()
    assert (d["mhl"]["pos"] == t.pos[:, 0]).all() and np.abs(d["mhl"]["mhl"].astype(np.float64) - t.val).max() <= 1e-6
    t, q = ora.fdrp(min_depth=1, max_depth=64, min_overlap=10), ora.qfdrp(min_depth=1, max_depth=64, min_overlap=10)
    assert d["fdrp"]["pos"].dtype == np.int32 and d["fdrp"]["pos"][0] == -1 and (d["fdrp"]["tid"] == tid).all()
    assert (d["fdrp"]["pos"] == t.pos[:, 0]).all() and (bits(d["fdrp"]["fdrp"]) == bits(t.val)).all() and (bits(d["fdrp"]["qfdrp"]) == bits(q.val)).all()
    t, m = ora.pm(min_depth=1), ora.me(min_depth=1)
    g = d["quartet"]
    order = np.lexsort((g["pos"][:, 3], g["pos"][:, 2], g["pos"][:, 1], g["pos"][:, 0]))
    assert g["pos"].dtype == np.int32 and g["pos"][order][0, 0] == -1 and (g["tid"] == tid).all()
    assert (g["pos"][order] == t.pos).all() and (g["cnt"][order] == t.cnt).all() and (bits(g["pm"][order]) == bits(t.val)).all()
    assert np.abs(g["me"][order].astype(np.float64) - m.val).max() <= 1e-6
    t = ora.lpmd(pairs=True)["pairs"]
    g = d["pairs"]
    assert g["pos1"].dtype == np.int32 and (g["pos1"][0], g["pos2"][0]) == (-1, 1) and (g["tid"] == tid).all()
    assert (g["pos1"] == t.pos[:, 0]).all() and (g["pos2"] == t.pos[:, 1]).all() and (bits(g["lpmd"]) == bits(t.val)).all()
    assert (g["n_concordant"] == t.cnt[:, 0]).all() and (g["n_discordant"] == t.cnt[:, 1]).all()


@pytest.mark.parametrize("device", [None, "cuda:0"])
@pytest.mark.parametrize("form", [None, "fused", "split"])
def test_c_abi_single_contig_group(files, device, form):
    """Engine, a group of ONE contig at voff = 4096: every fetch returns position -1 as int32, first in its contig"""
    import metheor_amd
    e = metheor_amd.Engine(0)
    try:
        for tid in (0, 1):
            c, ora = _contig(files, tid)
            h = e.group_define([tid + 5], [BASE])
            bt = util.device_batch(_lifted(c, h), device=device)
            assert ora.pdr(min_depth=1, min_cpgs=1).pos[0, 0] == -1
            ora5 = _retid(files, tid, tid + 5)              # (under the tid the group maps to: the FDRP reservoir is keyed by it)
            _check_rows(_fetch_all(e, bt, form), ora5, tid + 5)
            # the reservoir at site -1 (voff - 1 in the batch): the draw is keyed by the mapped-back (tid + 5, -1)
            bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
            for seed in S.RES_SEEDS:
                e.reset()
                if form is None:
                    e.fdrp_accumulate(bt, seed=seed, **S.RES)
                else:
                    e.multi_accumulate(bt, want=("fdrp",), form=form, min_depth=3, max_depth=3, min_overlap=10, seed=seed)
                d = e.fdrp_fetch()
                t, q = ora5.fdrp(seed=seed, **S.RES), ora5.qfdrp(seed=seed, **S.RES)
                assert d["pos"][0] == -1 and (d["pos"] == t.pos[:, 0]).all() and (d["tid"] == tid + 5).all(), seed
                assert (bits(d["fdrp"]) == bits(t.val)).all() and (bits(d["qfdrp"]) == bits(q.val)).all(), seed
    finally:
        e.close()


def _retid(files, tid, new_tid):
    _, rec, _, _ = files["sorted"]
    sub = rec.subset(np.nonzero(rec.tid == tid)[0])
    sub.refs = [("c%d" % k, 1000) for k in range(new_tid + 1)]
    sub.tid = np.full(len(sub), new_tid, np.int32)
    return pyoracle.Reads.decode(sub)


PLAIN = [(m, d) for m in ("pdr_lpmd", "pdr_lpmd_wide", "pdr_lpmd_runs", "mhl", "fdrp", "quartet", "pairs", "multi", "multi_fused", "prepared")
         for d in (None, "cuda:0")]


@pytest.mark.parametrize("measure,device", PLAIN, ids=["%s-%s" % (m, d or "host") for m, d in PLAIN])
def test_plain_batch_that_carries_the_word(files, device, measure, monkeypatch):
    """a plain batch (region_beg 0) with the word 0x7fffffff: the reference's rows or MTH_ERR_RANGE (-7) -- never fewer rows without an
    error, never MTH_ERR_SPAN.  A host batch is refused before anything is copied or launched.  A device-resident one is found by the
    read index build (k_build_index<2> for the dense PDR + LPMD kernel, <1> for every other pass and for mth_batch_prepare; a launch
    of its own, k_minus_one_check, in the run form that builds no index), which runs in front of the tile kernels -- those see the word:
      dense PDR + LPMD tile / run kernel   packed form: the call's add lands in the last low-margin word of the tile's own LDS row, never
                                           read; 16-bit form: a span violation, the read skips the scatter; no-margin form: clamped to the
                                           lane's trash word
      wide PDR (+ fused ME / PM)           a span violation: the read is skipped for PDR; site insert and quartet window test the position
                                           against the stretch / tile first
      quartet and pairs tile kernels       the window / pair whose first position is outside the tile is not the tile's: returned at once
      MHL tile, count-only and row check   position - P0 >= width: skipped; the row check hands the sites under such a read to the walk,
                                           which only compares positions
      MHL / PDR site walks                 compare positions, index nothing by them
      FDRP walks                           bit_of look-ups clamped to the 403-slot window; the tile form's bit_at tests the range
    so nothing outside a kernel's own tables is touched, and the batch's error is RANGE, reported before SPAN."""
    import metheor_amd
    for k in ("MTH_PDR_WIDE", "MTH_TILE_RUNS"):
        monkeypatch.delenv(k, raising=False)
    if measure in ("pdr_lpmd", "pdr_lpmd_runs"):
        monkeypatch.setenv("MTH_PDR_WIDE", "0")
    if measure == "pdr_lpmd_wide":
        monkeypatch.setenv("MTH_PDR_WIDE", "14")
    if measure == "pdr_lpmd_runs":
        monkeypatch.setenv("MTH_TILE_RUNS", "1")
    c, ora = _contig(files, 0)
    e = metheor_amd.Engine(0)
    prep = None
    try:
        bt = util.device_batch(c, device=device)
        kw = dict(min_depth=1, min_cpgs=1)
        try:
            if measure.startswith("pdr_lpmd"):
                e.pdr_lpmd_accumulate(bt, metheor_amd.PdrLpmdParams(**kw)); got = e.pdr_fetch()["pos"]; want = ora.pdr(**kw).pos[:, 0]
            elif measure.startswith("mhl"):
                e.mhl_accumulate(bt, **kw); got = e.mhl_fetch()["pos"]; want = ora.mhl(**kw).pos[:, 0]
            elif measure == "fdrp":
                e.fdrp_accumulate(bt, min_depth=1, max_depth=64, min_overlap=10); got = e.fdrp_fetch()["pos"]; want = ora.fdrp(min_depth=1, max_depth=64, min_overlap=10).pos[:, 0]
            elif measure == "quartet":
                e.quartet_accumulate(bt); got = np.sort(e.quartet_fetch(min_depth=1)["pos"][:, 0]); want = np.sort(ora.pm(min_depth=1).pos[:, 0])
            elif measure == "pairs":
                e.lpmd_pairs_accumulate(bt); got = e.lpmd_pairs_fetch()["pos1"]; want = ora.lpmd(pairs=True)["pairs"].pos[:, 0]
            elif measure == "prepared":
                prep = e.batch_prepare(bt)
                e.mhl_accumulate(prep, **kw); got = e.mhl_fetch()["pos"]; want = ora.mhl(**kw).pos[:, 0]
            else:
                e.multi_accumulate(bt, want=("pdr", "lpmd", "quartet", "mhl", "fdrp", "pairs"), form="fused" if measure == "multi_fused" else "auto",
                                   max_depth=64, min_overlap=10, **kw)
                got = e.pdr_fetch()["pos"]; want = ora.pdr(**kw).pos[:, 0]
        except metheor_amd.MthError as err:
            assert err.status == -7, err
        else:
            assert len(got) == len(want) and (np.asarray(got) == want).all()
    finally:
        if prep is not None:
            try:
                prep.release()
            except metheor_amd.MthError:
                pass
        e.close()
