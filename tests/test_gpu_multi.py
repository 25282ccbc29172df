"""mth_multi_accumulate (include/metheor_hip.h, "several measures over one batch") and `metheor all`.

The entry point runs every requested measure over ONE batch, prepared once: its rows and the LPMD counters must be those of the single
entry points bit for bit (which the per-measure suites pin against the oracle), and PDR / LPMD also the oracle's here.  `metheor all`
must write, for every output it is given, the bytes the matching single command writes with the same parameters on the same input --
and exit 101 where one of those single runs would."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
ALL7 = ("pdr", "lpmd", "quartet", "mhl", "fdrp", "pairs")
KW = dict(min_depth=3, min_cpgs=2, min_qual=10, min_distance=2, max_distance=16, max_depth=40, min_overlap=35, seed=7)


def _singles(eng, batches, kw=KW):
    from metheor_amd import PdrLpmdParams
    eng.reset()
    for b in batches:
        eng.pdr_lpmd_accumulate(b, PdrLpmdParams(min_depth=kw["min_depth"], min_cpgs=kw["min_cpgs"], min_qual=kw["min_qual"],
                                                 lpmd_min_qual=kw["min_qual"], min_distance=kw["min_distance"], max_distance=kw["max_distance"]))
        eng.quartet_accumulate(b, min_qual=kw["min_qual"])
        eng.mhl_accumulate(b, min_depth=kw["min_depth"], min_cpgs=kw["min_cpgs"], min_qual=kw["min_qual"])
        eng.fdrp_accumulate(b, min_qual=kw["min_qual"], min_depth=kw["min_depth"], max_depth=kw["max_depth"], min_overlap=kw["min_overlap"], seed=kw["seed"])
        eng.lpmd_pairs_accumulate(b, min_distance=kw["min_distance"], max_distance=kw["max_distance"], min_qual=kw["min_qual"])
    return _fetch(eng)


def _fetch(eng, want=ALL7):
    out = {}
    if "pdr" in want:
        out["pdr"] = eng.pdr_fetch()
    if "lpmd" in want:
        out["lpmd"] = eng.lpmd_global()
    if "quartet" in want:
        out["quartet"] = eng.quartet_fetch(min_depth=0)
    if "mhl" in want:
        out["mhl"] = eng.mhl_fetch()
    if "fdrp" in want:
        out["fdrp"] = eng.fdrp_fetch()
    if "pairs" in want:
        out["pairs"] = eng.lpmd_pairs_fetch()
    return out


def _multi(eng, batches, want=ALL7, form="auto", kw=KW):
    eng.reset()
    for b in batches:
        eng.multi_accumulate(b, want=want, form=form, **kw)
    return _fetch(eng, want)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for m in a:
        for k in a[m]:
            x, y = np.asarray(a[m][k]), np.asarray(b[m][k])
            assert x.shape == y.shape, (m, k, x.shape, y.shape)
            if x.dtype.kind == "f":
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (m, k)
            else:
                assert (x == y).all(), (m, k)


def _contigs(rng, kind):
    from metheor_amd import synth
    if kind == "config3":            # config-3-like: a chr1-sized stretch at WGBS density and depth (the wide PDR form)
        return [synth.make_contig(0, 3_000_000, 200_000, 0.0091, rng), synth.make_contig(1, 400_000, 30_000, 0.0091, rng)]
    if kind == "wgbs":
        return [synth.make_contig(0, 1_500_000, 150_000, 0.012, rng)]
    return [synth.make_contig(0, 600_000, 90_000, 0.03, rng), synth.make_contig(1, 200_000, 40_000, 0.05, rng)]   # dense


@pytest.mark.parametrize("kind", ["config3", "wgbs", "dense"])
def test_multi_equals_single_entry_points(kind):
    """three densities x plain host / device-resident / prepared batches x AUTO, FUSED and SPLIT: every measure's rows and the LPMD
    counters equal the single entry points' on the same batches; PDR / LPMD equal the oracle's.  The stats say which form ran: the
    fused tile pass on the sparse batches under AUTO (and on every batch under FUSED), the split form on the dense ones.  (-p 4, the CLI
    default: AUTO fuses where the PDR + LPMD pass takes its wide form, which also depends on how many reads pass min_cpgs.)"""
    import metheor_amd
    from metheor_amd import synth
    rng = np.random.default_rng({"config3": 3, "wgbs": 4, "dense": 5}[kind])
    cs = _contigs(rng, kind)
    eng = metheor_amd.Engine(0)
    try:
        host = [util.device_batch(c) for c in cs]
        dev = [util.device_batch(c, device="cuda:0") for c in cs]
        kw = dict(KW, min_cpgs=4)
        want = _singles(eng, dev, kw)
        assert len(want["pdr"]["pos"]) > 100 and len(want["quartet"]["pos"]) > 100 and len(want["fdrp"]["pos"]) > 100
        prepared = [eng.batch_prepare(b) for b in dev]
        for batches in (host, dev, prepared):
            for form in ("auto", "fused", "split"):
                got = _multi(eng, batches, form=form, kw=kw)
                _same(want, got)
                st = eng.multi_stats()
                fused = form == "fused" or (form == "auto" and kind != "dense")
                assert st["batches_fused"] == (len(cs) if fused else 0) and st["batches_split"] == (0 if fused else len(cs)), (form, st)
                assert (st["tiles_fused"] > 0) == fused and st["tiles_handed_back"] <= st["tiles_fused"], (form, st)
                if fused and kind != "dense":
                    assert st["tiles_handed_back"] < st["tiles_fused"], st
        for p in prepared:
            p.release()
        reads = pyoracle.Reads.from_soa(*synth.concat_oracle_soa(cs))
        o = reads.pdr(min_depth=3, min_cpgs=4, min_qual=10)
        assert (want["pdr"]["pos"] == o.pos[:, 0]).all() and (want["pdr"]["n_concordant"] == o.cnt[:, 0]).all()
        assert (want["pdr"]["n_discordant"] == o.cnt[:, 1]).all()
        ol = reads.lpmd()
        assert all(want["lpmd"][k] == ol[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read"))
    finally:
        eng.close()


def test_fused_hand_back(monkeypatch):
    """every reason a fused tile is handed back to the single ME / PM pass gives the single entry points' rows: more distinct quartets
    than the LDS table holds (a dense batch), more than 65 535 candidate reads in a tile, CpGs >= 2048 bp apart (6-kbp reads at a
    sparse density), and the test knob that hands back every tile"""
    import metheor_amd
    from metheor_amd import synth
    rng = np.random.default_rng(31)
    cases = [("overflow", [synth.make_contig(0, 300_000, 60_000, 0.05, rng)]),
             ("candidates", [synth.make_contig(0, 40_000, 200_000, 0.0091, rng)]),
             ("wide", [synth.make_contig(0, 600_000, 3_000, 0.0003, rng, read_len=6000)]),
             ("knob", [synth.make_contig(0, 900_000, 60_000, 0.0091, rng)])]
    eng = metheor_amd.Engine(0)
    try:
        for name, cs in cases:
            if name == "knob":
                monkeypatch.setenv("MTH_MULTI_FORCE_HANDBACK", "1")
            dev = [util.device_batch(c, device="cuda:0") for c in cs]
            want = _singles(eng, dev) if name != "wide" else None
            sub = ("pdr", "lpmd", "quartet")
            if name == "wide":                     # (FDRP would reproduce the reference's crash on reads of 203..403 bp: not asked for)
                from metheor_amd import PdrLpmdParams
                eng.reset()
                for b in dev:
                    eng.pdr_lpmd_accumulate(b, PdrLpmdParams(min_depth=3, min_cpgs=2))
                    eng.quartet_accumulate(b, min_qual=10)
                want = _fetch(eng, sub)
            else:
                want = {m: want[m] for m in sub}
            got = _multi(eng, dev, want=sub, form="fused")
            _same(want, got)
            st = eng.multi_stats()
            assert st["batches_fused"] == len(cs) and st["tiles_handed_back"] > 0, (name, st)
            if name == "knob":
                assert st["tiles_handed_back"] == st["tiles_fused"]
                monkeypatch.delenv("MTH_MULTI_FORCE_HANDBACK")
            assert len(got["quartet"]["pos"]) > 10, name
    finally:
        eng.close()


def test_multi_subsets_reset_and_refusals():
    """any subset of the measures; several batches in a row, then mth_reset, then again: nothing is left over (and the stats start
    over); an empty or unknown `want` or `form` is refused; an unsorted batch is the call's own error"""
    import metheor_amd
    rng = np.random.default_rng(11)
    cs = _contigs(rng, "dense") + _contigs(rng, "wgbs")
    for k, c in enumerate(cs):
        c["tid"] = k
    eng = metheor_amd.Engine(0)
    try:
        dev = [util.device_batch(c, device="cuda:0") for c in cs]
        want = _singles(eng, dev)
        for sub in (("pdr",), ("lpmd",), ("quartet",), ("mhl", "fdrp"), ("pdr", "lpmd", "pairs"), ("lpmd", "quartet"), ("pdr", "quartet")):
            for form in ("auto", "fused"):
                got = _multi(eng, dev, want=sub, form=form)
                _same({m: want[m] for m in sub}, got)
        got1 = _multi(eng, dev, form="fused")
        eng.reset()
        assert eng.multi_stats() == dict(batches_fused=0, batches_split=0, tiles_fused=0, tiles_handed_back=0)
        got2 = _multi(eng, dev, form="fused")
        _same(want, got1)
        _same(want, got2)
        for form, w in (("auto", ()), (7, ALL7)):
            with pytest.raises(metheor_amd.MthError) as ei:
                eng.multi_accumulate(dev[0], want=w, form=form)
            assert ei.value.status == -1
        c = dict(cs[0])
        rs = c["read_start"].copy(); rs[1000], rs[1001] = rs[1001] + 500, rs[1000]
        c["read_start"] = rs
        for form in ("auto", "fused"):
            eng.reset()
            with pytest.raises(metheor_amd.MthError) as ei:
                eng.multi_accumulate(util.device_batch(c, device="cuda:0"), want=("pdr", "quartet"), form=form)
            assert "sorted" in str(ei.value)
        eng.reset()
        _same(want, _multi(eng, dev))
    finally:
        eng.close()


def test_multi_fuzz():
    """small random jobs (density, depth, read length, parameters): FUSED == SPLIT == the single entry points, bit for bit"""
    import metheor_amd
    from metheor_amd import synth
    eng = metheor_amd.Engine(0)
    fused_tiles = 0
    try:
        for seed in range(50):
            rng = np.random.default_rng(1000 + seed)
            dens = float(rng.choice([0.005, 0.0091, 0.02, 0.05]))
            rl = int(rng.choice([100, 150, 180]))        # (below the 203 bp where FDRP reproduces the reference's panic)
            n = int(rng.integers(200, 6000))
            cs = [synth.make_contig(k, int(rng.integers(20_000, 200_000)), n, dens, rng, read_len=rl) for k in range(int(rng.integers(1, 3)))]
            kw = dict(min_depth=int(rng.integers(0, 6)), min_cpgs=int(rng.integers(1, 6)), min_qual=int(rng.choice([0, 10, 30])),
                      min_distance=int(rng.integers(0, 4)), max_distance=int(rng.choice([8, 16, 40])), max_depth=int(rng.choice([10, 40])),
                      min_overlap=int(rng.choice([10, 35])), seed=seed)
            dev = [util.device_batch(c, device="cuda:0") for c in cs]
            want = _singles(eng, dev, kw)
            _same(want, _multi(eng, dev, form="split", kw=kw))
            _same(want, _multi(eng, dev, form="fused", kw=kw))
            fused_tiles += eng.multi_stats()["tiles_fused"]
        assert fused_tiles > 0
    finally:
        eng.close()


# ---- metheor all ---------------------------------------------------------------------------------------------------------------------
OUT = ("pdr", "lpmd", "mhl", "me", "pm", "fdrp", "qfdrp")
SINGLE_FLAGS = dict(pdr="dpq", lpmd="mMq", mhl="dpq", me="dq", pm="dq", fdrp="qdDl", qfdrp="qdDl")


def run(env, *args):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE, *[str(x) for x in args]], capture_output=True, text=True, cwd=ROOT, timeout=600, env=e)


def check_all(tmp_path, inp, params=None, extra=(), env=None, outs=OUT, pairs=True, expect_rc=0):
    """`metheor all` with `outs` (+ the pairs table) against the single commands: equal bytes per file, equal exit status (0, or 101
    when any single run gives 101), LPMD's stderr line"""
    params = params or {}
    d = tmp_path / ("c%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    args = ["all", "-i", inp] + ["-%s%s" % (f, v) for f, v in params.items()] + list(extra)
    for m in outs:
        args += ["--" + m, d / ("all." + m)]
    if pairs and "lpmd" in outs:
        args += ["--lpmd-pairs", d / "all.pairs"]
    ra = run(env, *args)
    rcs = []
    for m in outs:
        sa = ["-%s%s" % (f, v) for f, v in params.items() if f in SINGLE_FLAGS[m]]
        if m == "lpmd" and pairs:
            sa += ["-p", d / "one.pairs"]
        r = run(env, m, "-i", inp, "-o", d / ("one." + m), *sa, *extra)
        rcs.append(r.returncode)
        if r.returncode == 0 and ra.returncode == 0:
            assert (d / ("all." + m)).read_bytes() == (d / ("one." + m)).read_bytes(), (m, args)
            if m == "lpmd":
                assert r.stderr.splitlines()[0] in ra.stderr.splitlines()
                if pairs:
                    assert (d / "all.pairs").read_bytes() == (d / "one.pairs").read_bytes()
        elif r.returncode == 101:
            assert ra.returncode == 101, (m, ra.stderr)
    want_rc = 101 if 101 in rcs else max(rcs)
    assert ra.returncode == want_rc == expect_rc, (ra.returncode, rcs, ra.stderr)
    return ra


def test_all_cli_golden_fixtures(golden_dir, tmp_path):
    for k in range(1, 7):
        check_all(tmp_path, os.path.join("tests", "golden", "test%d.bam" % k), {"d": 2, "p": 2})
    check_all(tmp_path, os.path.join("tests", "golden", "test1.bam"))                       # the defaults


def test_all_cli_synthetic(tmp_path, golden_dir):
    """a two-contig synthetic BAM (sorted; contig groups), the RRBS SAM fixture given as text, --cpg-set, the host-decode fallback,
    --region from the index, and a noXM input (exit 101 as `pdr` does)"""
    from metheor_amd import hostapi, synth
    rng = np.random.default_rng(21)
    cs = [synth.make_contig(0, 300_000, 40_000, 0.03, rng), synth.make_contig(1, 900_000, 60_000, 0.0091, rng)]
    bam = str(tmp_path / "two.bam")
    hostapi.write_synthetic_bam_multi(bam, cs, ["chrS1", "chrS2"], seed=3, threads=4)
    bamio.write_bai(bam)
    p = {"d": 3, "p": 2, "q": 20, "m": 1, "M": 20, "D": 30, "l": 20}
    check_all(tmp_path, bam, p, env={"METHEOR_SEED": "9"})
    check_all(tmp_path, bam, p, env={"METHEOR_SEED": "9", "METHEOR_HOST_DECODE": "1"})
    check_all(tmp_path, bam, {"d": 2, "p": 1}, extra=("--region", "chrS2:200001-700000"))
    check_all(tmp_path, bam, {"d": 2, "p": 1}, outs=("lpmd",), extra=("-r", "chrS1"))
    reads = pyoracle.Reads.from_soa(*synth.concat_oracle_soa(cs))
    sites = np.unique(reads.soa()["cpg_pos"] & 0x7fffffff)[::3]
    bed = tmp_path / "set.bed"
    bed.write_text("".join("chrS2\t%d\t%d\n" % (s, s + 2) for s in sites))
    check_all(tmp_path, bam, {"d": 2, "p": 1}, extra=("-c", str(bed)))
    sam = os.path.join(golden_dir, "test.chr19.XM.sam")
    check_all(tmp_path, sam, {"d": 2, "p": 2, "l": 10})
    check_all(tmp_path, sam, {"d": 2, "p": 2}, outs=("lpmd", "me"))
    noxm = os.path.join(golden_dir, "test.chr19.noXM.sam")
    check_all(tmp_path, noxm, outs=("pdr", "lpmd"), expect_rc=101)
    # lpmd alone takes lpmd's own XM rule (mapq first): its single run decides
    r = check_all(tmp_path, noxm, outs=("lpmd",), pairs=False, expect_rc=run(None, "lpmd", "-i", noxm, "-o", tmp_path / "x").returncode)
    assert r.returncode in (0, 101)


def test_all_cli_unsorted(tmp_path):
    """a shuffled two-contig BAM: pdr / mhl / fdrp / qfdrp replayed in file order (one replay each; the reservoir is reached: max
    depth 8 under METHEOR_SEED), lpmd / me / pm from the device-sorted stream; and the host-decode fallback (pdr refuses: 101)"""
    from metheor_amd import synth
    rng = np.random.default_rng(23)
    cs = [synth.make_contig(0, 60_000, 9_000, 0.03, rng), synth.make_contig(1, 30_000, 5_000, 0.03, rng)]
    r0, r1 = util.contig_to_records(cs[0], "chrS1"), util.contig_to_records(cs[1], "chrS2")
    rec = bamio.Records([r0.refs[0], r1.refs[0]], np.concatenate([r0.tid, r1.tid + 1]), np.concatenate([r0.pos, r1.pos]),
                        np.concatenate([r0.flag, r1.flag]), np.concatenate([r0.mapq, r1.mapq]), r0.cigars + r1.cigars, r0.xms + r1.xms)
    perm = np.random.default_rng(5).permutation(len(rec.tid))
    sh = bamio.Records(rec.refs, rec.tid[perm], rec.pos[perm], rec.flag[perm], rec.mapq[perm], [rec.cigars[i] for i in perm], [rec.xms[i] for i in perm])
    bam = str(tmp_path / "unsorted.bam")
    bamio.write_bam(bam, sh)
    r = check_all(tmp_path, bam, {"d": 2, "p": 2, "D": 8}, env={"METHEOR_SEED": "5", "METHEOR_TIMING": "1"})
    assert r.stderr.count("file-order replay") == 3 and "device sort by (tid, start)" in r.stderr
    check_all(tmp_path, bam, {"d": 2}, outs=("lpmd", "me", "pm"), env={"METHEOR_HOST_DECODE": "1"})
    check_all(tmp_path, bam, {"d": 2}, outs=("pdr", "lpmd"), env={"METHEOR_HOST_DECODE": "1"}, expect_rc=101)
