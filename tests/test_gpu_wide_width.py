"""The hashed-site tile pass (tile_pass in mth_pdr_wide.hip: k_pdr_lpmd_wide and the fused k_multi_tile) at a NARROWED tile width.

plan_pdr_lpmd (mth_plan.h) narrows the tile below its scratch slice (TileArgs::tile_w_rt) where the last round of workgroups would be less than
half full -- contigs beyond ~29 Mbp, which no other test reaches -- or where MTH_PDR_WIDE_W says so.  Then tile origins are
region_beg + t * width with the width only a multiple of 64, the slice stays 2^shift wide, a stretch redone in halves ends on a piece
that is no power of two, the quartet side owns [T0, T1) of the narrowed tile, and the fine index has less slack behind region_end.

Every comparison is against the CPU oracle: PDR rows, the four LPMD counters and the LPMD f32, quartet keys, histograms and PM bit for
bit; ME and MHL within 1e-6 (the bars of test_gpu_quartet.py / test_gpu_mhl.py); FDRP and qFDRP bit for bit.  The inputs come from
tests/wide_width_util.py; tests/test_wide_width_inputs.py shows on the CPU what they hold."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import util
from tests import wide_width_util as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")

f32 = np.float32
ME_TOL = MHL_TOL = 1e-6
LPMD_KEYS = ("n_concordant", "n_discordant", "n_read", "n_valid_read")
# (PDR keywords, LPMD keywords) of the oracle; the device takes the same numbers
PARAMS = [(dict(min_depth=3, min_cpgs=2, min_qual=10), dict(min_distance=2, max_distance=16, min_qual=10)),
          (dict(min_depth=0, min_cpgs=0, min_qual=0), dict(min_distance=1, max_distance=60, min_qual=0))]
DISCOVERY = [(14, 8960), (15, 23936), (16, 46336)]
KNOBS = ("MTH_PDR_WIDE", "MTH_PDR_WIDE_W", "MTH_TILE_RUNS", "MTH_MHL_WALK", "MTH_MULTI_FORCE_HANDBACK")


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def force(monkeypatch, shift, w):
    monkeypatch.setenv("MTH_PDR_WIDE", str(shift))
    monkeypatch.setenv("MTH_PDR_WIDE_W", str(w))


_cache = {}


def batch(read_len):
    """the boundary batch, its meta data and its oracle reads (built once per module)"""
    key = ("batch", read_len)
    if key not in _cache:
        from metheor_amd import synth
        c, meta = W.boundary_batch(read_len)
        _cache[key] = (c, meta, pyoracle.Reads.from_soa(*synth.to_oracle_soa(c)))
    return _cache[key]


def long_contig(length):
    key = ("long", length)
    if key not in _cache:
        from metheor_amd import synth
        c, _ = W.long_sparse_contig(length, W.narrowed_width(length, 14))
        _cache[key] = (c, pyoracle.Reads.from_soa(*synth.to_oracle_soa(c)))
    return _cache[key]


def oracle(reads, tag, measure, **kw):
    """an oracle table, computed once and shared (never modified)"""
    key = (tag, measure, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = getattr(reads, measure)(**kw)
    return _cache[key]


def pdr_params(pk, lk):
    from metheor_amd import PdrLpmdParams
    return PdrLpmdParams(min_depth=pk["min_depth"], min_cpgs=pk["min_cpgs"], min_qual=pk["min_qual"], lpmd_min_qual=lk["min_qual"],
                         min_distance=lk["min_distance"], max_distance=lk["max_distance"])


def check_pdr_lpmd(p, l, o, ol, what):
    """PDR rows and the LPMD result against the oracle's, bit for bit; the message names the first row that differs"""
    got = np.stack([p["pos"].astype(np.int64), p["n_concordant"].astype(np.int64), p["n_discordant"].astype(np.int64),
                    p["pdr"].view(np.uint32).astype(np.int64)], 1)
    want = np.stack([o.pos[:, 0].astype(np.int64), o.cnt[:, 0].astype(np.int64), o.cnt[:, 1].astype(np.int64),
                     o.val.view(np.uint32).astype(np.int64)], 1)
    n = min(len(got), len(want))
    bad = np.nonzero((got[:n] != want[:n]).any(1))[0]
    first = int(bad[0]) if len(bad) else (n if len(got) != len(want) else -1)
    assert first < 0, (what, "rows", len(got), len(want), "first difference at row", first,
                       got[first].tolist() if first < len(got) else None, want[first].tolist() if first < len(want) else None)
    assert (p["tid"] == o.tid).all()
    gl, wl = tuple(int(l[k]) for k in LPMD_KEYS), tuple(int(ol[k]) for k in LPMD_KEYS)
    assert gl == wl, (what, LPMD_KEYS, gl, wl)                # n_read / n_valid_read: a read owned twice or by no tile shows here
    a, b = f32(l["lpmd"]), f32(ol["lpmd"])
    assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32), (what, a, b)


def check_quartets(d, om, op, what):
    """quartet keys, 16-bin histograms and PM bit for bit, ME within ME_TOL"""
    assert len(d["tid"]) == len(om) == len(op), (what, len(d["tid"]), len(om))
    order = np.lexsort((d["pos"][:, 3], d["pos"][:, 2], d["pos"][:, 1], d["pos"][:, 0], d["tid"]))
    assert (d["pos"][order] == om.pos).all() and (d["tid"][order] == om.tid).all(), what
    assert (d["cnt"][order] == om.cnt).all(), what
    assert (d["pm"][order].view(np.uint32) == op.val.view(np.uint32)).all(), what
    diff = np.abs(d["me"][order].astype(np.float64) - om.val.astype(np.float64))
    assert len(diff) == 0 or diff.max() <= ME_TOL, (what, diff.max())


def region_batches(c, regs, device="cuda:0"):
    from metheor_amd import shard
    return [util.device_batch(shard.slice_region(c, b, e), region=(b, e), device=device) for b, e in regs]


def ceil_div(a, b):
    return -(-a // b)


# ---- a. PDR + LPMD at every forced width -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len", [150, 300])
@pytest.mark.parametrize("shift,w", W.FORCED)
def test_forced_width_pdr_lpmd(eng, monkeypatch, shift, w, read_len):
    """the whole contig as one host batch and, for the 150-bp batch, as device-resident region batches whose cuts lie off every grid
    (the pipelined lanes), under two parameter sets.  300-bp reads: 16-bit relative positions, and PDR by the exact walk, whose site
    discovery and LPMD-only launch both go through the wide form."""
    force(monkeypatch, shift, w)
    c, meta, reads = batch(read_len)
    if read_len == 300:
        assert c["cpg_rel"].dtype == np.uint16 and int((c["read_end"] - c["read_start"]).max()) + 1 > 256
    tag = "b%d" % read_len
    for pk, lk in PARAMS:
        o, ol = oracle(reads, tag, "pdr", **pk), oracle(reads, tag, "lpmd", **lk)
        assert len(o) > 5000 and ol["n_concordant"] > 10_000 and ol["n_read"] == len(c["read_start"])
        eng.reset()
        eng.pdr_lpmd_accumulate(util.device_batch(c, region=(0, meta["length"])), pdr_params(pk, lk))
        check_pdr_lpmd(eng.pdr_fetch(), eng.lpmd_global(), o, ol, ("host", shift, w, read_len, pk))
        if read_len == 150:
            regs = W.off_grid_regions(meta["length"], w)
            eng.reset()
            keep = region_batches(c, regs)
            for bt in keep:
                eng.pdr_lpmd_accumulate(bt, pdr_params(pk, lk))
            check_pdr_lpmd(eng.pdr_fetch(), eng.lpmd_global(), o, ol, ("regions", shift, w, regs, pk))


# ---- b. the fused pass of `metheor all` --------------------------------------------------------------------------------------------
FUSED_KW = dict(min_depth=3, min_cpgs=2, min_qual=10, min_distance=2, max_distance=16)


def run_fused(eng, batches, form="fused", kw=FUSED_KW):
    eng.reset()
    for bt in batches:
        eng.multi_accumulate(bt, want=("pdr", "lpmd", "quartet"), form=form, **kw)
    return eng.pdr_fetch(), eng.lpmd_global(), eng.quartet_fetch(min_depth=0), eng.multi_stats()


def fused_oracle(reads, tag, kw=FUSED_KW):
    return (oracle(reads, tag, "pdr", min_depth=kw["min_depth"], min_cpgs=kw["min_cpgs"], min_qual=kw["min_qual"]),
            oracle(reads, tag, "lpmd", min_distance=kw["min_distance"], max_distance=kw["max_distance"], min_qual=kw["min_qual"]),
            oracle(reads, tag, "me", min_depth=0, min_qual=kw["min_qual"]), oracle(reads, tag, "pm", min_depth=0, min_qual=kw["min_qual"]))


def fused_tiles(regs, w):
    """(batches, tiles) the fused kernel takes: a batch whose tiles fit the pass's tile-row table (region_len / 8192 + 2 rows)"""
    nt = [ceil_div(e - b, w) for b, e in regs if ceil_div(e - b, w) <= (e - b) // 8192 + 2]
    return len(nt), sum(nt)


@pytest.mark.parametrize("shift,w", W.FORCED)
def test_forced_width_fused(eng, monkeypatch, shift, w):
    """PDR, LPMD and ME / PM of multi_accumulate's fused form against the oracle, on the whole contig and on the off-grid regions; the
    tile count of multi_stats proves that the width was in effect.  Below 8192 the whole contig has more tiles than the fused pass's
    table: the wide kernel and the single ME / PM pass run instead, with the same rows."""
    force(monkeypatch, shift, w)
    c, meta, reads = batch(150)
    o, ol, om, op = fused_oracle(reads, "b150")
    assert len(om) > 4000
    length = meta["length"]
    for regs in ([(0, length)], W.off_grid_regions(length, w)):
        p, l, q, st = run_fused(eng, region_batches(c, regs))
        check_pdr_lpmd(p, l, o, ol, ("fused", shift, w, regs))
        check_quartets(q, om, op, ("fused", shift, w, regs))
        nb, nt = fused_tiles(regs, w)
        assert st["batches_fused"] == nb and st["batches_split"] == len(regs) - nb and st["tiles_fused"] == nt, (w, regs, st)
        if w >= 8192:
            assert nb == len(regs) and nt == sum(ceil_div(e - b, w) for b, e in regs)
        elif len(regs) == 1:
            assert st["tiles_fused"] == 0
        if w == W.SPECIAL_W and len(regs) == 1:
            assert 0 < st["tiles_handed_back"] < st["tiles_fused"], st           # the dense stretch: more quartets than the table holds


def test_forced_width_fused_hand_back(eng, monkeypatch):
    """every narrowed tile handed back to the single ME / PM pass: the same rows"""
    force(monkeypatch, 14, W.SPECIAL_W)
    monkeypatch.setenv("MTH_MULTI_FORCE_HANDBACK", "1")
    c, meta, reads = batch(150)
    o, ol, om, op = fused_oracle(reads, "b150")
    p, l, q, st = run_fused(eng, region_batches(c, [(0, meta["length"])]))
    check_pdr_lpmd(p, l, o, ol, "hand-back")
    check_quartets(q, om, op, "hand-back")
    assert st["tiles_fused"] == ceil_div(meta["length"], W.SPECIAL_W) and st["tiles_handed_back"] == st["tiles_fused"], st


# ---- c. the wide form as the site-discovery pass -----------------------------------------------------------------------------------
@pytest.mark.parametrize("consumer", ["mhl_walk", "fdrp", "pdr_exact"])
@pytest.mark.parametrize("shift,w", DISCOVERY)
def test_forced_width_site_discovery(eng, monkeypatch, shift, w, consumer):
    """the measures that start from the wide form's site list, one case each: MHL in its walk form (MTH_MHL_WALK=1; its default tile
    pass finds its sites itself, it runs here too), FDRP / qFDRP on a batch with more than two calls per read (site discovery, then the
    walk), both on the 150-bp batch; PDR by the exact walk on the 300-bp batch"""
    force(monkeypatch, shift, w)
    if consumer == "mhl_walk":
        c, meta, reads = batch(150)
        bt = util.device_batch(c, region=(0, meta["length"]), device="cuda:0")
        o = oracle(reads, "b150", "mhl", min_depth=3, min_cpgs=2)
        assert len(o) > 5000
        for walk in (True, False):
            if walk:
                monkeypatch.setenv("MTH_MHL_WALK", "1")
            else:
                monkeypatch.delenv("MTH_MHL_WALK")
            eng.reset()
            eng.mhl_accumulate(bt, min_depth=3, min_cpgs=2)
            d = eng.mhl_fetch()
            assert len(d["pos"]) == len(o) and (d["pos"] == o.pos[:, 0]).all(), ("mhl", walk, len(d["pos"]), len(o))
            assert np.abs(d["mhl"].astype(np.float64) - o.val).max() <= MHL_TOL
    elif consumer == "fdrp":
        c, meta, reads = batch(150)
        assert float(c["cpg_off"][-1]) / len(c["read_start"]) > 2.0          # (FDRP's one-pass tile form is not taken)
        bt = util.device_batch(c, region=(0, meta["length"]), device="cuda:0")
        of, oq = oracle(reads, "b150", "fdrp", min_depth=2), oracle(reads, "b150", "qfdrp", min_depth=2)
        assert len(of) > 5000
        eng.reset()
        eng.fdrp_accumulate(bt, min_depth=2)
        d = eng.fdrp_fetch()
        assert len(d["pos"]) == len(of) and (d["pos"] == of.pos[:, 0]).all(), ("fdrp", len(d["pos"]), len(of))
        assert (d["fdrp"].view(np.uint32) == of.val.view(np.uint32)).all() and (d["qfdrp"].view(np.uint32) == oq.val.view(np.uint32)).all()
    else:
        # the exact PDR walk: only batches with spans beyond 150 take it -- this one must
        c3, meta3, reads3 = batch(300)
        bt3 = util.device_batch(c3, region=(0, meta3["length"]), device="cuda:0")
        assert c3["cpg_rel"].dtype == np.uint16 and bt3.c.max_span > 150 and bt3.c.cpg_rel16 and not bt3.c.cpg_rel
        pk, lk = PARAMS[0]
        eng.timing_enable(True)
        eng.timing_reset()
        eng.reset()
        eng.pdr_lpmd_accumulate(bt3, pdr_params(pk, lk))
        p, l = eng.pdr_fetch(), eng.lpmd_global()
        t = eng.timing()
        eng.timing_enable(False)
        eng.timing_reset()
        ran = {k for k, v in t.items() if v[1] > 0}
        assert "k_pdr_walk" in ran and "k_pdr_lpmd_wide" in ran and "k_pdr_lpmd_tile" not in ran, t
        check_pdr_lpmd(p, l, oracle(reads3, "b300", "pdr", **pk), oracle(reads3, "b300", "lpmd", **lk), ("exact walk", shift, w))


# ---- d. the width the host chooses by itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [32_000_000, 40_000_000, 45_000_000])
def test_chooser_narrows_long_contigs(eng, length):
    """nothing forced: contigs of 32 and 40 Mbp take 8960- and 11200-position tiles by plan_pdr_lpmd's own rule (1.09 and 1.36 rounds
    of 16384-position tiles over 1792 workgroups), one of 45 Mbp (1.53 rounds) keeps 16384.  The fused pass's tile count says which
    width ran; the plain PDR + LPMD call on the same batch must run k_pdr_lpmd_wide alone."""
    assert "MTH_PDR_WIDE" not in os.environ and "MTH_PDR_WIDE_W" not in os.environ
    width = W.narrowed_width(length, 14)
    assert width == {32_000_000: 8960, 40_000_000: 11200, 45_000_000: 0}[length]
    c, reads = long_contig(length)
    tag = "long%d" % length
    kw = dict(FUSED_KW, min_cpgs=4)
    o, ol, om, op = fused_oracle(reads, tag, kw)
    assert len(o) >= 300 and len(om) >= 100
    bt = util.device_batch(c, region=(0, length), device="cuda:0")
    p, l, q, st = run_fused(eng, [bt], form="auto", kw=kw)
    check_pdr_lpmd(p, l, o, ol, ("chooser, fused", length))
    check_quartets(q, om, op, ("chooser, fused", length))
    assert st["batches_fused"] == 1 and st["batches_split"] == 0, st
    if width:
        assert st["tiles_fused"] == ceil_div(length, width) > ceil_div(length, 16384), (st, width)
    else:
        assert st["tiles_fused"] == ceil_div(length, 16384), st
    eng.timing_enable(True)
    eng.timing_reset()
    eng.reset()
    eng.pdr_lpmd_accumulate(bt, pdr_params(dict(min_depth=3, min_cpgs=4, min_qual=10), dict(min_distance=2, max_distance=16, min_qual=10)))
    p, l = eng.pdr_fetch(), eng.lpmd_global()
    t = eng.timing()
    eng.timing_enable(False)
    eng.timing_reset()
    assert {k for k, v in t.items() if v[1] > 0 and k.startswith("k_pdr_lpmd")} == {"k_pdr_lpmd_wide"}, t
    check_pdr_lpmd(p, l, o, ol, ("chooser, plain", length))


# ---- e. the command line -----------------------------------------------------------------------------------------------------------
def test_forced_width_cli(tmp_path):
    """`metheor all` on the 150-bp batch as a BAM, in child processes with and without a narrowed width in their environment: every
    output byte for byte the same, and every output of the narrowed run the oracle's text (PDR, LPMD, PM and MHL's sites byte for byte;
    ME and MHL values within 1e-6) -- a knob the child ignored could satisfy the first half alone, a wrong narrowed tile neither"""
    from metheor_amd import hostapi
    from oracle import bamio
    c, meta, reads = batch(150)
    bam = str(tmp_path / "wide.bam")
    hostapi.write_synthetic_bam_multi(bam, [c], ["chrW"], seed=3, threads=4)
    bamio.write_bai(bam)
    outs = ("pdr", "lpmd", "me", "pm", "mhl")
    got = {}
    for name, env in (("narrow", {"MTH_PDR_WIDE": "14", "MTH_PDR_WIDE_W": str(W.SPECIAL_W)}), ("plain", {})):
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env)
        d = tmp_path / name
        d.mkdir()
        args = [EXE, "all", "-i", bam, "-d3", "-p2"]
        for m in outs:
            args += ["--" + m, str(d / m)]
        r = subprocess.run(args, capture_output=True, text=True, cwd=ROOT, timeout=300, env=e)
        assert r.returncode == 0, (name, r.stderr)
        got[name] = {m: (d / m).read_text() for m in outs}
    flags = dict(pdr=["-d", "3", "-p", "2"], mhl=["-d", "3", "-p", "2"], me=["-d", "3"], pm=["-d", "3"], lpmd=[])
    for m in outs:
        want, _ = util.oracle_text(reads, ["chrW"], m, input_name=bam, **util.oracle_kwargs(m, flags[m]))
        assert want.count("\n") > (1 if m == "lpmd" else 1000), m
        if m == "mhl":                                 # positions byte for byte, the value within MHL_TOL
            g, w_ = [x.split("\t") for x in got["narrow"][m].splitlines()], [x.split("\t") for x in want.splitlines()]
            assert len(g) == len(w_) and all(a[:3] == b[:3] and abs(float(a[3]) - float(b[3])) <= MHL_TOL for a, b in zip(g, w_)), m
        else:
            util.assert_tsv_equals_oracle(m, got["narrow"][m], want)
    for m in outs:
        assert got["narrow"][m] == got["plain"][m] and len(got["plain"][m]) > 0, m
