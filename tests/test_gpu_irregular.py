"""GPU parity on irregular reads (tests/irregular_util.py): clipped, gapped, long-query and shifted-flag reads, CpG sites one
position apart, calls far apart in site rank -- every measure in every forced kernel form against the CPU oracle, with the
per-measure suites' check functions and bars (integers and PDR / LPMD / PM / FDRP / qFDRP floats bit for bit where they are
there; ME and MHL within 1e-6).  synth.make_contig, which every other randomized GPU test draws from, makes none of these."""
import contextlib
import os

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import irregular_util as I
from tests import test_gpu_fdrp as T_fdrp
from tests import test_gpu_fuzz as T_fuzz
from tests import test_gpu_mhl as T_mhl
from tests import test_gpu_multi as T_multi
from tests import test_gpu_pairs as T_pairs
from tests import test_gpu_pdr_lpmd as T_pdr
from tests import test_gpu_quartet as T_quartet
from tests import util

pytestmark = pytest.mark.gpu
PDR_FORMS = ({"MTH_PDR_WIDE": "14"}, {"MTH_PDR_WIDE": "15"}, {"MTH_PDR_WIDE": "16"}) + T_fuzz.pdr_env_forms(0)[1:]
WTILE_FORMS = ({"METHEOR_FDRP_WTILE": "1"}, {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_SUB": "1"},
               {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_HEAVY": "1"}, {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_W": "64"},
               {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_W": "128"}, {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_W": "256"})


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def pdr_lpmd_every_form(eng, cs, reads, pk, lk, rel16s=(False, True)):
    """PDR + LPMD against the oracle in the engine's own choice and every forced form, both widths of cpg_rel"""
    from metheor_amd import PdrLpmdParams
    p = PdrLpmdParams(min_distance=lk["min_distance"], max_distance=lk["max_distance"], lpmd_min_qual=lk["min_qual"], **pk)
    for rel16 in rel16s:
        for form in ({},) + PDR_FORMS:
            with env(**form):
                d, l = T_pdr.run_device(eng, cs, p, rel16=rel16)
            T_pdr.check_against_oracle(d, l, reads, pk, lk)


def fdrp_named(dev, reads, fk, what):
    """T_fdrp.check, after naming the first row that differs (the assertion alone says only that one does)"""
    of, oq = reads.fdrp(**fk), reads.qfdrp(**fk)
    if len(dev["pos"]) == len(of):
        bad = np.nonzero((dev["pos"] != of.pos[:, 0]) | (dev["n_reads"] != of.cnt[:, 0]) |
                         ~((dev["fdrp"] == of.val) | (np.isnan(dev["fdrp"]) & np.isnan(of.val))) |
                         ~((dev["qfdrp"] == oq.val) | (np.isnan(dev["qfdrp"]) & np.isnan(oq.val))))[0]
        assert len(bad) == 0, "%s: %d rows differ, first at pos %d: device (fdrp %r, qfdrp %r, reads %d), oracle (%r, %r, %d)" % (
            what, len(bad), int(of.pos[bad[0], 0]), float(dev["fdrp"][bad[0]]), float(dev["qfdrp"][bad[0]]), int(dev["n_reads"][bad[0]]),
            float(of.val[bad[0]]), float(oq.val[bad[0]]), int(of.cnt[bad[0], 0]))
    T_fdrp.check(dev, reads, fk)


def fdrp_every_form(eng, cs, reads, fk, forms=WTILE_FORMS):
    """test_gpu_fuzz.fdrp_checked (AUTO against the oracle, seven forced forms against AUTO), then the tile pass's own forms against
    the oracle"""
    T_fuzz.fdrp_checked(eng, cs, fk, None, reads)
    for form in forms:
        with env(**form):
            fdrp_named(T_fdrp.run_device(eng, cs, fk), reads, fk, form)


def multi_every_form(eng, cs, reads, kw):
    """Engine.multi_accumulate in AUTO / FUSED / SPLIT equals the single entry points (test_gpu_multi), which equal the oracle here"""
    dev = [util.device_batch(c, device="cuda:0") for c in cs]
    want = T_multi._singles(eng, dev, kw)
    pk = dict(min_depth=kw["min_depth"], min_cpgs=kw["min_cpgs"], min_qual=kw["min_qual"])
    lk = dict(min_distance=kw["min_distance"], max_distance=kw["max_distance"], min_qual=kw["min_qual"])
    T_pdr.check_against_oracle(want["pdr"], want["lpmd"], reads, pk, lk)
    T_pairs.check(want["pairs"], reads, lk)
    T_quartet.check(want["quartet"], reads, kw["min_qual"], 0)
    T_mhl.check(want["mhl"], reads, pk)
    T_fdrp.check(want["fdrp"], reads, dict(min_qual=kw["min_qual"], min_depth=kw["min_depth"], max_depth=kw["max_depth"],
                                           min_overlap=kw["min_overlap"], seed=kw["seed"]))
    for form in ("auto", "fused", "split"):
        T_multi._same(want, T_multi._multi(eng, dev, form=form, kw=kw))


def all_measures(eng, rec, rng, fdrp_cap):
    reads, cs = I.contigs(rec)
    mq = int(rng.choice([0, 10, 10, 30]))
    pk = dict(min_depth=int(rng.choice([0, 1, 3])), min_cpgs=int(rng.choice([0, 1, 2, 4])), min_qual=mq)
    lk = dict(min_distance=int(rng.choice([0, 1, 2, 3, 5])), max_distance=int(rng.choice([2, 8, 16, 40, 300])), min_qual=mq)
    pdr_lpmd_every_form(eng, cs, reads, pk, lk, rel16s=(bool(rng.integers(0, 2)),))
    T_pairs.check(T_pairs.run_device(eng, cs, lk), reads, lk)
    qd = int(rng.choice([0, 2]))
    T_quartet.check(T_quartet.run_device(eng, cs, mq, qd), reads, mq, qd)
    mk = dict(min_depth=int(rng.choice([0, 1, 3])), min_cpgs=int(rng.choice([1, 2, 4])), min_qual=mq)
    m0 = T_mhl.run_device(eng, cs, mk)
    T_mhl.check(m0, reads, mk)
    T_fuzz.mhl_forms_same(eng, cs, mk, None, m0)
    frec = I.fdrp_safe(rec, fdrp_cap)
    freads, fcs = I.contigs(frec)
    fk = dict(min_qual=mq, min_depth=int(rng.choice([0, 2, 3])), max_depth=int(rng.choice([8, 40, 64])),
              min_overlap=int(rng.choice([0, 1, 35])), seed=int(rng.integers(0, 1 << 30)))
    fdrp_every_form(eng, fcs, freads, fk, forms=WTILE_FORMS[2:4] if fdrp_cap else ())
    kw = dict(min_depth=pk["min_depth"], min_cpgs=max(1, pk["min_cpgs"]), min_qual=mq, min_distance=lk["min_distance"],
              max_distance=lk["max_distance"], max_depth=fk["max_depth"], min_overlap=fk["min_overlap"], seed=fk["seed"])
    multi_every_form(eng, fcs, freads, kw)
    return reads


@pytest.mark.parametrize("seed", range(32))
def test_irregular_fuzz(eng, seed):
    """every measure, every forced form, on seeded irregular input (each knob on with probability 0.8); FDRP on the records without
    the reference's panic, and on even seeds without the reads spanning > 200 bp either (the tile pass takes only those batches)"""
    rng = np.random.default_rng(500 + seed)
    knobs = {k: bool(rng.random() < 0.8) for k in I.KNOBS}
    rec, _ = I.make_records(7000 + seed, n_contigs=int(rng.integers(1, 3)), length=int(rng.integers(4_000, 16_000)),
                            n_reads=int(rng.integers(200, 1_800)), density=float(rng.choice([0.01, 0.03, 0.06])), **knobs)
    all_measures(eng, rec, rng, 200 if seed % 2 == 0 else None)


# ---- targeted cases --------------------------------------------------------------------------------------------------------------
def _pair_read(pos, flag, lead, gap_op, gap, d_rel, meth, tail_m=40):
    """two calls d_rel query bases apart with an `gap_op` of `gap` between them (after `lead` soft-clipped bases); -> row"""
    x1 = 30
    ops = ([("S", lead)] if lead else []) + [("M", x1), (gap_op, gap), ("M", tail_m)]
    qlen = sum(n for op, n in ops if op in "MIS")
    q1 = lead + x1 - 1
    q2 = q1 + d_rel
    xm = ["."] * qlen
    xm[q1] = "Z" if meth[0] else "z"
    xm[q2] = "Z" if meth[1] else "z"
    assert ops[-1][0] == "M" and q2 >= qlen - tail_m
    return (0, pos, flag, 42, ops, "".join(xm))


def test_lpmd_by_query_offset(eng):
    """LPMD counts a pair when min_distance <= the QUERY-offset distance <= max_distance (readutil.rs:184-196: relpos counts soft
    clips and insertions, not deletions), whatever the positions say.  Pins the forms that read cpg_rel -- k_pdr_lpmd_tile,
    k_pdr_lpmd_runs, k_pdr_lpmd_wide, the pairs table, k_multi_tile -- at distance min - 1, min, max and max + 1 with the position
    distance on the other side of the bound: an I between the calls, a D between them, a leading S"""
    for m, M in ((2, 16), (3, 8), (5, 40)):
        rows, at = [], 1000
        pats = [("I", 3, M + 1), ("I", M, M + 1), ("D", 7, M), ("D", 1, M), ("I", 1, m), ("I", 2, m + 1), ("D", 4, m - 1), ("D", 2, m),
                ("N", 30, M), ("I", 5, M)]
        for lead in (0, 25, 200):
            for gap_op, gap, d_rel in pats:
                if gap_op == "I" and d_rel < gap + 1:
                    continue
                for k, fl in enumerate((0, 16, 97, 99, 163, 0)):
                    rows.append(_pair_read(at + (k % 2), fl, lead, gap_op, gap, d_rel, (k % 3 != 0, k % 2 == 0)))
                at += 400
        rec = I.records_from_rows([("chrL", at + 1000)], sorted(rows, key=lambda r: r[1]))
        reads, cs = I.contigs(rec)
        lk = dict(min_distance=m, max_distance=M, min_qual=10)
        pk = dict(min_depth=1, min_cpgs=1, min_qual=10)
        l = reads.lpmd(**lk)
        assert l["n_concordant"] > 0 and l["n_discordant"] > 0
        soa = reads.soa()                               # the position rule would count otherwise: the case discriminates
        off = soa["cpg_off"].astype(np.int64)
        pos = (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
        by_pos = sum(int(m <= pos[off[i] + 1] - pos[off[i]] <= M) for i in range(len(off) - 1) if off[i + 1] - off[i] == 2)
        assert by_pos != l["n_concordant"] + l["n_discordant"]
        pdr_lpmd_every_form(eng, cs, reads, pk, lk)
        T_pairs.check(T_pairs.run_device(eng, cs, lk), reads, lk)
        dev = [util.device_batch(c, device="cuda:0") for c in cs]
        for form in ("fused", "auto", "split"):                # (the fused pass is PDR + LPMD + ME / PM: k_multi_tile)
            eng.reset()
            for b in dev:
                eng.multi_accumulate(b, want=("pdr", "lpmd", "quartet", "pairs"), form=form, min_depth=1, min_cpgs=1, min_qual=10,
                                     min_distance=m, max_distance=M)
            T_pdr.check_against_oracle(eng.pdr_fetch(), eng.lpmd_global(), reads, pk, lk)
            T_pairs.check(eng.lpmd_pairs_fetch(), reads, lk)
            T_quartet.check(eng.quartet_fetch(min_depth=0), reads, 10, 0)
            if form == "fused":
                assert eng.multi_stats()["tiles_fused"] > 0


def test_u16_rel_on_the_fast_forms(eng):
    """query offsets above 255 on reads spanning <= 150 bp (cpg_rel is 16 bits wide in such a batch): the dense tile, run, wide and
    fused forms take the pairs' distances from all 16 bits -- some pairs straddle offset 255 / 256"""
    rng = np.random.default_rng(5)
    sites = np.arange(1003, 9000, 6)
    rows = []
    for s in np.sort(rng.integers(1000, 8500, size=900)):
        s = int(s)
        lead = int(rng.integers(150, 240)) if rng.random() < 0.7 else int(rng.integers(0, 20))
        sp = int(rng.integers(60, 151))
        ops = ([("S", lead)] if lead else []) + ([("M", sp)] if rng.random() < 0.6 else [("M", sp // 2), ("I", int(rng.integers(1, 25))), ("M", sp - sp // 2)])
        ops.append(("S", int(rng.integers(1, 30))))
        fl = int(rng.choice([0, 16, 99, 147]))
        xm = I.xm_for(s, fl, ops, set(int(x) for x in sites), lambda c: 0.5 if (c // 6) % 3 else 0.9, rng)
        rows.append((0, s, fl, 42 if rng.random() < 0.9 else 3, ops, xm))
    rec = I.records_from_rows([("chrU", 10_000)], rows)
    reads, cs = I.contigs(rec)
    assert cs[0]["cpg_rel"].dtype == np.uint16 and int(cs[0]["cpg_rel"].max()) > 300
    for lk in (dict(min_distance=2, max_distance=16, min_qual=10), dict(min_distance=1, max_distance=40, min_qual=10),
               dict(min_distance=0, max_distance=300, min_qual=10)):
        pk = dict(min_depth=2, min_cpgs=2, min_qual=10)
        pdr_lpmd_every_form(eng, cs, reads, pk, lk, rel16s=(False,))
        T_pairs.check(T_pairs.run_device(eng, cs, lk), reads, lk)
    multi_every_form(eng, cs, reads, dict(min_depth=2, min_cpgs=2, min_qual=10, min_distance=2, max_distance=16, max_depth=40,
                                          min_overlap=20, seed=3))


def test_mixed_spans_across_the_pdr_flush_margin(eng):
    """reads of 36..240 bp in one batch, either side of PDR_FLUSH_MARGIN = 150 (pdr.rs:160-177): the tile form for spans <= 150 and
    k_pdr_walk beyond, in every form; the same reads cut to spans <= 150 take the tile form for PDR too"""
    rec, _ = I.make_records(77, n_contigs=2, length=9_000, n_reads=1_500, density=0.05,
                            **{k: k in ("mixed_len", "piles", "drops", "low_mapq") for k in I.KNOBS})
    soa = pyoracle.Reads.decode(rec).soa()
    span = soa["end"].astype(np.int64) - soa["start"] + 1
    assert (span > 150).any() and (span <= 150).any()
    for r in (rec, rec.subset(np.nonzero(span <= 150)[0])):
        reads, cs = I.contigs(r)
        for pk in (dict(min_depth=0, min_cpgs=0, min_qual=10), dict(min_depth=3, min_cpgs=2, min_qual=10)):
            pdr_lpmd_every_form(eng, cs, reads, pk, dict(min_distance=2, max_distance=16, min_qual=10))


def _aliasing_records():
    """CG repeats (a site every 2 bp), 2000 bp apart; over each, two-call filler reads at every site (all methylated; each site has
    two readers, plus one) and ONE test read with two unmethylated calls k window ranks apart and none between"""
    rows, islands = [], []
    base = 1000
    for k in (33, 40, 47, 65, 15, 16, 32, 48):
        n = k + 8
        sites = base + 2 * np.arange(n)
        for j in range(n - 1):                                    # filler: calls sites j, j + 1 ("3M", methylated)
            rows.append((0, int(sites[j]), 0, 42, [("M", 3)], "Z.Z"))
        r0 = 3
        span = 2 * k + 1
        xm = ["."] * span
        xm[0] = xm[-1] = "z"
        rows.append((0, int(sites[r0]), 0, 42, [("M", span)], "".join(xm)))
        islands.append((k, int(sites[r0]), int(sites[r0 + k])))
        base += 2000
    rows.sort(key=lambda r: r[1])
    return I.records_from_rows([("chrA", base + 1000)], rows), islands


@pytest.mark.parametrize("form", ["wtile", "wtile_sub", "auto"])
def test_wtile_rank_aliasing(eng, form):
    """k_fdrp_wtile keeps a reader's calls as a 32-bit mask, bit = window rank mod 32, and hands back the sites of a reader spanning
    > 16 window sites.  That span must come from the read's true first and last call rank: read off the folded mask, calls 33, 40, 47
    or 65 ranks apart look 1..15 apart, and the reader is listed at a site it does not call (and not at one it does).  Controls at
    15 (computed here), 16, 32 and 48 (handed back).  Each site has <= 3 readers."""
    rec, islands = _aliasing_records()
    reads, cs = I.contigs(rec)
    fk = dict(min_qual=10, min_depth=2, max_depth=40, min_overlap=0, seed=1)
    of = reads.fdrp(**fk)
    for k, a, b in islands:                                         # the test read's sites have rows, discordant ones
        for p in (a, b):
            i = np.searchsorted(of.pos[:, 0], p)
            assert of.pos[i, 0] == p and of.val[i] > 0, (k, p)
    e = {"wtile": {"METHEOR_FDRP_WTILE": "1"}, "wtile_sub": {"METHEOR_FDRP_WTILE": "1", "METHEOR_FDRP_WTILE_SUB": "1"}, "auto": {}}[form]
    with env(**e):
        fdrp_named(T_fdrp.run_device(eng, cs, fk), reads, fk, form)


def _island_records(seed=9):
    """the issue's instance: 60 reads of 100 bp over a 200-bp CG repeat, flags {0, 97, 1123, 16, 83} (sites at p - 1 next to p),
    plus the generator's islands with shifted flags and dropped calls"""
    rng = np.random.default_rng(seed)
    a = 2000
    sites = set(range(a, a + 200, 2))
    lv = lambda c: 0.8 if (c // 2) % 3 else 0.2
    rows = []
    for s in np.sort(rng.integers(a - 20, a + 120, size=60)):
        fl = int(rng.choice([0, 97, 1123, 16, 83]))
        rows.append((0, int(s), fl, 42, [("M", 100)], I.xm_for(int(s), fl, [("M", 100)], sites, lv, rng,
                                                              drop=int(rng.integers(5, 40)) if rng.random() < 0.5 else None)))
    for s in np.sort(rng.integers(a - 20, a + 190, size=120)):            # short reads with few calls: the tile pass computes them
        fl = int(rng.choice([0, 97, 1123, 16, 83, 147]))
        rows.append((0, int(s), fl, 42, [("M", 6)], I.xm_for(int(s), fl, [("M", 6)], sites, lv, rng)))
    rows.sort(key=lambda r: r[1])
    r1 = I.records_from_rows([("chrJ", 5000)], rows)
    r2, _ = I.make_records(seed, length=8_000, n_reads=900, density=0.02,
                           **{k: k in ("islands", "shifted", "drops", "piles") for k in I.KNOBS})
    return r1, r2


@pytest.mark.parametrize("which", [0, 1])
def test_adjacent_sites_every_form(eng, which):
    """CpG sites one position apart: > 32 sites in 48 positions (k_fdrp_wtile halves a stretch down to FW_SC positions, which can
    hold no more -- it used to stop at 48 and never leave the loop), > W / 2 sites in a tile of 64..256 positions (W rows a tile:
    W / 2 overflowed); every measure, every form, the tile pass's count-only path included"""
    rec = _island_records()[which]
    reads, cs = I.contigs(rec)
    pos = I.called_sites(reads) & 0xffffffff
    assert np.diff(pos).min() == 1 and I.max_sites_in(pos, 48) > 32 and I.max_sites_in(pos, 64, aligned=True) > 32
    for pk, lk in ((dict(min_depth=1, min_cpgs=1, min_qual=10), dict(min_distance=1, max_distance=16, min_qual=10)),
                   (dict(min_depth=3, min_cpgs=4, min_qual=10), dict(min_distance=2, max_distance=40, min_qual=10))):
        pdr_lpmd_every_form(eng, cs, reads, pk, lk)
        T_pairs.check(T_pairs.run_device(eng, cs, lk), reads, lk)
    T_quartet.check(T_quartet.run_device(eng, cs, 10, 0), reads, 10, 0)
    mk = dict(min_depth=1, min_cpgs=1, min_qual=10)
    m0 = T_mhl.run_device(eng, cs, mk)
    T_mhl.check(m0, reads, mk)
    T_fuzz.mhl_forms_same(eng, cs, mk, None, m0)
    frec = I.fdrp_safe(rec, 200)
    freads, fcs = I.contigs(frec)
    for fk in (dict(min_qual=10, min_depth=2, max_depth=40, min_overlap=0, seed=4), dict(min_qual=10, min_depth=1, max_depth=64, min_overlap=20, seed=5)):
        fdrp_every_form(eng, fcs, freads, fk)
    multi_every_form(eng, fcs, freads, dict(min_depth=2, min_cpgs=2, min_qual=10, min_distance=2, max_distance=16, max_depth=40,
                                            min_overlap=20, seed=3))


# ---- the CLI: BAM -> device inflate + decode (CIGARs, flags) -> kernels -> TSV ---------------------------------------------------
@pytest.mark.parametrize("wtile", ["auto", "1"])
def test_cli_all_and_singles(tmp_path, wtile):
    """`metheor all` against the seven single commands (test_gpu_multi.check_all), and each single command's bytes against the
    oracle's text, on a BAM written from the generator"""
    rec, names = I.make_records(31, n_contigs=2, length=10_000, n_reads=1_600, density=0.03)
    rec = I.fdrp_safe(rec, 200 if wtile == "1" else None)
    bam = str(tmp_path / "irregular.bam")
    bamio.write_bam(bam, rec)
    reads = pyoracle.Reads.decode(rec)
    e = {"METHEOR_SEED": "9"}
    if wtile != "auto":
        e["METHEOR_FDRP_WTILE"] = wtile
    params = {"d": 2, "p": 2, "q": 10, "m": 2, "M": 16, "D": 40, "l": 20}
    d = tmp_path / ("c%d" % len(list(tmp_path.iterdir())))         # the directory check_all is about to make
    T_multi.check_all(tmp_path, bam, params, env=e)
    for sub in T_multi.OUT:
        flags = []
        for f, v in params.items():
            if f in T_multi.SINGLE_FLAGS[sub]:
                flags += ["-" + f, str(v)]
        want, want_pairs = util.oracle_text(reads, names, sub, input_name=bam, seed=9, **util.oracle_kwargs(sub, flags))
        util.assert_tsv_equals_oracle(sub, (d / ("one." + sub)).read_text(), want)
        if sub == "lpmd":
            assert (d / "one.pairs").read_text() == want_pairs
