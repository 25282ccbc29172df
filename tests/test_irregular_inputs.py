"""The irregular-read generator (tests/irregular_util.py) on the CPU: its output holds the input classes the GPU tests of
tests/test_gpu_irregular.py exist for -- so that a later edit cannot quietly make them trivial -- and on small instances of every
knob the C++ oracle equals the second restatement of the reference, tools/gen_golden_unpinned.py (written from the Rust sources,
independent of oracle/).  That pins the GPU tests' reference on exactly these input classes, adjacent CpG sites included, which
the stored cases of tests/golden/unpinned_cases.json.gz never hold.  Integers and PDR / LPMD / PM / FDRP / qFDRP floats bit for bit;
MHL and ME within 1e-6 (tests/unpinned_util.same_f32)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import pyoracle
from tests import irregular_util as I
from tests import unpinned_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _translit():
    spec = importlib.util.spec_from_file_location("gen_golden_unpinned", os.path.join(ROOT, "tools", "gen_golden_unpinned.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def big():
    rec, names = I.make_records(1)
    return rec, pyoracle.Reads.decode(rec)


def test_adjacent_and_crowded_sites(big):
    """sites one position apart; more than FW_SC = 32 sites in 48 positions (k_fdrp_wtile's old halving floor); more than W / 2
    sites in a tile of every width METHEOR_FDRP_WTILE_W takes in the GPU tests (its old rows per tile)"""
    _, rd = big
    pos = I.called_sites(rd) & 0xffffffff
    assert np.diff(pos).min() == 1
    assert I.max_sites_in(pos, 48) > 32
    for w in (64, 128, 256):
        assert I.max_sites_in(pos, w, aligned=True) > w // 2, w


def test_calls_far_apart_in_rank(big):
    """reads whose consecutive calls lie 33..47 or 65..79 site ranks apart: a 32-bit mask with bit = rank mod 32 folds them onto
    a span of 1..15"""
    _, rd = big
    g = np.concatenate(I.rank_gaps(rd))
    assert (((g >= 33) & (g <= 47)) | ((g >= 65) & (g <= 79))).sum() >= 10


def test_query_offset_and_position_distances_disagree(big):
    """LPMD takes a pair's distance from the query offsets (readutil.rs:184-196): pairs where that and the position distance fall on
    opposite sides of min_distance and of max_distance"""
    _, rd = big
    for lo, hi in ((2, 16), (3, 8), (5, 40)):
        n_min, n_max = I.lpmd_bound_pairs(rd, lo, hi)
        assert n_min > 0 and n_max > 0, (lo, hi, n_min, n_max)


def test_long_queries_on_short_spans(big):
    """query offsets above 255 on reads spanning <= 150 bp (16-bit cpg_rel where an 8-bit one would fit the span)"""
    _, rd = big
    soa = rd.soa()
    off = soa["cpg_off"].astype(np.int64)
    span = soa["end"].astype(np.int64) - soa["start"] + 1
    n = sum(1 for i in range(len(span)) if off[i + 1] > off[i] and span[i] <= 150 and soa["cpg_rel"][off[i]:off[i + 1]].max() > 255)
    assert n >= 10


def test_every_measure_has_rows(big):
    rec, rd = big
    assert len(rd.pdr(min_depth=3, min_cpgs=2)) > 200
    assert len(rd.mhl(min_depth=3, min_cpgs=2)) > 200
    assert len(rd.me(min_depth=2)) > 100 and len(rd.pm(min_depth=2)) > 100
    l = rd.lpmd(pairs=True)
    assert l["n_concordant"] > 1000 and l["n_discordant"] > 100 and len(l["pairs"]) > 1000
    for cap in (None, 200):
        f = pyoracle.Reads.decode(I.fdrp_safe(rec, cap))
        assert len(f.fdrp(min_depth=2, min_overlap=10)) > 200 and len(f.qfdrp(min_depth=2, min_overlap=10)) > 200


def test_knobs_switch_their_class_off():
    """all knobs off: gapless single-length reads, no shifted flag, no island -- the classes above disappear"""
    rec, _ = I.make_records(2, n_reads=400, **{k: False for k in I.KNOBS})
    rd = pyoracle.Reads.decode(rec)
    assert all(len(rec.cigars[i]) == 1 for i in range(len(rec)))
    assert set(rec.flag.tolist()) <= set(I.FLAGS_PLAIN)
    pos = I.called_sites(rd) & 0xffffffff
    assert np.diff(pos).min() >= 1 and I.max_sites_in(pos, 48) <= 24
    assert (rec.mapq == 42).all()


CASES = [(k, 40 + i) for i, k in enumerate(I.KNOBS)] + [("shifted+islands", 60), ("all", 61), ("all", 62)]


def _instance(knob, seed):
    if knob == "all":
        kn = {}
    else:
        on = set(knob.split("+"))
        kn = {k: k in on for k in I.KNOBS}
    return I.make_records(seed, n_contigs=2 if seed % 2 else 1, length=2_400, n_reads=110, density=0.04, **kn)


@pytest.mark.parametrize("knob,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_oracle_equals_the_transliteration(knob, seed):
    G = _translit()
    rec, _ = _instance(knob, seed)
    recs = I.to_translit(rec)
    rd = pyoracle.Reads.decode(rec)
    soa = rd.soa()
    for i, r in enumerate(recs):                                    # readutil.rs:24-53, 323-345
        br = G.bismark_read(r)
        o0, o1 = int(soa["cpg_off"][i]), int(soa["cpg_off"][i + 1])
        assert (int(soa["start"][i]), int(soa["end"][i])) == (br["start_pos"], br["end_pos"]), i
        assert [[int(a), U.signed_pos(p), int(p >> 31)] for a, p in zip(soa["cpg_rel"][o0:o1], soa["cpg_pos"][o0:o1])] == \
            [[c["relpos"], c["abspos"][1], int(c["methylated"])] for c in br["cpgs"]], i
    for p in (dict(min_depth=0, min_cpgs=0, min_qual=10), dict(min_depth=3, min_cpgs=2, min_qual=10)):
        t, want = rd.pdr(**p), G.pdr(recs, **p)
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [list(k) for k in want], p
        assert t.cnt.tolist() == [[v[1], v[2]] for v in want.values()]
        assert U.same_f32(t.val, [v[0] for v in want.values()])
    for p in (dict(min_distance=2, max_distance=16, min_qual=10), dict(min_distance=0, max_distance=40, min_qual=0),
              dict(min_distance=5, max_distance=4, min_qual=10), dict(min_distance=1, max_distance=300, min_qual=10)):
        l, want = rd.lpmd(pairs=True, **p), G.lpmd(recs, **p)
        assert [l[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")] == \
            [want[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")], p
        assert U.same_f32([l["lpmd"]], [want["lpmd"]])
        t = l["pairs"]
        assert [[int(a), int(q[0]), int(q[1])] for a, q in zip(t.tid, t.pos)] == [[k[0][0], k[0][1], k[1][1]] for k, _, _, _ in want["pairs"]]
        assert t.cnt.tolist() == [[c, d] for _, _, c, d in want["pairs"]]
        assert U.same_f32(t.val, [v for _, v, _, _ in want["pairs"]])
    for p in (dict(min_depth=0, min_cpgs=1, min_qual=10), dict(min_depth=3, min_cpgs=2, min_qual=10)):
        t, want = rd.mhl(**p), G.mhl(recs, **p)
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [list(k) for k in want], p
        assert U.same_f32(t.val, list(want.values()), tol=1e-6)
    me, pm, want = rd.me(min_depth=0, min_qual=10), rd.pm(min_depth=0, min_qual=10), G.me_pm(recs, min_qual=10)
    key = lambda t: sorted(range(len(t)), key=lambda i: (int(t.tid[i]), *t.pos[i].tolist()))
    om, op = key(me), key(pm)
    assert [[int(me.tid[i]), *me.pos[i].tolist()] for i in om] == [[q[0][0], q[0][1], q[1][1], q[2][1], q[3][1]] for q in want]
    assert [me.cnt[i].tolist() for i in om] == [v[0] for v in want.values()] == [pm.cnt[i].tolist() for i in op]
    assert U.same_f32(me.val[om], [v[1] for v in want.values()], tol=1e-6)
    assert U.same_f32(pm.val[op], [v[2] for v in want.values()])
    frec = I.fdrp_safe(rec)
    frecs, frd = I.to_translit(frec), pyoracle.Reads.decode(frec)
    for p in (dict(min_qual=10, min_depth=0, max_depth=100_000, min_overlap=0), dict(min_qual=10, min_depth=3, max_depth=100_000, min_overlap=35)):
        f, q, want = frd.fdrp(**p), frd.qfdrp(**p), G.fdrp_qfdrp(frecs, **p)
        keys = [list(k) for k in want]
        assert [[int(a), int(b)] for a, b in zip(f.tid, f.pos[:, 0])] == keys == [[int(a), int(b)] for a, b in zip(q.tid, q.pos[:, 0])], p
        assert f.cnt[:, 0].tolist() == [v[2] for v in want.values()]
        assert U.same_f32(f.val, [v[0] for v in want.values()]) and U.same_f32(q.val, [v[1] for v in want.values()]), p
