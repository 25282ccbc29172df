"""Which kernel form, tile width and index a batch gets (metheor_amd/csrc/mth_plan.h), on the CPU: the header compiled as plain C++
with a small driver that reads shapes from stdin and prints one plan per line.  mth_plan.h itself includes nothing of HIP and never
reads the environment (shown below); the driver takes its knobs through mth_knobs.h, from real environment variables, so that each
knob's parsing and clamping is what the engine does.

The width rule is compared with its independent restatement (tests/wide_width_util.py), the density chooser with the predicate built
from that module's figures; every other switch has one shape on each side, with the expected plan worked out by hand."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import plan_util as P
from tests import wide_width_util as W

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mth_knobs.h"
using namespace mth;

// a line: the rule's name, then integers.  Every rule starts with the shape: n_reads n_cpgs max_span region_beg region_end rel8 al16
int main() {
    char rule[32], name[64], value[64];
    while (scanf("%31s", rule) == 1) {
        if (!strcmp(rule, "env")) { if (scanf("%63s %63s", name, value) != 2) return 2; setenv(name, value, 1); continue; }
        if (!strcmp(rule, "unenv")) { if (scanf("%63s", name) != 1) return 2; unsetenv(name); continue; }
        long long v[7];
        for (int k = 0; k < 7; ++k) if (scanf("%lld", &v[k]) != 1) return 2;
        const BatchShape s{(uint32_t)v[0], (uint32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], v[5] != 0, v[6] != 0};
        long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int extra = !strcmp(rule, "pdr") ? 7 : !strcmp(rule, "fdrp") ? 1 : !strcmp(rule, "mhl") ? 1 : !strcmp(rule, "pairs") ? 2 :
                          !strcmp(rule, "index") ? 1 : !strcmp(rule, "budget") ? 2 : 0;
        for (int k = 0; k < extra; ++k) if (scanf("%lld", &a[k]) != 1) return 2;
        if (!strcmp(rule, "pdr")) {          // want_pdr min_cpgs has_sink fused_force pipelined prepared_idx_base prepared_nq
            mth_pdr_lpmd_params_t p{};
            p.want_pdr = (uint8_t)a[0]; p.want_lpmd = 1; p.pdr_min_cpgs = (uint32_t)a[1]; p.pdr_min_depth = 10;
            const PdrPlan pl = plan_pdr_lpmd(s, p, pdr_knobs_from_env(), a[2] != 0, a[3] != 0, a[4] != 0, (int32_t)a[5], (uint32_t)a[6]);
            printf("%d %d %u %u %u %d %u %d %d %u %d %d %u %u\n", pl.wide_shift, pl.tile_w, pl.tile_w_rt, pl.tile_step, pl.ntiles, pl.idx_base, pl.nq,
                   (int)pl.prepared_fits, (int)pl.coarse, pl.coarse_stride, (int)pl.runs, pl.tile_b, pl.nbk, pl.n_bucket_words);
        } else if (!strcmp(rule, "fdrp")) {  // max_depth
            mth_fdrp_params_t p{};
            p.max_depth = (uint32_t)a[0];
            const FdrpPlan pl = plan_fdrp(s, p, fdrp_knobs_from_env());
            printf("%d %d %d %d %d %llu\n", (int)pl.wtile, (int)pl.dense, pl.walk4, pl.win, (int)pl.tile, (unsigned long long)pl.bound);
        } else if (!strcmp(rule, "budget")) {  // max_depth bound
            mth_fdrp_params_t p{};
            p.max_depth = (uint32_t)a[0];
            printf("%llu\n", (unsigned long long)fdrp_term_budget(s, p, (uint64_t)a[1]));
        } else if (!strcmp(rule, "wtile")) {
            printf("%d\n", plan_fdrp_wtile(s, fdrp_wtile_knobs_from_env()));
        } else if (!strcmp(rule, "mhl")) {   // min_cpgs
            mth_mhl_params_t p{};
            p.min_cpgs = (uint32_t)a[0]; p.min_depth = 10;
            const MhlPlan pl = plan_mhl(s, p, mhl_knobs_from_env());
            printf("%d %d\n", (int)pl.rowchk, pl.shift);
        } else if (!strcmp(rule, "quartet")) {
            printf("%d\n", quartet_tile_shift(s, tile_shift_knob("MTH_QUARTET")));
        } else if (!strcmp(rule, "pairs")) { // min_distance max_distance
            mth_lpmd_pairs_params_t p{};
            p.min_distance = (int32_t)a[0]; p.max_distance = (int32_t)a[1];
            printf("%d\n", pairs_tile_shift(s, p, tile_shift_knob("MTH_PAIRS")));
        } else if (!strcmp(rule, "index")) { // tile width
            const IndexGeom g = index_geometry(s, (uint32_t)a[0]);
            printf("%d %d %u %u\n", g.ext, g.idx_base, g.nq, g.ntiles);
        } else return 3;
    }
    return 0;
}
"""

KNOBS = ("MTH_PDR_WIDE", "MTH_PDR_WIDE_W", "MTH_COARSE_INDEX", "MTH_TILE_RUNS", "MTH_TILE_B", "METHEOR_FDRP_WTILE", "METHEOR_FDRP_WALK4",
         "METHEOR_FDRP_TILE", "METHEOR_FDRP_WIN", "METHEOR_FDRP_TILE_WIDE_ROWS", "METHEOR_FDRP_WTILE_W", "METHEOR_FDRP_WTILE_SUB",
         "METHEOR_FDRP_WTILE_HEAVY", "MTH_MHL_WALK", "MTH_MHL_ROWCHK", "MTH_MHL_TILE_SHIFT", "MTH_MHL_FORCE_SUB", "MTH_MHL_FORCE_HAND_ON",
         "MTH_MHL_NO_WAVE_WALK", "MTH_QUARTET_TILE_SHIFT", "MTH_PAIRS_TILE_SHIFT")
PDR_FIELDS = ("wide_shift", "tile_w", "tile_w_rt", "tile_step", "ntiles", "idx_base", "nq", "prepared_fits", "coarse", "coarse_stride", "runs",
              "tile_b", "nbk", "n_bucket_words")
FDRP_FIELDS = ("wtile", "dense", "walk4", "win", "tile", "bound")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the driver, built once: the compile succeeding is the check that the two headers need nothing of HIP"""
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "plan_driver.cpp"
    src.write_text(DRIVER)
    out = d / "plan_driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


def ask(exe, queries):
    """queries: (rule, shape, extra integers, {knob: value}) -> one list of integers each, in order"""
    lines = []
    for rule, s, extra, knobs in queries:
        lines += ["env %s %s" % kv for kv in knobs.items()]
        lines.append(" ".join([rule] + [str(int(x)) for x in (s["n_reads"], s["n_cpgs"], s["max_span"], s.get("region_beg", 0), s["region_end"],
                                                             s.get("rel8", 1), s.get("al16", 1))] + [str(int(x)) for x in extra]))
        lines += ["unenv %s" % k for k in knobs]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(out) == len(queries)
    return out


def sh(n_reads, n_cpgs, max_span, region_len, **kw):
    return dict(n_reads=n_reads, n_cpgs=n_cpgs, max_span=max_span, region_beg=0, region_end=region_len, **kw)


def pdr(exe, s, want_pdr=1, min_cpgs=4, sink=0, fused_force=0, pipelined=0, prep=(0, 0), **knobs):
    return dict(zip(PDR_FIELDS, ask(exe, [("pdr", s, (want_pdr, min_cpgs, sink, fused_force, pipelined) + tuple(prep), knobs)])[0]))


def fdrp(exe, s, max_depth=40, **knobs):
    return dict(zip(FDRP_FIELDS, ask(exe, [("fdrp", s, (max_depth,), knobs)])[0]))


def test_plan_header_is_pure(tmp_path):
    """mth_plan.h compiles on its own with a plain C++ compiler, includes nothing of HIP and does not read the environment; the
    environment is read in mth_knobs.h and nowhere else on the launch path"""
    text = open(os.path.join(CSRC, "mth_plan.h")).read()
    assert "getenv" not in text and "hip/" not in text and "mth_common.h" not in text
    src = tmp_path / "alone.cpp"
    src.write_text('#include "mth_plan.h"\nint main() { return mth::index_ext(150) == 160 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "alone"), str(src)])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    for name in ("mth_quartet.hip", "mth_pairs.hip", "mth_tile_rows.hip", "mth_multi.hip", "mth_sites.hip", "mth_fdrp_wtile.hip"):
        assert "getenv" not in open(os.path.join(CSRC, name)).read(), name


# ---- the shipped width rule --------------------------------------------------------------------------------------------------------
SPARSE = dict(n_reads=1000, n_cpgs=900, max_span=100)       # (the width rule reads the region alone; the slice is forced)

PINS = [(29_360_128, 14, 0), (30_000_000, 14, 8384), (32_000_000, 14, 8960), (40_000_000, 14, 11200), (45_000_000, 14, 0),
        (60_000_000, 14, 11200), (75_000_000, 14, 0), (248_956_422, 16, 46336)]          # test_wide_width_inputs.test_narrowed_width_pins


def test_width_rule_pins(exe):
    got = ask(exe, [("pdr", dict(SPARSE, region_end=n), (1, 4, 0, 0, 0, 0, 0), {"MTH_PDR_WIDE": shift}) for n, shift, _ in PINS])
    for (n, shift, want), g in zip(PINS, got):
        pl = dict(zip(PDR_FIELDS, g))
        assert pl["wide_shift"] == shift and pl["tile_w"] == 1 << shift and pl["tile_w_rt"] == want, (n, shift, pl)
        assert pl["tile_step"] == (want or 1 << shift) and pl["ntiles"] == -(-n // pl["tile_step"])
        assert W.narrowed_width(n, shift) == want


@pytest.mark.parametrize("shift", [14, 15, 16])
def test_width_rule_equals_restatement(exe, shift):
    """a seeded sweep of region lengths up to nine rounds of tiles, with every whole number of rounds k * 1792 * 2^shift and the
    positions beside it"""
    rng = np.random.default_rng(shift)
    slots = 1792 << shift
    lens = set(int(x) for x in np.exp(rng.uniform(math.log(1 << shift), math.log(9 * slots), size=100_000)))
    lens |= set(int(x) for x in rng.integers(slots, 8 * slots, size=20_000))
    for k in range(1, 10):
        lens |= {k * slots - 1, k * slots, k * slots + 1}
        lens |= {int(k * slots + f * slots) + d for f in (0.02, 0.5) for d in (-1, 0, 1)}       # the two fractions the rule cuts at
    lens = sorted(n for n in lens if 0 < n < 2**31 - 1)
    assert len(lens) >= 100_000
    got = ask(exe, [("pdr", dict(SPARSE, region_end=n), (1, 4, 0, 0, 0, 0, 0), {"MTH_PDR_WIDE": shift}) for n in lens])
    want = [W.narrowed_width(n, shift) for n in lens]
    bad = [(n, g[2], w) for n, g, w in zip(lens, got, want) if g[2] != w]
    assert not bad, bad[:5]
    assert sum(1 for w in want if w) > 10_000 and sum(1 for w in want if not w) > 10_000


def test_width_knob_domain(exe):
    """MTH_PDR_WIDE_W: [1024, slice), rounded down to 64; anything else leaves the tile as wide as its slice.  MTH_PDR_WIDE: any value
    outside 14 .. 16 means the dense form."""
    s = dict(SPARSE, region_end=32_000_000)
    for w, want in ((1023, 0), (1024, 1024), (1087, 1024), (8960, 8960), (16383, 16320), (16384, 0), (0, 0), (-64, 0)):
        assert pdr(exe, s, MTH_PDR_WIDE=14, MTH_PDR_WIDE_W=w)["tile_w_rt"] == want, w
    for k, want in ((0, 0), (13, 0), (14, 14), (15, 15), (16, 16), (17, 0), ("x", 0)):
        assert pdr(exe, s, MTH_PDR_WIDE=k)["wide_shift"] == want, k
    assert pdr(exe, s, MTH_PDR_WIDE=0, MTH_PDR_WIDE_W=8960)["tile_w_rt"] == 0          # the dense form has no narrowed width


# ---- the sparse / dense choice -----------------------------------------------------------------------------------------------------
def figures_batch(n_reads, n_cpgs, span):
    """what W.chooser_figures reads of a batch, without the batch"""
    z = np.zeros(n_reads, np.int32)
    return dict(read_start=z, read_end=z + (span - 1), cpg_off=np.array([0, n_cpgs], np.int64))


def wide_by_figures(c, region_len, min_cpgs):
    sites_per_bp, ins_per_read = W.chooser_figures(c, min_cpgs)
    return sites_per_bp <= 0.012 and len(c["read_start"]) / region_len * 4096.0 <= 900.0 and ins_per_read <= 0.6


def test_density_chooser(exe):
    qs, want = [], []
    for length in (32_000_000, 40_000_000, 45_000_000):            # the contigs of test_chooser_narrows_long_contigs
        c, _ = W.long_sparse_contig(length, W.narrowed_width(length, 14))
        span = int((c["read_end"].astype(np.int64) - c["read_start"]).max()) + 1
        for min_cpgs in (4, 1):
            qs.append(("pdr", sh(len(c["read_start"]), int(c["cpg_off"][-1]), span, length), (1, min_cpgs, 0, 0, 0, 0, 0), {}))
            want.append(wide_by_figures(c, length, min_cpgs))
        assert want[-2] and not want[-1]                           # wide under the CLI's min_cpgs, dense where every call is inserted
    # config-2-like (chr19 at density 0.02, 25 x) and config-3-like (chr1 at 0.0091, 10 x), a tenth of the reads on a tenth of the contig
    for n, cpr, span, length in ((1_000_000, 2.94, 150, 5_861_761), (1_600_000, 1.365, 150, 24_895_642)):
        for min_cpgs in (4, 1):
            c = figures_batch(n, int(n * cpr), span)
            qs.append(("pdr", sh(n, int(n * cpr), span, length), (1, min_cpgs, 0, 0, 0, 0, 0), {}))
            want.append(wide_by_figures(c, length, min_cpgs))
    assert want[-4:] == [False, False, True, False]
    rng = np.random.default_rng(5)
    for _ in range(3000):                                          # figures only
        n = int(np.exp(rng.uniform(math.log(10), math.log(200_000))))
        cpr = float(np.exp(rng.uniform(math.log(0.1), math.log(8.0))))
        span = int(rng.choice([50, 100, 150, 151, 300]))
        length = int(np.exp(rng.uniform(math.log(n), math.log(n * 400))))
        min_cpgs = int(rng.integers(0, 7))
        c = figures_batch(n, int(n * cpr), span)
        qs.append(("pdr", sh(n, int(n * cpr), span, length), (1, min_cpgs, 0, 0, 0, 0, 0), {}))
        want.append(wide_by_figures(c, length, min_cpgs))
    got = [g[0] != 0 for g in ask(exe, qs)]
    assert got == want
    assert 500 < sum(want) < len(want) - 500
    # LPMD alone inserts nothing: the insertion limit does not bind
    s = sh(100_000, 90_000, 100, 1_000_000)
    assert pdr(exe, s, want_pdr=1, min_cpgs=1)["wide_shift"] == 0 and pdr(exe, s, want_pdr=0, min_cpgs=1)["wide_shift"] == 14


def test_slice_drop(exe):
    """while (wide_shift > 14 && (region_len >> wide_shift) < 3584) --wide_shift: 0.05 reads and 0.00045 calls a position take 65536-position
    slices where the region gives 3584 of them"""
    def shift(n):
        reads = n // 20
        return pdr(exe, sh(reads, reads * 9 // 10, 100, n))["wide_shift"]
    assert shift(3584 << 16) == 16 and shift((3584 << 16) - 1) == 15
    assert shift(3584 << 15) == 15 and shift((3584 << 15) - 1) == 14
    assert shift(131072) == 14 and shift(100) == 14


def test_coarse_index_and_threads(exe):
    """coarse: the dense form outside site discovery, without a prepared index that fits, unless MTH_COARSE_INDEX=0.  tile_b: 128 for a
    pipelined batch with 8-bit relative positions alone; MTH_TILE_B overrides it for 8-bit batches."""
    dense, sparse = sh(100_000, 300_000, 100, 1_000_000), sh(100_000, 90_000, 100, 1_000_000)
    geo = dict(zip(("ext", "idx_base", "nq", "ntiles"), ask(exe, [("index", dense, (65536,), {})])[0]))
    for sink in (0, 1):
        for prep in ((0, 0), (geo["idx_base"], geo["nq"]), (geo["idx_base"] + 32, geo["nq"]), (geo["idx_base"], 100)):
            for off in (None, "0", "1"):
                for s in (dense, sparse):
                    kn = {} if off is None else {"MTH_COARSE_INDEX": off}
                    pl = pdr(exe, s, sink=sink, prep=prep, **kn)
                    fits = prep == (geo["idx_base"], geo["nq"])
                    assert pl["prepared_fits"] == fits, (prep, pl)
                    assert pl["coarse"] == (not sink and not fits and pl["wide_shift"] == 0 and off != "0"), (sink, prep, off, pl)
                    assert pl["wide_shift"] == (0 if s is dense else 14)
    assert pdr(exe, dense)["coarse_stride"] == (245 + 2 + 3) & ~3 and pdr(exe, dense)["ntiles"] == 245
    for pipelined in (0, 1):
        for rel8 in (0, 1):
            for knob, forced in ((None, None), (128, 128), (256, 256), (64, None), (0, None)):
                kn = {} if knob is None else {"MTH_TILE_B": knob}
                want = 256 if not rel8 else forced if forced else 128 if pipelined else 256
                assert pdr(exe, dict(dense, rel8=rel8), pipelined=pipelined, **kn)["tile_b"] == want, (pipelined, rel8, knob)
    # the run form: MTH_TILE_RUNS=1 alone, the dense form on 8-bit relative positions alone
    assert pdr(exe, dense, MTH_TILE_RUNS=1)["runs"] == 1 and pdr(exe, dense, MTH_TILE_RUNS=2)["runs"] == 0 and pdr(exe, dense)["runs"] == 0
    assert pdr(exe, dict(dense, rel8=0), MTH_TILE_RUNS=1)["runs"] == 0 and pdr(exe, sparse, MTH_TILE_RUNS=1)["runs"] == 0
    # MTH_MULTI_FUSED on a dense batch: 16384-position slices
    assert pdr(exe, dense, fused_force=1)["wide_shift"] == 14 and pdr(exe, dense, fused_force=1, MTH_PDR_WIDE=0)["wide_shift"] == 14


# ---- FDRP / qFDRP ------------------------------------------------------------------------------------------------------------------
def F(wtile=0, dense=0, walk4=0, tile=0, win=None):
    return dict(wtile=wtile, dense=dense, walk4=walk4, tile=tile, win=win)


def check_fdrp(exe, s, max_depth, want, **knobs):
    got = fdrp(exe, s, max_depth, **knobs)
    for k, v in want.items():
        if v is not None:
            assert got[k] == v, (s, max_depth, knobs, k, got)


def test_fdrp_switches(exe):
    """region of 1 000 000 positions, max_span 98: cand = n_reads / 10 000 (the reads that can call a site)"""
    R = 1_000_000
    # calls a read 2.0 (cand 10; 10 + 4 sqrt(10) = 22.6 <= 40)
    check_fdrp(exe, sh(100_000, 200_000, 98, R), 40, F(wtile=1))
    check_fdrp(exe, sh(100_000, 200_001, 98, R), 40, F(walk4=16))
    # max_span 200 (cand = 50 000 * 202 / 1e6 = 10.1) and 201: no form but the general walk beyond 200
    check_fdrp(exe, sh(50_000, 50_000, 200, R), 40, F(wtile=1))
    check_fdrp(exe, sh(50_000, 50_000, 201, R), 40, F())
    # cand 24 (24 + 4 sqrt(24) = 43.6 <= 64)
    check_fdrp(exe, sh(240_000, 240_000, 98, R), 64, F(wtile=1))
    check_fdrp(exe, sh(240_001, 240_001, 98, R), 64, F(tile=1))
    # cand + 4 sqrt(cand) against max_depth: cand 16 gives exactly 32
    check_fdrp(exe, sh(160_000, 160_000, 98, R), 32, F(wtile=1))
    check_fdrp(exe, sh(160_000, 160_000, 98, R), 31, F(walk4=16))
    # ... against 40: cand 21 -> 39.3, cand 22 -> 40.8 (beyond 16: the read x read form)
    check_fdrp(exe, sh(210_000, 210_000, 98, R), 40, F(wtile=1))
    check_fdrp(exe, sh(220_000, 220_000, 98, R), 40, F(tile=1))
    # ... against 20: cand 8 -> 19.3, cand 9 -> 21
    check_fdrp(exe, sh(80_000, 80_000, 98, R), 20, F(wtile=1))
    check_fdrp(exe, sh(90_000, 90_000, 98, R), 20, F(walk4=16))
    # cand 16 for walk4 (max_depth 20: no wtile)
    check_fdrp(exe, sh(160_000, 160_000, 98, R), 20, F(walk4=16))
    check_fdrp(exe, sh(160_001, 160_001, 98, R), 20, F(tile=1))
    # 6.0 calls a read for dense (cand 10): dense batches keep the wave-per-site walk behind the read x read form
    check_fdrp(exe, sh(100_000, 600_000, 98, R), 40, F(dense=0, walk4=16))
    check_fdrp(exe, sh(100_000, 600_001, 98, R), 40, F(dense=1, tile=1))
    # win: calls per read and position * 402 <= 12; max_span 100: 2.985 / 100 * 402 = 11.9997, 2.986 -> 12.0037
    check_fdrp(exe, sh(100_000, 298_500, 100, R), 40, F(walk4=16, win=32))
    check_fdrp(exe, sh(100_000, 298_600, 100, R), 40, F(walk4=16, win=64))
    # wtile's bound: a site per call or per position, whichever is fewer
    assert fdrp(exe, sh(100_000, 150_000, 98, R))["bound"] == 150_000 and fdrp(exe, sh(1000, 1500, 98, 1200), METHEOR_FDRP_WTILE=1)["bound"] == 1200
    # no reads: nothing by itself
    check_fdrp(exe, sh(0, 0, 98, R), 40, F(walk4=16))        # (cand 0: the four-sites-per-wave kernel over no sites, as before)


def test_fdrp_knobs(exe):
    R = 1_000_000
    shallow, deep, long_ = sh(100_000, 100_000, 98, R), sh(300_000, 300_000, 98, R), sh(50_000, 50_000, 201, R)
    check_fdrp(exe, shallow, 40, F(wtile=1))
    check_fdrp(exe, deep, 40, F(tile=1))
    check_fdrp(exe, shallow, 40, F(walk4=16), METHEOR_FDRP_WTILE=0)
    check_fdrp(exe, deep, 40, F(wtile=1), METHEOR_FDRP_WTILE=1)
    check_fdrp(exe, long_, 40, F(), METHEOR_FDRP_WTILE=1)                      # never beyond 200 bp
    # METHEOR_FDRP_WALK4: 1 = 16; 16 / 32; anything else none.  Set at all: no wtile by itself
    for k, lanes in ((1, 16), (16, 16), (32, 32), (0, 0), (8, 0)):
        check_fdrp(exe, shallow, 40, F(walk4=lanes, tile=0 if lanes else 1), METHEOR_FDRP_WALK4=k)
        check_fdrp(exe, deep, 40, F(walk4=lanes, tile=0 if lanes else 1), METHEOR_FDRP_WALK4=k)
        check_fdrp(exe, long_, 40, F(), METHEOR_FDRP_WALK4=k)
    check_fdrp(exe, shallow, 40, F(wtile=1), METHEOR_FDRP_WALK4=32, METHEOR_FDRP_WTILE=1)      # the tile pass wins over both
    # METHEOR_FDRP_TILE: set at all -- even to 0 -- it excludes the wtile choice
    check_fdrp(exe, shallow, 40, F(walk4=16), METHEOR_FDRP_TILE=0)
    check_fdrp(exe, shallow, 40, F(tile=1), METHEOR_FDRP_TILE=1)
    check_fdrp(exe, deep, 40, F(), METHEOR_FDRP_TILE=0)
    check_fdrp(exe, long_, 40, F(), METHEOR_FDRP_TILE=1)
    check_fdrp(exe, shallow, 40, F(wtile=1), METHEOR_FDRP_TILE=1, METHEOR_FDRP_WTILE=1)
    # METHEOR_FDRP_WIN: 32, anything else 64
    for k, win in ((32, 32), (64, 64), (16, 64)):
        check_fdrp(exe, shallow, 20, F(walk4=16, win=win), METHEOR_FDRP_WIN=k)
    # the term list of the read x read form: calls * (min(max_depth, 64) - 1) / 2 + 64 * sites + 64
    s = sh(100_000, 300_000, 98, R)
    assert ask(exe, [("budget", s, (40, 1000), {}), ("budget", s, (100, 1000), {}), ("budget", s, (0, 7), {})]) == \
        [[300_000 * 39 // 2 + 64_064], [300_000 * 63 // 2 + 64_064], [7 * 64 + 64]]


def test_fdrp_wtile_width(exe):
    """the widest tile whose reads (128 slots, 2 sigma kept free: 105.4) and calls (256, 224) fit, max_span less, rounded down to 64,
    within [256, FW_WMAX = 1600]"""
    def width(n_reads, n_cpgs, region, span=100, **knobs):
        return ask(exe, [("wtile", sh(n_reads, n_cpgs, span, region), (), knobs)])[0][0]
    R = 1_000_000
    assert width(100_000, 100_000, R) == 896         # 105.4 / 0.1 - 100 = 953 (the calls would allow 2240 - 100)
    assert width(100_000, 300_000, R) == 640         # the calls take over: 224 / 0.3 - 100 = 646
    assert width(10_000, 10_000, R) == 1600          # 10 437: FW_WMAX
    assert width(60_000, 60_000, R) == 1600          # 1656
    assert width(62_000, 62_000, R) == 1536          # 1599.5
    assert width(1_000_000, 1_000_000, R) == 256     # 5: the floor
    assert width(296_000, 296_000, R) == 256 and width(294_000, 294_000, R) == 256      # 255.9 / 258.4 -> 256 either way
    assert width(250_000, 250_000, R) == 320         # 321.5
    for k, want in ((0, 64), (64, 64), (100, 64), (1000, 960), (1600, 1600), (5000, 1600)):      # METHEOR_FDRP_WTILE_W: [64, FW_WMAX], down to 64
        assert width(100_000, 100_000, R, METHEOR_FDRP_WTILE_W=k) == want, k


# ---- MHL ---------------------------------------------------------------------------------------------------------------------------
def mhl(exe, s, min_cpgs=4, **knobs):
    return tuple(ask(exe, [("mhl", s, (min_cpgs,), knobs)])[0])


def test_mhl_plan(exe):
    R = 1_000_000
    # rowchk at 1.8 calls a read
    assert mhl(exe, sh(100_000, 180_000, 100, R))[0] == 1 and mhl(exe, sh(100_000, 180_001, 100, R))[0] == 0
    assert mhl(exe, sh(100_000, 300_000, 100, R), MTH_MHL_ROWCHK=1)[0] == 1 and mhl(exe, sh(100_000, 90_000, 100, R), MTH_MHL_ROWCHK=0)[0] == 0
    # the slot limit: sites per position * 2^(shift + 1) <= 0.65 * 256 = 166.4 -> 0.0203 for 8192, 0.01016 for 16384
    assert mhl(exe, sh(100_000, 300_000, 100, R)) == (0, 12)          # 0.03
    assert mhl(exe, sh(100_000, 204_000, 100, R)) == (0, 12)          # 0.0204 * 8192 = 167.1
    assert mhl(exe, sh(100_000, 203_000, 100, R)) == (0, 13)          # 0.0203 * 8192 = 166.3
    assert mhl(exe, sh(100_000, 102_000, 100, R)) == (1, 13)          # 0.0102 * 16384 = 167.1
    assert mhl(exe, sh(100_000, 101_000, 100, R)) == (1, 14)          # 0.0101 * 16384 = 165.5
    # the read limit: reads per position * (2^(shift + 1) + max_span + 64) <= 0.75 * 8191 = 6143.25
    assert mhl(exe, sh(735_000, 661_500, 100, R)) == (1, 13)          # 0.735 * 8356 = 6141.7
    assert mhl(exe, sh(736_000, 662_400, 100, R)) == (1, 12)          # 0.736 * 8356 = 6150.0
    assert mhl(exe, sh(371_000, 333_900, 100, R)) == (1, 14)          # 0.371 * 16548 = 6139.3
    assert mhl(exe, sh(372_000, 334_800, 100, R)) == (1, 13)          # 0.372 * 16548 = 6155.9
    # 32768-position tiles: the row check, three rounds of 1536 tiles, and the contributors' sites within half the slots
    # (0.05 reads and 0.009 calls a position: share 0.135 of the sites, 39.8 a tile)
    L15 = 3 * 1536 * 32768
    n = L15 // 20
    assert mhl(exe, sh(n, n * 9 // 10, 100, L15)) == (1, 15)
    assert mhl(exe, sh(n, n * 9 // 10, 100, L15 - 1)) == (1, 14)
    assert mhl(exe, sh(n, n * 9 // 10, 100, L15), MTH_MHL_ROWCHK=0) == (0, 14)
    assert mhl(exe, sh(n, n * 9 // 10, 100, L15), min_cpgs=1) == (1, 14)      # every covering read contributes: 0.009 * 32768 = 295 > 128
    # MTH_MHL_TILE_SHIFT clamps to 12 .. 16
    for k, want in ((11, 12), (12, 12), (15, 15), (16, 16), (17, 16), (0, 12)):
        assert mhl(exe, sh(100_000, 300_000, 100, R), MTH_MHL_TILE_SHIFT=k)[1] == want, k


# ---- ME / PM and LPMD pairs --------------------------------------------------------------------------------------------------------
def test_quartet_and_pairs_shift(exe):
    def q(s, **knobs):
        return ask(exe, [("quartet", s, (), knobs)])[0][0]

    def p(s, lo=2, hi=16, **knobs):
        return ask(exe, [("pairs", s, (lo, hi), knobs)])[0][0]
    config2 = sh(10_000_000, 29_400_000, 150, 58_617_616)      # chr19, 2.94 calls a read: 0.0196 sites a position
    config3 = sh(16_000_000, 21_840_000, 150, 248_956_422)     # chr1 at 10 x, 1.365 calls a read: 0.0091
    # quartets: sites * P(>= 3 more within the span) * 2^(shift + 1) <= 0.4 * 512 = 204.8
    #   config 2: lam 2.94, P = 0.565: 0.01107 a position -> 16384 * 0.01107 = 181 fits, 32768 does not: shift 14
    #   config 3: lam 1.365, P = 0.158: 0.00144 a position -> 65536 * 0.00144 = 94 fits: shift 16
    assert q(config2) == 14 and q(config3) == 16
    assert q(sh(1_000_000, 6_000_000, 150, 10_000_000)) == 13      # lam 6, P = 0.938: 0.0375 * 16384 = 614
    assert q(sh(1_000_000, 2_000_000, 150, 10_000_000)) == 15      # lam 2, P = 0.323: 0.00431 * 65536 = 282, * 32768 = 141
    # pairs: sites * 2^(shift + 1) * max(1, sites * window) <= 0.3 * 2048 = 614.4, window = min(16 - 2 + 1, span)
    #   config 2: 0.0196 * 16384 = 321 fits, 32768 does not: 14; config 3: 0.0091 * 65536 = 596 fits: 16
    assert p(config2) == 14 and p(config3) == 16
    assert p(sh(1_000_000, 6_000_000, 150, 10_000_000)) == 13      # 0.04 * 16384 = 655
    assert p(sh(1_000_000, 2_000_000, 150, 10_000_000)) == 15      # 0.01333 * 65536 = 874, * 32768 = 437
    assert p(config3, lo=0, hi=400) == 15                           # window 150: 0.0091 * 150 = 1.365 -> 65536 * 0.0091 * 1.365 = 814
    # the read limit: reads per position * (2^(shift + 1) + span + 64) <= 30000
    # 0.9 reads a position: the step to 32768 (0.9 * (32768 + 214) = 29 684) is taken, the step to 65536 (0.9 * 65750 = 59 175) is not
    assert q(sh(9_000_000, 900_000, 150, 10_000_000)) == 15 and p(sh(9_000_000, 900_000, 150, 10_000_000)) == 15
    assert q(sh(9_100_000, 910_000, 150, 10_000_000)) == 14 and p(sh(9_100_000, 910_000, 150, 10_000_000)) == 14     # 0.91 * 32982 = 30 014
    # empty batches and regions: the narrowest
    assert q(sh(0, 0, 150, 1_000_000)) == 13 and p(sh(1000, 1000, 150, 0)) == 13
    # the knobs clamp to 13 .. 16
    for k, want in ((12, 13), (13, 13), (15, 15), (16, 16), (17, 16), (0, 13)):
        assert q(config2, MTH_QUARTET_TILE_SHIFT=k) == want and p(config2, MTH_PAIRS_TILE_SHIFT=k) == want, k
    assert q(config2, MTH_PAIRS_TILE_SHIFT=16) == 14 and p(config2, MTH_QUARTET_TILE_SHIFT=16) == 14        # each its own


# ---- the index geometry ------------------------------------------------------------------------------------------------------------
def test_index_geometry(exe):
    """ext: max_span + 2 up to whole 32-position quanta; idx_base below the region by that; one entry per quantum over the tiles and
    the extent, and two"""
    qs, want = [], []
    for span, ext in ((1, 32), (30, 32), (31, 64), (150, 160), (300, 320)):
        for beg in (0, 1000, 999_937):
            for length in (0, 1, 4095, 4096, 4097, 65536, 1_000_000, 3 * 8960, 3 * 8960 + 1):
                for w in (256, 1600, 4096, 8960, 16384, 65536):
                    qs.append(("index", dict(n_reads=10, n_cpgs=10, max_span=span, region_beg=beg, region_end=beg + length), (w,), {}))
                    nt = -(-length // w)
                    want.append([ext, beg - ext, ((nt * w + ext) >> 5) + 2, nt])
    assert ask(exe, qs) == want
    # what launch_pdr_lpmd hands its kernels is the same geometry at the plan's tile step
    s = sh(1000, 900, 150, 32_000_000)
    pl = pdr(exe, s, MTH_PDR_WIDE=14)
    assert pl["tile_step"] == 8960 and [160, pl["idx_base"], pl["nq"], pl["ntiles"]] == ask(exe, [("index", s, (8960,), {})])[0]
    assert pl["nbk"] == -(-pl["ntiles"] // 256) and pl["n_bucket_words"] == 5 * pl["nbk"]


# ---- the shapes the GPU runs (tests/test_gpu_plan_forms.py) ------------------------------------------------------------------------
def test_gpu_shapes_take_the_expected_forms(exe):
    for name, max_depth, want, _ in P.FDRP_CASES:
        check_fdrp(exe, P.shape(name), max_depth, dict(F(), **want))
    for name, want in P.MHL_CASES:
        assert mhl(exe, P.shape(name))[0] == want["rowchk"], name
    for name, min_cpgs, launches, _ in P.PDR_CASES:
        for sink, want_pdr, shift in launches:
            pl = pdr(exe, P.shape(name), want_pdr=want_pdr, min_cpgs=min_cpgs, sink=sink)
            assert pl["wide_shift"] == shift and pl["ntiles"] == P.LENGTH >> (shift or 12), (name, min_cpgs, sink, pl)
    assert P.shape("J")["rel8"] == 0 and P.shape("J")["max_span"] == 300 and P.shape("A")["rel8"] == 1 and P.shape("A")["max_span"] == 100
