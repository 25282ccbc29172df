"""The launch functions do what the plan says.  tests/test_launch_plan.py pins on the CPU which form each shape of tests/plan_util.py
takes (mth_plan.h); here the same shapes run with nothing forced in the environment and the launches timed, and each case asserts

  * that the kernels with a launch count in eng.timing() are the expected form's, and
  * that the rows are the oracle's, as tests/test_gpu_fdrp.py, test_gpu_mhl.py and test_gpu_wide_width.py compare them: FDRP / qFDRP
    and MHL within 1e-6 on the same sites and depths, PDR rows and the LPMD counters bit for bit.

A launch function that reads the wrong field of its plan passes every forced-form test and fails here."""
import os

import numpy as np
import pytest

from oracle import pyoracle
from tests import plan_util as P
from tests import util

pytestmark = pytest.mark.gpu

TOL = 1e-6
LPMD_KEYS = ("n_concordant", "n_discordant", "n_read", "n_valid_read")
KNOBS = ("MTH_PDR_WIDE", "MTH_PDR_WIDE_W", "MTH_COARSE_INDEX", "MTH_TILE_RUNS", "MTH_TILE_B", "METHEOR_FDRP_WTILE", "METHEOR_FDRP_WALK4",
         "METHEOR_FDRP_TILE", "METHEOR_FDRP_WIN", "METHEOR_FDRP_WTILE_W", "MTH_MHL_WALK", "MTH_MHL_ROWCHK", "MTH_MHL_TILE_SHIFT")


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def nothing_forced():
    assert not [k for k in KNOBS if k in os.environ]


_reads = {}


def batch(name):
    """the contig as a device-resident batch over the whole region, and its oracle reads (made once)"""
    from metheor_amd import synth
    c = P.contig(name)
    if name not in _reads:
        _reads[name] = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
    bt = util.device_batch(c, region=(0, P.LENGTH), device="cuda:0")
    s = P.shape(name)
    assert (bt.c.n_reads, bt.c.n_cpgs, bt.c.max_span) == (s["n_reads"], s["n_cpgs"], s["max_span"]) and bool(bt.c.cpg_rel) == bool(s["rel8"])
    return bt, _reads[name]


def timed(eng, run):
    """run() with the launches timed -> (its result, the kernels that were launched)"""
    eng.timing_enable(True)
    eng.timing_reset()
    eng.reset()
    try:
        out = run()
        t = eng.timing()
    finally:
        eng.timing_enable(False)
        eng.timing_reset()
    return out, {k for k, v in t.items() if v[1] > 0}


def close(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    d = np.abs(a - b)
    d[np.isnan(a) & np.isnan(b)] = 0
    return not np.isnan(d).any() and (len(d) == 0 or d.max() <= TOL)


@pytest.mark.parametrize("name,max_depth,plan,kernels", P.FDRP_CASES, ids=["%s-D%d" % (c[0], c[1]) for c in P.FDRP_CASES])
def test_fdrp_form(eng, name, max_depth, plan, kernels):
    bt, reads = batch(name)
    kw = dict(min_qual=10, min_depth=4, max_depth=max_depth, min_overlap=35, seed=11)

    def run():
        eng.fdrp_accumulate(bt, **kw)
        return eng.fdrp_fetch()
    d, ran = timed(eng, run)
    assert ran & P.FDRP_KERNELS == kernels and "k_fdrp_walk" in ran, (name, max_depth, sorted(ran))
    of, oq = reads.fdrp(**kw), reads.qfdrp(**kw)
    assert len(of) > 400 and len(d["pos"]) == len(of) == len(oq)
    assert (d["pos"] == of.pos[:, 0]).all() and (d["n_reads"] == of.cnt[:, 0]).all()
    assert close(d["fdrp"], of.val) and close(d["qfdrp"], oq.val)


@pytest.mark.parametrize("name,plan", P.MHL_CASES, ids=[c[0] for c in P.MHL_CASES])
def test_mhl_form(eng, name, plan):
    bt, reads = batch(name)

    def run():
        eng.mhl_accumulate(bt, min_depth=3, min_cpgs=2)
        return eng.mhl_fetch()
    d, ran = timed(eng, run)
    assert "k_mhl_tile" in ran and ("k_mhl_rowcheck" in ran) == bool(plan["rowchk"]), (name, sorted(ran))
    o = reads.mhl(min_depth=3, min_cpgs=2)
    assert len(o) > 300 and len(d["pos"]) == len(o) and (d["pos"] == o.pos[:, 0]).all()
    assert np.abs(d["mhl"].astype(np.float64) - o.val).max() <= TOL


@pytest.mark.parametrize("name,min_cpgs,launches,kernels", P.PDR_CASES, ids=["%s-p%d" % (c[0], c[1]) for c in P.PDR_CASES])
def test_pdr_lpmd_form(eng, name, min_cpgs, launches, kernels):
    from metheor_amd import PdrLpmdParams
    bt, reads = batch(name)

    def run():
        eng.pdr_lpmd_accumulate(bt, PdrLpmdParams(min_depth=3, min_cpgs=min_cpgs, min_qual=10, lpmd_min_qual=10, min_distance=2, max_distance=16))
        return eng.pdr_fetch(), eng.lpmd_global()
    (p, l), ran = timed(eng, run)
    assert ran & P.PDR_KERNELS == kernels and ("k_pdr_walk" in ran) == (len(launches) == 2), (name, min_cpgs, sorted(ran))
    o, ol = reads.pdr(min_depth=3, min_cpgs=min_cpgs, min_qual=10), reads.lpmd(min_distance=2, max_distance=16, min_qual=10)
    assert len(o) > (20 if min_cpgs == 4 and name == "A" else 300) and ol["n_concordant"] > 300
    got = np.stack([p["pos"].astype(np.int64), p["n_concordant"].astype(np.int64), p["n_discordant"].astype(np.int64),
                    p["pdr"].view(np.uint32).astype(np.int64)], 1)
    want = np.stack([o.pos[:, 0].astype(np.int64), o.cnt[:, 0].astype(np.int64), o.cnt[:, 1].astype(np.int64),
                     o.val.view(np.uint32).astype(np.int64)], 1)
    assert got.shape == want.shape and (got == want).all(), (name, min_cpgs, got.shape, want.shape)
    assert tuple(int(l[k]) for k in LPMD_KEYS) == tuple(int(ol[k]) for k in LPMD_KEYS)
    a, b = np.float32(l["lpmd"]), np.float32(ol["lpmd"])
    assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)
