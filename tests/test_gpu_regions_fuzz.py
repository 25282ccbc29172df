"""GPU parity of the four per-interval passes (`lpmd --intervals`, `mhl-regions`, `pdr-regions`, `me-regions` / `pm-regions`),
randomised: seeded scenarios -- tests/test_gpu_fuzz.py's reads, or long reads with hundreds of calls -- against interval sets that lean
on the branches of the frame (tests/regions_fuzz_util.py: tilings, windows nested deeper than each LDS cap, thousands of copies of one
line, empty and single-base intervals, boundaries on called positions, open ends, contigs without reads or without intervals), through
the C ABI on host batches, whole contigs or ownership slices, with a grid bound and one differential form of each pass by seed.  The
bars are the per-pass modules' (their check functions): every counter exact, LPMD / PDR / PM / MHL bit for bit, ME within 1e-6 -- against
the restatements of the utility modules (narrowed: tests/test_regions_fuzz_inputs.py ties them to the modules' own and to the oracle's
pinned primitives, and lists which seed reaches which branch)."""
import contextlib
import os

import numpy as np
import pytest

from oracle import pyoracle
from tests import lpmd_intervals_util as L
from tests import mhl_regions_util as M
from tests import regions_fuzz_util as U
from tests import test_gpu_lpmd_intervals as T_lpmd
from tests import test_gpu_mhl_regions as T_mhl
from tests import test_gpu_pairs as T_pairs
from tests import test_gpu_pdr_regions as T_pdr
from tests import test_gpu_quartet_regions as T_quartet
from tests import util

pytestmark = pytest.mark.gpu

KNOBS = ("MTH_REGIONS_GRID", "MTH_PAIRS_FORCE_GLOBAL", "MTH_MHL_REGIONS_LIST", "MTH_PDR_REGIONS_SPAN", "MTH_PDR_REGIONS_LDS_CAP") + T_quartet.KNOBS


@contextlib.contextmanager
def engine(grid=None, form=None):
    """a fresh engine under the grid bound and the form's settings (some are read once per context), and nothing else of KNOBS"""
    import metheor_amd
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(form or {})
    if grid:
        os.environ["MTH_REGIONS_GRID"] = str(grid)
    eng = metheor_amd.Engine(0)
    try:
        yield eng
    finally:
        eng.close()
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def arrays(iv):
    return tuple(np.array([x[k] for x in iv], np.int32) for k in range(3))


def run_lpmd(eng, cs, regions, lk, iv):
    T_pairs.run_device(eng, cs, lk, regions=regions)
    return eng.lpmd_intervals_fetch(*arrays(iv))


def check_lpmd(got, want):
    nc, nd = want
    assert (got["n_concordant"] == nc).all() and (got["n_discordant"] == nd).all()
    assert T_lpmd.same_bits(got["lpmd"], np.array([L.lpmd_f32(c, d) for c, d in zip(nc, nd)], np.float32))


def feed(accumulate, batches, **kw):
    keep = [util.device_batch(sub, region=region) for sub, region in batches]
    for b in keep:
        accumulate(b, **kw)
    return keep


@pytest.mark.parametrize("seed", U.SEEDS)
def test_random_scenario_all_passes(seed):
    s = U.scenario(seed)
    iv, bt = s.iv, U.batches(s)
    reads = pyoracle.Reads.from_soa(*s.soa)
    nar = U.Narrowed(M.Calls.from_soa(*s.soa))
    kw = dict(min_cpgs=s.min_cpgs, min_qual=s.min_qual)

    with engine(s.grid, s.forms["lpmd"]) as eng:
        check_lpmd(run_lpmd(eng, s.cs, s.regions, s.lk, iv), U.reduce_table(U.pairs_table(reads, s.lk), iv))

    with engine(s.grid, s.forms["mhl"]) as eng:
        eng.mhl_regions_begin(*arrays(iv))
        feed(eng.mhl_regions_accumulate, bt, **kw)
        T_mhl.check(eng.mhl_regions_fetch(min_depth=s.min_depth), U.restate_mhl(nar, iv, s.min_depth, **kw), (seed, s.kind))

    with engine(s.grid, s.forms["pdr"]) as eng:
        eng.pdr_regions_begin(*arrays(iv))
        keep = feed(eng.pdr_regions_accumulate, bt, **kw)
        T_pdr.check(eng.pdr_regions_fetch(min_depth=s.min_depth), U.restate_pdr(nar, iv, s.min_depth, **kw), (seed, s.kind))

    with engine(s.grid, s.forms["quartet"]) as eng:
        eng.quartet_regions_begin(*arrays(iv))
        keep = feed(eng.quartet_regions_accumulate, bt, min_qual=s.min_qual)
        want = U.restate_quartet(nar, iv, s.min_depth, s.min_qual)
        T_quartet.check(eng.quartet_regions_fetch(min_depth=s.min_depth), want, (seed, s.kind))
        T_quartet.check_counts(eng.quartet_regions_counts(), want, (seed, s.kind))
    del keep
