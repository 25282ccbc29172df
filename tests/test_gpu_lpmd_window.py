"""LPMD window bounds on both sides of the byte form's domain (mth_lpmd_bytes.h: min_distance <= 128, max_distance <= 127; outside
it the kernels count on 16-bit fields): the four LPMD counters equal the oracle's, exactly, for every window of the grid, in the
dense tile kernel, the persistent run form and the hashed-site form; 8-bit and 16-bit relative positions.

One small batch: 150-bp reads with 0..12 calls, runs of calls at adjacent positions, pairs exactly 126..129 bases apart, and last
reads so short that their 8-slot windows end past the call arrays (the clamped loads of the tile that holds them)."""

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

MIN_D = (-1, 0, 1, 2, 127, 128, 129)
MAX_D = (0, 1, 16, 126, 127, 128, 200, 255, 300)
FORMS = {"tile": {"MTH_PDR_WIDE": "0"}, "wide14": {"MTH_PDR_WIDE": "14"}, "runs": {"MTH_PDR_WIDE": "0", "MTH_TILE_RUNS": "1"}}
LPMD_KEYS = ("n_concordant", "n_discordant", "n_read", "n_valid_read")


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


def make_batch(read_len, n_reads=3000, length=40_000, seed=77):
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.integers(0, length - read_len - 2, size=n_reads)).astype(np.int32)
    ncall = rng.integers(0, 13, size=n_reads)
    ncall[-6:] = (2, 3, 5, 1, 4, 2)                       # the batch ends inside the last reads' 8-slot windows
    pos, rel, off = [], [], [0]
    for i in range(n_reads):
        n, kind = int(ncall[i]), i % 4
        if kind == 0:                                     # a run of adjacent positions somewhere in the read, the rest scattered
            run = min(n, int(rng.integers(2, 7)))
            r0 = int(rng.integers(0, read_len - run))
            r = set(range(r0, r0 + run))
            while len(r) < n:
                r.add(int(rng.integers(0, read_len)))
        elif kind == 1 and n >= 2:                        # first and last call an exact distance apart: 126 .. 129 (150-bp reads)
            d = int(rng.choice([126, 127, 128, 129])) if read_len <= 256 else int(rng.choice([127, 128, 255, 256, 290]))
            r0 = int(rng.integers(0, read_len - d))
            r = {r0, r0 + d}
            while len(r) < n:
                r.add(int(rng.integers(r0, r0 + d + 1)))
        else:
            r = set(int(x) for x in rng.choice(read_len, size=n, replace=False))
        r = np.sort(np.fromiter(r, np.int64, len(r)))
        m = (rng.random(len(r)) < (0.85 if rng.random() < 0.5 else 0.15)).astype(np.uint32)
        pos.append((starts[i] + r).astype(np.uint32) | (m << np.uint32(31)))
        rel.append(r)
        off.append(off[-1] + len(r))
    rel = np.concatenate(rel)
    mapq = np.where(rng.random(n_reads) < 0.1, 3, 40).astype(np.uint8)
    c = dict(tid=0, length=length, read_start=starts, read_end=(starts + read_len - 1).astype(np.int32), read_mapq=mapq,
             read_fwd=np.ones(n_reads, np.uint8), cpg_off=np.array(off, np.uint32), cpg_pos=np.concatenate(pos).astype(np.uint32),
             cpg_rel=rel.astype(np.uint8 if read_len <= 256 else np.uint16))
    n = np.diff(np.array(off))
    assert n.max() > 8 and (n == 0).any() and off[-1] - off[-6] < 24
    return c


_cache = {}


def batch_and_oracle(read_len):
    """the batch and, per window of the grid, the oracle's LPMD result (shared by the kernel forms)"""
    if read_len not in _cache:
        from metheor_amd import synth
        c = make_batch(read_len)
        reads = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
        want = {(mi, ma): reads.lpmd(min_distance=mi, max_distance=ma, min_qual=10) for mi in MIN_D for ma in MAX_D}
        # not vacuous: windows inside the byte form's domain, beyond it and empty ones all occur, and the counts differ across the edges
        tot = {k: w["n_concordant"] + w["n_discordant"] for k, w in want.items()}
        assert tot[(2, 16)] > 1000 and tot[(0, 127)] < tot[(0, 128)] < tot[(0, 200)] and tot[(128, 200)] > tot[(129, 200)] > 0
        assert tot[(127, 127)] > 0 and tot[(128, 128)] > 0 and tot[(129, 128)] == 0 and tot[(0, 0)] == 0 and tot[(-1, 1)] == tot[(0, 1)] > 0
        _cache[read_len] = (c, want)
    return _cache[read_len]


def run_grid(eng, monkeypatch, form, read_len):
    from metheor_amd import PdrLpmdParams
    from tests import util
    for k in ("MTH_PDR_WIDE", "MTH_TILE_RUNS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    c, want = batch_and_oracle(read_len)
    bt = util.device_batch(c, region=(0, c["length"]))
    for (mi, ma), w in want.items():
        eng.reset()
        eng.pdr_lpmd_accumulate(bt, PdrLpmdParams(min_depth=0, min_cpgs=0, min_qual=10, min_distance=mi, max_distance=ma, lpmd_min_qual=10))
        g = eng.lpmd_global()
        got = tuple(int(g[k]) for k in LPMD_KEYS)
        assert got == tuple(int(w[k]) for k in LPMD_KEYS), (form, read_len, mi, ma, got, [int(w[k]) for k in LPMD_KEYS])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_window_grid_rel8(eng, monkeypatch, form):
    run_grid(eng, monkeypatch, form, 150)
    assert batch_and_oracle(150)[0]["cpg_rel"].dtype == np.uint8


@pytest.mark.parametrize("form", sorted(FORMS))
def test_window_grid_rel16(eng, monkeypatch, form):
    """300-bp reads: 16-bit relative positions, the instantiations the byte form does not touch"""
    run_grid(eng, monkeypatch, form, 300)
    c = batch_and_oracle(300)[0]
    assert c["cpg_rel"].dtype == np.uint16 and int(c["cpg_rel"].max()) > 255
