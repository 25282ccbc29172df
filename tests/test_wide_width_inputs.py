"""The inputs of tests/test_gpu_wide_width.py on the CPU (tests/wide_width_util.py): the restated width rule gives the widths worked
out by hand from the rule of plan_pdr_lpmd (mth_plan.h), and the generated batches hold every feature the GPU cases rely on -- calls, read starts and
quartets on both sides of every narrowed tile boundary, a tile with more distinct sites and quartets than the LDS tables hold, a tile
with more candidate reads than the queues hold, reads with no call and with more than 8, a batch that ends inside its last reads'
8-slot windows, and long contigs that stay in the chooser's sparse branch -- so that a later edit cannot quietly make them trivial."""
import numpy as np
import pytest

from metheor_amd import synth
from oracle import pyoracle
from tests import wide_width_util as W


# ---- the width rule: 1792 slots, 1 < rounds < 8, 0.02 < frac < 0.5, ceil(len / (ceil(rounds) * 1792)) rounded up to 64, in [w/2, w) ----
@pytest.mark.parametrize("region_len,shift,want", [
    (29_360_128, 14, 0),            # exactly one round (16384 * 1792): rounds is not > 1
    (30_000_000, 14, 8384),         # 1.0218 rounds; ceil(30e6 / 3584) = 8371 -> 8384
    (32_000_000, 14, 8960),         # 1.0899 rounds; 8929 -> 8960
    (40_000_000, 14, 11200),        # 1.3624 rounds; 11161 -> 11200
    (45_000_000, 14, 0),            # 1.5327 rounds: the last round is more than half full
    (60_000_000, 14, 11200),        # 2.0436 rounds; ceil(60e6 / 5376) = 11161 -> 11200
    (75_000_000, 14, 0),            # 2.5545 rounds
    (248_956_422, 16, 46336),       # chr1: 2.1198 rounds; ceil(len / 5376) = 46309 -> 46336
])
def test_narrowed_width_pins(region_len, shift, want):
    assert W.narrowed_width(region_len, shift) == want


def test_forced_pairs_are_in_the_knobs_domain():
    """MTH_PDR_WIDE_W takes [1024, slice width), rounded down to a multiple of 64: every forced width is one it takes as it is"""
    for shift, w in W.FORCED:
        assert 1024 <= w < (1 << shift) and w % 64 == 0, (shift, w)
    assert {s for s, _ in W.FORCED} == {14, 15, 16}


@pytest.fixture(scope="module", params=[150, 300])
def batch(request):
    c, meta = W.boundary_batch(request.param)
    rd = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
    return request.param, c, meta, rd


def _calls(c):
    off = c["cpg_off"].astype(np.int64)
    pos = (c["cpg_pos"] & 0x7fffffff).astype(np.int64)
    n = np.diff(off)
    has = n > 0
    first = np.where(has, pos[np.minimum(off[:-1], len(pos) - 1)], np.iinfo(np.int64).max)
    last = np.where(has, pos[np.maximum(off[1:] - 1, 0)], -1)
    return n, first, last


def test_boundary_batch_shape(batch):
    read_len, c, meta, rd = batch
    n, _, _ = _calls(c)
    assert 299_000 < meta["length"] < 304_000 and 15_000 < len(n) < 36_000
    assert c["cpg_rel"].dtype == (np.uint8 if read_len == 150 else np.uint16)
    assert int((c["read_end"] - c["read_start"]).max()) + 1 == read_len
    assert (np.diff(c["read_start"]) >= 0).all()
    assert n.max() > 8 and (n == 0).any()
    assert tuple(n[-6:]) == W.SHORT_LAST and int(c["cpg_off"][-1]) - int(c["cpg_off"][-7]) < 24
    assert len(rd.pdr(min_depth=3, min_cpgs=2)) > 5000 and len(rd.me(min_depth=0)) > 4000 and len(rd.mhl(min_depth=3, min_cpgs=2)) > 5000


def test_every_interior_boundary_is_straddled(batch):
    """at every interior boundary of every width some read has calls on both sides (first call < B <= last call)"""
    _, c, meta, _ = batch
    _, first, last = _calls(c)
    for w in W.WIDTHS:
        for B in W.interior_boundaries(meta["length"], w):
            assert ((first < B) & (last >= B)).any(), (w, B)


def test_planted_boundaries(batch):
    read_len, c, meta, rd = batch
    planted = meta["planted"]
    # k = 1, 2 and the true last interior boundary of every width; only 1024 under 300-bp reads, whose tail of five read lengths is
    # longer than that width, takes the last boundary before the tail instead
    assert meta["no_true_last"] == ([] if read_len == 150 else [1024])
    for w in W.WIDTHS:
        last = ((meta["length"] - 1) // w) * w if w not in meta["no_true_last"] else ((meta["tail"] - 80) // w) * w
        assert {w, 2 * w, last} <= set(planted), (w, last)
    pdr = rd.pdr(min_depth=3, min_cpgs=2, min_qual=10)
    depth = dict(zip(pdr.pos[:, 0].tolist(), pdr.cnt.sum(1).tolist()))
    me = rd.me(min_depth=0, min_qual=10)
    starts = set(c["read_start"].tolist())
    for B in planted:
        assert depth.get(B - 1, 0) >= 3 and depth.get(B + 1, 0) >= 3, B
        assert {B - 1, B, B + 1} <= starts, B
        assert ((me.pos[:, 0] < B) & (me.pos[:, 3] >= B)).any(), B


def test_dense_stretch_and_pile(batch):
    _, c, meta, rd = batch
    w = W.SPECIAL_W
    lo, hi, Bd = meta["dense"]
    assert Bd % w == 0 and lo < Bd < hi
    pdr = rd.pdr(min_depth=3, min_cpgs=2, min_qual=10)
    t0 = Bd - w                                                 # the tile below the boundary
    assert ((pdr.pos[:, 0] >= t0) & (pdr.pos[:, 0] < Bd)).sum() > 1024
    assert ((pdr.pos[:, 0] >= Bd) & (pdr.pos[:, 0] <= hi)).sum() > 300          # and the stretch goes on in the next tile
    me = rd.me(min_depth=0, min_qual=10)
    assert ((me.pos[:, 0] >= t0) & (me.pos[:, 0] < Bd)).sum() > 512
    Bp = meta["pile"]
    assert Bp % w == 0
    s = c["read_start"]
    assert ((s >= Bp) & (s < Bp + w)).sum() > 3072 and ((s >= Bp - 100) & (s < Bp)).sum() > 100


def test_off_grid_regions():
    length = W.boundary_batch(150)[1]["length"]
    for _, w in W.FORCED:
        regs = W.off_grid_regions(length, w)
        assert regs[0][0] == 0 and regs[-1][1] == length and all(a[1] == b[0] for a, b in zip(regs, regs[1:]))
        assert all(b % 64 != 0 for b, _ in regs[1:]) and min(e - b for b, e in regs) < w
        lens = [e - b for b, e in regs]
        if 997 + 9 * w + 1 < length:
            assert lens[1:4] == [3 * w, 3 * w + 1, 3 * w - 1]


@pytest.mark.parametrize("length", [32_000_000, 40_000_000, 45_000_000])
def test_long_sparse_contig(length):
    width = W.narrowed_width(length, 14)
    assert width == {32_000_000: 8960, 40_000_000: 11200, 45_000_000: 0}[length]
    c, centres = W.long_sparse_contig(length, width)
    n = len(c["read_start"])
    assert 25_000 <= n <= 35_000 and int(c["read_end"].max()) == length - 1 and c["cpg_rel"].dtype == np.uint8
    # the chooser's sparse branch under min_cpgs = 4, and no drop to a narrower slice than 16384
    sites_per_bp, ins_per_read = W.chooser_figures(c, 4)
    assert sites_per_bp <= 0.012 and ins_per_read <= 0.6, (sites_per_bp, ins_per_read)
    assert n / length * 4096.0 <= 900.0
    step = width or 16384
    assert len(centres) >= 5 and centres[0] == step and centres[-1] == ((length - 1) // step) * step
    s = c["read_start"].astype(np.int64)
    for B in centres:
        assert ((s >= B - 15_000) & (s < B + 15_000)).sum() >= 5_000, B
    rd = pyoracle.Reads.from_soa(*synth.to_oracle_soa(c))
    pdr = rd.pdr(min_depth=3, min_cpgs=4, min_qual=10)
    me = rd.me(min_depth=0, min_qual=10)
    assert len(pdr) >= 300 and len(me) >= 100, (len(pdr), len(me))
    at = (pdr.pos[:, 0].astype(np.int64) + 150) // step                 # the boundary a row lies within 150 bp of, if any
    near_b = {int(m) for m, p in zip(at, pdr.pos[:, 0].astype(np.int64)) if m >= 1 and m != (p - 150) // step}
    assert len(near_b) >= 3, near_b
    rows, starts = set(pdr.pos[:, 0].tolist()), set(s.tolist())
    for B in centres:                   # a row at the last position of the tile below B, and reads owned on both sides of B
        assert B - 1 in rows and B + 1 in rows and {B - 1, B, B + 1} <= starts, B
        assert ((me.pos[:, 0] < B) & (me.pos[:, 3] >= B)).any(), B
