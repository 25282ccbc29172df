"""Small batches on either side of the switches of mth_plan.h, and the form each must take with nothing forced in the environment.
tests/test_launch_plan.py asserts the plan on exactly these shapes on the CPU; tests/test_gpu_plan_forms.py runs them and checks that
the launch functions did what the plan says.  numpy only; nothing here computes a measure.

One contig of 131 072 positions (32 dense tiles, 8 slices of 16 384), 100-bp reads unless said otherwise.  With
cand = n_reads * (max_span + 2) / region_len (the reads that can call a site) and cpr = calls per read (about 100 x density):

    contig   reads   density  cand   cpr
    A        12 850  0.0091   10.0   0.9
    B        28 270  0.0091   22.0   0.9
    C        33 410  0.0091   26.0   0.9
    D        17 990  0.0091   14.0   0.9
    E        23 130  0.0091   18.0   0.9
    F        12 850  0.018    10.0   1.77
    G        12 850  0.023    10.0   2.25
    H        12 850  0.05     10.0   4.8
    I        12 850  0.075    10.0   7.0
    J         4 300  0.0091    9.9   2.7    300-bp reads: max_span 300, 16-bit relative positions
"""
import numpy as np

from metheor_amd import synth

LENGTH = 131072
CONTIGS = {
    "A": (12850, 0.0091, 100), "B": (28270, 0.0091, 100), "C": (33410, 0.0091, 100), "D": (17990, 0.0091, 100),
    "E": (23130, 0.0091, 100), "F": (12850, 0.018, 100), "G": (12850, 0.023, 100), "H": (12850, 0.05, 100),
    "I": (12850, 0.075, 100), "J": (4300, 0.0091, 300),
}

FDRP_KERNELS = {"k_fdrp_wtile", "k_fdrp_walk4", "k_fdrp_tile", "k_fdrp_chain"}      # (k_fdrp_walk runs behind every form)
WTILE, WALK4, TILE, WALK = {"k_fdrp_wtile"}, {"k_fdrp_walk4"}, {"k_fdrp_tile", "k_fdrp_chain"}, set()

# (contig, max_depth) -> plan fields (win only where walk4 runs) and the FDRP kernels beside k_fdrp_walk
#   wtile: cpr <= 2, max_span <= 200, cand <= 24 and cand + 4 sqrt(cand) <= max_depth; walk4: else cand <= 16 and cpr <= 6; else tile
FDRP_CASES = [
    ("A", 40, dict(wtile=1, dense=0, walk4=0, tile=0), WTILE),             # 10 + 12.6 = 22.6 <= 40
    ("A", 20, dict(wtile=0, dense=0, walk4=16, tile=0, win=32), WALK4),    # 22.6 > 20; 0.009 x 402 = 3.7 sites a window
    ("B", 64, dict(wtile=1, dense=0, walk4=0, tile=0), WTILE),             # cand 22 <= 24; 22 + 18.8 = 40.8 <= 64
    ("C", 64, dict(wtile=0, dense=0, walk4=0, tile=1), TILE),              # cand 26 > 24 (and > 16)
    ("D", 20, dict(wtile=0, dense=0, walk4=16, tile=0, win=32), WALK4),    # cand 14 <= 16; 14 + 15 = 29 > 20
    ("E", 20, dict(wtile=0, dense=0, walk4=0, tile=1), TILE),              # cand 18 > 16
    ("F", 40, dict(wtile=1, dense=0, walk4=0, tile=0), WTILE),             # 1.77 calls a read <= 2
    ("G", 40, dict(wtile=0, dense=0, walk4=16, tile=0, win=32), WALK4),    # 2.25 calls a read > 2; 0.0225 x 402 = 9.0 <= 12
    ("H", 40, dict(wtile=0, dense=0, walk4=16, tile=0, win=64), WALK4),    # 0.048 x 402 = 19 > 12
    ("I", 40, dict(wtile=0, dense=1, walk4=0, tile=1), TILE),              # 7 calls a read > 6: the 16-register walk, no walk4
    ("J", 40, dict(wtile=0, dense=0, walk4=0, tile=0), WALK),              # max_span 300 > 200: the general walk alone
]

# contig -> rowchk (calls a read <= 1.8)
MHL_CASES = [("A", dict(rowchk=1)), ("G", dict(rowchk=0)), ("J", dict(rowchk=0))]

PDR_KERNELS = {"k_pdr_lpmd_tile", "k_pdr_lpmd_wide"}
# (contig, min_cpgs) -> the plans of the launches the call makes, as (has_sink, want_pdr, wide_shift), and the tile kernels that run.
#   wide: calls per read and position <= 0.012, reads per 4096 bp <= 900, expected insertions per read <= 0.6; 131 072 >> 15 is fewer
#   than 3584 tiles: the slice drops to 16 384
PDR_CASES = [
    ("A", 4, [(0, 1, 14)], {"k_pdr_lpmd_wide"}),          # 0.91 P(N >= 3) = 0.06 insertions a read
    ("A", 1, [(0, 1, 0)], {"k_pdr_lpmd_tile"}),           # every call is inserted: 0.91 > 0.6
    ("G", 4, [(0, 1, 0)], {"k_pdr_lpmd_tile"}),           # 0.0225 calls per read and position > 0.012
    # max_span 300 > 150: LPMD alone through the tile pass (nothing inserted: wide), PDR by the exact walk behind a discovery pass
    # through a sink (2.7 P(N >= 3) = 1.37 insertions a read: dense)
    ("J", 4, [(0, 0, 14), (1, 1, 0)], {"k_pdr_lpmd_wide", "k_pdr_lpmd_tile"}),
]

_cache = {}


def contig(name):
    """the contig of CONTIGS[name], generated once (never modified)"""
    if name not in _cache:
        n, density, read_len = CONTIGS[name]
        rng = np.random.default_rng(1000 + ord(name))
        _cache[name] = synth.make_contig(0, LENGTH, n, density, rng, read_len=read_len)
    return _cache[name]


def shape(name):
    """the four figures the plan reads, as the batch over the whole contig carries them, and whether its relative positions are 8-bit"""
    c = contig(name)
    span = int((c["read_end"].astype(np.int64) - c["read_start"]).max()) + 1
    return dict(n_reads=len(c["read_start"]), n_cpgs=int(c["cpg_off"][-1]), max_span=span, region_beg=0, region_end=LENGTH,
                rel8=int(c["cpg_rel"].dtype == np.uint8))
