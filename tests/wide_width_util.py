"""Inputs for the hashed-site tile pass at a narrowed tile width (TileArgs::tile_w_rt, mth_pdr_wide.hip) and a plain restatement of
the host rule that picks the width (plan_pdr_lpmd in mth_plan.h, "Wide form: the tile need not be as wide as its slice";
tests/test_launch_plan.py compares the two).  numpy only; nothing
here computes a measure.  tests/test_wide_width_inputs.py shows on the CPU that the inputs hold what they claim,
tests/test_gpu_wide_width.py runs them."""
import math

import numpy as np

from metheor_amd import synth

# every (slice shift, tile width) pair the GPU tests force with MTH_PDR_WIDE / MTH_PDR_WIDE_W
FORCED = [(14, 1024), (14, 4160), (14, 8192), (14, 8960), (14, 16320), (15, 16448), (15, 23936), (16, 46336), (16, 65472)]
WIDTHS = tuple(w for _, w in FORCED)
SPECIAL_W = 8960            # the width the dense stretch and the pile are placed for
SHORT_LAST = (2, 3, 5, 1, 4, 2)
SLOTS = 7 * 256             # resident workgroups of the wide form


def narrowed_width(region_len, shift):
    """the tile width plan_pdr_lpmd (mth_plan.h) chooses by itself for a region of region_len positions under 2^shift-position slices; 0 where
    the tile stays as wide as its slice"""
    tile_w = 1 << shift
    rounds = float(region_len) / float(tile_w) / float(SLOTS)
    frac = rounds - math.floor(rounds)
    if not (1.0 < rounds < 8.0 and 0.02 < frac < 0.5):
        return 0
    w = int(math.ceil(float(region_len) / (math.ceil(rounds) * float(SLOTS))))
    w = (w + 63) & ~63
    return w if tile_w // 2 <= w < tile_w else 0


def _tail(T, L):
    """the batch's final six reads -> (starts, sites, contig length): a chain in which every read shares its last site with the next
    one, so that a tile boundary anywhere between the first and the last site has a read with calls on both sides of it.  A forward
    read started at s calls the sites in [s, s + L), a reverse one those in [s - 1, s + L - 1): every site keeps at least two positions
    from each window edge it must be inside or outside of, so the reads call SHORT_LAST = 2, 3, 5, 1, 4, 2 sites whichever strand the
    generator draws (boundary_batch asserts the counts)."""
    s0 = T
    r0 = [s0 + 4, s0 + L - 6]                                  # read 0: 2 calls, one at either end of its window
    s1 = r0[-1] - 3                                            # read 1 starts just below read 0's last site ...
    r1 = [r0[-1], s0 + L + 2, s1 + L - 6]                      # ... 3 calls: that site, one just past read 0's window, one at its own end
    s2 = r1[-1] - 3
    first = s1 + L + 2                                         # (just past read 1's window)
    r2 = [r1[-1], first, first + 4, first + 8, s2 + L - 6]     # read 2: 5 calls
    s3 = r2[-1] - 12                                           # read 3: 1 call, read 2's last site (the next site lies past its window)
    r3 = [r2[-1]]
    s4 = r2[-1] - 3                                            # read 4 starts 9 positions later: its window ends 9 positions later
    first = s3 + L + 1                                         # (just past read 3's window, inside read 4's)
    r4 = [r2[-1], first, first + 2, first + 4]                 # read 4: 4 calls
    s5 = r4[-1]                                                # read 5 starts at read 4's last site (its last but one is 2 below)
    r5 = [r4[-1], s5 + L - 6]                                  # read 5: 2 calls
    assert tuple(len(r) for r in (r0, r1, r2, r3, r4, r5)) == SHORT_LAST
    return [s0, s1, s2, s3, s4, s5], sorted(set(r0 + r1 + r2 + r3 + r4 + r5)), s5 + L + 2


def _free(lo, hi, taken):
    return all(hi < a or lo > b for a, b in taken)


def boundary_batch(read_len, widths=WIDTHS, seed=1):
    """-> (contig, meta).  One contig of about 300 kbp: a uniform background (CpG density 0.03, depth about 15) and, planted on it,

      * for every width w and k in {1, 2, last}: with B = k * w, CpG sites at B - 6, B - 1, B + 1 and B + 6, reads that start at
        exactly B - 1, B and B + 1, and reads from B - 60 whose four consecutive calls straddle B ("last" is the last boundary that
        still lies in the background; a boundary inside the hand-placed tail carries no planted sites);
      * a dense stretch: a CpG every 2 bp over 3 kbp across a boundary B of SPECIAL_W, [B - 2301, B + 697] -- off-centre, so that
        ONE tile of that width holds more distinct sites than the site table's 1024 slots and more distinct quartets than the fused
        pass's 512, and its reads carry far more than 8 calls;
      * a pile: 3 500 reads starting within 100 bp across another boundary of SPECIAL_W, 3 220 of them inside one tile (more
        candidates in one stretch than the 3072- and 2048-read queues hold);
      * a site within 40 bp on either side of every other interior boundary of every width (the background has gaps wider than a read);
      * a read without any call (in a hole with no boundary of any width within 50 bp);
      * the final six reads with SHORT_LAST calls: the batch ends inside their 8-slot windows.

    meta: length, planted (the boundaries B), dense (lo, hi, B), pile (B), hole (read start), tail (first start of the final six),
    no_true_last (the widths whose true last interior boundary lies in the tail, so that "last" is the one before it)"""
    rng = np.random.default_rng(seed)
    L = int(read_len)
    ws = sorted(set(int(w) for w in widths) | {SPECIAL_W})
    # where the tail begins: as many widths as possible keep their true last interior boundary in the background
    best = None
    for T in range(300_000, 301_100, 3):
        length = _tail(T, L)[2]
        ok = sum(1 for w in ws if ((length - 1) // w) * w <= T - 80)
        if best is None or ok > best[0]:
            best = (ok, T)
        if ok == len(ws):
            break
    T = best[1]
    tail_starts, tail_sites, length = _tail(T, L)
    no_true_last = [w for w in ws if ((length - 1) // w) * w > T - 80]       # (the tail is five reads long: 1024 under 300-bp reads)
    planted = sorted({k * w for w in ws for k in (1, 2, (T - 80) // w) if 0 < k * w <= T - 80})
    taken = [(B - L - 80, B + L + 80) for B in planted]
    # the dense stretch and the pile: boundaries of SPECIAL_W whose surroundings are free
    kd = next(k for k in range(5, 30) if _free(k * SPECIAL_W - 2301 - L, k * SPECIAL_W + 697 + L, taken))
    Bd = kd * SPECIAL_W
    dense = (Bd - 2301, Bd + 697)
    taken.append((dense[0] - L, dense[1] + L))
    kp = next(k for k in range(kd + 2, 33) if _free(k * SPECIAL_W - 400 - L, k * SPECIAL_W + 400 + L, taken))
    Bp = kp * SPECIAL_W
    taken.append((Bp - 400 - L, Bp + 400 + L))
    hole = next(h for h in range(100_000, 250_000, 7)
                if _free(h - L, h + 2 * L, taken) and all((h - 50) // w == (h + L + 50) // w for w in ws))
    taken.append((hole - 4, hole + L + 4))

    add = set(tail_sites) | set(range(dense[0], dense[1] + 1, 2))
    for B in planted:
        add |= {B - 6, B - 1, B + 1, B + 6}
    add = np.array(sorted(add), np.int64)
    bg = synth.make_sites(T, 0.03, rng).astype(np.int64)
    bg = bg[bg < T - 2]
    near = np.searchsorted(add, bg - 1, side="left") < np.searchsorted(add, bg + 1, side="right")      # a planted site within 1
    in_dense = (bg >= dense[0] - 1) & (bg <= dense[1] + 1)
    near_B = np.zeros(len(bg), bool)
    for B in planted:
        near_B |= (bg >= B - 8) & (bg <= B + 8)
    in_hole = (bg >= hole - 2) & (bg <= hole + L + 2)
    sites = np.unique(np.concatenate([bg[~(near | in_dense | near_B | in_hole)], add]))
    # the background leaves gaps wider than a read: every other interior boundary gets a site within 40 bp on either side
    extra = []
    for B in sorted({B for w in ws for B in interior_boundaries(T, w)} - set(planted)):
        i = int(np.searchsorted(sites, B))
        if i == 0 or sites[i - 1] < B - 40:
            extra.append(B - 21)
        if i == len(sites) or sites[i] > B + 40:
            extra.append(B + 20)
    sites = np.unique(np.concatenate([sites, np.array(extra, np.int64)]))
    assert np.diff(sites).min() >= 2

    n_bg = 300_000 * 15 // L
    parts = [rng.integers(0, T, size=n_bg), np.array([hole]), Bp - 8 + (np.arange(3500) % 100), np.array(tail_starts)]
    for B in planted:
        parts.append(np.array([B - 1, B - 1, B, B, B + 1, B + 1, B - 60, B - 60, B - 60, B - 60]))
    starts = np.sort(np.concatenate(parts)).astype(np.int32)
    c = synth.make_contig(0, length, len(starts), 0.03, rng, read_len=L, sites=sites.astype(np.int32), starts=starts, low_mapq_frac=0.03)
    ncall = np.diff(c["cpg_off"].astype(np.int64))
    assert tuple(ncall[-6:]) == SHORT_LAST and int(c["read_end"].max()) < length
    return c, dict(length=length, planted=planted, dense=(dense[0], dense[1], Bd), pile=Bp, hole=hole, tail=T, no_true_last=no_true_last)


def interior_boundaries(length, w):
    return range(w, length, w)


def off_grid_regions(length, w):
    """regions that cover [0, length) with every cut off every grid (no region but the first begins at a multiple of 64): a lead region
    of 997 positions (shorter than any width), then 3 w, 3 w + 1 and 3 w - 1 positions, then the rest"""
    cuts = [0]
    for n in (997, 3 * w, 3 * w + 1, 3 * w - 1):
        if cuts[-1] + n < length:
            cuts.append(cuts[-1] + n)
    cuts.append(length)
    regs = list(zip(cuts[:-1], cuts[1:]))
    assert all(b % 64 for b, _ in regs[1:]) and any(e - b < w for b, e in regs)
    return regs


def long_sparse_contig(length, width, seed=1):
    """-> (contig, cluster centres).  A contig long enough for the host's own width rule (density 0.0091, 150-bp reads, at most 35 000
    of them): six clusters of 5 000 reads, each spread over +-15 kbp around a multiple B of `width` (of 16384 where width is 0) -- the
    first, the last interior one and four between --, 3 000 reads in the first 20 kbp, 1 000 single reads anywhere and one read that
    ends at the contig's end.  At that density few reads pass min_cpgs = 4, so every centre B also gets six CpG sites within 33 bp
    (B - 1 and B + 1 among them) and reads that start at exactly B - 1, B and B + 1: rows and owned reads right at the boundary."""
    rng = np.random.default_rng(seed)
    step = int(width) if width else 16384
    nb = (length - 1) // step
    ks = sorted({1, nb // 5, (2 * nb) // 5, (3 * nb) // 5, (4 * nb) // 5, nb})
    parts = [np.clip(k * step + rng.integers(-15_000, 15_000, size=5_000), 0, length - 150) for k in ks]
    parts += [rng.integers(0, 20_000, size=3_000), rng.integers(0, length - 150, size=1_000), np.array([length - 150])]
    parts += [np.array([k * step - 1, k * step, k * step + 1]) for k in ks]
    starts = np.sort(np.concatenate(parts)).astype(np.int32)
    assert len(starts) <= 35_000
    sites = synth.make_sites(length, 0.0091, rng).astype(np.int64)
    for k in ks:
        B = k * step
        sites = np.concatenate([sites[(sites < B - 40) | (sites > B + 40)], B + np.array([-30, -12, -1, 1, 14, 33])])
    sites = np.unique(sites)
    assert np.diff(sites).min() >= 2
    c = synth.make_contig(0, length, len(starts), 0.0091, rng, sites=sites.astype(np.int32), starts=starts)
    return c, [k * step for k in ks]


def chooser_figures(c, min_cpgs=4):
    """the two quantities the density chooser of plan_pdr_lpmd (mth_plan.h) weighs: calls per read per position of the span, and the expected
    insertions per read E[n; n >= min_cpgs] for Poisson calls"""
    n_reads = len(c["read_start"])
    lam = float(c["cpg_off"][-1]) / n_reads
    span = int((c["read_end"].astype(np.int64) - c["read_start"]).max()) + 1
    term, cdf = math.exp(-lam), 0.0
    for k in range(max(min_cpgs, 1) - 1):
        cdf += term
        term *= lam / (k + 1)
    return lam / span, lam * max(0.0, 1.0 - cdf)
