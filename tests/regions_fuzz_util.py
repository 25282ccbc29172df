"""What the randomised and the work-item tests of the per-interval passes share (`lpmd --intervals`, `mhl-regions`, `pdr-regions`,
`me-regions` / `pm-regions`): seeded scenarios (tests/test_gpu_fuzz.py's, plus a long-read mode), interval sets that lean on the
branches of the frame (mth_intervals_dev.h, mth_regions_host.h), the restatements of the four utility modules narrowed to the calls an
interval can hold, and a CPU model of what a workgroup meets: its work items in order, and per length class the candidate entries of
each.  Nothing here touches a device.  tests/test_regions_fuzz_inputs.py ties the narrowed forms to the modules' own and shows which
seed reaches which branch."""
import functools

import numpy as np

from tests import lpmd_intervals_util as L
from tests import mhl_regions_util as M
from tests import pdr_regions_util as P
from tests import quartet_regions_util as Q

INT32_MAX = 2 ** 31 - 1
RG_B = 256                       # reads of a work item (mth_intervals_dev.h)
SEEDS = range(48)
GRIDS = (None, 1, 2, 5, 1)       # MTH_REGIONS_GRID, drawn per seed
LPMD_FORMS = ({}, {"MTH_PAIRS_FORCE_GLOBAL": "1"})
MHL_FORMS = ({}, {"MTH_MHL_REGIONS_LIST": "2"})
PDR_FORMS = ({}, {"MTH_PDR_REGIONS_SPAN": "0"}, {"MTH_PDR_REGIONS_LDS_CAP": "4"}, {"MTH_PDR_REGIONS_LDS_CAP": "0"})
QUARTET_FORMS = ({}, {"MTH_QUARTET_REGIONS_LDS_CAP": "4"}, {"MTH_QUARTET_REGIONS_LDS_CAP": "0"}, {"MTH_QUARTET_REGIONS_SUMMARY": "0"}, {"MTH_QUARTET_REGIONS_CARRY": "0"},
                 {"MTH_QUARTET_REGIONS_LDS_CAP": "4", "MTH_QUARTET_REGIONS_SUMMARY": "0", "MTH_QUARTET_REGIONS_CARRY": "0"})
# entries of one length class a workgroup sums in LDS: MR_ACC, QUARTET_REGIONS_LDS_CAP, PDR_REGIONS_LDS_CAP, IV_ACC; starts it stages: IV_LDS
CAPS = dict(mhl=32, quartet=240, pdr=1024, lpmd=1024, lpmd_starts=2048)
WAVE_ROUND = 64 * 64             # entries of a slice above which iv_upper_wave takes a second round
BINS = M.BINS
PACKED_CALLS = 18                # calls of a read the quartet pass packs a histogram for (mth_quartet_regions_dev.h)
MAX_READS, MAX_INTERVALS = 4000, 6000


def length_class(n):
    """IvDomains::add_domain: two bit lengths per class, 1 .. 16 (class 0 of the seventeen holds nothing: no interval has length 0)"""
    return (int(n).bit_length() + 1) // 2


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------------
def long_contig(tid, length, n_reads, density, rng):
    """reads of 2 - 20 kbp with dozens to thousands of calls (synth.make_contig with a length per read); sites are almost always or
    almost never methylated by stretches, so methylated runs pass the 64 lengths of a dense MHL row"""
    from metheor_amd import synth
    sites = synth.make_sites(length, density, rng)
    block = np.cumsum(rng.random(len(sites)) < 0.01)                  # stretches of about a hundred sites share a level
    level = np.where(rng.random(int(block[-1]) + 1 if len(sites) else 1) < 0.75, 0.995, 0.02).astype(np.float32)[block]
    lens = rng.integers(2_000, 20_001, size=n_reads).astype(np.int64)
    starts = np.sort(rng.integers(0, max(length - 2_000, 1), size=n_reads)).astype(np.int64)
    lens = np.minimum(lens, length - starts)
    rev = rng.random(n_reads) < 0.5
    mapq = np.where(rng.random(n_reads) < 0.1, rng.integers(0, 10, size=n_reads), 42).astype(np.uint8)
    lo = np.searchsorted(sites, starts - rev, side="left")
    hi = np.searchsorted(sites, starts + lens - rev, side="left")
    cnt = (hi - lo).astype(np.int64)
    off = np.zeros(n_reads + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    read_of = np.repeat(np.arange(n_reads, dtype=np.int64), cnt)
    site_idx = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1] - lo, cnt)
    pos = sites[site_idx].astype(np.int64)
    meth = rng.random(len(pos), dtype=np.float32) < level[site_idx]
    return dict(tid=tid, length=int(length), read_start=starts.astype(np.int32), read_end=(starts + lens - 1).astype(np.int32), read_mapq=mapq,
                read_fwd=(~rev).astype(np.uint8), cpg_off=off.astype(np.uint32),
                cpg_pos=(pos.astype(np.uint32) | (meth.astype(np.uint32) << np.uint32(31))).astype(np.uint32),
                cpg_rel=(pos - starts[read_of] + rev[read_of]).astype(np.uint16))


def without_minus_one(c):
    """-> (the contig without the reads that call position -1, how many those were): a host batch may not carry that word"""
    from tests import util
    n = np.diff(c["cpg_off"].astype(np.int64))
    bad = np.zeros(len(n), bool)
    w = (c["cpg_pos"] & np.uint32(0x7fffffff)) == np.uint32(0x7fffffff)
    if w.any():
        bad[np.unique(np.repeat(np.arange(len(n)), n)[w])] = True
    return (util.subset_reads(c, ~bad) if bad.any() else c), int(bad.sum())


class Scenario:
    pass


@functools.lru_cache(maxsize=4)
def scenario(seed):
    """tests/test_gpu_fuzz.py's scenario of the seed (every fourth seed: long reads instead), its ownership, parameters, forms and
    intervals"""
    from metheor_amd import shard, synth
    from tests import test_gpu_fuzz as F
    rng, cs, regions, read_len = F.scenario(seed)
    s = Scenario()
    s.seed, s.long = seed, seed % 4 == 3
    if s.long:
        cs = [long_contig(t, int(rng.integers(30_000, 120_000)), int(rng.integers(300, 1500)), float(rng.choice([0.01, 0.03, 0.08])), rng) for t in range(len(cs))]
        regions = [shard.plan_regions(c, int(rng.integers(2, 4))) for c in cs] if regions is not None else None
    s.removed = 0
    out = []
    for c in cs:
        c, k = without_minus_one(c)
        s.removed += k
        out.append(c)
    s.cs, s.regions = out, regions
    s.n_reads = sum(len(c["read_start"]) for c in s.cs)
    assert all(len(c["read_start"]) <= MAX_READS for c in s.cs)
    s.soa = synth.concat_oracle_soa(s.cs)
    s.min_qual = int(rng.choice([0, 10, 10, 43]))
    s.min_cpgs = int(rng.choice([1, 4, 9]))
    s.min_depth = int(rng.choice([0, 3, 10]))
    s.lk = dict(min_distance=int(rng.choice([0, 1, 2, 5])), max_distance=int(rng.choice([1, 4, 16, 60, 300])), min_qual=s.min_qual)
    if s.long:      # (pairs 300 bases apart within reads of 20 kbp: a table of 10^5 rows, ten seconds in the one workgroup of a grid of 1)
        s.lk["max_distance"] = min(s.lk["max_distance"], 60)
    # the grid bound, the differential form of each pass (the default form as likely as all the others together) and the kind of interval
    # set: each drawn on its own, so that long reads, forms and kinds meet in every combination over the seeds
    s.grid = GRIDS[int(rng.integers(0, len(GRIDS)))]
    pick = lambda forms: forms[0] if rng.random() < 0.5 else forms[int(rng.integers(1, len(forms)))]
    s.forms = dict(lpmd=pick(LPMD_FORMS), mhl=pick(MHL_FORMS), pdr=pick(PDR_FORMS), quartet=pick(QUARTET_FORMS))
    s.kind = KINDS[int(rng.integers(0, len(KINDS)))]
    s.iv = intervals(s, rng)
    assert len(s.iv) <= MAX_INTERVALS
    return s


def batches(s):
    """-> [(contig dict of the batch's reads, (region_beg, region_end))]: one batch per contig, or one per ownership slice -- a read is
    owned by the slice that holds its start, so every read counts once"""
    from metheor_amd import shard
    out = []
    for ci, c in enumerate(s.cs):
        for b, e in (s.regions[ci] if s.regions else [(0, c["length"])]):
            out.append((shard.slice_region(c, b, e) if s.regions else c, (b, e)))
    return out


# ---- interval sets -----------------------------------------------------------------------------------------------------------------------
def called(c):
    return np.unique((c["cpg_pos"] & np.uint32(0x7fffffff)).astype(np.int64))


def tiling(t, length, step, rng, at_most=1500):
    b0 = 0 if length // step <= at_most else int(rng.integers(0, length - at_most * step))
    return [(t, b, b + step, None) for b in range(b0, min(length, b0 + at_most * step), step)]


def sliding(t, p, depth):
    """`depth` windows one base apart, one length class, all of which hold position p (when p lies far enough from the contig's start)"""
    s0 = max(p - depth - 10, 0)
    return [(t, s0 + k, s0 + k + depth + 64, None) for k in range(depth)]


def edges(t, c, pos, rng):
    """zero-length and single-base intervals, boundaries on, before and behind called positions, whole-contig and open-ended ones,
    intervals beyond the last read"""
    ln = c["length"]
    iv = [(t, 0, ln, "whole"), (t, 0, INT32_MAX, "open"), (t, ln // 2, INT32_MAX, "open_half"), (t, ln + 100, ln + 1100, "beyond"),
          (t, 0, 0, "empty_0"), (t, 0, 1, "first_base"), (t, INT32_MAX - 1, INT32_MAX, "last_base")]
    if len(pos):
        iv += [(t, int(pos[-1]) + 1, INT32_MAX, "behind_the_last_call"), (t, int(pos[-1]), int(pos[-1]) + 1, "the_last_call")]
        for p in (int(x) for x in rng.choice(pos, size=min(3, len(pos)), replace=False)):
            iv += [(t, p, p, "empty"), (t, p, p + 1, "one_base"), (t, max(p - 1, 0), p, "one_base_before")]
            iv += [(t, max(p + d, 0), p + 150, "start%+d" % d) for d in (-1, 0, 1)] + [(t, max(p - 150, 0), p + d, "end%+d" % d) for d in (-1, 0, 1)]
    return iv


def ladder(t, p):
    """one interval of every length class that can exist: lengths 2^k from 1 to 2^30, from a called position on"""
    return [(t, p, min(p + (1 << k), INT32_MAX), "bits_%d" % (k + 1)) for k in range(0, 31) if p + (1 << k) <= INT32_MAX or k == 30]


def blocks(t, length, k):
    """k disjoint equal intervals with gaps between them: one length class whose single candidate changes along the contig"""
    w = length // (2 * k)
    return [(t, 2 * i * w, 2 * i * w + w + w // 2, "block_%d" % i) for i in range(k)]


KINDS = ("slide_40", "slide_300", "slide_1100", "slide_40_ladder", "slide_2100", "dup_4200", "blocks_dup_40_ladder", "dup_600_blocks")


def intervals(s, rng):
    kind = s.kind
    iv = []
    n_c = len(s.cs)
    bare = 1 if (n_c == 2 and s.seed % 3 == 0) else -1            # a contig with reads and no interval
    for t, c in enumerate(s.cs):
        if t == bare:
            continue
        pos = called(c)
        iv += edges(t, c, pos, rng)
        iv += tiling(t, c["length"], int(rng.choice([20, 50, 200, 1000, 5000])), rng, at_most=1500 // n_c)
        if t > 0:
            continue
        p = int(pos[(2 * len(pos)) // 3]) if len(pos) else c["length"] // 2
        if kind.startswith("slide_"):
            iv += sliding(t, p, int(kind.split("_")[1]))
        if "ladder" in kind:
            iv += ladder(t, p)
        if "dup_" in kind:
            k = int(kind.split("dup_")[1].split("_")[0])
            iv += [(t, max(p - 40, 0), p + 40, "dup")] * k
        iv += blocks(t, c["length"], int(rng.integers(2, 5)) + (2 if "blocks" in kind else 0))
    iv += [(n_c, 0, 5000, "no_reads"), (n_c, 100, 200, None), (n_c, 0, INT32_MAX, "no_reads_open")]        # a contig with intervals and no reads
    order = rng.permutation(len(iv))                               # any order: the table is sorted by the library
    return [iv[i] for i in order]


# ---- the restatements, narrowed ------------------------------------------------------------------------------------------------------------
class Narrowed:
    """a Calls (tests/mhl_regions_util.py) and, per contig, its calls sorted by position: view(t, b, e) is the same Calls whose contig t
    holds only the calls with b <= position < e, in their original order -- what the modules' own masks keep of the contig's calls, found
    by two searches instead of two comparisons per call.  The definition is the modules': their counts_of / histograms run on the view."""

    def __init__(self, calls):
        self.calls, self.order, self.sorted_pos = calls, {}, {}
        for t, idx in calls.by_tid.items():
            o = np.argsort(calls.pos[idx], kind="stable")
            self.sorted_pos[t], self.order[t] = calls.pos[idx][o], idx[o]

    def view(self, t, b, e):
        v = M.Calls.__new__(M.Calls)
        v.__dict__.update(self.calls.__dict__)
        v.by_tid = {}
        if t in self.order:
            lo, hi = np.searchsorted(self.sorted_pos[t], [b, e], side="left")
            v.by_tid = {t: np.sort(self.order[t][lo:hi])}
        return v


def _per_interval(iv, fn):
    memo = {}
    out = []
    for t, b, e, _ in iv:
        if (t, b, e) not in memo:
            memo[t, b, e] = fn(t, b, e)
        out.append(memo[t, b, e])
    return out


def restate_mhl(nar, iv, min_depth, min_cpgs, min_qual):
    """M.restate with the narrowed calls (and one evaluation per distinct line)"""
    out = _per_interval(iv, lambda t, b, e: M.finalise(*M.histograms(nar.view(t, b, e), t, b, e, min_cpgs, min_qual)[:2], min_depth=min_depth))
    return (np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.int64))


def restate_pdr(nar, iv, min_depth, min_cpgs, min_qual):
    """P.restate likewise"""
    k = np.array(_per_interval(iv, lambda t, b, e: P.counts_of(nar.view(t, b, e), t, b, e, min_cpgs, min_qual)), np.int64).reshape(len(iv), 3)
    pdr = np.array([P.finalise(int(m + u), int(d), min_depth) for m, u, d in k], np.float32)
    return pdr, k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()


def restate_quartet(nar, iv, min_depth, min_qual):
    """Q.restate likewise"""
    k = _per_interval(iv, lambda t, b, e: Q.counts_of(nar.view(t, b, e), t, b, e, min_qual))
    bins = np.array([x[0] for x in k], np.int64).reshape(len(iv), 16)
    memo = {}
    f = []
    for b in bins:
        key = b.tobytes()
        if key not in memo:
            memo[key] = Q.finalise(b, min_depth)
        f.append(memo[key])
    return (np.array([x[0] for x in f], np.float32), np.array([x[1] for x in f], np.float32), np.array([x[2] for x in f], np.int64),
            np.array([x[1] for x in k], np.int64), bins)


def reduce_table(table, iv):
    """L.reduce_table with the rows of a contig sorted by cpg1: those with start <= cpg1 < end by two searches, then cpg2 < end by mask
    (cpg1 < cpg2 in every row, so a row with cpg1 >= end is out either way)"""
    tid, p1, p2, c, d = table
    assert (p1 < p2).all()
    per = {}
    for t in set(x[0] for x in iv):
        s = np.nonzero(tid == t)[0]
        o = np.argsort(p1[s], kind="stable")
        per[t] = (s[o], p1[s][o])

    def one(t, b, e):
        rows, key = per[t]
        lo, hi = np.searchsorted(key, [b, e], side="left")
        m = rows[lo:hi]
        m = m[p2[m] < e]
        return int(c[m].sum()), int(d[m].sum())
    out = _per_interval(iv, one)
    return np.array([x[0] for x in out], np.int64), np.array([x[1] for x in out], np.int64)


def pairs_table(reads, lk):
    t = reads.lpmd(pairs=True, **lk)["pairs"]
    return (t.tid.astype(np.int64), t.pos[:, 0].astype(np.int64), t.pos[:, 1].astype(np.int64), t.cnt[:, 0].astype(np.int64), t.cnt[:, 1].astype(np.int64))


def to_records(cs):
    """the contigs as oracle.bamio.Records (one M operation and an XM string per read), for the definition tests' oracle_route"""
    from oracle import bamio
    tid, pos, flag, mapq, cig, xms = [], [], [], [], [], []
    for c in cs:
        n = len(c["read_start"])
        lens = c["read_end"].astype(np.int64) - c["read_start"] + 1
        xo = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=xo[1:])
        xm = np.full(int(xo[-1]), ord("."), np.uint8)
        k = np.diff(c["cpg_off"].astype(np.int64))
        at = np.repeat(xo[:-1], k) + c["cpg_rel"].astype(np.int64)
        xm[at] = np.where(c["cpg_pos"] >> np.uint32(31), ord("Z"), ord("z"))
        raw = xm.tobytes()
        tid += [c["tid"]] * n; pos += c["read_start"].tolist(); flag += np.where(c["read_fwd"] == 1, 0, 16).tolist(); mapq += c["read_mapq"].tolist()
        cig += [[(int(l) << 4) | 0] for l in lens]
        xms += [raw[xo[i]:xo[i + 1]] for i in range(n)]
    refs = [("fz%d" % c["tid"], int(c["length"])) for c in cs]
    return bamio.Records(refs, tid, pos, flag, mapq, cig, xms)


# ---- what a workgroup meets ------------------------------------------------------------------------------------------------------------------
def slices_of(entries):
    """[(start, end)] of one domain -> {class: (start, end, running maximum of the ends) sorted by start}, as IvDomains::add_domain"""
    cls = {}
    for b, e in entries:
        if b < e:
            cls.setdefault(length_class(e - b), []).append((b, e))
    out = {}
    for k, v in cls.items():
        v.sort()
        st, en = np.array([x[0] for x in v], np.int64), np.array([x[1] for x in v], np.int64)
        out[k] = (st, en, np.maximum.accumulate(en))
    return out


def read_spans(calls_pos, off, mapq, start, region, min_qual, need):
    """per read of a batch: its smallest and largest call, and whether the pass takes it (rg_owned_read)"""
    n = np.diff(off)
    first, last = np.full(len(n), INT32_MAX, np.int64), np.full(len(n), -1, np.int64)
    has = n > 0
    if has.any():
        first[has] = np.minimum.reduceat(calls_pos, off[:-1][has])
        last[has] = np.maximum.reduceat(calls_pos, off[:-1][has])
    elig = has & (n >= max(need, 1)) & (mapq >= min_qual) & (start >= region[0]) & (start < region[1])
    return first, last, elig


def work_items(first, last, elig, sl):
    """per work item (RG_B consecutive reads) None when no read is eligible, else (wmin, wmax, {class: (w_min, w_hi)} of the classes with
    candidates): iv_candidates of mth_intervals_dev.h with std::upper_bound for its searches"""
    out = []
    for r0 in range(0, len(first), RG_B):
        m = elig[r0:r0 + RG_B]
        if not m.any():
            out.append(None)
            continue
        wmin, wmax = int(first[r0:r0 + RG_B][m].min()), int(last[r0:r0 + RG_B][m].max())
        cand = {}
        for k, (st, en, mx) in sl.items():
            w_hi = int(np.searchsorted(st, wmax, side="right"))
            if w_hi == 0:
                continue
            w_min = int(np.searchsorted(mx[:w_hi], wmin, side="right"))
            if w_min != w_hi:
                cand[k] = (w_min, w_hi)
        out.append((wmin, wmax, cand))
    return out


def routes(items, sl, k, grid):
    """per workgroup of a launch with `grid` workgroups, what its work items in order meet in class k: ("none",), ("single", entry,
    holds the span) or ("rows", candidates)"""
    n_wg = min(grid or len(items), len(items)) or 1
    out = [[] for _ in range(n_wg)]
    for ch, it in enumerate(items):
        if it is None:
            continue
        wmin, wmax, cand = it
        if k not in cand:
            r = ("none",)
        else:
            w_min, w_hi = cand[k]
            st, en, _ = sl[k]
            r = ("single", w_min, bool(st[w_min] <= wmin and wmax < en[w_min])) if w_hi - w_min == 1 else ("rows", w_hi - w_min)
        out[ch % n_wg].append(r)
    return out


def single_changes(seq):
    """the single candidate of a class changes within one workgroup's sequence: how often"""
    s = [r[1] for r in seq if r[0] == "single"]
    return sum(1 for a, b in zip(s, s[1:]) if a != b)


def point_depth(sl_k, pos):
    """the most entries of a slice that hold one called position: a work item with a read that calls it has at least as many candidates"""
    st, en, _ = sl_k
    if not len(pos):
        return 0
    return int((np.searchsorted(st, pos, side="right") - np.searchsorted(np.sort(en), pos, side="right")).max())
