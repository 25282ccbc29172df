"""Inputs and expectations shared by the per-interval MHL tests (`metheor mhl-regions`, `all --mhl-intervals`, mth_mhl_regions_*): the
CPU restatement of the definition in numpy on the oracle's decoded reads, float32 step by step; the same value
by the route through the oracle's pinned primitives; the records, the interval set and the file the command line writes.  Nothing here
touches a device.

Definition.  For an interval [start, end) on contig c take each record once: keep the calls with start <= abspos < end on c
(filter_isin, readutil.rs:87-94, with the set "every position of the interval"); with n calls kept the read contributes if
mapq >= min_qual and n >= max(min_cpgs, 1) (mhl.rs:176-183); a contributing read adds n to num_cpgs and its get_stretch_info()
(readutil.rs:147-164) to stretch_info (mhl.rs:75-80, 36-41); the value is compute_mhl() (mhl.rs:43-73), NaN below max(min_depth, 1)
contributing reads."""
import functools

import numpy as np

from oracle import bamio, pyoracle
from tests import lpmd_intervals_util as L

REFS, NAMES, INT32_MAX = L.REFS, L.NAMES, L.INT32_MAX
HEADER = "chrom\tstart\tend\tname\tmhl\tn_reads\tmax_cpgs\n"
DEFAULT_KW = dict(min_depth=10, min_cpgs=4, min_qual=10)
BINS = 64                                   # MHL_REGIONS_BINS (mth_knobs.h): lengths of a dense per-interval row
LONG_AT, LONG_LEN, LONG_STEP = 20_000, 2_000, 20       # the long reads: contig ivB, a call every 20 bases -> 100 calls


def _long_xm(pattern):
    b = bytearray(b"." * LONG_LEN)
    for k, m in enumerate(pattern):
        b[k * LONG_STEP + 3] = ord("Z" if m else "z")
    return bytes(b)


@functools.lru_cache(maxsize=None)
def records():
    """the records of the per-interval LPMD tests (indels, reverse reads calling at -1, the 180x island) plus two reads of 2 kbp
    with 100 calls each: one with a methylated run of 70 (longer than a dense row) and shorter ones, one with another pattern"""
    r = L.records()
    n_calls = LONG_LEN // LONG_STEP
    pat_a = [1] * 70 + [0] + [1] * 5 + [0, 0] + [1] * 22
    pat_b = [(k % 7) != 0 for k in range(n_calls)]
    assert len(pat_a) == n_calls == 100
    tid, pos, flag, mapq = r.tid.tolist(), r.pos.tolist(), r.flag.tolist(), r.mapq.tolist()
    cig, xms = list(r.cigars), list(r.xms)
    for pat in (pat_a, pat_b):
        tid.append(1); pos.append(LONG_AT); flag.append(0); mapq.append(42); cig.append([(LONG_LEN << 4) | 0]); xms.append(_long_xm(pat))
    order = sorted(range(len(tid)), key=lambda i: (tid[i], pos[i], i))
    return bamio.Records(REFS, [tid[i] for i in order], [pos[i] for i in order], [flag[i] for i in order], [mapq[i] for i in order],
                         [cig[i] for i in order], [xms[i] for i in order])


class Calls:
    """the decoded reads flattened: per call its read, contig, position (-1 for the word of position -1) and state"""

    def __init__(self, rec, cpg_set=None):
        self._fill(pyoracle.Reads.decode(rec, cpg_set=cpg_set).soa())

    @classmethod
    def from_soa(cls, *soa):
        """the same of reads that never were records: the argument tuple of pyoracle.Reads.from_soa, through the oracle and back"""
        c = cls.__new__(cls)
        c._fill(pyoracle.Reads.from_soa(*soa).soa())
        return c

    def _fill(self, s):
        off = s["cpg_off"].astype(np.int64)
        self.n_reads = len(s["tid"])
        self.read = np.repeat(np.arange(self.n_reads), np.diff(off))
        self.tid = s["tid"].astype(np.int64)[self.read]
        w = s["cpg_pos"]
        p = (w & 0x7fffffff).astype(np.int64)
        self.pos = np.where(p == 0x7fffffff, -1, p)
        self.meth = (w >> 31).astype(bool)
        self.mapq = s["mapq"].astype(np.int64)
        self.by_tid = {int(t): np.nonzero(self.tid == t)[0] for t in np.unique(self.tid)}


@functools.lru_cache(maxsize=None)
def default_calls():
    return Calls(records())


def histograms(calls, t, b, e, min_cpgs=4, min_qual=10):
    """-> (R, C, n_per_read of the contributing reads in record order): R[r] maximal methylated runs of length r among the kept calls
    of the contributing reads, C[n] contributing reads with n kept calls (index 0 unused)"""
    idx = calls.by_tid.get(t, np.zeros(0, np.int64))
    idx = idx[(calls.pos[idx] >= b) & (calls.pos[idx] < e)]              # original order: the calls of a read stay together
    rd, m = calls.read[idx], calls.meth[idx]
    n_per = np.bincount(rd, minlength=calls.n_reads)
    contrib = (calls.mapq >= min_qual) & (n_per >= max(min_cpgs, 1))
    ok = contrib[rd]
    rd, m = rd[ok], m[ok]
    n_list = n_per[contrib]
    C = np.bincount(n_list) if len(n_list) else np.zeros(1, np.int64)
    if len(rd):
        same_prev = np.r_[False, rd[1:] == rd[:-1]]
        same_next = np.r_[rd[:-1] == rd[1:], False]
        first = m & ~(np.r_[False, m[:-1]] & same_prev)
        last = m & ~(np.r_[m[1:], False] & same_next)
        lengths = np.nonzero(last)[0] - np.nonzero(first)[0] + 1
        R = np.bincount(lengths) if len(lengths) else np.zeros(1, np.int64)
    else:
        R = np.zeros(1, np.int64)
    return R.astype(np.int64), C.astype(np.int64), n_list


def suffix_windows(H, top):
    """out[l] = sum over k >= l of H[k] (k - l + 1), l = 1..top, as Python integers (exact)"""
    out = [0] * (top + 2)
    cnt = acc = 0
    for l in range(top, 0, -1):
        cnt += int(H[l]) if l < len(H) else 0
        acc += cnt
        out[l] = acc
    return out


def finalise(R, C, min_depth=10, denominators=None):
    """compute_mhl (mhl.rs:43-73) from the histograms, float32 step by step -> (mhl f32, n_reads, max_cpgs).  denominators: per l the
    f32 to divide by instead of the exact integer converted once (the reference's read-order sum)"""
    n_reads = int(C[1:].sum())
    maxn = int(np.nonzero(C)[0].max()) if n_reads else 0
    if n_reads < max(min_depth, 1):
        return np.float32(np.nan), n_reads, maxn
    top = max(maxn, len(R) - 1)
    S, D = suffix_windows(R, top), suffix_windows(C, top)
    l_sum = np.float32(0)
    for l in range(1, maxn + 1):
        l_sum = np.float32(l_sum + np.float32(l))
    mhl = np.float32(0)
    for l in range(1, top + 1):
        if S[l] > 0:
            d = np.float32(D[l]) if denominators is None else denominators[l]
            t = np.float32(np.float32(np.float32(l) * np.float32(S[l])) / d)
            mhl = np.float32(mhl + t)
    return np.float32(mhl / l_sum), n_reads, maxn


def read_order_denominators(n_list, top):
    """mhl.rs:53-58: per l, (num_cpg - l + 1) as f32 added read by read, in record order"""
    out = [np.float32(0)] * (top + 2)
    n = np.asarray(n_list, np.int64)
    for l in range(1, top + 1):
        v = (n[n >= l] - l + 1).astype(np.float32)
        out[l] = np.add.accumulate(v, dtype=np.float32)[-1] if len(v) else np.float32(0)
    return out


def restate(calls, iv, min_depth=10, min_cpgs=4, min_qual=10):
    """-> (mhl f32[n], n_reads int64[n], max_cpgs int64[n]) of the intervals [(tid, start, end, name)]"""
    out = [finalise(*histograms(calls, t, b, e, min_cpgs, min_qual)[:2], min_depth=min_depth) for t, b, e, _ in iv]
    return (np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.int64))


@functools.lru_cache(maxsize=None)
def default_expected():
    return restate(default_calls(), intervals(), **DEFAULT_KW)


def oracle_route(rec, t, b, e, min_depth=10, min_cpgs=4, min_qual=10):
    """the same value through the oracle's pinned primitives alone: Reads.decode with the interval's positions as the -c set
    (filter_isin), stretch_info(i) and the calls per read, then compute_mhl's arithmetic with its read-order f32 denominator"""
    hi = min(e, dict(enumerate(l for _, l in rec.refs))[t] + 4096)
    reads = pyoracle.Reads.decode(rec, cpg_set=[(t, p) for p in range(b, hi)])
    s = reads.soa()
    n = np.diff(s["cpg_off"].astype(np.int64))
    who = np.nonzero((s["mapq"] >= min_qual) & (n >= max(min_cpgs, 1)))[0]
    n_list = n[who]
    if len(who) < max(min_depth, 1):
        return np.float32(np.nan), len(who), int(n_list.max()) if len(who) else 0
    maxn = int(n_list.max())
    S = np.zeros(maxn + 2, np.int64)
    for i in who:
        si = reads.stretch_info(int(i), cap=int(n[i]) + 1)
        S[1:1 + len(si)] += si
    den = read_order_denominators(n_list, maxn)
    l_sum = np.float32(0)
    for l in range(1, maxn + 1):
        l_sum = np.float32(l_sum + np.float32(l))
    mhl = np.float32(0)
    for l in range(1, maxn + 1):
        if S[l] > 0:
            mhl = np.float32(mhl + np.float32(np.float32(np.float32(l) * np.float32(np.int32(S[l]))) / den[l]))
    return np.float32(mhl / l_sum), len(who), maxn


def boundary_calls():
    """a read of the sorted part of ivA with at least 5 calls: (its first call, a middle call, its last call)"""
    c = default_calls()
    idx = c.by_tid[0]
    rd = c.read[idx]
    n = np.bincount(rd)
    for r in np.nonzero(n >= 5)[0]:
        p = c.pos[idx[rd == r]]
        if 30_000 < p[0] < 31_000:
            return int(p[0]), int(p[len(p) // 2]), int(p[-1])
    raise AssertionError("no such read")


def hub_intervals(k=6):
    """intervals around three neighbouring called positions at most 50 bp apart, in the evenly covered part of ivA: every read that
    holds all three contributes with -p 3, and such a read starts before any read that holds only the later ones"""
    c = default_calls()
    p = np.unique(c.pos[c.by_tid[0]])
    p = p[(p >= 40_000) & (p < 60_000)]
    at = np.nonzero(p[2:] - p[:-2] <= 50)[0]
    pick = at[np.linspace(0, len(at) - 1, k).astype(int)]
    return [(0, int(p[i]), int(p[i + 2]) + 1, "hub_%d" % n) for n, i in enumerate(pick)]


@functools.lru_cache(maxsize=None)
def intervals():
    """-> [(tid, start, end, name or None)]"""
    iv = []
    iv += [(0, b, b + 1000, "tile_a_%d" % (b // 1000)) for b in range(0, REFS[0][1], 1000)]            # 1 kbp tiling on both contigs
    iv += [(1, b, b + 1000, None) for b in range(0, REFS[1][1], 1000)]
    iv += [(0, b, b + 2000, "slide_%d" % b) for b in range(62_000, 70_001, 500)]                        # 2 kbp windows, 500 bp step, over the island
    iv += [(0, 66_000, 68_000, "nest_outer"), (0, 66_500, 67_500, "nest_mid"), (0, 66_900, 67_000, "nest_inner")]
    iv += [(0, 150_000, 152_000, "twin"), (0, 150_000, 152_000, "twin")]                                # two identical lines
    iv += [(0, 0, REFS[0][1], "whole_a"), (1, 0, INT32_MAX, "whole_b_open_end")]
    iv += [(2, 0, REFS[2][1], "no_reads"), (2, 100, 200, None)]
    iv += [(0, 0, 1, "first_base"), (0, 500, 500, "empty"), (0, 0, 9, "after_minus_one")]               # beside the calls at -1, 3, 8
    first, mid, last = boundary_calls()
    iv += [(0, first, last + 1, "read_exact"),                 # exactly a read's first and last call
           (0, first + 1, last + 1, "cut_after_first"), (0, first, last, "cut_before_last"),
           (0, first - 700, mid, "end_on_a_call"), (0, first - 700, mid + 1, "end_past_a_call"),
           (0, mid, last + 700, "start_on_a_call"), (0, mid + 1, last + 700, "start_past_a_call")]
    iv += [(1, LONG_AT - 1000, LONG_AT + LONG_LEN + 1000, "long_reads"),                                # 100 kept calls of each long read
           (1, LONG_AT, LONG_AT + 70 * LONG_STEP, "long_run_70"), (1, LONG_AT + 600, LONG_AT + 2000, "long_tail_70_calls")]
    iv += [(0, L.INDEL_AT, L.INDEL_AT + 100, "deletion"), (0, L.INS_AT, L.INS_AT + 100, "insertion")]
    iv += hub_intervals()
    return iv


def bed_text(iv=None):
    return L.bed_text(iv if iv is not None else intervals())


def table_text(iv, mhl, n_reads, max_cpgs, names=NAMES):
    return HEADER + "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (names[t], b, e, "." if name is None else name, pyoracle.format_f32(v), n, mx)
                            for (t, b, e, name), v, n, mx in zip(iv, mhl.tolist(), n_reads.tolist(), max_cpgs.tolist()))


def sam_text(rec):
    """the records as SAM text (SEQ all N: the XM route never looks at it)"""
    ops = "MIDNSHP=X"
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + ["@SQ\tSN:%s\tLN:%d" % r for r in rec.refs]
    for i in range(len(rec)):
        cig = "".join("%d%s" % (c >> 4, ops[c & 15]) for c in rec.cigars[i])
        lines.append("r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\tXM:Z:%s" % (i, rec.flag[i], rec.refs[rec.tid[i]][0], rec.pos[i] + 1, rec.mapq[i], cig,
                                                                           "N" * len(rec.xms[i]), rec.xms[i].decode()))
    return "\n".join(lines) + "\n"


def same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())
