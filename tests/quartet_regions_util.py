"""Inputs and expectations shared by the per-interval ME / PM tests (`metheor me-regions`, `pm-regions`, `all --me-intervals /
--pm-intervals`, mth_quartet_regions_*): the CPU restatement of the definition in numpy on the oracle's decoded
reads, float32 step by step; the same counts by the route through the oracle's pinned primitives; the file the command line writes.
The records and the 307 intervals are those of the per-interval MHL tests (tests/mhl_regions_util.py).  Nothing here touches a device.

Definition.  For an interval [start, end) on contig c take each record once: keep the calls with start <= abspos < end on c, in the
read's call order (filter_isin, readutil.rs:87-94, with the set "every position of the interval"); the read contributes if
mapq >= min_qual (me.rs:115) and at least 4 calls are kept (readutil.rs:101); a contributing read adds one pattern
8*m1 + 4*m2 + 2*m3 + m4 per window of four consecutive kept calls (readutil.rs:97-132) to the interval's ONE 16-bin histogram
(me.rs:121-125 with every quartet mapped to the same stat).  n_patterns = the sum of the bins, n_reads = the contributing reads; ME =
compute_me (me.rs:42-55) and PM = compute_pm (pm.rs:42-51) of the histogram, NaN below max(min_depth, 1) patterns."""
import functools

import numpy as np

from oracle import pyoracle
from tests import mhl_regions_util as M
from tests import util

REFS, NAMES, INT32_MAX = M.REFS, M.NAMES, M.INT32_MAX
HEADER_ME = "chrom\tstart\tend\tname\tme\tn_patterns\tn_reads\n"
HEADER_PM = "chrom\tstart\tend\tname\tpm\tn_patterns\tn_reads\n"
DEFAULT_KW = dict(min_depth=10, min_qual=10)
records, intervals, default_calls, Calls, bed_text, sam_text, same_bits = (M.records, M.intervals, M.default_calls, M.Calls, M.bed_text,
                                                                            M.sam_text, M.same_bits)


def counts_of(calls, t, b, e, min_qual=10):
    """-> (bins int64[16], n_reads): the pooled pattern histogram of the interval and its contributing reads"""
    idx = calls.by_tid.get(t, np.zeros(0, np.int64))
    idx = idx[(calls.pos[idx] >= b) & (calls.pos[idx] < e)]              # original order: the calls of a read stay together, in call order
    rd, m = calls.read[idx], calls.meth[idx].astype(np.int64)
    n = np.bincount(rd, minlength=calls.n_reads)
    contrib = (calls.mapq >= min_qual) & (n >= 4)
    bins = np.zeros(16, np.int64)
    if len(rd) >= 4:
        win = (rd[:-3] == rd[3:]) & contrib[rd[:-3]]                     # a window: four consecutive kept calls of one contributing read
        pat = 8 * m[:-3] + 4 * m[1:-2] + 2 * m[2:-1] + m[3:]
        bins = np.bincount(pat[win], minlength=16).astype(np.int64)
    return bins, int(contrib.sum())


def finalise(bins, min_depth=10):
    """me.rs:42-55 and pm.rs:42-51 in float32 step by step, every counter and the total converted once -> (me, pm, n_patterns);
    NaN below max(min_depth, 1) patterns"""
    total = int(np.sum(bins))
    if total < max(min_depth, 1):
        return np.float32(np.nan), np.float32(np.nan), total
    tf = np.float32(total)
    me, pm = np.float32(0), np.float32(1)
    for c in bins:
        p = np.float32(np.float32(int(c)) / tf)
        if c > 0:
            me = np.float32(me + np.float32(p * np.log2(p, dtype=np.float32)))
        pm = np.float32(pm - np.float32(p * p))
    return np.float32(me * np.float32(-0.25)), pm, total


def restate(calls, iv, min_depth=10, min_qual=10):
    """-> (me f32[n], pm f32[n], n_patterns int64[n], n_reads int64[n], bins int64[n, 16]) of the intervals [(tid, start, end, name)]"""
    k = [counts_of(calls, t, b, e, min_qual) for t, b, e, _ in iv]
    bins = np.array([x[0] for x in k], np.int64).reshape(len(iv), 16)
    f = [finalise(b, min_depth) for b in bins]
    return (np.array([x[0] for x in f], np.float32), np.array([x[1] for x in f], np.float32), np.array([x[2] for x in f], np.int64),
            np.array([x[1] for x in k], np.int64), bins)


@functools.lru_cache(maxsize=None)
def default_expected():
    return restate(default_calls(), intervals(), **DEFAULT_KW)


def oracle_route(rec, t, b, e, min_qual=10):
    """the same counts through the oracle's pinned primitives alone: Reads.decode with the interval's positions as the -c set
    (filter_isin), then the 16-bin histograms of Reads.me at depth 0 summed over its rows; the contributing reads from the decoded
    reads themselves (mapq and at least 4 calls left)"""
    hi = min(e, dict(enumerate(l for _, l in rec.refs))[t] + 4096)
    reads = pyoracle.Reads.decode(rec, cpg_set=[(t, p) for p in range(b, hi)])
    cnt = reads.me(min_depth=0, min_qual=min_qual).cnt
    bins = cnt.astype(np.int64).sum(axis=0) if len(cnt) else np.zeros(16, np.int64)
    s = reads.soa()
    n = np.diff(s["cpg_off"].astype(np.int64))
    return bins, int(((s["mapq"] >= min_qual) & (n >= 4)).sum())


def table_text(iv, values, n_patterns, n_reads, which="me", names=NAMES):
    """the file `me-regions` (which="me") or `pm-regions` ("pm") writes"""
    return (HEADER_ME if which == "me" else HEADER_PM) + "".join(
        "%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (names[t], b, e, "." if name is None else name, pyoracle.format_f32(v), p, r)
        for (t, b, e, name), v, p, r in zip(iv, values.tolist(), n_patterns.tolist(), n_reads.tolist()))


def expected_texts(iv, want, names=NAMES):
    me, pm, n_patterns, n_reads = want[:4]
    return table_text(iv, me, n_patterns, n_reads, "me", names), table_text(iv, pm, n_patterns, n_reads, "pm", names)


def assert_me_text(got, want):
    """an ME table against the restatement's by tests/util.py's ME rule: every other column equal, the value within 1e-6 (log2f of two
    C libraries may differ in the last ulp); the header and the NaN rows byte for byte"""
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w) and g[0] == w[0], (len(g), len(w), g[:1])
    def split(lines):
        nan = [l for l in lines if l.split("\t")[4] == "NaN"]
        rest = ["\t".join((f[0], f[1], f[2], f[3], f[5] + "/" + f[6], f[4])) for f in (l.split("\t") for l in lines) if f[4] != "NaN"]
        return nan, rest
    gn, gr = split(g[1:])
    wn, wr = split(w[1:])
    assert gn == wn
    # (the rule sorts its lines; both sides are keyed by the same leading columns, duplicates included)
    util.assert_tsv_equals_oracle("me", "\n".join(gr), "\n".join(wr))
    for a, b in zip(g[1:], w[1:]):
        assert a.split("\t")[:4] == b.split("\t")[:4]                     # ... and the rows are in BED order
