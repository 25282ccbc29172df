"""Inputs and expectations shared by the per-interval PDR tests (`metheor pdr-regions`, `all --pdr-intervals`, mth_pdr_regions_*): the
CPU restatement of the definition in numpy on the oracle's decoded reads; the same counts by the route through
the oracle's pinned primitives; the file the command line writes.  The records and the 307 intervals are those of the per-interval MHL
tests (tests/mhl_regions_util.py).  Nothing here touches a device.

Definition.  For an interval [start, end) on contig c take each record once: keep the calls with start <= abspos < end on c
(filter_isin, readutil.rs:87-94, with the set "every position of the interval"); with n calls kept the read contributes if
mapq >= min_qual and n >= max(min_cpgs, 1) (pdr.rs:147-157); a contributing read is methylated (every kept call is Z), unmethylated
(none is) or discordant (get_concordance_state(), readutil.rs:134-145); n_concordant = methylated + unmethylated and the value is
n_discordant as f32 / (n_concordant as f32 + n_discordant as f32) (pdr.rs:47-49), NaN below max(min_depth, 1) contributing reads."""
import functools

import numpy as np

from oracle import pyoracle
from tests import mhl_regions_util as M

REFS, NAMES, INT32_MAX = M.REFS, M.NAMES, M.INT32_MAX
HEADER = "chrom\tstart\tend\tname\tpdr\tn_concordant\tn_discordant\tn_methylated\n"
DEFAULT_KW = dict(min_depth=10, min_cpgs=4, min_qual=10)
records, intervals, default_calls, Calls, bed_text, sam_text, same_bits = (M.records, M.intervals, M.default_calls, M.Calls, M.bed_text,
                                                                            M.sam_text, M.same_bits)


def counts_of(calls, t, b, e, min_cpgs=4, min_qual=10):
    """-> (methylated, unmethylated, discordant): the contributing reads of the interval by class"""
    idx = calls.by_tid.get(t, np.zeros(0, np.int64))
    idx = idx[(calls.pos[idx] >= b) & (calls.pos[idx] < e)]
    rd = calls.read[idx]
    n = np.bincount(rd, minlength=calls.n_reads)
    m = np.bincount(rd[calls.meth[idx]], minlength=calls.n_reads)
    contrib = (calls.mapq >= min_qual) & (n >= max(min_cpgs, 1))
    meth, unmeth = contrib & (m == n), contrib & (m == 0)
    return int(meth.sum()), int(unmeth.sum()), int((contrib & ~meth & ~unmeth).sum())


def finalise(n_concordant, n_discordant, min_depth=10):
    """pdr.rs:47-49 in float32, each counter converted once; NaN below max(min_depth, 1) contributing reads"""
    if n_concordant + n_discordant < max(min_depth, 1):
        return np.float32(np.nan)
    c, d = np.float32(n_concordant), np.float32(n_discordant)
    return np.float32(d / np.float32(c + d))


def restate(calls, iv, min_depth=10, min_cpgs=4, min_qual=10):
    """-> (pdr f32[n], methylated, unmethylated, discordant int64[n]) of the intervals [(tid, start, end, name)]"""
    k = np.array([counts_of(calls, t, b, e, min_cpgs, min_qual) for t, b, e, _ in iv], np.int64).reshape(len(iv), 3)
    pdr = np.array([finalise(int(m + u), int(d), min_depth) for m, u, d in k], np.float32)
    return pdr, k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()


@functools.lru_cache(maxsize=None)
def default_expected():
    return restate(default_calls(), intervals(), **DEFAULT_KW)


def oracle_route(rec, t, b, e, min_cpgs=4, min_qual=10):
    """the same three counts through the oracle's pinned primitives alone: Reads.decode with the interval's positions as the -c set
    (filter_isin), then per read the call count, the mapq test and is_discordant(i); a concordant read is methylated when its first
    kept call is"""
    hi = min(e, dict(enumerate(l for _, l in rec.refs))[t] + 4096)
    reads = pyoracle.Reads.decode(rec, cpg_set=[(t, p) for p in range(b, hi)])
    s = reads.soa()
    off = s["cpg_off"].astype(np.int64)
    n = np.diff(off)
    out = [0, 0, 0]
    for i in np.nonzero((s["mapq"] >= min_qual) & (n >= max(min_cpgs, 1)))[0]:
        if reads.is_discordant(int(i)):
            out[2] += 1
        else:
            out[0 if s["cpg_pos"][off[i]] >> 31 else 1] += 1
    return tuple(out)


def table_text(iv, pdr, methylated, unmethylated, discordant, names=NAMES):
    return HEADER + "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\n" % (names[t], b, e, "." if name is None else name, pyoracle.format_f32(v), m + u, d, m)
                            for (t, b, e, name), v, m, u, d in zip(iv, pdr.tolist(), methylated.tolist(), unmethylated.tolist(), discordant.tolist()))


def deep_nesting(cap):
    """windows of 3 kbp at a 2-bp step over the island of contig ivA, 1.45 x `cap` of them (1484 for a cap of 1024): all of them hold
    the 30 bases before 66,000, so a workgroup whose reads lie there has that many candidates of one length class -- more than `cap`
    -- and its reads overlap most of them in part"""
    depth = cap * 29 // 20
    assert depth > cap and 2 * depth < 3000
    return [(0, 63_000 + 2 * k, 66_000 + 2 * k, None) for k in range(depth)]
