"""Inputs and expectations shared by the per-interval LPMD tests (`lpmd --intervals`, mth_lpmd_intervals_fetch): the synthetic
records, the interval set, the oracle's pairs table summed under the invariant (same contig, start <= cpg1, cpg2 < end), and the
file the command line writes for it.  Nothing here touches a device."""
import functools

import numpy as np

from oracle import bamio, pyoracle
from tests import util

REFS = [("ivA", 200_000), ("ivB", 60_000), ("ivEmpty", 30_000)]
NAMES = [n for n, _ in REFS]
INT32_MAX = 2 ** 31 - 1
HEADER = "chrom\tstart\tend\tname\tlpmd\tn_concordant\tn_discordant\n"
DEFAULT_KW = dict(min_distance=2, max_distance=16, min_qual=10)
# a CpG island under ~180x: more than 2048 distinct pairs start in the 8192-bp tile that holds it, so the pairs pass leaves that tile
# (and, at wider tiles, the one around it) to its global path and the rows come unsorted behind the contig's sorted ones
ISLAND = (66_000, 68_000)
HOT_TILE = (65_536, 73_728)
INDEL_AT, INS_AT = 120_000, 130_000


def lpmd_f32(c, d):
    """lpmd.rs:51-55 on i32 counters: n_discordant as f32 / (n_concordant + n_discordant) as f32"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.int32(d)) / np.float32(np.int32(c + d))


@functools.lru_cache(maxsize=None)
def records():
    """-> Records, coordinate-sorted: two synthetic contigs (200 kbp with ~40 k reads and the island, 60 kbp), a third without reads,
    reverse-strand reads at position 0 that call at -1, reads with a deletion and with an insertion"""
    from metheor_amd import synth
    rng = np.random.default_rng(905)
    s0 = np.unique(np.r_[synth.make_sites(REFS[0][1], 0.03, rng), ISLAND[0] + synth.make_sites(ISLAND[1] - ISLAND[0], 0.45, rng)])
    s0 = s0[np.r_[True, np.diff(s0) >= 2]].astype(np.int32)          # a CpG is two bases
    st0 = np.sort(np.r_[rng.integers(0, REFS[0][1] - 150, 38_000), rng.integers(ISLAND[0] - 100, ISLAND[1] - 50, 2_500)]).astype(np.int32)
    c0 = synth.make_contig(0, REFS[0][1], None, None, rng, sites=s0, starts=st0)
    c1 = synth.make_contig(1, REFS[1][1], 12_000, 0.03, rng)
    tid, pos, flag, mapq, cig, xms = [], [], [], [], [], []
    for t, c in ((0, c0), (1, c1)):
        r = util.contig_to_records(c, NAMES[t])
        tid += [t] * len(r); pos += r.pos.tolist(); flag += r.flag.tolist(); mapq += r.mapq.tolist(); cig += r.cigars; xms += r.xms

    def xm(n, calls):
        b = bytearray(b"." * n)
        for q, ch in calls:
            b[q] = ord(ch)
        return bytes(b)

    M, I, D = 0, 1, 2
    extra = []
    # flag 16 at position 0, calls on query bases 0, 4, 9: abspos - 1 = -1, 3, 8 (readutil.rs:338)
    for k in range(12):
        extra.append((0, 0, 16, 42, [(150 << 4) | M], xm(150, [(0, "Z"), (4, "z" if k % 3 else "Z"), (9, "Z")])))
    # 40M5D110M: query 30 -> +30, query 45 -> +50, query 52 -> +57: relpos distances 15 / 7 / 22, abspos distances 20 / 7 / 27
    for k in range(10):
        extra.append((0, INDEL_AT, 0, 42, [(40 << 4) | M, (5 << 4) | D, (110 << 4) | M], xm(150, [(30, "Z"), (45, "z" if k % 2 else "Z"), (52, "Z")])))
    # 50M3I97M: query 48 -> +48, query 60 -> +57: relpos distance 12, abspos distance 9
    for k in range(10):
        extra.append((0, INS_AT, 0, 42, [(50 << 4) | M, (3 << 4) | I, (97 << 4) | M], xm(150, [(48, "z"), (60, "Z" if k % 2 else "z")])))
    for e in extra:
        tid.append(e[0]); pos.append(e[1]); flag.append(e[2]); mapq.append(e[3]); cig.append(e[4]); xms.append(e[5])
    # coordinate order, the extra records first among equal positions: the reads at 0 open the file
    order = sorted(range(len(tid)), key=lambda i: (tid[i], pos[i], 0 if i >= len(tid) - len(extra) else 1))
    return bamio.Records(REFS, [tid[i] for i in order], [pos[i] for i in order], [flag[i] for i in order], [mapq[i] for i in order],
                         [cig[i] for i in order], [xms[i] for i in order])


def pairs_table(rec, cpg_set=None, **kw):
    """the oracle's pairs table of the records: (tid, cpg1, cpg2, n_concordant, n_discordant) as int64 arrays"""
    t = pyoracle.Reads.decode(rec, cpg_set=cpg_set).lpmd(pairs=True, **kw)["pairs"]
    return (t.tid.astype(np.int64), t.pos[:, 0].astype(np.int64), t.pos[:, 1].astype(np.int64), t.cnt[:, 0].astype(np.int64), t.cnt[:, 1].astype(np.int64))


@functools.lru_cache(maxsize=None)
def default_table():
    return pairs_table(records(), **DEFAULT_KW)


def boundary_rows():
    """two rows of the default table the boundary intervals are cut at: one of the sorted part, one of the island"""
    tid, p1, p2, c, d = default_table()
    a = np.nonzero((tid == 0) & (p1 > 30_000) & (p1 < 31_000))[0][0]
    b = np.nonzero((tid == 0) & (p1 > ISLAND[0] + 900))[0][0]
    return (int(p1[a]), int(p2[a])), (int(p1[b]), int(p2[b]))


@functools.lru_cache(maxsize=None)
def intervals():
    """-> [(tid, start, end, name or None)], ~300 of them"""
    iv = []
    iv += [(0, b, b + 1000, "tile_a_%d" % (b // 1000)) for b in range(0, 130_000, 1000)]            # 1 kbp tiling windows
    iv += [(1, b, b + 1000, None) for b in range(0, 60_000, 1000)]
    iv += [(0, b, b + 2000, "slide_%d" % b) for b in range(60_000, 98_001, 500)]                     # 2 kbp windows, 500 bp step
    iv += [(0, 66_000, 68_000, "nest_outer"), (0, 66_500, 67_500, "nest_mid"), (0, 66_900, 67_000, "nest_inner")]
    iv += [(0, 150_000, 152_000, "twin"), (0, 150_000, 152_000, "twin")]                             # two identical lines
    iv += [(0, 0, 1, "first_base"), (0, 500, 500, "empty"), (1, 59_999, 59_999, None)]
    iv += [(0, 0, REFS[0][1], "whole_a"), (1, 0, INT32_MAX, "whole_b_open_end")]
    iv += [(2, 0, REFS[2][1], "no_reads"), (2, 100, 200, None)]
    iv += [(0, HOT_TILE[0], HOT_TILE[1], "pairs_tile"), (0, 8_192, 16_384, "pairs_tile_2"), (0, 32_768, 65_536, "pairs_tile_wide")]
    (a1, a2), (b1, b2) = boundary_rows()
    for tag, q1, q2 in (("s", a1, a2), ("h", b1, b2)):
        iv += [(0, q1, q2 + 1, tag + "_exact"),               # start == cpg1, end - 1 == cpg2
               (0, q1 - 1500, q2, tag + "_end_on_cpg2"),       # end == cpg2: that pair is out, cpg1 inside and cpg2 outside
               (0, q1 + 1, q2 + 1500, tag + "_start_past_cpg1")]
    iv += [(0, 0, 9, "after_minus_one"), (0, 0, 4, None)]                                            # (3, 8) is inside; (-1, 3) and (-1, 8) are not
    iv += [(0, INDEL_AT, INDEL_AT + 100, "deletion"), (0, INDEL_AT + 30, INDEL_AT + 51, "deletion_pair"), (0, INS_AT, INS_AT + 100, "insertion")]
    return iv


def bed_text(iv=None):
    """the BED of the intervals: names where given, comment / track / empty lines and extra columns in between"""
    out = ["# per-interval LPMD test set\n", "track name=intervals\n", "\n"]
    for k, (t, b, e, name) in enumerate(iv if iv is not None else intervals()):
        out.append("%s\t%d\t%d%s\n" % (NAMES[t], b, e, "" if name is None else "\t" + name + ("\t0\t+" if k % 7 == 0 else "")))
        if k == 5:
            out.append("browser position ivA:1-100\n")
    return "".join(out)


def reduce_table(table, iv):
    """the invariant: rows of the same contig with start <= cpg1 and cpg2 < end, summed -> (n_concordant[n], n_discordant[n])"""
    tid, p1, p2, c, d = table
    nc, nd = np.zeros(len(iv), np.int64), np.zeros(len(iv), np.int64)
    per = {t: np.nonzero(tid == t)[0] for t in set(x[0] for x in iv)}
    for k, (t, b, e, _) in enumerate(iv):
        s = per[t]
        m = s[(p1[s] >= b) & (p2[s] < e)]
        nc[k], nd[k] = c[m].sum(), d[m].sum()
    return nc, nd


def table_text(iv, nc, nd, names=NAMES):
    return HEADER + "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (names[t], b, e, "." if name is None else name,
                                                           pyoracle.format_f32(lpmd_f32(c, d)), c, d)
                            for (t, b, e, name), c, d in zip(iv, nc.tolist(), nd.tolist()))


def parse_pairs_file(text, names):
    """a --pairs file -> table as pairs_table gives it"""
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    col = lambda k: np.array([int(r[k]) for r in rows], np.int64)
    return (np.array([names.index(r[0]) for r in rows], np.int64), col(1), col(2), col(4), col(5))


def record_stream(path):
    """BGZF-inflate a BAM, skip the header -> (record bytes as uint8, uint64 offsets of the records (n + 1))"""
    import gzip
    import struct
    raw = gzip.decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, o)
        o += 8 + l_name
    body = np.frombuffer(raw, np.uint8)[o:]
    offs = [0]
    while offs[-1] < len(body):
        bs, = struct.unpack_from("<i", raw, o + offs[-1])
        offs.append(offs[-1] + 4 + bs)
    return np.ascontiguousarray(body), np.array(offs, np.uint64)
