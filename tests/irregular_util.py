"""Seeded Bismark-like input that breaks what metheor_amd.synth.make_contig never does: CIGARs with clips, indels, skips, =/X
and hard clips; the paired, duplicate and secondary flags whose calls the reference shifts by -1 (readutil.rs:332-340), which
puts CpG sites one position apart; CG-repeat islands (a site every 2 bp) in a sparse background; calls dropped over runs of
sites; read lengths mixed within a contig, query lengths above 255 on short spans; low mapq and piles.

The output is coordinate-sorted oracle.bamio.Records, so the same input goes to the oracle (pyoracle.Reads.decode), to device
batches (contigs()) and, written with bamio.write_bam, to the CLI.  Every knob can be switched off."""
import numpy as np

from oracle import bamio, pyoracle

UNSHIFTED = (0, 99, 147)                      # readutil.rs:332: every other flag reports abspos - 1
FLAGS_PLAIN = (0, 16, 99, 147, 83, 163)
FLAGS_SHIFTED_FWD = (65, 97, 1024 | 99, 256)  # forward-strand reads whose call of the C is reported one position left
KNOBS = ("clips", "indels", "skips", "eqx", "hard", "shifted", "islands", "drops", "mixed_len", "long_query", "low_mapq", "piles")


def _sites(length, rng, density, islands):
    """sorted C positions of the CpGs (gaps >= 2): a sparse background, plus CG repeats (every 2 bp) when `islands`"""
    gaps = rng.geometric(density, size=int(length * density * 1.2) + 16) + 1
    s = np.cumsum(gaps) + 2
    s = s[s < length - 300]
    isl = []
    if islands:
        for _ in range(max(1, length // 4000)):
            a = int(rng.integers(300, max(301, length - 600)))
            n = int(rng.integers(30, 120))
            isl.append((a, a + 2 * n))
            s = s[(s < a - 2) | (s >= a + 2 * n + 2)]
            s = np.concatenate([s, a + 2 * np.arange(n)])
    return np.unique(s), isl


def _cigar(rng, span, k):
    """a CIGAR with `span` reference bases (M / = / X / D / N), shape drawn from the knobs"""
    shapes = ["M"]
    if k["clips"]:
        shapes += ["S", "S"]
    if k["indels"]:
        shapes += ["I", "D", "ID"]
    if k["skips"]:
        shapes += ["N"]
    if k["eqx"]:
        shapes += ["EQX"]
    if k["long_query"]:
        shapes += ["LQ"]
    sh = shapes[int(rng.integers(0, len(shapes)))]
    ops = []
    if sh == "M":
        ops = [("M", span)]
    elif sh == "S":
        ops = [("S", int(rng.integers(1, 40))), ("M", span)] + ([("S", int(rng.integers(1, 20)))] if rng.random() < 0.5 else [])
    elif sh in ("I", "D", "ID", "N"):
        gap = {"I": 0, "D": int(rng.integers(1, 121)), "ID": int(rng.integers(1, 20)), "N": int(rng.integers(20, 160))}[sh]
        m = max(span - gap, 12)
        a = int(rng.integers(5, m - 5))
        mid = {"I": [("I", int(rng.integers(1, 31)))], "D": [("D", gap)], "ID": [("I", int(rng.integers(1, 31))), ("D", gap)], "N": [("N", gap)]}[sh]
        ops = [("M", a)] + mid + [("M", m - a)]
    elif sh == "EQX":
        a = int(rng.integers(3, span - 3))
        ops = [("=", a), ("X", 1), ("M", span - a - 1)]
    elif sh == "LQ":                          # query > 255 bases on <= 150 reference bases: 16-bit relative positions
        sp = min(span, int(rng.integers(60, 151)))
        lead = int(rng.integers(100, 200))
        ops = [("S", lead), ("M", sp // 2), ("I", int(rng.integers(1, 31))), ("M", sp - sp // 2)]
        ops.append(("S", max(1, 256 - lead - sp) + int(rng.integers(0, 30))))
    if k["hard"] and rng.random() < 0.15:
        ops = [("H", int(rng.integers(1, 10)))] + ops + ([("H", 3)] if rng.random() < 0.5 else [])
    return ops


def positions(pos, ops):
    """readutil.rs:24-33 / rust-htslib reference_positions_full: one entry per query base, None on I and S"""
    out, g = [], pos
    for op, n in ops:
        if op in "M=X":
            out.extend(range(g, g + n)); g += n
        elif op in "IS":
            out.extend([None] * n)
        elif op in "DN":
            g += n
    return out


def xm_for(pos, flag, ops, site_set, level, rng, drop=None):
    """Bismark's XM: a forward-strand read calls the C of a CpG (its position), a reverse-strand one the G (position + 1) --
    whatever the flag; the reference then shifts the reported site by -1 unless the flag is 0, 99 or 147"""
    rev = bool(flag & 16)
    out = []
    calls = []
    for q, ap in enumerate(positions(pos, ops)):
        if ap is None:
            out.append("Z" if rng.random() < 0.1 else ".")        # calls on inserted / clipped bases are ignored (readutil.rs:331)
            continue
        c = ap - 1 if rev else ap
        if c in site_set:
            out.append("Z" if rng.random() < level(c) else "z")
            calls.append(q)
        else:
            out.append("x" if rng.random() < 0.03 else ".")
    if drop is not None and len(calls) > 3:                        # a run of sites left uncalled (XM '.')
        i = int(rng.integers(1, len(calls) - 1))
        j = min(len(calls) - 1, i + drop)
        for q in calls[i:j]:
            out[q] = "."
    return "".join(out)


def make_records(seed, n_contigs=1, length=12_000, n_reads=1_500, density=0.02, unaligned=False, **knobs):
    """-> (Records coordinate-sorted, contig names).  knobs: any of KNOBS set False switches that input class off.  unaligned:
    per contig, also a few records without an aligned base (all-S CIGAR, calls on clipped bases only) and a few without a call
    (off by default: the draws of every existing seed stay as they were)."""
    k = {n: bool(knobs.get(n, True)) for n in KNOBS}
    unknown = set(knobs) - set(KNOBS)
    assert not unknown, unknown
    rng = np.random.default_rng(seed)
    refs, rows = [], []
    for tid in range(n_contigs):
        name = "chrI%d" % tid
        refs.append((name, length))
        sites, isl = _sites(length, rng, density, k["islands"])
        site_set = set(int(x) for x in sites)
        lv = {int(s): (0.85 if rng.random() < 0.6 else 0.15) for s in sites}
        level = lambda c: lv.get(c, 0.5)
        starts = rng.integers(50, length - 400, size=n_reads)
        if k["islands"]:                                        # a share of the reads over the islands
            for i in range(n_reads // 3):
                a, b = isl[int(rng.integers(0, len(isl)))]
                starts[i] = int(rng.integers(max(50, a - 120), b))
        if k["piles"]:
            spots = rng.integers(50, length - 400, size=4)
            m = n_reads // 10
            starts[-m:] = spots[rng.integers(0, len(spots), size=m)]
        for s in starts:
            span = int(rng.choice([36, 60, 100, 120, 149, 150, 151, 180, 200, 201, 240])) if k["mixed_len"] else 150
            ops = _cigar(rng, span, k)
            flags = FLAGS_PLAIN + (FLAGS_SHIFTED_FWD * 2 if k["shifted"] else ())
            fl = int(rng.choice(flags))
            mq = int(rng.integers(0, 10)) if (k["low_mapq"] and rng.random() < 0.12) else 42
            drop = int(rng.integers(4, 60)) if (k["drops"] and rng.random() < 0.3) else None
            xm = xm_for(int(s), fl, ops, site_set, level, rng, drop)
            rows.append((tid, int(s), fl, mq, ops, xm))
        if unaligned:
            for s in rng.integers(50, length - 400, size=6):
                q = int(rng.integers(20, 160))
                rows.append((tid, int(s), int(rng.choice(FLAGS_PLAIN)), 42, [("S", q)], "".join(rng.choice(list("Zz.."), size=q))))
            for s in rng.integers(50, length - 400, size=6):
                rows.append((tid, int(s), int(rng.choice(FLAGS_PLAIN)), 42, [("M", 100)], "." * 100))
    rows.sort(key=lambda r: (r[0], r[1]))                       # stable: ties keep their drawing order
    rec = records_from_rows(refs, rows)
    return rec, [n for n, _ in refs]


def records_from_rows(refs, rows):
    """rows: (tid, pos, flag, mapq, [(op, n)], xm str) -> bamio.Records"""
    cig = [[(n << 4) | bamio.CIGAR_OPS.index(op) for op, n in r[4]] for r in rows]
    return bamio.Records(refs, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], cig,
                         [r[5].encode() for r in rows], names=["q%d" % i for i in range(len(rows))])


def ops_of(rec, i):
    return [(bamio.CIGAR_OPS[c & 15], c >> 4) for c in rec.cigars[i]]


def fdrp_safe(rec, max_span=None):
    """the records without the shifted-arm reads that span >= 202 bp, where the reference indexes its window at -1 and panics
    (fdrp.rs:69-71; tests/test_oracle_panics.py); with max_span, also without every read spanning more (k_fdrp_wtile takes
    batches of spans <= 200 only)"""
    soa = pyoracle.Reads.decode(rec).soa()
    span = soa["end"].astype(np.int64) - soa["start"].astype(np.int64) + 1
    shifted = ~np.isin(rec.flag, UNSHIFTED)
    keep = ~(shifted & (span >= 202))
    if max_span is not None:
        keep &= span <= max_span
    out = rec.subset(np.nonzero(keep)[0])
    rd = pyoracle.Reads.decode(out)
    rd.fdrp(min_depth=0, max_depth=64, min_overlap=0, min_qual=0)      # raises pyoracle.ReferencePanic if one is left
    return out


def contigs(rec, rel16=False):
    """Records -> (oracle Reads, [contig dict per tid]) -- the device batches' input (tests/util.contig_from_oracle_soa)"""
    from tests import util
    reads = pyoracle.Reads.decode(rec)
    soa = reads.soa()
    cs = [util.contig_from_oracle_soa(soa, tid, ln) for tid, (_, ln) in enumerate(rec.refs)]
    if rel16:
        for c in cs:
            c["cpg_rel"] = c["cpg_rel"].astype(np.uint16)
    return reads, [c for c in cs if len(c["read_start"])]


def to_translit(rec):
    """Records -> the record dicts of tools/gen_golden_unpinned.py"""
    return [dict(tid=int(rec.tid[i]), pos=int(rec.pos[i]), flag=int(rec.flag[i]), mapq=int(rec.mapq[i]), cigar=ops_of(rec, i),
                 xm=rec.xms[i].decode()) for i in range(len(rec))]


# ---- what the input holds (the non-vacuity checks of tests/test_irregular_inputs.py) -------------------------------------------
def called_sites(reads, min_qual=10):
    soa = reads.soa()
    n = np.diff(soa["cpg_off"].astype(np.int64))
    ok = np.repeat(soa["mapq"] >= min_qual, n)
    key = soa["tid"].astype(np.int64).repeat(n) << 32 | (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    return np.unique(key[ok])


def max_sites_in(sites, width, aligned=False):
    """most sites in `width` positions: any window, or the tiles [k width, (k + 1) width)"""
    if len(sites) == 0:
        return 0
    if aligned:
        return int(np.unique(sites // width, return_counts=True)[1].max())
    return int((np.searchsorted(sites, sites + width, side="left") - np.arange(len(sites))).max())


def rank_gaps(reads, min_qual=10):
    """per read with >= 2 calls, the rank distance (among the called sites) of each pair of consecutive calls"""
    soa = reads.soa()
    sites = called_sites(reads, min_qual)
    off = soa["cpg_off"].astype(np.int64)
    key = soa["tid"].astype(np.int64).repeat(np.diff(off)) << 32 | (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    rk = np.searchsorted(sites, key)
    out = []
    for i in range(len(off) - 1):
        if soa["mapq"][i] >= min_qual and off[i + 1] - off[i] >= 2:
            out.append(np.diff(rk[off[i]:off[i + 1]]))
    return out


def lpmd_bound_pairs(reads, min_distance, max_distance):
    """pairs of calls of one read whose query-offset distance and position distance fall on opposite sides of a bound:
    (n across min_distance, n across max_distance)"""
    soa = reads.soa()
    off = soa["cpg_off"].astype(np.int64)
    rel = soa["cpg_rel"].astype(np.int64)
    pos = (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    n_min = n_max = 0
    for i in range(len(off) - 1):
        r, p = rel[off[i]:off[i + 1]], pos[off[i]:off[i + 1]]
        if len(r) < 2:
            continue
        dr, dp = r[None, :] - r[:, None], p[None, :] - p[:, None]
        up = np.triu(np.ones_like(dr, bool), 1)
        n_min += int(((dr >= min_distance) != (dp >= min_distance))[up].sum())
        n_max += int(((dr <= max_distance) != (dp <= max_distance))[up].sum())
    return n_min, n_max


# ---- file orders: what the unsorted paths replay (tests/test_gpu_irregular_paths.py) -----------------------------------------------
ORDERS = ("shuffled", "strides", "moved", "nearly", "flush_trap")
TRAPS = ("far", "low_mapq", "no_call", "other_contig")


def rows_of(rec):
    """bamio.Records -> rows (records_from_rows' input)"""
    return [(int(rec.tid[i]), int(rec.pos[i]), int(rec.flag[i]), int(rec.mapq[i]), ops_of(rec, i), rec.xms[i].decode()) for i in range(len(rec))]


def read_calls(rec):
    """-> (soa, calls per record, first reported call position per record (-1: none))"""
    soa = pyoracle.Reads.decode(rec).soa()
    off = soa["cpg_off"].astype(np.int64)
    n = np.diff(off)
    first = np.full(len(n), -1, np.int64)
    first[n > 0] = (soa["cpg_pos"][off[:-1][n > 0]] & 0x7fffffff).astype(np.int64)
    return soa, n, first


def flush_traps(rec, rng, kinds=TRAPS, per_kind=12, min_qual=10):
    """the coordinate order of `rec` with, between two consecutive passing readers A, B of a site s, one record moved there from
    elsewhere -- each a case where flushing by the wrong key or at the wrong step changes what the reference computes:
      far           passing, same contig, start <= s + 150 < first call: flushes s for PDR (margin 150), MHL and FDRP; by its start it would not
      low_mapq      below min_qual, calls beyond s: flushes s for MHL only (mhl.rs:162 comes before the filters of :176-183)
      no_call       no call, same contig, start > s + 150: flushes nothing (by its start it would)
      other_contig  passing, a later contig: flushes every site of s's contig
    -> (permutation, [(kind, tid, s, moved record)])"""
    soa, n, first = read_calls(rec)
    start, mq, tid = soa["start"].astype(np.int64), soa["mapq"].astype(np.int64), rec.tid.astype(np.int64)
    off = soa["cpg_off"].astype(np.int64)
    site = (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    rd = np.repeat(np.arange(len(n)), n)
    ok = mq[rd] >= min_qual
    key = tid[rd] << 32 | site
    o = np.lexsort((rd[ok], key[ok]))
    k_, r_ = key[ok][o], rd[ok][o]
    pairs = np.nonzero((k_[1:] == k_[:-1]) & (r_[1:] != r_[:-1]))[0]         # (A, B) = (r_[j], r_[j + 1]): consecutive readers of k_[j]
    rng.shuffle(pairs)
    used, after, traps = set(), {}, []
    want = {kd: per_kind for kd in kinds}
    for j in pairs:
        a, b, t, s = int(r_[j]), int(r_[j + 1]), int(k_[j] >> 32), int(k_[j] & 0xffffffff)
        if a in used or b in used or not any(want.values()):
            continue
        for kd in kinds:
            if not want[kd]:
                continue
            if kd == "far":
                m = (tid == t) & (mq >= 42) & (n >= 4) & (first > s + 150) & (start <= s + 150)
            elif kd == "low_mapq":
                m = (tid == t) & (mq < min_qual) & (n >= 1) & (first > s)
            elif kd == "no_call":
                m = (tid == t) & (n == 0) & (start > s + 150)
            else:
                m = (tid > t) & (mq >= 42) & (n >= 1)
            c = [int(x) for x in np.nonzero(m)[0] if int(x) not in used]
            if not c:
                continue
            x = c[int(rng.integers(0, len(c)))]
            used.update((a, b, x))
            after.setdefault(a, []).append(x)
            traps.append((kd, t, s, x))
            want[kd] -= 1
            break
    moved = set(x for _, _, _, x in traps)
    perm = []
    for i in range(len(n)):
        if i not in moved:
            perm.append(i)
            perm += after.get(i, [])
    assert sorted(perm) == list(range(len(n)))
    return np.array(perm), traps


def shuffle(rec, kind, rng):
    """`rec` (coordinate-sorted) in one of ORDERS: the four of tests/test_gpu_fileorder.py (fully shuffled, interleaved sorted
    strides, blocks of the sorted file moved, nearly sorted with the contigs mixed) and flush_traps -> (Records, permutation)"""
    n = len(rec)
    if kind == "shuffled":
        perm = rng.permutation(n)
    elif kind == "strides":
        perm = np.argsort(np.arange(n) % int(rng.integers(2, 9)), kind="stable")
    elif kind == "moved":
        perm = np.arange(n)
        for _ in range(int(rng.integers(2, 6))):
            a, b = sorted(rng.integers(0, n, size=2))
            perm = np.concatenate([perm[:a], perm[b:], perm[a:b]])
    elif kind == "nearly":
        perm = np.argsort(rec.pos + rng.integers(-60, 60, size=n), kind="stable")
    elif kind == "flush_trap":
        perm, _ = flush_traps(rec, rng)
    else:
        raise ValueError(kind)
    return rec.subset(perm), perm


def shifted_starts(rec):
    """the records whose first reported call is at start - 1 (a shifted flag on a read starting at a CpG's C, or a reverse-strand
    read starting at its G): a shard cut / region end at such a record's start p leaves it a call on the other side"""
    soa, n, first = read_calls(rec)
    return np.nonzero((n > 0) & (first == soa["start"].astype(np.int64) - 1))[0]


REGION_END = 16384          # a multiple of the .bai's 16-kb leaf bins: a record starting there opens a bin that [.., end) misses
PILE_AT = 23001


def forced_records(seed=3):
    """two contigs of irregular reads, plus, on the first: a reverse-strand read starting at REGION_END whose first base is the G
    of the CpG at REGION_END - 1 (reported REGION_END - 1), and a pile of 240 reads starting at PILE_AT, a third of them such
    readers of PILE_AT - 1; without the reads the reference's FDRP panics on (fdrp_safe) -> (Records coordinate-sorted, names,
    index of the read at REGION_END)"""
    rec, names = make_records(seed, n_contigs=2, length=24_000, n_reads=2_400, density=0.03)
    rng = np.random.default_rng(seed)
    e = REGION_END
    planted = [(0, e, 16, 42, [("M", 100)], "z" + "." * 49 + "Z" + "." * 49), (0, e - 1, 0, 42, [("M", 60)], "Z" + "." * 59)]
    for k in range(240):
        xm = ["."] * 120
        if k % 3 == 0:                                             # flag 16: the call at PILE_AT reports PILE_AT - 1
            xm[0] = "Zz"[k % 2]
        for q in (11, 12, 40, 41, 90):
            xm[q] = "Z" if rng.random() < 0.7 else "z"
        planted.append((0, PILE_AT, 16 if k % 3 == 0 else int(rng.choice([0, 99, 65])), 42, [("M", 120)], "".join(xm)))
    rows = planted + rows_of(rec)
    rows.sort(key=lambda r: (r[0], r[1]))
    out = fdrp_safe(records_from_rows(rec.refs, rows))
    at = int(np.nonzero((out.tid == 0) & (out.pos == e) & (out.flag == 16))[0][0])
    return out, names, at


def record_blocks(bam):
    """BGZF block index (from the top of the file, as mth_host_bgzf_blocks counts) of every record of a block-aligned BAM"""
    recs, _ = bamio.bam_record_offsets(bam)
    return np.array([r[5] for r in recs], np.int64)


def readers(rec, beg, end):
    """records that report a call at a site in [beg, end) or start in it; beg / end are (tid, pos), compared as tuples"""
    soa, n, _ = read_calls(rec)
    site = (soa["cpg_pos"] & 0x7fffffff).astype(np.int64)
    rd = np.repeat(np.arange(len(n)), n)
    t = rec.tid.astype(np.int64)
    lin = lambda tt, p: tt * (1 << 33) + p
    lo, hi = lin(*beg), lin(*end)
    c = lin(t[rd], site)
    s = lin(t, soa["start"].astype(np.int64))
    keep = np.zeros(len(n), bool)
    keep[rd[(c >= lo) & (c < hi)]] = True
    keep |= (s >= lo) & (s < hi) & (soa["start"] >= 0)
    return np.nonzero(keep)[0]
