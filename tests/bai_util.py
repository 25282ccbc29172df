"""The .bai index as a model in plain Python (tests/test_bai_model.py, test_gpu_bai.py, test_gpu_tag_index.py).

index_rows(): the index of explicit records, block cuts and block file offsets -- the tables mth_bai_finish returns, or the
refusal.  bai_bytes(): the whole index file of a BAM on disk, built on oracle.bamio.bam_record_offsets / build_bai (pinned on
the reference's samtools-made fixtures by tests/test_bai.py) plus the two parts that model leaves out: samtools' metadata
pseudo-bin 37450 and the trailing n_no_coor.  HAND: the hand-made record set the CPU and GPU tests share."""
import struct
import zlib
from collections import namedtuple

import numpy as np

from oracle import bamio

OPS = "MIDNSHP=X"
MAX_END = 1 << 29
MTH_ERR_UNSORTED, MTH_ERR_RANGE, MTH_ERR_FORMAT = -4, -7, -10

# a record: refID, pos, flag, [(length, op letter)], bytes appended behind the CIGAR (they stand for the read, its qualities and tags)
Rec = namedtuple("Rec", "ref pos flag cigar extra")


def rec(ref, pos, cigar="", flag=0, extra=0):
    ops, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            ops.append((int(num), ch)); num = ""
    return Rec(ref, pos, flag, ops, extra)


def reflen(r):
    return sum(l for l, o in r.cigar if o in "MDN=X")


def end_of(r):
    return r.pos + max(1, reflen(r))


def record_bytes(r, k=0):
    name = b"r%d\0" % k
    cig = b"".join(struct.pack("<I", (l << 4) | OPS.index(o)) for l, o in r.cigar)
    body = struct.pack("<iiBBHHHiiii", r.ref, r.pos, len(name), 30, 0, len(r.cigar), r.flag, 0, -1, -1, 0) + name + cig + bytes(r.extra)
    return struct.pack("<i", len(body)) + body


def pack(records):
    """-> (raw bytes of the records back to back, uint64[n + 1] offsets)"""
    parts = [record_bytes(r, k) for k, r in enumerate(records)]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(parts), off


def cuts_at_record_ends(off, limit):
    """block cuts as the BAM writer makes them: a block takes whole records while they fit `limit` bytes; a record longer than a
    block starts one and fills consecutive blocks"""
    off = [int(x) for x in off]
    cuts, start = [0], 0
    for k in range(len(off) - 1):
        if off[k + 1] - start > limit and off[k] > start:
            cuts.append(off[k]); start = off[k]
        while off[k + 1] - start > limit:
            start += limit; cuts.append(start)
    if off[-1] > cuts[-1]:
        cuts.append(off[-1])
    return cuts


def reg2bin(beg, end):
    return bamio.reg2bin(beg, end)


def sort_key(ref, pos):
    return (1 << 40, 0) if ref < 0 else (ref, pos)


def first_refusal(records, ref_len):
    """(status, ordinal) of the lowest record the index refuses, or None"""
    before = None
    for k, r in enumerate(records):
        if r.ref >= len(ref_len):
            return MTH_ERR_RANGE, k
        if before is not None and sort_key(r.ref, r.pos) < before:
            return MTH_ERR_UNSORTED, k
        if r.ref >= 0 and (r.pos < 0 or end_of(r) > MAX_END or end_of(r) > ref_len[r.ref]):
            return MTH_ERR_RANGE, k
        before = sort_key(r.ref, r.pos)
    return None


def voffsets(off, cuts, coffs):
    """per record (vbeg, vend): oracle.bamio.bam_record_offsets' rule over explicit cuts -- the last block that starts at or before
    the byte; a record END that falls on a block's start keeps the block before"""
    starts = np.asarray(cuts, np.uint64)
    out = []
    for k in range(len(off) - 1):
        so, se = int(off[k]), int(off[k + 1])
        b = int(np.searchsorted(starts, so, side="right")) - 1
        e = int(np.searchsorted(starts, se, side="right")) - 1
        if se == int(starts[e]) and e > 0:
            e -= 1
        out.append(((int(coffs[b]) << 16) | (so - int(starts[b])), (int(coffs[e]) << 16) | (se - int(starts[e]))))
    return out


def tables(entries, ref_len, n_no_coor):
    """entries: per placed record, file order, (ref, beg, end, flag, vbeg, vend) -> the tables of mth_bai_finish"""
    n_refs = len(ref_len)
    runs = []                                            # [ref, bin, vbeg, vend] per run of consecutive records of one (ref, bin)
    lin = [dict() for _ in range(n_refs)]
    meta = np.zeros((n_refs, 4), np.uint64)
    seen = [False] * n_refs
    for ref, beg, end, flag, vb, ve in entries:
        b = reg2bin(beg, end)
        if runs and runs[-1][0] == ref and runs[-1][1] == b:
            runs[-1][3] = ve
        else:
            runs.append([ref, b, vb, ve])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[ref][w] = min(lin[ref].get(w, vb), vb)
        if not seen[ref]:
            seen[ref] = True
            meta[ref, 0] = vb
        meta[ref, 0] = min(int(meta[ref, 0]), vb); meta[ref, 1] = max(int(meta[ref, 1]), ve)
        meta[ref, 3 if flag & 4 else 2] += 1
    for t in range(n_refs):
        if not seen[t]:
            meta[t, 0] = (1 << 64) - 1                   # the device's "no record": min over nothing
    order = sorted(range(len(runs)), key=lambda k: (runs[k][0], runs[k][1]))      # stable: file order inside a bin
    bins = []
    for k in order:
        if bins and bins[-1][0] == runs[k][0] and bins[-1][1] == runs[k][1]:
            bins[-1][2] += 1
        else:
            bins.append([runs[k][0], runs[k][1], 1])
    lin_off = np.zeros(n_refs + 1, np.uint64)
    lin_off[1:] = np.cumsum([(min(int(l), MAX_END) + 16383) >> 14 for l in ref_len])
    n_intv = np.array([max(l) + 1 if l else 0 for l in lin], np.uint32)
    flat = np.full(int(lin_off[-1]), (1 << 64) - 1, np.uint64)
    for t in range(n_refs):
        last = 0
        for w in range(int(n_intv[t])):
            last = lin[t].get(w, last)
            flat[int(lin_off[t]) + w] = last
    return dict(n_refs=n_refs, n_no_coor=n_no_coor,
                chunk_beg=np.array([runs[k][2] for k in order], np.uint64), chunk_end=np.array([runs[k][3] for k in order], np.uint64),
                bin_ref=np.array([b[0] for b in bins], np.int32), bin_id=np.array([b[1] for b in bins], np.uint32),
                bin_n_chunks=np.array([b[2] for b in bins], np.uint32),
                ref_n_bins=np.bincount(np.array([b[0] for b in bins], np.int64), minlength=n_refs).astype(np.uint32),
                ref_n_intv=n_intv, lin_off=lin_off, lin=flat, meta=meta)


def index_rows(records, cuts, coffs, ref_len):
    """the model over explicit inputs: ("error", status, ordinal) or the tables"""
    bad = first_refusal(records, ref_len)
    if bad:
        return ("error",) + bad
    _, off = pack(records)
    vo = voffsets(off, cuts, coffs)
    ent = [(r.ref, r.pos, end_of(r), r.flag, vb, ve) for r, (vb, ve) in zip(records, vo) if r.ref >= 0]
    return tables(ent, ref_len, sum(1 for r in records if r.ref < 0))


def same_tables(got, want):
    """[] or the names of the tables that differ; the linear table is compared where it is defined (below n_intv per reference)"""
    bad = [k for k in ("n_refs", "n_no_coor") if int(got[k]) != int(want[k])]
    for k in ("chunk_beg", "chunk_end", "bin_ref", "bin_id", "bin_n_chunks", "ref_n_bins", "ref_n_intv", "lin_off"):
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            bad.append(k)
    if not bad:
        for t in range(int(want["n_refs"])):
            o, n = int(want["lin_off"][t]), int(want["ref_n_intv"][t])
            if not np.array_equal(got["lin"][o:o + n], want["lin"][o:o + n]):
                bad.append("lin[%d]" % t)
            has = int(want["meta"][t, 2]) + int(want["meta"][t, 3]) > 0
            if not np.array_equal(got["meta"][t, 2:], want["meta"][t, 2:]) or (has and not np.array_equal(got["meta"][t], want["meta"][t])):
                bad.append("meta[%d]" % t)
    return bad


def frame(t):
    """the tables as the bytes of a .bai file (what mth_host_bai_write writes)"""
    out = bytearray(b"BAI\1") + struct.pack("<i", int(t["n_refs"]))
    b = c = 0
    for r in range(int(t["n_refs"])):
        has = int(t["meta"][r, 2]) + int(t["meta"][r, 3]) > 0
        nb = int(t["ref_n_bins"][r])
        out += struct.pack("<i", nb + (1 if has else 0))
        for _ in range(nb):
            nc = int(t["bin_n_chunks"][b])
            out += struct.pack("<Ii", int(t["bin_id"][b]), nc)
            for _ in range(nc):
                out += struct.pack("<QQ", int(t["chunk_beg"][c]), int(t["chunk_end"][c])); c += 1
            b += 1
        if has:
            out += struct.pack("<Ii4Q", 37450, 2, *[int(x) for x in t["meta"][r]])
        o, n = int(t["lin_off"][r]), int(t["ref_n_intv"][r])
        out += struct.pack("<i", n) + np.asarray(t["lin"][o:o + n], "<u8").tobytes()
    return bytes(out + struct.pack("<Q", int(t["n_no_coor"])))


def bam_flags(path):
    """flag of every record of a BAM file, file order"""
    raw, o, parts = open(path, "rb").read(), 0, []
    while o < len(raw):
        bsize, = struct.unpack_from("<H", raw, o + 16)
        parts.append(zlib.decompress(raw[o + 18:o + bsize + 1 - 8], -15))
        o += bsize + 1
    d = b"".join(parts)
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p); p += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", d, p); p += 8 + l
    flags = []
    while p < len(d):
        bs, = struct.unpack_from("<i", d, p)
        flags.append(struct.unpack_from("<H", d, p + 18)[0])
        p += 4 + bs
    return flags


def bai_bytes(bam_path):
    """the index file of a coordinate-sorted BAM: oracle.bamio.build_bai's bins, chunks and linear index, plus per reference with
    records the pseudo-bin 37450 (first offset, last end; records with flag 0x4 clear, set) and the trailing n_no_coor"""
    recs, n_ref = bamio.bam_record_offsets(bam_path)
    refs = bamio.build_bai(bam_path)
    flags = bam_flags(bam_path)
    assert len(flags) == len(recs)
    out = bytearray(b"BAI\1") + struct.pack("<i", n_ref)
    for t, r in enumerate(refs):
        mine = [(x, f) for x, f in zip(recs, flags) if x[0] == t]
        out += struct.pack("<i", len(r["bins"]) + (1 if mine else 0))
        for b in sorted(r["bins"]):
            out += struct.pack("<Ii", b, len(r["bins"][b]))
            for cb, ce in r["bins"][b]:
                out += struct.pack("<QQ", cb, ce)
        if mine:
            out += struct.pack("<Ii4Q", 37450, 2, min(x[3] for x, _ in mine), max(x[4] for x, _ in mine),
                               sum(1 for _, f in mine if not f & 4), sum(1 for _, f in mine if f & 4))
        out += struct.pack("<i", len(r["ioffset"])) + struct.pack("<%dQ" % len(r["ioffset"]), *r["ioffset"])
    return bytes(out + struct.pack("<Q", sum(1 for x in recs if x[0] < 0)))


# ---- the hand-made record set -------------------------------------------------------------------------------------------------
# three contigs, the middle one without records; c2 is as long as a .bai reaches
HAND_REF_LEN = [70_000_000, 5000, 1 << 29]
HAND = [
    rec(0, 0, "50M", extra=40),                                    # pos = 0; level-5 bin 4681
    rec(0, 100, "20S", flag=0, extra=10),                          # zero reference length: S only
    rec(0, 120, "", flag=4, extra=30),                             # placed-unmapped, no CIGAR
    rec(0, 200, "10M5I10M", extra=500),
    rec(0, 16000, "100M500N100M", extra=20),                       # crosses 2^14: level 4
    rec(0, 16380, "30M", extra=20),                                # crosses 2^14 again: a second record of bin 585, same run
    rec(0, 20000, "50M", extra=700),                               # longer than two 300-byte blocks: covers three
    rec(0, 20010, "5I", extra=11),                                 # zero reference length: I only
    rec(0, 131000, "50M100N50M", extra=20),                        # crosses 2^17: level 3
    rec(0, 1048500, "50M100N50M", extra=20),                       # crosses 2^20: level 2
    rec(0, 8388600, "5M20N5M", extra=20),                          # crosses 2^23: level 1
    rec(0, 8388700, "40M", extra=20),                              # level 5, bin A
    rec(0, 8388800, "40M", extra=20),                              #          bin A (same run)
    rec(0, 8388900, "10M20000N10M", extra=20),                     # the parent bin (level 4) between two runs of bin A
    rec(0, 8389000, "40M", extra=20),                              # level 5, bin A again: its second chunk
    rec(0, 67108800, "50M100N50M", extra=20),                      # crosses 2^26: level 0
    rec(0, 69999950, "50M", extra=20),                             # ends exactly at LN
    rec(2, 5, "30M", extra=20),
    rec(2, (1 << 29) - 40, "40M", extra=20),                       # ends at 2^29 on a contig of that length
    rec(-1, -1, "", flag=4, extra=25),
    rec(-1, -1, "", flag=4, extra=25),
]


def generated(seed=7, n=70_000):
    """n coordinate-sorted records over four contigs (one longer than 2^26), a few trailing ones without a contig -> (records, ref_len)"""
    rng = np.random.default_rng(seed)
    ref_len = [3_000_000, 80_000_000, 40_000, 9_000_000]
    share = [0.3, 0.4, 0.05, 0.25]
    out = []
    for t, ln in enumerate(ref_len):
        k = int(n * share[t])
        long = ln > 100_000                                # room for spliced records
        pos = np.sort(rng.integers(0, ln - (70_000 if long else 300), k))
        kind = rng.random(k)
        m = rng.integers(20, 150, k)
        gap = rng.integers(100, 60_000, k)
        extra = rng.integers(0, 60, k)
        for i in range(k):
            if kind[i] < 0.9 or (kind[i] < 0.97 and not long):
                cg = [(int(m[i]), "M")]
            elif kind[i] < 0.97:
                cg = [(int(m[i]), "M"), (int(gap[i]), "N"), (int(m[i]), "M")]
            else:
                cg = [(int(m[i]), "S")]
            out.append(Rec(t, int(pos[i]), 4 if kind[i] > 0.99 else 0, cg, int(extra[i])))
    out += [Rec(-1, -1, 4, [], 10)] * (n - len(out))
    return out, ref_len
