"""Inputs and a CPU model for the device walk over records that straddle BGZF blocks (mth_bgzf_decode_straddle; tests/
test_straddle_inputs.py checks the inputs on the CPU, tests/test_gpu_straddle.py runs them): BAMs re-cut at a byte count as htsjdk,
sambamba and most writers that are not htslib cut them, records carrying decoy record headers in an aux array, records far longer
than a block, the guess rule of k_straddle_guess restated, and the true record offsets to hold the guesses against."""
import gzip
import struct

import numpy as np

from oracle import bamio

MAX_ROUNDS = 64                      # MTH_STRADDLE_MAX_ROUNDS


def header_bytes(raw):
    l_text, = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, o)
        o += 8 + l_name
    return o


def reblock(src, dst, cut):
    """re-cut a BAM's inflated stream, header included, every `cut` bytes (+ the EOF block): nearly every block then starts inside a
    record"""
    raw = gzip.decompress(open(src, "rb").read())
    with open(dst, "wb") as fh:
        for o in range(0, len(raw), cut):
            fh.write(bamio._bgzf_block(raw[o:o + cut]))
        fh.write(bamio._bgzf_block(b""))
    return dst


def write_cut(path, rec, cut, realistic=False):
    """bamio.write_bam cuts every 60 000 bytes itself; any other cut goes through reblock"""
    if cut == 60000:
        bamio.write_bam(path, rec, realistic=realistic)
    else:
        bamio.write_bam(path + ".60000", rec, realistic=realistic)
        reblock(path + ".60000", path, cut)
    return path


# ---- decoys and giants: aux arrays in front of XM:Z (bamio.write_bam's aux_extra) ------------------------------------------------
def _fake_header(block_size, l_read_name, l_seq):
    h = struct.pack("<iiiBBHHHiiii", block_size, 0, 0, l_read_name, 0, 4680, 0, 0, l_seq, -1, -1, 0)
    assert len(h) == 36 and 32 + l_read_name + (l_seq + 1) // 2 + l_seq <= block_size
    return h + bytes(4 + block_size - 36)


DECOY_PAIR = _fake_header(48, 1, 8) + _fake_header(36, 2, 0)      # each passes the guess rule and leads exactly to the next


def add_decoys(rec, every, repeats=6):
    """every `every`-th record carries ZD:B:C = `repeats` chained pairs of fake record headers"""
    body = DECOY_PAIR * repeats
    pre = b"ZDBC" + struct.pack("<i", len(body)) + body + b"NMC\0"
    rec.aux_extra = [(pre, b"XRZCT\0") if i % every == 0 else (b"NMC\0", b"XRZCT\0") for i in range(len(rec))]
    return rec


def add_giants(rec, every=500, n_bytes=150_000, seed=11):
    """every `every`-th record carries a ZG:B:C array of n_bytes random bytes: records that cover whole blocks"""
    rng = np.random.default_rng(seed)
    extra = list(getattr(rec, "aux_extra", None) or [(b"NMC\0", b"XRZCT\0")] * len(rec))
    for i in range(0, len(rec), every):
        extra[i] = (b"ZGBC" + struct.pack("<i", n_bytes) + rng.integers(0, 256, size=n_bytes, dtype=np.uint8).tobytes() + extra[i][0], extra[i][1])
    rec.aux_extra = extra
    return rec


# ---- what a file holds --------------------------------------------------------------------------------------------------------
class Layout:
    """a BAM file as the device load sees it: the inflated stream, the blocks with data (stream bounds), the true record offsets"""

    def __init__(self, path):
        from tests.test_gpu_inflate import block_table
        self.path = path
        self.fb, self.coff, self.csize, self.isize, self.hbytes, raw = block_table(path)
        self.raw = bytes(raw)
        self.total = len(self.raw)
        assert self.hbytes == header_bytes(self.raw)
        self.b1 = np.cumsum(self.isize.astype(np.int64))
        self.b0 = self.b1 - self.isize.astype(np.int64)
        # true record starts as stream offsets: bam_record_offsets gives virtual offsets (file offset of the block << 16 | offset in it)
        recs, _ = bamio.bam_record_offsets(path)
        hdr_at = {int(c) - 18: int(b) for c, b in zip(self.coff, self.b0)}          # bamio's blocks: 18 header bytes, then the payload
        self.starts = np.array([hdr_at[r[3] >> 16] + (r[3] & 0xffff) for r in recs], np.int64)
        self.ends = np.concatenate([self.starts[1:], [self.total]]).astype(np.int64)
        assert len(self.starts) == 0 or self.starts[0] == self.hbytes

    def blocks_cut_inside_a_record(self):
        """share of the blocks (after the one the records start in) whose first byte is not a record start"""
        later = self.b0[self.b0 > self.hbytes]
        return float(np.mean(~np.isin(later, self.starts))) if len(later) else 0.0

    def first_start_in(self):
        """per block: the first true record start inside it, -1 if none"""
        k = np.searchsorted(self.starts, np.maximum(self.b0, self.hbytes), side="left")
        s = np.where(k < len(self.starts), self.starts[np.minimum(k, len(self.starts) - 1)], self.total)
        return np.where(s < self.b1, s, -1)

    def guesses(self):
        """k_straddle_guess restated: per block its guess, -1 if it has none"""
        ok, nxt = plausible_all(self.raw)
        n = len(ok)
        follow = nxt == self.total                        # the record leads to another offset that passes, or exactly to the stream's end
        idx = np.nonzero(ok & (nxt < n))[0]
        follow[idx] = ok[nxt[idx]]
        good = ok & follow
        out = np.full(len(self.b0), -1, np.int64)
        for b, (lo, hi) in enumerate(zip(self.b0, self.b1)):
            if lo <= self.hbytes:
                out[b] = self.hbytes                      # the block that holds first_byte (and the header blocks before it) start there
                continue
            w = good[lo:min(hi, n)]
            if w.any():
                out[b] = lo + int(np.argmax(w))
        return out

    def wrong_guesses(self):
        """blocks whose guess is not the first record start inside them (a block without a guess or without a start counts)"""
        g, s = self.guesses(), self.first_start_in()
        later = self.b0 > self.hbytes
        return int(np.sum(later & ((g != s) | (g < 0))))

    def carry_after(self, n_blocks):
        """bytes from the start of the record the stream of the first n_blocks blocks ends in to that stream's end"""
        end = int(self.b1[n_blocks - 1])
        if end <= self.hbytes:
            return 0
        k = int(np.searchsorted(self.starts, end, side="left"))     # records starting before `end`
        if k == 0:
            return 0
        return end - int(self.starts[k - 1]) if self.ends[k - 1] > end else 0

    def call(self, eng, b0, b1, first_byte, **flags):
        """blocks [b0, b1) through Engine.bgzf_decode_straddle, as a caller that hands over only their file bytes"""
        lo = int(self.coff[b0])
        hi = int(self.coff[b1 - 1] + self.csize[b1 - 1]) + 8
        return eng.bgzf_decode_straddle(self.fb[lo:hi], self.coff[b0:b1] - np.uint64(lo), self.csize[b0:b1], self.isize[b0:b1], first_byte, **flags)

    def in_calls(self, eng, cuts, last=True):
        """the whole file as len(cuts) + 1 calls cut before the blocks `cuts` -> [info of each call]"""
        edges = [0] + list(cuts) + [len(self.coff)]
        infos = []
        for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            fin = i == len(edges) - 2
            first_byte = max(0, self.hbytes - int(self.b0[a]))
            infos.append(self.call(eng, a, b, first_byte, append=i > 0, last=fin and last)[2])
        return infos


def plausible_all(raw):
    """the guess rule at every offset p with p + 36 <= len(raw) -> (passes, where its block_size leads)"""
    u = np.frombuffer(raw, np.uint8).astype(np.int64)
    n = len(u) - 35
    if n <= 0:
        return np.zeros(0, bool), np.zeros(0, np.int64)

    def i32(off):
        v = u[off:off + n] | (u[off + 1:off + 1 + n] << 8) | (u[off + 2:off + 2 + n] << 16) | (u[off + 3:off + 3 + n] << 24)
        return np.where(v >= 1 << 31, v - (1 << 32), v)
    bs, ref, pos, l_seq, next_ref, next_pos = i32(0), i32(4), i32(8), i32(20), i32(24), i32(28)
    l_name = u[12:12 + n]
    n_cigar = u[16:16 + n] | (u[17:17 + n] << 8)
    ok = (bs >= 32) & (ref >= -1) & (next_ref >= -1) & (pos >= -1) & (next_pos >= -1) & (l_name >= 1) & (l_seq >= 0) & \
         (32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq <= bs)
    return ok, np.arange(n, dtype=np.int64) + 4 + (bs & 0xffffffff)


# ---- the scheme itself on the CPU: what info.rounds / info.repaired_blocks of one whole-file call should be ----------------------
NONE, PAST = -1, 1 << 62


def _walk(lay, entry, b1):
    """records that start in [entry, b1) -> (exit, count); as str_walk of mth_inflate.hip"""
    if entry == NONE:
        return PAST, 0
    p, n, raw, total = entry, 0, lay.raw, lay.total
    while p < b1:
        if p + 4 > total:
            return PAST, n
        bs, = struct.unpack_from("<i", raw, p)
        if bs < 32 or p + 4 + bs > total:
            return PAST, n
        n += 1
        p += 4 + bs
    return p, n


def model(lay):
    """guess, walk, then rounds of link check + repair -> dict(rounds, repaired_blocks, settled, offsets of the records found)"""
    nb = len(lay.b0)
    entry = [int(g) for g in lay.guesses()]
    walked = [_walk(lay, entry[b], int(lay.b1[b])) for b in range(nb)]
    ex, cnt = [w[0] for w in walked], [w[1] for w in walked]
    rounds = repaired = 0
    settled = False
    for r in range(MAX_ROUNDS + 1):
        want = [lay.hbytes] + ex[:-1]
        bad = [b for b in range(nb) if entry[b] != want[b]]
        if not bad:
            settled = True
            break
        if r == MAX_ROUNDS:
            break
        # from a predecessor that agrees with its own; an exit that says "cannot go on" is believed only of the first block in doubt
        fix = [b for b in bad if b == bad[0] or (entry[b - 1] == want[b - 1] and want[b] < PAST)]
        for b in fix:                                       # (all from the state before the round: two generations on the device)
            entry[b] = want[b]
        for b in fix:
            ex[b], cnt[b] = _walk(lay, entry[b], int(lay.b1[b]))
        repaired += len(fix)
        rounds = r + 1
    offs = []
    if settled:
        for b in range(nb):
            p = entry[b]
            for _ in range(cnt[b]):
                offs.append(p)
                p += 4 + struct.unpack_from("<i", lay.raw, p)[0]
    return dict(rounds=rounds, repaired_blocks=repaired, settled=settled, offsets=np.array(offs, np.int64))


# ---- the inputs of the tests --------------------------------------------------------------------------------------------------
CUTS = (60000, 4093, 700)


def weird():
    from tests.test_host_decode import _weird_records
    return _weird_records()


def irregular():
    from tests import irregular_util
    return irregular_util.make_records(950, n_contigs=2, length=8_000, n_reads=1_200, density=0.03)[0]


def chunk_edges(lay, limit=1 << 20):
    """first block of every chunk the CLI's loader cuts at METHEOR_DEVICE_CHUNK_MB=1 (whole blocks, <= limit file bytes each)"""
    edges, b0, nb = [], 0, len(lay.coff)
    while b0 < nb:
        edges.append(b0)
        b1 = b0
        while b1 < nb and (b1 == b0 or int(lay.coff[b1]) + int(lay.csize[b1]) - int(lay.coff[b0]) <= limit):
            b1 += 1
        b0 = b1
    return edges


def inside_cuts(lay, n_calls):
    """n_calls - 1 block indices, about evenly spaced, each a block that starts inside a record"""
    nb, cuts = len(lay.b0), []
    for k in range(1, n_calls):
        b = max(k * nb // n_calls, (cuts[-1] + 1) if cuts else 1)
        while b < nb and (lay.b0[b] in lay.starts or lay.b0[b] <= lay.hbytes):
            b += 1
        cuts.append(b)
    assert cuts[-1] < nb and len(set(cuts)) == len(cuts)
    return cuts


def block_inside_one_record(lay):
    """the last block that lies wholly inside one record (no start in it, none at its first byte or at the next block's)"""
    s = lay.first_start_in()
    for b in range(len(lay.b0) - 2, 0, -1):
        if s[b] < 0 and lay.b0[b] not in lay.starts and lay.b1[b] not in lay.starts and lay.b1[b] < lay.total:
            return b
    return None


RECIPES = {
    # name: (records, cut, realistic)
    "sparse": (lambda: add_decoys(irregular(), 40), None, True),
    "dense": (lambda: add_decoys(irregular(), 1, repeats=10), None, True),
    "giant": (lambda: add_giants(irregular(), 500), None, True),
}


def chunked_records():
    """irregular reads the reference's FDRP does not panic on, every 150th with a 150 000-byte array: ~3 MB that do not compress"""
    from tests import irregular_util
    return add_giants(irregular_util.fdrp_safe(irregular()), 150)


CHUNKED_CUT = 20000


def region_inputs(d):
    """irregular_util.forced_records() written raw, re-cut every 4 093 bytes, and its block-aligned copy, both indexed
    -> (records, names, straddling path, aligned path)"""
    import os
    from tests import irregular_util, util
    rec, names, _ = irregular_util.forced_records()
    raw, cut, ali = os.path.join(d, "raw.bam"), os.path.join(d, "cut.bam"), os.path.join(d, "aligned.bam")
    bamio.write_bam(raw, rec)
    reblock(raw, cut, 4093)
    util.reblock_aligned(raw, ali)
    bamio.write_bai(cut)
    bamio.write_bai(ali)
    return rec, names, cut, ali


SECOND_REGION = (1, 3000, 12000)        # (tid, beg, end): its first record lies mid-file, so the plan cannot start at the top


def flush_trap_file(d):
    """the unsorted GPU input in a flush-trap order, cut every 4 093 bytes -> (records in file order, path)"""
    import os
    from tests import irregular_util
    from tests import test_irregular_paths as P
    sh, _ = irregular_util.shuffle(P.unsorted_records(0), "flush_trap", np.random.default_rng(2))
    return sh, write_cut(os.path.join(d, "flush_trap.bam"), sh, 4093)


def genome_files(d):
    """an untagged generated input (tests/genome_util.py) as the SAM converter writes it -- whole records per block -- and cut every
    4 093 bytes, plus its FASTA -> (aligned path, cut path, fasta path)"""
    import os
    from metheor_amd import hostapi
    from tests import genome_util as gu
    from tests import tag_util
    g = gu.generate(1)
    recs, _ = gu.runnable(g)
    sam, fa, ali, cut = (os.path.join(d, x) for x in ("g_in.sam", "g.fa", "g_in.bam", "g_cut.bam"))
    open(sam, "w").write(gu.sam_text([(g["name"], len(g["contig"]))], recs))
    tag_util.write_fasta(fa, g["name"], g["contig"])
    f = hostapi.BamFile(sam)
    open(ali, "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    reblock(ali, cut, 4093)
    return ali, cut, fa
