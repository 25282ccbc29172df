"""Inputs and restated rules of the chunked-load tests (tests/test_gpu_chunked_load.py on the GPU, tests/test_chunked_load_inputs.py on
the CPU): BGZF layouts, call plans over their blocks, the CLI's chunk planner (load_chunks in csrc/host/cli_main.cpp) and the pieced
copy's launch rule (inflate_blocks in csrc/mth_inflate.hip) written again in Python, and the files every case needs.  Nothing here
touches a GPU."""
import gzip
import os
import struct
import zlib

import numpy as np

MIB = 1 << 20


# ---- BGZF layout of a file ---------------------------------------------------------------------------------------------------------
def bgzf_block(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    bsize = len(comp) + 25
    assert bsize <= 65536 and len(data) <= 65536
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + comp + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def bam_header_bytes(raw):
    l_text, = struct.unpack_from("<i", raw, 4)
    h = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, h); h += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, h); h += 8 + l_name
    return h


class Layout:
    """a BAM file as the load calls see it: the bytes as ONE np.uint8 array (slices of it keep base + offset, what staging matches on),
    payload offset / payload size / inflated size of every block with data, the inflated stream, the header's size in it"""

    def __init__(self, path):
        self.path = path
        self.arr = np.fromfile(path, np.uint8)
        fb = self.arr.tobytes()
        o, coff, csize, isize = 0, [], [], []
        while o < len(fb):
            xlen, = struct.unpack_from("<H", fb, o + 10)
            assert xlen == 6 and fb[o + 12:o + 14] == b"BC"
            total = struct.unpack_from("<H", fb, o + 16)[0] + 1
            isz, = struct.unpack_from("<I", fb, o + total - 4)
            if isz:
                coff.append(o + 18); csize.append(total - 26); isize.append(isz)
            o += total
        self.coff, self.csize, self.isize = np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32)
        self.raw = gzip.decompress(fb)
        self.hbytes = bam_header_bytes(self.raw)
        self.u1 = np.cumsum(self.isize.astype(np.int64))
        self.u0 = self.u1 - self.isize.astype(np.int64)
        self.n_blocks = len(coff)

    def first_data_block(self):
        """the block the first record starts in"""
        return int(np.searchsorted(self.u1, self.hbytes, side="right"))

    def call(self, b0, b1):
        """blocks [b0, b1) as one library call: (view of the file bytes, offsets relative to it, csize, isize, first_byte)"""
        if b1 == b0:
            return self.arr[0:0], np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
        lo, hi = int(self.coff[b0]), int(self.coff[b1 - 1]) + int(self.csize[b1 - 1]) + 8
        first = min(max(self.hbytes - int(self.u0[b0]), 0), int(self.u1[b1 - 1] - self.u0[b0]))
        return self.arr[lo:hi], self.coff[b0:b1] - np.uint64(lo), self.csize[b0:b1], self.isize[b0:b1], first

    def record_block_starts(self):
        """per block: index of the first record that starts in it (records never straddle here), and the record count"""
        o, starts = self.hbytes, []
        while o < len(self.raw):
            starts.append(o)
            o += 4 + struct.unpack_from("<i", self.raw, o)[0]
        starts = np.array(starts, np.int64)
        return np.searchsorted(starts, self.u0, side="left"), len(starts)


def relayout(src, dst, cut_before=(), stored_blocks=0, header_block=0xff00, block_bytes=0xff00, cut_bytes=0):
    """rewrite a BAM with whole records per block, as htslib lays a file out: the header in blocks of its own (header_block bytes
    each), then records packed greedily into <= block_bytes-byte blocks, a new block also before the record indices in cut_before; the
    first stored_blocks record blocks are written at level 0 (stored: as large as their content).  cut_bytes: the record stream is
    cut every cut_bytes bytes instead, records straddle the blocks (what htsjdk-family writers do)"""
    raw = gzip.decompress(open(src, "rb").read())
    o = bam_header_bytes(raw)
    cut = set(int(i) for i in cut_before)
    with open(dst, "wb") as fh:
        for k in range(0, o, header_block):
            fh.write(bgzf_block(raw[k:min(k + header_block, o)]))
        blk, i, n_out = bytearray(), 0, 0
        def flush():
            nonlocal blk, n_out
            fh.write(bgzf_block(bytes(blk), 0 if n_out < stored_blocks else 6))
            blk = bytearray(); n_out += 1
        if cut_bytes:
            for k in range(o, len(raw), cut_bytes):
                blk = bytearray(raw[k:k + cut_bytes])
                flush()
            o = len(raw)
        while o < len(raw):
            n = 4 + struct.unpack_from("<i", raw, o)[0]
            if blk and (len(blk) + n > block_bytes or i in cut):
                flush()
            blk += raw[o:o + n]
            o += n; i += 1
        if blk:
            flush()
        fh.write(bgzf_block(b""))


# ---- call plans over a layout's blocks ---------------------------------------------------------------------------------------------
def plan_every(n_blocks, k):
    """k blocks per call"""
    return [(b, min(b + k, n_blocks)) for b in range(0, n_blocks, k)]


def plan_cuts(n_blocks, cuts):
    c = sorted(set(int(x) for x in cuts if 0 < int(x) < n_blocks))
    return list(zip([0] + c, c + [n_blocks]))


def plan_random(n_blocks, seed, n_cuts=9):
    rng = np.random.default_rng(seed)
    return plan_cuts(n_blocks, rng.choice(np.arange(1, n_blocks), size=min(n_cuts, n_blocks - 1), replace=False))


def plan_with_empty_call(plan, at):
    """the plan with a call of zero blocks before its call number `at`"""
    b = plan[at][0]
    return plan[:at] + [(b, b)] + plan[at:]


def expected_paths(lay, plan, staged):
    """(staged-taken calls, in-line calls) of a plan: with every next chunk announced before the current call each call but the
    first takes the staged copy -- a call of zero bytes cannot be announced (n_bytes = 0 withdraws) and copies nothing in line"""
    if not staged:
        return 0, len(plan)
    taken = sum(1 for k, (b0, b1) in enumerate(plan) if k > 0 and b1 > b0)
    return taken, len(plan) - taken


# ---- the CLI's chunk planner, restated (load_chunks) ---------------------------------------------------------------------------------
def plan_chunks(coff, csize, isize, env=None, blk_beg=0):
    """-> list of dict(b0, b1, nbytes, ubytes): runs of whole blocks, the first at most chunk_first file bytes, every later one at most
    min(chunk, chunk_first * growth^k); a block that is too large alone is still a chunk"""
    env = env or {}
    chunk_first, chunk, growth = 512 * MIB, 2048 * MIB, 64
    def num(name, lo, hi):
        v = env.get(name)
        return int(v) if v is not None and lo <= int(v) <= hi else None
    k = num("METHEOR_DEVICE_CHUNK_MB", 1, 65536)
    if k is not None:
        chunk_first = chunk = k * MIB; growth = 1
    k = num("METHEOR_FIRST_CHUNK_MB", 1, 65536)
    if k is not None:
        chunk_first = k * MIB
    k = num("METHEOR_CHUNK_GROWTH", 1, 64)
    if k is not None:
        growth = k
    coff, csize, isize = [np.asarray(a).astype(np.int64) for a in (coff, csize, isize)]
    out, b0, n = [], blk_beg, len(coff)
    while b0 < n:
        lim = chunk_first
        for _ in range(len(out)):
            if lim >= chunk:
                break
            lim = min(chunk, lim * growth)
        b1 = b0
        while b1 < n and (b1 == b0 or coff[b1] + csize[b1] - coff[b0] <= lim):
            b1 += 1
        out.append(dict(b0=b0, b1=b1, nbytes=int(coff[b1 - 1] + csize[b1 - 1] + 8 - coff[b0]), ubytes=int(isize[b0:b1].sum()), lim=lim))
        b0 = b1
    return out


def chunk_paths(chunks, hbytes, env=None, piece_mb=0):
    """what the CLI's per-chunk lines must say for a whole-file plan: per chunk "header only" (not loaded), "staged", "pieced" or
    "in line", and the piece launches are left to piece_plan"""
    env = env or {}
    stage = "METHEOR_NO_STAGE" not in env
    out, left, prev_loaded = [], hbytes, False
    for ci, c in enumerate(chunks):
        if left > c["ubytes"] and ci + 1 < len(chunks):
            out.append("header only"); left -= c["ubytes"]; prev_loaded = False
            continue
        left -= min(left, c["ubytes"])
        if stage and prev_loaded:
            out.append("staged")
        elif is_pieced(c["nbytes"], c["b1"] - c["b0"], piece_mb * MIB):
            out.append("pieced")
        else:
            out.append("in line")
        prev_loaded = True
    return out


# ---- the pieced copy's rule, restated (inflate_blocks under METHEOR_COPY_PIECE_MB) -------------------------------------------------
def is_pieced(n_bytes, n_blocks, piece=MIB):
    return bool(piece) and n_bytes >= 2 * piece and n_blocks >= 2


def piece_plan(n_bytes, coff, csize, piece=MIB):
    """-> (piece lengths, [(first block, end block) of every k_inflate launch]): pieces of `piece` bytes, a rest shorter than half a
    piece joins the piece before it (no stub piece), and after each piece the blocks whose payload plus 64 bytes have arrived are
    launched -- all that are left after the last piece"""
    off, bl, pieces, launches, nb = 0, 0, [], [], len(coff)
    while off < n_bytes:
        ln = min(piece, n_bytes - off)
        if n_bytes - off - ln < piece // 2:
            ln = n_bytes - off
        off += ln
        pieces.append(ln)
        last = off == n_bytes
        b1 = bl
        while b1 < nb and (last or int(coff[b1]) + int(csize[b1]) + 64 <= off):
            b1 += 1
        if b1 > bl:
            launches.append((bl, b1))
        bl = b1
    return pieces, launches


def mixed_blocks(seed, min_file_bytes):
    """the random mixed blocks of test_gpu_inflate.py::test_random_mixed_blocks (every block its own size, content model, zlib level
    and strategy, arbitrary payload alignment), as many as it takes to pass min_file_bytes -> (file bytes, coff, csize, isize, payloads)"""
    rng = np.random.default_rng(seed)
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED]
    out, coff, csize, isize, want = bytearray(), [], [], [], []
    while len(out) < min_file_bytes:
        n = int(rng.choice([1, 2, 3, 17, 255, 256, 257, 258, 259, 4096, 65279, 65280])) if rng.random() < 0.3 else int(rng.integers(1, 65281))
        kind = int(rng.integers(0, 7))
        if kind == 0:
            c = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        elif kind == 1:
            c = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=n, p=[0.3, 0.2, 0.2, 0.29, 0.01]).tobytes()
        elif kind == 2:
            parts, have = [], 0
            while have < n:
                parts.append(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 700))); have += len(parts[-1])
            c = b"".join(parts)[:n]
        elif kind == 3:
            base = rng.integers(0, 256, size=int(rng.integers(1, 40000)), dtype=np.uint8).tobytes()
            c = (base * (n // len(base) + 1))[:n]
        elif kind == 4:
            p = 0.5 ** np.arange(1, 41); p /= p.sum()
            c = rng.choice(np.arange(40, dtype=np.uint8), size=n, p=p).tobytes()
        elif kind == 5:
            c = ((b"XM:Z:" + b"." * 40 + b"z..Z" + b"\0" + bytes(rng.integers(33, 74, size=30, dtype=np.uint8))) * (n // 80 + 1))[:n]
        else:
            c = bytes(n)
        co = zlib.compressobj(int(rng.choice([0, 1, 4, 6, 9])), zlib.DEFLATED, -15, int(rng.integers(1, 10)), int(rng.choice(strategies)))
        z = co.compress(c) + co.flush()
        coff.append(len(out)); csize.append(len(z)); isize.append(len(c)); want.append(c)
        out += z + struct.pack("<II", zlib.crc32(c) & 0xffffffff, len(c)) + bytes(int(rng.integers(0, 5)))
    return bytes(out), np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32), want


def placed_blocks(seed, n_bytes, ends):
    """a table of stored-or-deflated random blocks whose payloads END at the given file offsets (ascending, far enough apart), random
    filler in between and up to n_bytes: the launch rule's edges put where a test wants them"""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, size=n_bytes, dtype=np.uint8).tobytes())
    coff, csize, isize, want = [], [], [], []
    for k, end in enumerate(ends):
        c = rng.integers(0, 64, size=int(rng.integers(2000, 30000)), dtype=np.uint8).tobytes()
        co = zlib.compressobj(6 if k % 2 else 1, zlib.DEFLATED, -15)
        z = co.compress(c) + co.flush()
        at = end - len(z)
        assert at >= (coff[-1] + csize[-1] + 8 if coff else 0) and end + 8 <= n_bytes
        out[at:end + 8] = z + struct.pack("<II", zlib.crc32(c) & 0xffffffff, len(c))
        coff.append(at); csize.append(len(z)); isize.append(len(c)); want.append(c)
    return bytes(out), np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32), want


def pieced_tables():
    """name -> (file bytes, coff, csize, isize, payloads) of the pieced-copy cases, the same in the test and in its child process"""
    return {
        # 2 MiB and a little: two pieces, the second one the merged rest
        "mixed-2M": mixed_blocks(7100, 2 * MIB + 40_000),
        # 1 + 1 + 1 + 0.6 MiB: four pieces, nothing merged
        "mixed-3.6M": mixed_blocks(7101, 3 * MIB + 600_000),
        # a payload + 64 that ends exactly with piece 1 (<=, not <), alone in its piece; then blocks in pieces 2 and 3
        "edge-equal": placed_blocks(7102, 3 * MIB, [MIB - 64, MIB + 500_000, 2 * MIB + 300_000, 3 * MIB - 100]),
        # a payload that ends 10 bytes before piece 2 does (its 64 bytes of slack have not arrived), alone in that piece
        "edge-slack": placed_blocks(7103, 3 * MIB, [400_000, 2 * MIB - 10, 2 * MIB + 700_000]),
    }


# ---- the BAM files -----------------------------------------------------------------------------------------------------------------
def one_contig(path):
    """20 000 reads in about 130 blocks, as test_gpu_inflate.py::test_block_aligned_synthetic_bam_whole_path writes them"""
    from metheor_amd import hostapi, synth
    hostapi.write_synthetic_bam(path, synth.make_contig(0, 120_000, 20_000, 0.03, np.random.default_rng(5)), seed=3, threads=3)
    return path


THREE_NAMES = ["cA", "cB", "cC"]


def three_contigs(d):
    """three contigs of 3 000 / 4 000 / 2 500 reads, a block boundary at every contig change, the header in a block of its own
    -> (path, index of every contig's first record)"""
    from metheor_amd import hostapi, synth
    rng = np.random.default_rng(41)
    cs = [synth.make_contig(t, ln, n, 0.03, rng) for t, (ln, n) in enumerate(((60_000, 3000), (90_000, 4000), (50_000, 2500)))]
    tmp, p = os.path.join(d, "three_raw.bam"), os.path.join(d, "three.bam")
    hostapi.write_synthetic_bam_multi(tmp, cs, THREE_NAMES, seed=4, threads=2)
    firsts = [0, 3000, 7000]
    relayout(tmp, p, cut_before=firsts)
    return p, firsts


def low_yield_first(d):
    """a first contig of 6 000 reads without a single call (all-dot XM), then 6 000 dense ones: the first chunk's calls per byte say
    nothing about the rest -> (path, index of the second contig's first record)"""
    from metheor_amd import hostapi, synth
    rng = np.random.default_rng(42)
    a = synth.make_contig(0, 100_000, 6000, 0.03, rng)
    a = dict(a, cpg_off=np.zeros(len(a["read_start"]) + 1, a["cpg_off"].dtype), cpg_pos=a["cpg_pos"][:0], cpg_rel=a["cpg_rel"][:0])
    b = synth.make_contig(1, 100_000, 6000, 0.08, rng)
    tmp, p = os.path.join(d, "yield_raw.bam"), os.path.join(d, "yield.bam")
    hostapi.write_synthetic_bam_multi(tmp, [a, b], ["quiet", "dense"], seed=5, threads=2)
    relayout(tmp, p, cut_before=[6000])
    return p, 6000


def cli_reserve(total_u, done_u, n_reads, n_cpgs):
    """what load_chunks reserves after its first chunk"""
    f = 1.03 * float(total_u) / float(done_u)
    return int(float(n_reads) * f) + 4096, int(float(n_cpgs) * f) + 4096


def swapped_pair(d):
    """one contig of 4 000 reads with records 1999 and 2000 swapped (2000 starts later than 1999 did: the file is out of order
    there) and a block boundary right after the pair's first record -> (path, block index the second record opens)"""
    from metheor_amd import hostapi, synth
    c = synth.make_contig(0, 80_000, 4000, 0.03, np.random.default_rng(43))
    tmp, p = os.path.join(d, "swap_raw.bam"), os.path.join(d, "swap.bam")
    hostapi.write_synthetic_bam(tmp, c, seed=6, threads=2)
    raw = gzip.decompress(open(tmp, "rb").read())
    o, offs = bam_header_bytes(raw), []
    while o < len(raw):
        offs.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    offs.append(len(raw))
    i = 1999
    while struct.unpack_from("<i", raw, offs[i] + 8)[0] == struct.unpack_from("<i", raw, offs[i + 1] + 8)[0]:
        i += 1                                   # the two must start at different positions
    sw = raw[:offs[i]] + raw[offs[i + 1]:offs[i + 2]] + raw[offs[i]:offs[i + 1]] + raw[offs[i + 2]:]
    mid = os.path.join(d, "swap_mid.bam")
    with open(mid, "wb") as fh:
        for k in range(0, len(sw), 60000):
            fh.write(bgzf_block(sw[k:k + 60000]))
        fh.write(bgzf_block(b""))
    relayout(mid, p, cut_before=[i + 1])
    return p, i


def shuffled_runs(src, dst, k=250, seed=45):
    """the records of src in runs of k, the runs in a random order (a file that is not coordinate-sorted), whole records per block"""
    raw = gzip.decompress(open(src, "rb").read())
    h = bam_header_bytes(raw)
    o, offs = h, []
    while o < len(raw):
        offs.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    offs.append(len(raw))
    runs = [(offs[i], offs[min(i + k, len(offs) - 1)]) for i in range(0, len(offs) - 1, k)]
    order = np.random.default_rng(seed).permutation(len(runs))
    sw = raw[:h] + b"".join(raw[runs[j][0]:runs[j][1]] for j in order)
    mid = dst + ".mid"
    with open(mid, "wb") as fh:
        for j in range(0, len(sw), 60000):
            fh.write(bgzf_block(sw[j:j + 60000]))
        fh.write(bgzf_block(b""))
    relayout(mid, dst)
    os.remove(mid)
    return dst


def in_order(soa):
    """no read starts before its predecessor on the same contig (bit 2 of mth_decoded_contigs' flags is the negation)"""
    t, s = soa["tid"], soa["start"]
    return not bool(((t[1:] == t[:-1]) & (s[1:] >= 0) & (s[:-1] >= 0) & (s[1:] < s[:-1])).any())


# ---- the CLI's files -----------------------------------------------------------------------------------------------------------------
CLI_READS = 17_500        # the smallest count (in steps of 500) at which METHEOR_DEVICE_CHUNK_MB=1 makes four chunks: test_chunked_load_inputs.py


def cli_contig():
    from metheor_amd import synth
    return synth.make_contig(0, 400_000, CLI_READS, 0.03, np.random.default_rng(44))


def cli_bam(path, n_reads=None):
    from metheor_amd import hostapi, synth
    c = cli_contig() if n_reads is None else synth.make_contig(0, 400_000, n_reads, 0.03, np.random.default_rng(44))
    hostapi.write_synthetic_bam(path, c, contig="chrL", seed=7, threads=2)
    return c


CLI_SETTINGS = {       # name -> (environment, what the chunk lines must show)
    "default": {},
    "chunk1": {"METHEOR_DEVICE_CHUNK_MB": "1"},
    "chunk1-nostage": {"METHEOR_DEVICE_CHUNK_MB": "1", "METHEOR_NO_STAGE": "1"},
    "first1": {"METHEOR_FIRST_CHUNK_MB": "1"},
    "first1-growth2": {"METHEOR_FIRST_CHUNK_MB": "1", "METHEOR_CHUNK_GROWTH": "2"},
    "chunk3-pieced": {"METHEOR_DEVICE_CHUNK_MB": "3", "METHEOR_NO_STAGE": "1", "METHEOR_COPY_PIECE_MB": "1"},
}


def huge_header_records(n_contigs, seed):
    """n_contigs @SQ lines with 60-character random names (they do not compress), 1 500 reads on each of three of the contigs"""
    from metheor_amd import synth
    from oracle import bamio
    from tests import util
    rng = np.random.default_rng(seed)
    abc = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-", np.uint8)
    names = [bytes(r).decode() for r in abc[rng.integers(0, 64, size=(n_contigs, 60))]]
    refs = [(n, 50_000) for n in names]
    tid, pos, flag, mapq, cig, xms = [], [], [], [], [], []
    for t in (3, n_contigs // 2, n_contigs - 1):
        r = util.contig_to_records(synth.make_contig(t, 50_000, 1500, 0.04, rng), names[t])
        tid += [t] * len(r); pos += r.pos.tolist(); flag += r.flag.tolist(); mapq += r.mapq.tolist(); cig += r.cigars; xms += r.xms
    return bamio.Records(refs, tid, pos, flag, mapq, cig, xms)


# (contigs, stored record blocks): found on the CPU, pinned by test_chunked_load_inputs.py
HUGE = {"a": (13_000, 0), "b": (10_800, 2), "c": (24_000, 0), "b-cut": (10_800, 2)}     # b-cut: b with the record stream cut every 60 000 bytes


def huge_header_bam(d, case, n_contigs=None, header_block=0xff00):
    """-> (path, records) of case a (the header ends inside chunk 1 of METHEOR_DEVICE_CHUNK_MB=1: chunk 0 is header only), b (the header
    ends with chunk 0's last byte: the first record blocks are stored and too large to join) or c (the header covers two whole chunks)"""
    from oracle import bamio
    n, stored = HUGE[case]
    rec = huge_header_records(n_contigs or n, 50 + ord(case[0]))
    tmp, p = os.path.join(d, "huge_%s_raw.bam" % case), os.path.join(d, "huge_%s.bam" % case)
    bamio.write_bam(tmp, rec)
    relayout(tmp, p, stored_blocks=stored, header_block=header_block, cut_bytes=60000 if case == "b-cut" else 0)
    os.remove(tmp)
    return p, rec
