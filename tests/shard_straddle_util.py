"""Inputs, run cuts and a CPU model for the multi-GPU route over BAMs whose records straddle BGZF blocks (mth_bgzf_straddle_scan,
mth_host_plan_shard_straddle; tests/test_shard_straddle_inputs.py checks these on the CPU, tests/test_gpu_shard_straddle.py runs
them).  The small inputs of tests/straddle_util.py, with the first record padded by a few bytes so that a chosen block boundary
falls where a case needs it:
  (a) a run end inside a block_size field          (b) a block end inside the first 12 bytes of a record, inside a run
  (c) a run that starts exactly at a record start  (d) a run wholly inside one giant record
  (e) a run whose first block guesses wrong (the guess rule restated for a stream that starts at that block)
plus, on a file of the synthetic generator cut every 65 280 bytes (make_lookalike):
  (f) a run whose first block guesses a look-alike 4 bytes before a record start, whose block_size leads megabytes on INSIDE the stream
and the file's record table as the chain verification must leave it, from the true record offsets."""
import os
import struct

import numpy as np

from tests import straddle_util as S

CASES = "abcde"
N_RUNS = (2, 5, 9)
LOOKAHEAD = 36                                   # MTH_STRADDLE_LOOKAHEAD
NO_START, EXIT_BAD = 0xffffffff, (1 << 64) - 1
ROW = np.dtype([("start", np.uint32), ("ref_id", np.int32), ("pos", np.int32), ("pad_", np.uint32), ("exit", np.uint64)])
GIANT_BYTES = {60000: 150_000, 4093: 20_000, 700: 4_000}       # a few blocks each: a scan pays a round per block a record covers
OFFSET_IN_RECORD = dict(a=2, b=8, c=0, e=20)     # where in a record the chosen block boundary falls ((e): before the decoys, which lie in the aux)


def _records(case):
    if case == "e":
        return S.add_decoys(S.irregular(), 40)
    rec = S.irregular()
    rec.aux_extra = [(b"NMC\0", b"XRZCT\0")] * len(rec)
    return rec


def _pad_first(rec, n):
    """n >= 8 more bytes in record 0 (a ZP:B:C array of zeros in front of its other tags): every later record starts n bytes later"""
    assert n >= 8
    pre, post = rec.aux_extra[0]
    rec.aux_extra = [(b"ZPBC" + struct.pack("<i", n - 8) + bytes(n - 8) + pre, post)] + list(rec.aux_extra[1:])
    return rec


def make(d, case, cut):
    """the file of a case at a cut size -> (records, Layout, the block a run edge goes to (None for (b)), the block that holds the case)"""
    path = os.path.join(d, "shard_%s_%d.bam" % (case, cut))
    if case == "d":
        rec = S.add_giants(S.irregular(), 500, n_bytes=GIANT_BYTES[cut])
        lay = S.Layout(S.write_cut(path, rec, cut, realistic=True))
        b = S.block_inside_one_record(lay)
        return rec, lay, b, b
    rec = _records(case)
    lay = S.Layout(S.write_cut(path, rec, cut, realistic=True))
    # the record a boundary is moved into: the first past the middle of the stream (for (e): one that carries decoys)
    k = int(np.searchsorted(lay.starts, lay.total // 2))
    if case == "e":
        k += (-k) % 40
    want = int(lay.starts[k]) + OFFSET_IN_RECORD[case]
    bound = lay.b1[lay.b1 >= want + 8]
    rec = _pad_first(_records(case), int(bound[0]) - want)
    lay = S.Layout(S.write_cut(path, rec, cut, realistic=True))
    blk = int(np.searchsorted(lay.b0, int(lay.starts[k]) + OFFSET_IN_RECORD[case]))      # the block that begins at the boundary
    return rec, lay, (None if case == "b" else blk), blk


def holds(lay, case, blk):
    """does block `blk` hold the case?  ((a): the run END is blk's first byte; (c), (e): the run STARTS with blk)"""
    x = int(lay.b0[blk])
    k = int(np.searchsorted(lay.starts, x, side="right")) - 1          # the last record that starts at or before x
    into = x - int(lay.starts[k]) if k >= 0 else -1
    if case == "a":
        return 1 <= into <= 3
    if case == "b":
        return 4 <= into <= 11
    if case == "c":
        return into == 0
    if case == "d":
        return S.block_inside_one_record(lay) == blk
    g = guess_from(lay, blk, len(lay.b0))
    if case == "f":                     # the guess is no record start, and its block_size leads past the next block, inside the stream
        to = g + 4 + struct.unpack_from("<i", lay.raw, g)[0] if g >= 0 else -1
        return g >= 0 and g not in lay.starts and lay.b1[blk + 1] <= to < lay.total
    return g >= 0 and g != lay.first_start_in()[blk]          # (a guess in a block without a start is a wrong one too)


LOOKALIKE_CUT = 65280


def make_lookalike(d):
    """16 000 reads of the synthetic generator (hostapi.write_synthetic_bam), re-cut every 65 280 bytes: the file of profiles/
    straddle_walk.md in small.  A record there ends in XR:Z:CT\\0, whose last four bytes read as a block_size of 5 522 266, and the
    fields behind pass the guess rule -> (Layout, the first block whose guess, for a stream from that block to the file's end, is
    such a look-alike and leads to an offset inside that stream)"""
    from metheor_amd import hostapi, synth
    import gzip
    n = 16_000
    ali, cut = os.path.join(d, "lookalike_aligned.bam"), os.path.join(d, "lookalike.bam")
    hostapi.write_synthetic_bam(ali, synth.make_contig(0, 40 * n, n, 0.02, np.random.default_rng(21)), seed=4, threads=4)
    raw = gzip.decompress(open(ali, "rb").read())
    with open(cut, "wb") as fh:
        from oracle import bamio
        for o in range(0, len(raw), LOOKALIKE_CUT):
            fh.write(bamio._bgzf_block(raw[o:o + LOOKALIKE_CUT]))
        fh.write(bamio._bgzf_block(b""))
    lay = S.Layout(cut)
    first = lay.first_start_in()
    for b in range(max(N_RUNS) - 1, len(lay.b0) - 2):        # (room for the other runs in front of it: lookalike_edges)
        if guess_from(lay, b, len(lay.b0)) == first[b] - 4 and holds(lay, "f", b):
            return lay, b
    return lay, None


def lookalike_edges(n_runs, blk):
    """case (f): the run that starts at blk is the LAST one, so its stream reaches the file's end whatever n_runs is -- a look-alike
    is a guess only while the offset its block_size leads to lies inside the stream; the other n_runs - 1 runs share the blocks in
    front of blk"""
    out = [k * blk // (n_runs - 1) for k in range(n_runs - 1)] + [blk]
    assert len(set(out)) == n_runs
    return out


def _good(raw):
    """per offset: passes the guess rule and leads to another offset that passes, or exactly to the end of raw"""
    ok, nxt = S.plausible_all(raw)
    follow = nxt == len(raw)
    idx = np.nonzero(ok & (nxt < len(ok)))[0]
    follow[idx] = ok[nxt[idx]]
    return ok & follow


def guess_from(lay, blk, ahead_end):
    """Layout.guesses() for block blk of a stream that starts at blk and ends with block ahead_end - 1 (a later block's guess can
    depend on where the stream ends; the first block's only if a record of it leads to that very end)"""
    lo, hi = int(lay.b0[blk]), int(lay.b1[ahead_end - 1])
    if hi == lay.total:                  # to the file's end: the rule at absolute offsets, worked out once per file
        if not hasattr(lay, "good_to_end"):
            lay.good_to_end = _good(lay.raw)
        w = lay.good_to_end[lo:int(lay.b1[blk])]
    else:
        w = _good(lay.raw[lo:hi])[:int(lay.isize[blk])]
    return lo + int(np.argmax(w)) if w.any() else -1


def edges(lay, n_runs, at=None, avoid=None):
    """first blocks of n_runs runs, about even in blocks, run 0 from block 0; `at`: a block that must be one of them, or a tuple of
    such blocks (case (d): (b, b + 1), the run is that one block); `avoid`: a block that must not be one (case (b): an even cut
    that falls on it moves to the next block).  None when n_runs runs cannot hold them."""
    nb = len(lay.b0)
    must = [] if at is None else sorted(at) if isinstance(at, tuple) else [at]
    if len(must) > n_runs - 1:
        return None
    e = sorted(set(k * nb // n_runs + (1 if k * nb // n_runs == avoid else 0) for k in range(1, n_runs)) - set(must))
    while len(e) + len(must) > n_runs - 1:                # make room: drop the even cuts nearest to the forced ones
        e.remove(min(e, key=lambda x: min(abs(x - m) for m in must)))
    out = [0] + sorted(e + must)
    assert len(out) == n_runs and len(set(out)) == n_runs and 0 < out[1] and out[-1] < nb
    return out


def case_edges(lay, case, edge, blk, n_runs):
    """the run cuts a case is scanned with (make()'s edge and blk)"""
    return edges(lay, n_runs, (edge, edge + 1) if case == "d" else edge, avoid=blk if case == "b" else None)


def ahead_end(lay, run_end):
    """the look-ahead of a run that ends before block run_end: blocks until the stream reaches LOOKAHEAD bytes past it, or the data ends"""
    e, got = run_end, 0
    while e < len(lay.b0) and got < LOOKAHEAD:
        got += int(lay.isize[e])
        e += 1
    return e


def truth_table(lay):
    """the file's record table from the true offsets: per block the first record that starts in it, its refID and pos, and how far
    past the block's end the chain leaves it (the end of the last record that starts before the block's end; the header's end for a
    block of the header)"""
    t = np.zeros(len(lay.b0), ROW)
    first = lay.first_start_in()
    for b in range(len(lay.b0)):
        s, b1 = int(first[b]), int(lay.b1[b])
        t[b]["start"] = s - int(lay.b0[b]) if s >= 0 else NO_START
        t[b]["ref_id"], t[b]["pos"] = struct.unpack_from("<ii", lay.raw, s + 4) if s >= 0 else (-2 ** 31, -2 ** 31)
        k = int(np.searchsorted(lay.starts, b1, side="left")) - 1
        t[b]["exit"] = (int(lay.ends[k]) if k >= 0 else lay.hbytes) - b1
    return t


def same_table(got, want):
    for f in ("start", "exit"):
        assert (got[f] == want[f]).all(), (f, np.nonzero(got[f] != want[f])[0][:5])
    has = want["start"] != NO_START
    assert (got["ref_id"][has] == want["ref_id"][has]).all() and (got["pos"][has] == want["pos"][has]).all()


def run_call(lay, b0, b1):
    """the arguments of Engine.bgzf_straddle_scan for the run of blocks [b0, b1): its file bytes and those of its look-ahead"""
    e = ahead_end(lay, b1)
    lo, hi = int(lay.coff[b0]), int(lay.coff[e - 1] + lay.csize[e - 1]) + 8
    return lay.fb[lo:hi], lay.coff[b0:e] - np.uint64(lo), lay.csize[b0:e], lay.isize[b0:e], b1 - b0


def scan_file(eng, lay, run_edges):
    """the chain verification over one engine: every run but the first is scanned from a guess, then -- the runs before it being
    final -- held against the true entry and scanned again on a mismatch (the engine still holds it); an entry at or past the run's
    end passes on.  -> (table, runs scanned again, [summary of each scan])"""
    table = np.zeros(len(lay.b0), ROW)
    bounds = list(run_edges) + [len(lay.b0)]
    entry, rescans, infos = lay.hbytes, 0, []
    for r, (b0, b1) in enumerate(zip(bounds[:-1], bounds[1:])):
        rows, got = eng.bgzf_straddle_scan(*run_call(lay, b0, b1), entry=entry if r == 0 else None)
        infos.append(got)
        run_len = int(lay.b1[b1 - 1] - lay.b0[b0])
        if entry >= run_len:
            left = entry - np.cumsum(lay.isize[b0:b1].astype(np.int64))
            table[b0:b1]["start"], table[b0:b1]["exit"] = NO_START, left
            entry -= run_len
            continue
        if got["entry"] != entry:
            rows, got = eng.bgzf_straddle_rescan(entry)
            infos.append(got)
            rescans += 1
            assert got["entry"] == entry
        assert got["exit"] is not None, (r, got)
        table[b0:b1] = rows
        entry = got["exit"]
    assert entry == 0
    return table, rescans, infos


def owned(soa, beg, end):
    """indices of the reads of a decoded SoA whose (tid, start) lies in [beg, end); a read without a contig sorts last"""
    tid = np.where(soa["tid"] < 0, 2 ** 31 - 1, soa["tid"]).astype(np.int64)
    key = tid << 32 | (soa["start"].astype(np.int64) & 0xffffffff)
    lo = (beg[0] << 32 | (beg[1] & 0xffffffff)) if beg[0] >= 0 else -1
    return np.nonzero((key >= lo) & (key < (end[0] << 32 | (end[1] & 0xffffffff))))[0]


def soa_take(soa, idx):
    """the reads idx (ascending) of a decoded SoA, as an SoA"""
    off = soa["cpg_off"].astype(np.int64)
    calls = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    out = {k: soa[k][idx] for k in ("tid", "start", "end", "mapq", "fwd")}
    out["cpg_off"] = np.concatenate([[0], np.cumsum(off[idx + 1] - off[idx])]).astype(np.uint64)
    out["cpg_pos"], out["cpg_rel"] = soa["cpg_pos"][calls], soa["cpg_rel"][calls]
    return out


def soa_concat(parts):
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("tid", "start", "end", "mapq", "fwd", "cpg_pos", "cpg_rel")}
    n = np.concatenate([np.diff(p["cpg_off"].astype(np.int64)) for p in parts])
    out["cpg_off"] = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    return out


def genome_files_sorted(d):
    """straddle_util.genome_files with the records in the order of their first aligned base: the generator's records are sorted by
    pos, and a leading D / N moves the first aligned base of some past the next record's -- input that a shard plan refuses as
    unsorted, block-aligned or not (tests/test_gpu_genome.py sorts them the same way for --region and --gpus)
    -> (aligned path, cut path, fasta path)"""
    from metheor_amd import hostapi
    from tests import genome_util as gu
    from tests import tag_util
    from tests.test_gpu_genome import aligned_start
    g = gu.generate(1)
    recs, _ = gu.runnable(g)
    recs = [recs[k] for k in sorted(range(len(recs)), key=lambda k: (aligned_start(recs[k]), k))]
    sam, fa, ali, cut = (os.path.join(d, x) for x in ("gs_in.sam", "gs.fa", "gs_in.bam", "gs_cut.bam"))
    open(sam, "w").write(gu.sam_text([(g["name"], len(g["contig"]))], recs))
    tag_util.write_fasta(fa, g["name"], g["contig"])
    f = hostapi.BamFile(sam)
    open(ali, "wb").write(open(f.staged_path(), "rb").read())
    f.close()
    S.reblock(ali, cut, 4093)
    return ali, cut, fa
