"""`metheor pdr` on a BAM whose records straddle BGZF blocks: today's route (host inflate + device record decode) against the device
straddle walk (METHEOR_DEVICE_STRADDLE=1, mth_bgzf_decode_straddle), with the block-aligned file on the device route as the floor.
Whole-process wall times, five runs each, alternating; then the straddle walk's rounds and kernel times from one library call.

One synthetic file (hostapi.write_synthetic_bam: whole records per block, as htslib writes) and its copy re-cut every 65 280 bytes
(zlib level 1, at most 16 workers) as htsjdk-family writers cut.  The host route runs with METHEOR_THREADS=16: what a command on a
shared box gets.

Usage (GPU box): python tools/bench_straddle.py [reads] [reps] [--keep DIR]"""
import gzip, json, multiprocessing, os, shutil, statistics, struct, subprocess, sys, time, zlib
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUT = 65280


def bgzf_block(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25)
    return hdr + comp + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def block_table(path):
    """-> (file bytes, coff, csize, isize of the blocks with data)"""
    fb = open(path, "rb").read()
    o, coff, csize, isize = 0, [], [], []
    while o < len(fb):
        xlen, = struct.unpack_from("<H", fb, o + 10)
        total = struct.unpack_from("<H", fb, o + 16)[0] + 1          # the BC subfield comes first in every block written here
        isz, = struct.unpack_from("<I", fb, o + total - 4)
        if isz:
            coff.append(o + 12 + xlen); csize.append(total - 12 - xlen - 8); isize.append(isz)
        o += total
    return fb, np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32)


def header_bytes(raw):
    l_text, = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, o)
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return o


def main():
    from metheor_amd import Engine, hostapi, synth
    argv = list(sys.argv[1:])
    keep = None
    if "--keep" in argv:
        i = argv.index("--keep"); keep = argv[i + 1]; del argv[i:i + 2]
    n = int(argv[0]) if len(argv) > 0 else 1_500_000
    reps = int(argv[1]) if len(argv) > 1 else 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "metheor_amd", "metheor")
    d = keep or "/dev/shm/bench_straddle"
    os.makedirs(d, exist_ok=True)
    aligned, cut = os.path.join(d, "aligned.bam"), os.path.join(d, "cut.bam")

    import torch
    print("box: %s, ROCm %s, %d CPUs usable by this process" % (torch.cuda.get_device_name(0), torch.version.hip, len(os.sched_getaffinity(0))), flush=True)
    t0 = time.perf_counter()
    c = synth.make_contig(0, 40 * n, n, 0.02, np.random.default_rng(21))
    hostapi.write_synthetic_bam(aligned, c, seed=4, threads=16)
    raw = gzip.decompress(open(aligned, "rb").read())
    hbytes = header_bytes(raw)
    with multiprocessing.Pool(16) as pool, open(cut, "wb") as fh:
        for blk in pool.imap(bgzf_block, (raw[o:o + CUT] for o in range(0, len(raw), CUT)), chunksize=64):
            fh.write(blk)
        fh.write(bgzf_block(b""))
    n_blocks = (len(raw) + CUT - 1) // CUT
    print("input: %d reads, %d MB inflated; aligned BAM %d MB, re-cut every %d bytes %d MB in %d blocks (made in %.0f s)"
          % (n, len(raw) >> 20, os.path.getsize(aligned) >> 20, CUT, os.path.getsize(cut) >> 20, n_blocks, time.perf_counter() - t0), flush=True)
    del raw

    def timed(bam, out, env):
        t = time.perf_counter()
        r = subprocess.run([exe, "pdr", "-i", bam, "-o", out], capture_output=True, text=True,
                           env=dict(os.environ, METHEOR_TIMING="1", METHEOR_THREADS="16", **env))
        dt = time.perf_counter() - t
        assert r.returncode == 0, r.stderr[-2000:]
        return dt, r.stderr

    outs = {k: os.path.join(d, k + ".tsv") for k in "abc"}
    ts, err = {k: [] for k in "abc"}, {}
    timed(aligned, outs["c"], {})                                   # warm-up: page cache, code objects
    for _ in range(reps):
        for k, bam, env in (("a", cut, {}), ("b", cut, {"METHEOR_DEVICE_STRADDLE": "1"}), ("c", aligned, {})):
            dt, err[k] = timed(bam, outs[k], env)
            ts[k].append(dt)
    assert "  inflate + device record decode" in err["a"] and "straddle walk" not in err["a"]
    assert "straddle walk" in err["b"] and "  inflate + device record decode" not in err["b"]
    assert "  device inflate + walk + decode" in err["c"] and "  inflate + device record decode" not in err["c"]
    same = open(outs["a"], "rb").read() == open(outs["b"], "rb").read() == open(outs["c"], "rb").read()
    names = {"a": "(a) straddling copy, host inflate + device record decode (16 host threads)",
             "b": "(b) straddling copy, METHEOR_DEVICE_STRADDLE=1", "c": "(c) aligned file, device route (floor)"}
    for k in "abc":
        print("%-78s median %.3f s  best %.3f s  runs: %s" % (names[k], statistics.median(ts[k]), min(ts[k]), " ".join("%.3f" % t for t in ts[k])), flush=True)
    print("outputs byte-identical: %s (%d rows)" % (same, sum(1 for _ in open(outs["a"], "rb"))))
    for k in "ab":
        print("phases of the last %s run:\n" % k + "\n".join(l for l in err[k].splitlines() if "timing" in l), flush=True)

    # the walk itself: one library call over the whole file, every launch bracketed by events
    fb, coff, csize, isize = block_table(cut)
    eng = Engine(0)
    eng.bgzf_decode_straddle(fb, coff, csize, isize, hbytes, last=True)          # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    nr, _, info = eng.bgzf_decode_straddle(fb, coff, csize, isize, hbytes, last=True)
    tm = eng.timing()
    eng.close()
    kern = {k: {"avg_ms": round(tm[k][0], 4), "launches": int(tm[k][1])} for k in ("k_straddle_guess", "k_straddle_walk", "k_straddle_repair", "k_inflate", "k_crc32", "k_decode")}
    print("library call: %d records, info %s" % (nr, info))
    for k, v in kern.items():
        print("  %-18s %8.4f ms avg over %d launches" % (k, v["avg_ms"], v["launches"]))
    print(json.dumps({"reads": n, "blocks": n_blocks, "median_s": {k: round(statistics.median(ts[k]), 4) for k in "abc"},
                      "best_s": {k: round(min(ts[k]), 4) for k in "abc"}, "identical": same, "info": info, "kernels": kern}))
    if not keep:
        shutil.rmtree(d)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
