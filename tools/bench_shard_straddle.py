"""`metheor pdr --gpus 2` on a BAM whose records straddle BGZF blocks (METHEOR_SHARD_STRADDLE=1: every shard scans its run, the
chain is verified, every shard loads its plan -- the inflate is paid twice) against the single-GPU run of the same file on the
default route and against `--gpus 2` on the block-aligned file.  Whole-process wall times, five runs each, alternating, after one
warm-up run.  The input is tools/bench_straddle.py's: one synthetic file and its copy re-cut every 65 280 bytes.

Usage (GPU box): python tools/bench_shard_straddle.py [reads] [reps] [gpus]"""
import gzip, json, multiprocessing, os, re, shutil, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_straddle import CUT, bgzf_block


def main():
    from metheor_amd import hostapi, synth
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_500_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    gpus = sys.argv[3] if len(sys.argv) > 3 else "2"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "metheor_amd", "metheor")
    d = "/dev/shm/bench_shard_straddle"
    os.makedirs(d, exist_ok=True)
    aligned, cut = os.path.join(d, "aligned.bam"), os.path.join(d, "cut.bam")
    print("box: %s x %d, ROCm %s, %d CPUs usable by this process" % (torch.cuda.get_device_name(0), torch.cuda.device_count(), torch.version.hip,
                                                                     len(os.sched_getaffinity(0))), flush=True)
    t0 = time.perf_counter()
    c = synth.make_contig(0, 40 * n, n, 0.02, np.random.default_rng(21))
    hostapi.write_synthetic_bam(aligned, c, seed=4, threads=16)
    raw = gzip.decompress(open(aligned, "rb").read())
    with multiprocessing.Pool(16) as pool, open(cut, "wb") as fh:
        for blk in pool.imap(bgzf_block, (raw[o:o + CUT] for o in range(0, len(raw), CUT)), chunksize=64):
            fh.write(blk)
        fh.write(bgzf_block(b""))
    print("input: %d reads, %d MB inflated; aligned BAM %d MB, re-cut every %d bytes %d MB in %d blocks (made in %.0f s)"
          % (n, len(raw) >> 20, os.path.getsize(aligned) >> 20, CUT, os.path.getsize(cut) >> 20, (len(raw) + CUT - 1) // CUT, time.perf_counter() - t0), flush=True)
    del raw

    routes = {"a": ("(a) straddling copy, --gpus %s, METHEOR_SHARD_STRADDLE=1" % gpus, cut, ["--gpus", gpus], {"METHEOR_SHARD_STRADDLE": "1"}),
              "b": ("(b) straddling copy, one GPU, default route (host inflate, 16 threads)", cut, [], {}),
              "c": ("(c) aligned file, --gpus %s" % gpus, aligned, ["--gpus", gpus], {})}

    def timed(k):
        _, bam, more, env = routes[k]
        cmd = [exe, "pdr", "-i", bam, "-o", os.path.join(d, k + ".tsv"), *more]
        t = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, METHEOR_TIMING="1", METHEOR_THREADS="16", **env))
        dt = time.perf_counter() - t
        assert r.returncode == 0, r.stderr[-2000:]
        return dt, r.stderr, " ".join(["%s=%s" % kv for kv in sorted(env.items())] + ["METHEOR_THREADS=16", "metheor", *cmd[1:]])

    timed("c")                                                      # warm-up: page cache, code objects
    ts, err, cmds = {k: [] for k in routes}, {}, {}
    for _ in range(reps):
        for k in routes:
            dt, err[k], cmds[k] = timed(k)
            ts[k].append(dt)
    assert err["a"].count("straddle walk") == int(gpus) and "  inflate + device record decode" not in err["a"]
    assert "  inflate + device record decode" in err["b"] and "straddle walk" not in err["c"]
    same = open(os.path.join(d, "a.tsv"), "rb").read() == open(os.path.join(d, "b.tsv"), "rb").read() == open(os.path.join(d, "c.tsv"), "rb").read()
    for k in routes:
        print("%-76s median %.3f s  best %.3f s  runs: %s\n    %s" % (routes[k][0], statistics.median(ts[k]), min(ts[k]), " ".join("%.3f" % t for t in ts[k]), cmds[k]), flush=True)
    print("outputs byte-identical: %s (%d rows)" % (same, sum(1 for _ in open(os.path.join(d, "a.tsv"), "rb"))))
    print("phases of the last (a) run:\n" + "\n".join(l for l in err["a"].splitlines() if "timing" in l or "straddle" in l), flush=True)
    scan = re.search(r"shard scan: (\d+) runs, (\d+) scanned again, (\d+) rounds", err["a"])
    print(json.dumps({"reads": n, "gpus": int(gpus), "devices": torch.cuda.device_count(), "median_s": {k: round(statistics.median(ts[k]), 4) for k in routes},
                      "best_s": {k: round(min(ts[k]), 4) for k in routes}, "identical": same, "scan": [int(x) for x in scan.groups()] if scan else None}))
    shutil.rmtree(d)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
