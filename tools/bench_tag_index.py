"""`metheor tag -O bam --write-index` against `tag -O bam`, end to end, on the input of tools/bench_tag_bam.py (generated reads
without XM tags as a BAM file, and the FASTA they came from): whole-process wall time of
    index   this tree's `tag -O bam --write-index`
    bam     this tree's `tag -O bam`
    parent  another build's `tag -O bam` (--parent-exe: the `metheor` of the commit before; left out when not given)
all on the same input, writing to /dev/shm.  One warm-up round, then --reps rounds (default 5) with the configurations interleaved
inside every round; the median and the min-max spread of each are printed, whether the flag changes the BAM's bytes, then the
kernel times of one more `--write-index` run under METHEOR_TIMING=1 and the size of the index.
Usage (GPU box): python tools/bench_tag_index.py [--reads N] [--reps R] [--parent-exe PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metheor_amd import hostapi      # noqa: E402
from tests import tag_util           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--parent-exe", default=None)
ap.add_argument("--timeout", type=float, default=120.0, help="seconds a single run may take")
args = ap.parse_args()

n = args.reads
rng = np.random.default_rng(11)
L = 5_000_000
contig = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
fa = "/dev/shm/bench_tag_index.fa"
tag_util.write_fasta(fa, "chrT", contig.tobytes())
starts = np.sort(rng.integers(0, L - 150, size=n))
sam = "/dev/shm/bench_tag_index.sam"
with open(sam, "w") as fh:          # (the records of tools/bench_tag_bam.py)
    fh.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrT\tLN:%d\n" % L)
    q = "I" * 150
    for i, s in enumerate(starts):
        seq = contig[s:s + 150].copy()
        conv = rng.random(150) < 0.7
        if i & 1:
            seq[(seq == ord("G")) & conv] = ord("A"); flag = 16
        else:
            seq[(seq == ord("C")) & conv] = ord("T"); flag = 0
        fh.write("r%d\t%d\tchrT\t%d\t40\t150M\t*\t0\t0\t%s\t%s\tNM:i:0\n" % (i, flag, s + 1, seq.tobytes().decode(), q))
bam = "/dev/shm/bench_tag_index.in.bam"
f = hostapi.BamFile(sam)
open(bam, "wb").write(open(f.staged_path(), "rb").read())
del f
os.remove(sam)

exe = os.path.join(ROOT, "metheor_amd", "metheor")
configs = [("index", exe, ["-O", "bam", "--write-index"], "/dev/shm/bench_tag_index.ix.bam"), ("bam", exe, ["-O", "bam"], "/dev/shm/bench_tag_index.out.bam")]
if args.parent_exe:
    configs.append(("parent", args.parent_exe, ["-O", "bam"], "/dev/shm/bench_tag_index.parent.bam"))


def one(exe_, extra, out, timing=False):
    env = dict(os.environ)
    env.pop("METHEOR_TIMING", None)
    if timing:
        env["METHEOR_TIMING"] = "1"
    t0 = time.perf_counter()
    r = subprocess.run([exe_, "tag", "-i", bam, "-o", out, "-g", fa] + extra, capture_output=True, text=True, env=env, timeout=args.timeout)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("a run failed (status %d), nothing more is started: %s" % (r.returncode, r.stderr[-2000:]))
    return dt, r.stderr


times = {name: [] for name, _, _, _ in configs}
for rep in range(args.reps + 1):
    for name, exe_, extra, out in configs:
        dt, _ = one(exe_, extra, out)
        if rep:                      # round 0 warms the page cache and the device up
            times[name].append(dt)
res = {"reads": n, "reps": args.reps, "input_bytes": os.path.getsize(bam)}
for name, _, _, out in configs:
    t = times[name]
    med = statistics.median(t)
    res[name] = {"median_s": round(med, 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "output_bytes": os.path.getsize(out),
                 "runs_s": [round(x, 4) for x in t]}
    print("%-6s median %.3f s (min %.3f, max %.3f), output %.1f MB" % (name, med, min(t), max(t), os.path.getsize(out) / 1e6))
print("the flag adds %.1f ms to the median" % (1e3 * (res["index"]["median_s"] - res["bam"]["median_s"])))
same = open(configs[0][3], "rb").read() == open(configs[1][3], "rb").read()
print("the BAM's bytes with the flag equal those without: %s" % same)
res["bam_equal"] = same
if "parent" in res:
    lo, hi = res["parent"]["min_s"], res["parent"]["max_s"]
    m = res["bam"]["median_s"]
    print("no flag vs parent: median %.3f s against the parent's spread [%.3f, %.3f] s -> %s" % (m, lo, hi, "within" if lo <= m <= hi else ("faster" if m < lo else "SLOWER")))
    res["bam_equals_parent"] = open(configs[1][3], "rb").read() == open(configs[2][3], "rb").read()
    print("no flag: the BAM's bytes equal the parent's: %s" % res["bam_equals_parent"])

_, err = one(exe, ["-O", "bam", "--write-index"], configs[0][3], timing=True)
print("\n".join(x for x in err.splitlines() if "timing" in x and ("tag/" in x or "index" in x or "records" in x)))
res["timing"] = [x.strip() for x in err.splitlines() if "timing" in x]
res["index_bytes"] = os.path.getsize(configs[0][3] + ".bai")
print("index: %d bytes" % res["index_bytes"])
print(json.dumps(res))
for path in [fa, fa + ".fai", bam, configs[0][3] + ".bai"] + [c[3] for c in configs]:
    if os.path.exists(path):
        os.remove(path)
