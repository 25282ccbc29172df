"""`metheor tag --output-format bam` against the SAM route, end to end, on the input of tools/bench_tag.py (generated reads without
XM tags as a BAM file, and the FASTA they came from): whole-process wall time of
    bam     this tree's `tag -O bam`
    sam     this tree's `tag` (SAM text, the default)
    parent  another build's `tag` (--parent-exe: the `metheor` of the commit before; left out when not given)
all on the same input, writing to /dev/shm.  One warm-up round, then --reps rounds (default 5) with the configurations interleaved
inside every round, so that drift of the machine hits all of them alike; the median, the min-max spread and reads/s of each are
printed, then the phase and kernel times of one more `-O bam` run under METHEOR_TIMING=1 (k_tag_assemble, k_crc32, k_deflate,
k_bgzf_compact and the copy of the finished blocks back to the host, summed over the windows), and the compressed size against
zlib level 1 over the same blocks.
Usage (GPU box): python tools/bench_tag_bam.py [--reads N] [--reps R] [--parent-exe PATH]"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib

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
fa = "/dev/shm/bench_tag_bam.fa"
tag_util.write_fasta(fa, "chrT", contig.tobytes())
starts = np.sort(rng.integers(0, L - 150, size=n))
sam = "/dev/shm/bench_tag_bam.sam"
with open(sam, "w") as fh:          # (the records of tools/bench_tag.py)
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
bam = "/dev/shm/bench_tag_bam.in.bam"
f = hostapi.BamFile(sam)
open(bam, "wb").write(open(f.staged_path(), "rb").read())
del f
os.remove(sam)

exe = os.path.join(ROOT, "metheor_amd", "metheor")
configs = [("bam", exe, ["-O", "bam"], "/dev/shm/bench_tag_bam.out.bam"), ("sam", exe, [], "/dev/shm/bench_tag_bam.out.sam")]
if args.parent_exe:
    configs.append(("parent", args.parent_exe, [], "/dev/shm/bench_tag_bam.parent.sam"))


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
    res[name] = {"median_s": round(med, 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "reads_per_s": round(n / med),
                 "output_bytes": os.path.getsize(out), "runs_s": [round(x, 4) for x in t]}
    print("%-6s median %.3f s (min %.3f, max %.3f) = %.2f M reads/s, output %.1f MB" % (name, med, min(t), max(t), n / med / 1e6, os.path.getsize(out) / 1e6))
if "parent" in res:
    lo, hi = res["parent"]["min_s"], res["parent"]["max_s"]
    print("sam route vs parent: median %.3f s against the parent's spread [%.3f, %.3f] s -> %s" %
          (res["sam"]["median_s"], lo, hi, "within" if lo <= res["sam"]["median_s"] <= hi else ("faster" if res["sam"]["median_s"] < lo else "SLOWER")))
    print("bam route vs parent: %.2fx the parent's reads/s" % (res["parent"]["median_s"] / res["bam"]["median_s"]))
    same = open(configs[1][3], "rb").read() == open(configs[2][3], "rb").read()
    print("sam route's bytes equal the parent's: %s" % same)
    res["sam_equals_parent"] = same

_, err = one(exe, ["-O", "bam"], configs[0][3], timing=True)
print("\n".join(x for x in err.splitlines() if "timing" in x))
res["timing"] = [x.strip() for x in err.splitlines() if "timing" in x]

# the record blocks' DEFLATE payloads against zlib level 1 over the same uncompressed blocks (whole blocks inflate with zlib: a check)
data = open(configs[0][3], "rb").read()
p, dev, z1, raw_total, forms = 0, 0, 0, 0, [0, 0, 0]
while p < len(data):
    size = struct.unpack_from("<H", data, p + 16)[0] + 1
    payload = data[p + 18:p + size - 8]
    raw = zlib.decompress(payload, -15)
    assert zlib.crc32(raw) == struct.unpack_from("<I", data, p + size - 8)[0]
    if raw and raw[:4] != b"BAM\x01":
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        dev += len(payload); z1 += len(z.compress(raw) + z.flush()); raw_total += len(raw)
        forms[(payload[0] >> 1) & 3] += 1
    p += size
print("record blocks: %d uncompressed bytes -> %d payload bytes on the device, %d with zlib level 1: ratio %.4f; blocks stored / fixed / dynamic: %s"
      % (raw_total, dev, z1, dev / z1, forms))
res["deflate"] = {"raw_bytes": raw_total, "device_payload_bytes": dev, "zlib1_payload_bytes": z1, "ratio": round(dev / z1, 4), "forms": forms}
print(json.dumps(res))
for path in [fa, fa + ".fai", bam] + [c[3] for c in configs]:
    if os.path.exists(path):
        os.remove(path)
