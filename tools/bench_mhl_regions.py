#!/usr/bin/env python3
"""Times `metheor mhl-regions` on the benchmark's S-chr19-10M shape and writes profiles/mhl_regions.md.

Three interval sets on the same batch / BAM:
  1 kbp tiling                      the windows partition the contig
  5 kbp / 500 bp step               ten windows over every position
  1 kbp tiling + whole chromosome   one interval every read adds to, among the windows
Device time through the library with the launches timed (event-bracketed, best of runs + 1): the read x interval pass
(k_mhl_regions) beside the per-CpG MHL pass of mth_mhl_accumulate on the same batch, measured in the same run.  Whole command lines
(page cache, median of the runs after a warm-up round) against `metheor mhl`.

    python tools/bench_mhl_regions.py [--reads 10000000] [--runs 5] [--out profiles/mhl_regions.md]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_lpmd_intervals import timed_cli  # noqa: E402

MHL_KERNELS = ("k_mhl_tile", "k_mhl_rowcheck", "k_mhl_walk", "k_mhl_walk_big", "k_mhl_emit", "k_build_index")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mhl_regions.md"))
    ap.add_argument("--no-cli", action="store_true", help="device times only")
    a = ap.parse_args()
    import metheor_amd
    from metheor_amd import batches, build, hostapi, synth
    build.build()
    exe = os.path.join(ROOT, "metheor_amd", "metheor")
    c = synth.chr19_10m(n_reads=a.reads)
    length = c["length"]
    tiling = [(b, min(b + 1000, length)) for b in range(0, length, 1000)]
    sets = {"1 kbp tiling": tiling,
            "5 kbp / 500 bp step": [(b, min(b + 5000, length)) for b in range(0, length, 500)],
            "1 kbp tiling + whole chromosome": tiling + [(0, length)]}

    # device time: the launches bracketed by events
    eng = metheor_amd.Engine(0)
    bt = batches.device_batch(c, device="cuda:0")
    names = None
    mhl_best = None
    for _ in range(a.runs + 1):
        eng.reset()
        eng.timing_reset()
        eng.timing_enable(True)
        eng.mhl_accumulate(bt)
        n_sites = len(eng.mhl_fetch()["pos"])
        eng.timing_enable(False)
        t = eng.timing()
        names = sorted(k for k, v in t.items() if v[1] and k != "k_mhl_regions")
        cur = sum(t[k][0] * t[k][1] for k in names)
        mhl_best = cur if mhl_best is None or cur < mhl_best else mhl_best
    dev = []
    for name, iv in sets.items():
        t_ = np.zeros(len(iv), np.int32)
        b_, e_ = np.array([x[0] for x in iv], np.int32), np.array([x[1] for x in iv], np.int32)
        best, got = None, None
        for _ in range(a.runs + 1):
            eng.mhl_regions_begin(t_, b_, e_)
            eng.timing_reset()
            eng.timing_enable(True)
            eng.mhl_regions_accumulate(bt)
            eng.timing_enable(False)
            t = eng.timing()["k_mhl_regions"]
            cur = t[0] * t[1]
            best = cur if best is None or cur < best else best
        got = eng.mhl_regions_fetch()
        st = eng.mhl_regions_stats()
        dev.append((name, len(iv), best, int(got["n_reads"].sum()), int(np.isfinite(got["mhl"]).sum()), st[0]))
    eng.close()

    rows, res, cli = [], {}, []
    if not a.no_cli:
        d = tempfile.mkdtemp(prefix="mhl_regions_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        bam = os.path.join(d, "chr19.bam")
        hostapi.write_synthetic_bam(bam, c, contig="chr19", seed=7)
        o = os.path.join(d, "o.tsv")
        cli = [("mhl", ["mhl", "-i", bam, "-o", o])]
        for k, (name, iv) in enumerate(sets.items()):
            bed = os.path.join(d, "iv%d.bed" % k)
            with open(bed, "w") as f:
                f.write("".join("chr19\t%d\t%d\n" % x for x in iv))
            cli.append(("mhl-regions, " + name, ["mhl-regions", "-i", bam, "-o", o, "--intervals", bed]))
        res = timed_cli(exe, cli, a.runs)
        rows = [(name, statistics.median(res[name][0]), res[name][0][0], res[name][0][-1]) for name, _ in cli]
        shutil.rmtree(d, ignore_errors=True)

    with open(a.out, "w") as f:
        f.write("# `metheor mhl-regions`: what the read x interval pass costs\n\n")
        f.write("Input: S-chr19-10M as `bench.py` builds it (`synth.chr19_10m(n_reads=%d)`, %d bp, %d reads, %d calls).\n\n"
                % (a.reads, length, len(c["read_start"]), len(c["cpg_pos"])))
        f.write("Produced by `python tools/bench_mhl_regions.py --reads %d --runs %d` on one MI355X.\n\n" % (a.reads, a.runs))
        f.write("## Device time (event-bracketed launches through the library, best of %d)\n\n" % (a.runs + 1))
        f.write("The yardstick, measured in the same run: the per-CpG MHL pass (`mth_mhl_accumulate`: %s) on the same batch takes "
                "**%.3f ms** for %d sites.\n\n" % (" + ".join("`%s`" % k for k in names), mhl_best, n_sites))
        f.write("| interval set | intervals | k_mhl_regions ms | / per-CpG pass | sum n_reads | intervals with a value | overflow entries |\n|---|---|---|---|---|---|---|\n")
        for name, n, ms, nr, fin, ovf in dev:
            f.write("| %s | %d | %.3f | %.2f | %d | %d | %d |\n" % (name, n, ms, ms / mhl_best if mhl_best else float("nan"), nr, fin, ovf))
        base, hot = dev[0][2], dev[2][2]
        f.write("\nThe whole-chromosome interval among the windows costs %.2fx the tiling alone (the bound of the issue: 2x).\n" % (hot / base if base else float("nan")))
        if rows:
            f.write("\n## Whole command lines (wall time of the process; %d rounds after a warm-up round, the commands taking turns, BAM in the page cache)\n\n" % a.runs)
            f.write("| command | median s | min s | max s |\n|---|---|---|---|\n")
            for name, med, lo, hi in rows:
                f.write("| `metheor %s` | %.3f | %.3f | %.3f |\n" % (name, med, lo, hi))
            f.write("\nPhases of each command's last run, seconds (`METHEOR_TIMING=1`):\n\n")
            for name, _ in cli:
                f.write("* `metheor %s`: %s\n" % (name, ", ".join("%s %.4f" % kv for kv in res[name][1].items())))
    print(open(a.out).read())


if __name__ == "__main__":
    main()
