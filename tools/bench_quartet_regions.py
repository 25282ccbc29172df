#!/usr/bin/env python3
"""Times `metheor me-regions` on the benchmark's S-chr19-10M shape and writes profiles/quartet_regions.md.

The three interval sets of profiles/pdr_regions.md on the same batch / BAM:
  1 kbp tiling                      the windows partition the contig
  5 kbp / 500 bp step               ten windows over every position
  1 kbp tiling + whole chromosome   one interval every read adds to, among the windows
Device time through the library with the launches timed (event-bracketed, best of runs + 1): the read x interval pass
(k_quartet_regions) in four forms, each in a context of its own since the knobs are read once per context -- default, packed summary
off (MTH_QUARTET_REGIONS_SUMMARY=0), carried row off (MTH_QUARTET_REGIONS_CARRY=0), LDS cap 0 (MTH_QUARTET_REGIONS_LDS_CAP=0: every
add goes to memory) -- and in the same run, on the same batch, k_pdr_regions and k_mhl_regions over the same sets and the per-quartet
ME / PM pass of mth_quartet_accumulate.  Whole command lines (page cache, median of the runs after a warm-up round, with their
spread) against `metheor me`.

    python tools/bench_quartet_regions.py [--reads 10000000] [--runs 5] [--out profiles/quartet_regions.md] [--no-build] [--no-cli]
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
from bench_pdr_regions import arrays, time_regions  # noqa: E402

KNOBS = ("MTH_QUARTET_REGIONS_LDS_CAP", "MTH_QUARTET_REGIONS_SUMMARY", "MTH_QUARTET_REGIONS_CARRY")
FORMS = [("default", {}), ("summary off", {"MTH_QUARTET_REGIONS_SUMMARY": "0"}), ("carried row off", {"MTH_QUARTET_REGIONS_CARRY": "0"}),
         ("cap 0", {"MTH_QUARTET_REGIONS_LDS_CAP": "0"})]


def time_quartet_regions(eng, bt, iv, runs):
    """best of runs + 1 of one launch of k_quartet_regions over the intervals, and the counts it leaves"""
    best = None
    for _ in range(runs + 1):
        eng.quartet_regions_begin(*arrays(iv))
        eng.timing_reset()
        eng.timing_enable(True)
        eng.quartet_regions_accumulate(bt)
        eng.sync()                                      # (the pass is queued, not waited for)
        eng.timing_enable(False)
        t = eng.timing()["k_quartet_regions"]
        assert t[1] == 1
        best = t[0] if best is None or t[0] < best else best
    return best, eng.quartet_regions_counts(), eng.quartet_regions_fetch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartet_regions.md"))
    ap.add_argument("--no-cli", action="store_true", help="device times only")
    ap.add_argument("--no-build", action="store_true", help="take the binaries as they are")
    a = ap.parse_args()
    import metheor_amd
    from metheor_amd import batches, build, hostapi, synth
    if not a.no_build:
        build.build()
    exe = os.path.join(ROOT, "metheor_amd", "metheor")
    c = synth.chr19_10m(n_reads=a.reads)
    length = c["length"]
    tiling = [(b, min(b + 1000, length)) for b in range(0, length, 1000)]
    sets = {"1 kbp tiling": tiling,
            "5 kbp / 500 bp step": [(b, min(b + 5000, length)) for b in range(0, length, 500)],
            "1 kbp tiling + whole chromosome": tiling + [(0, length)]}

    for k in KNOBS:
        os.environ.pop(k, None)
    bt = batches.device_batch(c, device="cuda:0")
    dev = {name: dict(n=len(iv)) for name, iv in sets.items()}
    quartet_best, quartet_names, n_quartets = None, None, 0
    for form, env in FORMS:
        os.environ.update(env)
        eng = metheor_amd.Engine(0)
        for name, iv in sets.items():
            ms, counts, got = time_quartet_regions(eng, bt, iv, a.runs)
            v = dev[name]
            v[form] = ms
            if form == "default":
                v["counts"] = counts
                v["patterns"], v["reads"], v["fin"] = int(got["n_patterns"].sum()), int(got["n_reads"].sum()), int(np.isfinite(got["me"]).sum())
            else:
                assert (counts["bins"] == v["counts"]["bins"]).all() and (counts["reads"] == v["counts"]["reads"]).all(), "the forms disagree on " + name
        if form == "default":           # the baselines, in the same context: the other two read x interval passes and the per-quartet pass
            for name, iv in sets.items():
                dev[name]["pdr"], _ = time_regions(eng, bt, iv, a.runs, "pdr")
                dev[name]["mhl"], _ = time_regions(eng, bt, iv, a.runs, "mhl")
            for _ in range(a.runs + 1):
                eng.reset()
                eng.timing_reset()
                eng.timing_enable(True)
                eng.quartet_accumulate(bt)
                eng.sync()
                n_quartets = len(eng.quartet_fetch(min_depth=0)["tid"])
                eng.timing_enable(False)
                t = eng.timing()
                quartet_names = sorted(k for k, x in t.items() if x[1])
                cur = sum(t[k][0] * t[k][1] for k in quartet_names)
                quartet_best = cur if quartet_best is None or cur < quartet_best else quartet_best
        eng.close()
        for k in env:
            del os.environ[k]

    rows, res, cli = [], {}, []
    if not a.no_cli:
        d = tempfile.mkdtemp(prefix="quartet_regions_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        bam = os.path.join(d, "chr19.bam")
        hostapi.write_synthetic_bam(bam, c, contig="chr19", seed=7)
        o = os.path.join(d, "o.tsv")
        cli = [("me", ["me", "-i", bam, "-o", o])]
        for k, (name, iv) in enumerate(sets.items()):
            bed = os.path.join(d, "iv%d.bed" % k)
            with open(bed, "w") as f:
                f.write("".join("chr19\t%d\t%d\n" % x for x in iv))
            cli.append(("me-regions, " + name, ["me-regions", "-i", bam, "-o", o, "--intervals", bed]))
        cli.append(("pdr-regions, 1 kbp tiling", ["pdr-regions", "-i", bam, "-o", o, "--intervals", os.path.join(d, "iv0.bed")]))
        res = timed_cli(exe, cli, a.runs)
        rows = [(name, statistics.median(res[name][0]), res[name][0][0], res[name][0][-1]) for name, _ in cli]
        shutil.rmtree(d, ignore_errors=True)

    with open(a.out, "w") as f:
        f.write("# `metheor me-regions` / `pm-regions`: what the read x interval pass costs\n\n")
        f.write("Input: S-chr19-10M as `bench.py` builds it (`synth.chr19_10m(n_reads=%d)`, %d bp, %d reads, %d calls).\n\n"
                % (a.reads, length, len(c["read_start"]), len(c["cpg_pos"])))
        f.write("Produced by `python tools/bench_quartet_regions.py --reads %d --runs %d` on one MI355X.\n\n" % (a.reads, a.runs))
        f.write("## Device time (event-bracketed launches through the library, best of %d)\n\n" % (a.runs + 1))
        f.write("Measured in the same run, on the same batch: the per-quartet ME / PM pass (`mth_quartet_accumulate`: %s) takes **%.3f ms** for %d "
                "quartets; `k_pdr_regions` and `k_mhl_regions` run over the same interval sets.  Every form of `k_quartet_regions` left the same "
                "counts (checked).\n\n" % (" + ".join("`%s`" % k for k in quartet_names), quartet_best, n_quartets))
        f.write("| interval set | intervals | k_quartet_regions ms | summary off ms | carried row off ms | cap 0 ms | k_pdr_regions ms | k_mhl_regions ms | "
                "/ pdr | / mhl | / per-quartet pass | patterns | contributing reads | intervals with a value |\n" + "|---" * 14 + "|\n")
        for name, v in dev.items():
            f.write("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f | %.2f | %d | %d | %d |\n"
                    % (name, v["n"], v["default"], v["summary off"], v["carried row off"], v["cap 0"], v["pdr"], v["mhl"], v["default"] / v["pdr"],
                       v["default"] / v["mhl"], v["default"] / quartet_best, v["patterns"], v["reads"], v["fin"]))
        k = list(dev.values())
        f.write("\nThe whole-chromosome interval among the windows costs k_quartet_regions %.2fx the tiling alone (carried row off: %.2fx; "
                "k_pdr_regions in this run: %.2fx, k_mhl_regions: %.2fx).\n"
                % (k[2]["default"] / k[0]["default"], k[2]["carried row off"] / k[0]["carried row off"], k[2]["pdr"] / k[0]["pdr"], k[2]["mhl"] / k[0]["mhl"]))
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
