#!/usr/bin/env python3
"""Times `metheor pdr-regions` on the benchmark's S-chr19-10M shape and writes profiles/pdr_regions.md.

The three interval sets of profiles/mhl_regions.md on the same batch / BAM:
  1 kbp tiling                      the windows partition the contig
  5 kbp / 500 bp step               ten windows over every position
  1 kbp tiling + whole chromosome   one interval every read adds to, among the windows
Device time through the library with the launches timed (event-bracketed, best of runs + 1): the read x interval pass (k_pdr_regions)
in its default form and with the span route switched off (MTH_PDR_REGIONS_SPAN=0, a context of its own: the knob is read once per
context), and in the same run, on the same batch, k_mhl_regions over the same sets -- the same (read, interval) pairs -- and the
per-CpG PDR pass of mth_pdr_lpmd_accumulate.  Whole command lines (page cache, median of the runs after a warm-up round) against
`metheor pdr` and `metheor mhl-regions`.

    python tools/bench_pdr_regions.py [--reads 10000000] [--runs 5] [--out profiles/pdr_regions.md]
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


def arrays(iv):
    return np.zeros(len(iv), np.int32), np.array([x[0] for x in iv], np.int32), np.array([x[1] for x in iv], np.int32)


def time_regions(eng, bt, iv, runs, which):
    """best of runs + 1 of one launch of k_<which>_regions over the intervals, and the sums it leaves"""
    begin, acc, fetch = (getattr(eng, "%s_regions_%s" % (which, f)) for f in ("begin", "accumulate", "fetch"))
    best = None
    for _ in range(runs + 1):
        begin(*arrays(iv))
        eng.timing_reset()
        eng.timing_enable(True)
        acc(bt)
        eng.sync()                                      # (the PDR pass is queued, not waited for)
        eng.timing_enable(False)
        t = eng.timing()["k_%s_regions" % which]
        assert t[1] == 1
        best = t[0] if best is None or t[0] < best else best
    return best, fetch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdr_regions.md"))
    ap.add_argument("--no-cli", action="store_true", help="device times only")
    a = ap.parse_args()
    import metheor_amd
    from metheor_amd import batches, build, capi, hostapi, synth
    build.build()
    exe = os.path.join(ROOT, "metheor_amd", "metheor")
    c = synth.chr19_10m(n_reads=a.reads)
    length = c["length"]
    tiling = [(b, min(b + 1000, length)) for b in range(0, length, 1000)]
    sets = {"1 kbp tiling": tiling,
            "5 kbp / 500 bp step": [(b, min(b + 5000, length)) for b in range(0, length, 500)],
            "1 kbp tiling + whole chromosome": tiling + [(0, length)]}

    # device time: the launches bracketed by events
    os.environ.pop("MTH_PDR_REGIONS_SPAN", None)
    os.environ.pop("MTH_PDR_REGIONS_LDS_CAP", None)
    eng = metheor_amd.Engine(0)
    bt = batches.device_batch(c, device="cuda:0")
    names, pdr_best, n_sites = None, None, 0
    for _ in range(a.runs + 1):
        eng.reset()
        eng.timing_reset()
        eng.timing_enable(True)
        eng.pdr_lpmd_accumulate(bt, capi.PdrLpmdParams())
        n_sites = eng.pdr_count()
        eng.timing_enable(False)
        t = eng.timing()
        names = sorted(k for k, v in t.items() if v[1])
        cur = sum(t[k][0] * t[k][1] for k in names)
        pdr_best = cur if pdr_best is None or cur < pdr_best else pdr_best
    dev = {}
    for name, iv in sets.items():
        ms, got = time_regions(eng, bt, iv, a.runs, "pdr")
        ms_mhl, got_mhl = time_regions(eng, bt, iv, a.runs, "mhl")
        dev[name] = dict(n=len(iv), pdr=ms, mhl=ms_mhl, got=got, pairs=int(got["n_concordant"].sum() + got["n_discordant"].sum()),
                         pairs_mhl=int(got_mhl["n_reads"].sum()), fin=int(np.isfinite(got["pdr"]).sum()))
    eng.close()
    os.environ["MTH_PDR_REGIONS_SPAN"] = "0"
    eng = metheor_amd.Engine(0)
    for name, iv in sets.items():
        ms, got = time_regions(eng, bt, iv, a.runs, "pdr")
        dev[name]["off"] = ms
        same = all((got[k] == dev[name]["got"][k]).all() for k in ("n_concordant", "n_discordant", "n_methylated"))
        assert same, "the two forms disagree on " + name
    eng.close()
    del os.environ["MTH_PDR_REGIONS_SPAN"]

    rows, res, cli = [], {}, []
    if not a.no_cli:
        d = tempfile.mkdtemp(prefix="pdr_regions_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        bam = os.path.join(d, "chr19.bam")
        hostapi.write_synthetic_bam(bam, c, contig="chr19", seed=7)
        o = os.path.join(d, "o.tsv")
        cli = [("pdr", ["pdr", "-i", bam, "-o", o])]
        for k, (name, iv) in enumerate(sets.items()):
            bed = os.path.join(d, "iv%d.bed" % k)
            with open(bed, "w") as f:
                f.write("".join("chr19\t%d\t%d\n" % x for x in iv))
            cli.append(("pdr-regions, " + name, ["pdr-regions", "-i", bam, "-o", o, "--intervals", bed]))
            cli.append(("mhl-regions, " + name, ["mhl-regions", "-i", bam, "-o", o, "--intervals", bed]))
        res = timed_cli(exe, cli, a.runs)
        rows = [(name, statistics.median(res[name][0]), res[name][0][0], res[name][0][-1]) for name, _ in cli]
        shutil.rmtree(d, ignore_errors=True)

    with open(a.out, "w") as f:
        f.write("# `metheor pdr-regions`: what the read x interval pass costs\n\n")
        f.write("Input: S-chr19-10M as `bench.py` builds it (`synth.chr19_10m(n_reads=%d)`, %d bp, %d reads, %d calls).\n\n"
                % (a.reads, length, len(c["read_start"]), len(c["cpg_pos"])))
        f.write("Produced by `python tools/bench_pdr_regions.py --reads %d --runs %d` on one MI355X.\n\n" % (a.reads, a.runs))
        f.write("## Device time (event-bracketed launches through the library, best of %d)\n\n" % (a.runs + 1))
        f.write("Measured in the same run, on the same batch: the per-CpG PDR pass (`mth_pdr_lpmd_accumulate`: %s) takes **%.3f ms** for %d "
                "sites; `k_mhl_regions` runs over the same interval sets, that is over the same (read, interval) pairs.\n\n"
                % (" + ".join("`%s`" % k for k in names), pdr_best, n_sites))
        f.write("| interval set | intervals | k_pdr_regions ms | span route off ms | off / default | k_mhl_regions ms | pdr / mhl | / per-CpG PDR pass | "
                "sum of contributing reads | (MHL's) | intervals with a value |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for name, v in dev.items():
            f.write("| %s | %d | %.3f | %.3f | %.2f | %.3f | %.2f | %.2f | %d | %d | %d |\n"
                    % (name, v["n"], v["pdr"], v["off"], v["off"] / v["pdr"], v["mhl"], v["pdr"] / v["mhl"], v["pdr"] / pdr_best, v["pairs"], v["pairs_mhl"], v["fin"]))
        k = list(dev.values())
        f.write("\nThe whole-chromosome interval among the windows costs k_pdr_regions %.2fx the tiling alone (k_mhl_regions in this run: %.2fx; "
                "with the span route off: %.2fx).\n" % (k[2]["pdr"] / k[0]["pdr"], k[2]["mhl"] / k[0]["mhl"], k[2]["off"] / k[0]["off"]))
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
