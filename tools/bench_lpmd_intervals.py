#!/usr/bin/env python3
"""Times `lpmd --intervals` on the benchmark's S-chr19-10M shape and writes profiles/lpmd_intervals.md.

Three command lines on the same BAM (page cache, median of the runs after one warm-up):
  lpmd --pairs                      as before the option existed: the pairs table fetched and written
  lpmd --intervals  1 kbp tiling    the table reduced on the device, never fetched
  lpmd --intervals  5 kbp / 500 bp  ten windows over every position
and, through the library with the launches timed, the device time of the pairs pass (k_pairs_tile + k_pairs) and of the interval
reduction (k_pairs_intervals) for both interval sets.

    python tools/bench_lpmd_intervals.py [--reads 10000000] [--runs 4] [--out profiles/lpmd_intervals.md]
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def phases(stderr):
    out = {}
    for l in stderr.splitlines():
        if l.startswith("[metheor timing]") and l.rstrip().endswith(" s"):
            name, sec = l[len("[metheor timing]"):].rstrip()[:-2].rsplit(None, 1)
            out[name.strip()] = float(sec)
    return out


def timed_cli(exe, cmds, runs):
    """the command lines in turn, `runs` rounds after a warm-up round (the machine is shared: a difference between two of them counts
    only against their spread) -> {name: (sorted wall times, phases of the last run)}"""
    out = {name: ([], {}) for name, _ in cmds}
    for k in range(runs + 1):
        for name, args in cmds:
            t0 = time.perf_counter()
            r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, METHEOR_TIMING="1"), timeout=600)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit("metheor failed: " + r.stderr[-400:])
            if k:
                out[name][0].append(dt)
                out[name][1].update(phases(r.stderr))
    return {name: (sorted(w), ph) for name, (w, ph) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpmd_intervals.md"))
    a = ap.parse_args()
    import metheor_amd
    from metheor_amd import batches, build, hostapi, synth
    build.build()
    exe = os.path.join(ROOT, "metheor_amd", "metheor")
    c = synth.chr19_10m(n_reads=a.reads)
    length = c["length"]
    sets = {"1 kbp tiling": [(b, min(b + 1000, length)) for b in range(0, length, 1000)],
            "5 kbp / 500 bp step": [(b, min(b + 5000, length)) for b in range(0, length, 500)]}
    d = tempfile.mkdtemp(prefix="lpmd_iv_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    bam = os.path.join(d, "chr19.bam")
    hostapi.write_synthetic_bam(bam, c, contig="chr19", seed=7)
    beds = {}
    for k, (name, iv) in enumerate(sets.items()):
        beds[name] = os.path.join(d, "iv%d.bed" % k)
        with open(beds[name], "w") as f:
            f.write("".join("chr19\t%d\t%d\n" % x for x in iv))
    o, p, ivo = (os.path.join(d, x) for x in ("o.tsv", "pairs.tsv", "iv.tsv"))
    cli = [("lpmd (no table)", ["lpmd", "-i", bam, "-o", o]),
           ("lpmd --pairs", ["lpmd", "-i", bam, "-o", o, "--pairs", p])]
    for name in sets:
        cli.append(("lpmd --intervals, " + name, ["lpmd", "-i", bam, "-o", o, "--intervals", beds[name], "--intervals-output", ivo]))
    res = timed_cli(exe, cli, a.runs)
    rows = [(name, statistics.median(res[name][0]), res[name][0][0], res[name][0][-1], res[name][1].get("intervals BED (header + parse)"),
             res[name][1].get("interval reduction (kernel, sync)")) for name, _ in cli]
    n_pairs = sum(1 for _ in open(p)) - 1

    # device time: the launches bracketed by events (queueing is off while they are timed: one sync per batch)
    eng = metheor_amd.Engine(0)
    bt = batches.device_batch(c, device="cuda:0")
    dev = []
    for name, iv in sets.items():
        t_ = np.zeros(len(iv), np.int32)
        b_, e_ = np.array([x[0] for x in iv], np.int32), np.array([x[1] for x in iv], np.int32)
        best = None
        for _ in range(a.runs + 1):
            eng.reset()
            eng.timing_reset()
            eng.timing_enable(True)
            eng.lpmd_pairs_accumulate(bt)
            got = eng.lpmd_intervals_fetch(t_, b_, e_)
            eng.timing_enable(False)
            t = eng.timing()
            cur = (t["k_pairs_tile"][0] + t["k_pairs"][0], t["k_pairs_intervals"][0])
            best = cur if best is None or sum(cur) < sum(best) else best
        dev.append((name, len(iv), best[0], best[1], int(got["n_concordant"].sum()), int(got["n_discordant"].sum())))
    eng.close()

    with open(a.out, "w") as f:
        f.write("# `lpmd --intervals`: what the per-interval reduction costs\n\n")
        f.write("Input: S-chr19-10M as `bench.py` builds it (`synth.chr19_10m(n_reads=%d)`, %d bp, written with "
                "`hostapi.write_synthetic_bam(..., seed=7)`), BAM in the page cache.  The pairs table of this input has %d rows.\n\n"
                % (a.reads, length, n_pairs))
        f.write("Produced by `python tools/bench_lpmd_intervals.py --reads %d --runs %d` on one MI355X.\n\n" % (a.reads, a.runs))
        f.write("## Whole command lines (wall time of the process; %d rounds after a warm-up round, the commands taking turns)\n\n" % a.runs)
        f.write("| command | median s | min s | max s | BED phase s | `interval reduction` phase s |\n|---|---|---|---|---|---|\n")
        for name, med, lo, hi, bed, red in rows:
            f.write("| `metheor %s` | %.3f | %.3f | %.3f | %s | %s |\n" % (name, med, lo, hi, "-" if bed is None else "%.4f" % bed, "-" if red is None else "%.4f" % red))
        f.write("\nThe BED phase is reading the intervals against the input's header before anything else starts.  The reduction phase is `mth_lpmd_intervals_fetch` as the command line sees it (`METHEOR_TIMING=1`): the host-side sort of the "
                "intervals, the upload, the kernel, the read-back and the call's one synchronisation -- which also waits for the pairs pass "
                "queued in front of it.\n\n")
        f.write("Phases of each command's last run, seconds (`METHEOR_TIMING=1`; nested phases are listed beside their parents):\n\n")
        for name, _ in cli:
            f.write("* `metheor %s`: %s\n" % (name, ", ".join("%s %.4f" % kv for kv in res[name][1].items())))
        f.write("\n## Device time (event-bracketed launches through the library, best of %d)\n\n" % (a.runs + 1))
        f.write("| interval set | intervals | pairs pass ms (k_pairs_tile + k_pairs) | reduction ms (k_pairs_intervals) | reduction / pairs pass | "
                "sum n_concordant | sum n_discordant |\n|---|---|---|---|---|---|---|\n")
        for name, n, pairs_ms, red_ms, sc, sd in dev:
            f.write("| %s | %d | %.3f | %.3f | %.2f | %d | %d |\n" % (name, n, pairs_ms, red_ms, red_ms / pairs_ms if pairs_ms else float("nan"), sc, sd))
        f.write("\n(The tiling windows partition the contig: their sums are the table's pairs that do not straddle a window edge.  The "
                "5 kbp windows hold every pair ten times, less the edges.)\n")
    shutil.rmtree(d, ignore_errors=True)
    print(open(a.out).read())


if __name__ == "__main__":
    main()
