#!/usr/bin/env python3
"""`metheor all` against the single commands, and mth_multi_accumulate against the single entry points.

  cli   -- a synthetic config-2-depth BAM (default 10 M reads): wall time of `metheor all` with all seven outputs against the seven
           single runs back to back, and against one `metheor pdr` run (best of --repeat each; the outputs are compared byte for byte).
  api   -- BASELINE config 3 (24 hg38-sized contigs at WGBS density, --wgbs-reads, device-resident): the seven measures + pairs via the
           single entry points on prepared batches, against mth_multi_accumulate on the same batches in the split and the fused form
           (the only difference between those two: PDR + LPMD and ME / PM as one tile pass); host wall time per job, best of --repeat.
One JSON line per result on stdout.  Usage: python tools/bench_all.py [--reads N] [--wgbs-reads N] [--repeat K] [--skip cli|api]"""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
OUTS = ("pdr", "lpmd", "mhl", "me", "pm", "fdrp", "qfdrp")


def _run(args, env):
    t0 = time.perf_counter()
    r = subprocess.run([EXE, *args], capture_output=True, text=True, env=env, timeout=900)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (" ".join(args), r.returncode, r.stderr[-2000:]))
    return dt


def bench_cli(args):
    from metheor_amd import hostapi, synth
    n = args.reads
    L = int(synth.CHR19_LEN * n / 10_000_000)
    d = args.keep or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    bam = os.path.join(d, "all_%d.bam" % n)
    if not os.path.exists(bam):
        c = synth.make_contig(0, L, n, 0.02, np.random.default_rng(1234))
        hostapi.write_synthetic_bam(bam, c, contig="chr19", seed=1)
    env = dict(os.environ)
    env.setdefault("METHEOR_SEED", "1")
    one = lambda m: os.path.join(d, "one." + m)
    al = lambda m: os.path.join(d, "all." + m)
    t_all, t_seven, t_pdr = [], [], []
    for _ in range(args.repeat):
        t_all.append(_run(["all", "-i", bam] + sum((["--" + m, al(m)] for m in OUTS), []), env))
        ts = {m: _run([m, "-i", bam, "-o", one(m)], env) for m in OUTS}
        t_seven.append(sum(ts.values()))
        t_pdr.append(ts["pdr"])
    same = all(filecmp.cmp(al(m), one(m), shallow=False) for m in OUTS)
    res = {"bench": "cli", "reads": n, "bam_bytes": os.path.getsize(bam), "all_s": round(min(t_all), 3),
           "seven_single_runs_s": round(min(t_seven), 3), "one_pdr_run_s": round(min(t_pdr), 3),
           "all_over_pdr": round(min(t_all) / min(t_pdr), 2), "seven_over_all": round(min(t_seven) / min(t_all), 2),
           "outputs_identical": same}
    print(json.dumps(res), flush=True)


def bench_api(args):
    import torch
    import metheor_amd
    from metheor_amd import PdrLpmdParams, synth_device
    eng = metheor_amd.Engine(0)
    batches = [b for b, _ in synth_device.wgbs(n_reads=args.wgbs_reads)]
    torch.cuda.synchronize()
    prepared = [eng.batch_prepare(b) for b in batches]
    want = ("pdr", "lpmd", "quartet", "mhl", "fdrp", "pairs")

    def singles():
        eng.reset()
        for b in prepared:
            eng.pdr_lpmd_accumulate(b, PdrLpmdParams())
            eng.quartet_accumulate(b)
            eng.mhl_accumulate(b)
            eng.fdrp_accumulate(b)
            eng.lpmd_pairs_accumulate(b)
        eng.sync()

    def multi(form):
        def run():
            eng.reset()
            for b in prepared:
                eng.multi_accumulate(b, want=want, form=form)
            eng.sync()
        return run

    out = {}
    for name, fn in (("single_entry_points", singles), ("multi_split", multi("split")), ("multi_fused", multi("fused"))):
        fn()
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(min(ts) * 1e3, 2)
    st = eng.multi_stats()
    print(json.dumps({"bench": "api", "workload": "config 3: %d reads over %d contigs, every measure + pairs, prepared batches" %
                      (sum(b.n_reads for b in batches), len(batches)), "ms": out, "multi_stats": st}), flush=True)
    for p in prepared:
        p.release()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--wgbs-reads", type=int, default=200_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--keep", default=None, help="directory for the BAM and the outputs (reused)")
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    if "cli" not in args.skip:
        bench_cli(args)
    if "api" not in args.skip:
        bench_api(args)


if __name__ == "__main__":
    main()
