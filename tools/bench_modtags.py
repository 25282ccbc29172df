"""`metheor pdr --mm-tags` in its two kernel forms against the XM route on the equivalent file F' (flag & 0x10, XM:Z:X(record, T);
tests/modtags_util.py writes it), which is the yardstick: code the project had before the mode.  Two generated inputs, 150-bp
records and ~5 kbp records; whole-process wall times in alternating order, and the decode pass alone through mth_timing_get.
Writes the medians and the run-to-run spread as a markdown report.

Usage (GPU box): python tools/bench_modtags.py [--short N] [--long N] [--reps R] [--out profiles/modtags.md]"""
import os, shutil, statistics, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metheor_amd import capi, hostapi
from tests import modtags_util as M

argv = sys.argv[1:]
opt = {"--short": "60000", "--long": "1500", "--reps": "5", "--out": os.path.join("profiles", "modtags.md")}
for k in list(opt):
    if k in argv:
        i = argv.index(k); opt[k] = argv[i + 1]; del argv[i:i + 2]
assert not argv, argv
reps = int(opt["--reps"])
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
exe = os.path.join(root, "metheor_amd", "metheor")
d = tempfile.mkdtemp(prefix="bench_modtags_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
T = 128


def make_input(name, n, length, seed):
    """n records of `length` bases (+- 10 % when long) on one contig: both strands, C+m? lists over ~80 % of the read's Cs, ML random"""
    rng = np.random.default_rng(seed)
    clen = max(4 * length, n * length // 20)                       # depth ~20
    contig = M.make_contig(rng, clen)
    starts = np.sort(rng.integers(0, clen - 2 * length, n))
    recs = []
    for i in range(n):
        L = length if length <= 1000 else int(length * (0.9 + 0.2 * rng.random()))
        seq = contig[int(starts[i]):int(starts[i]) + L]
        rev = bool(i & 1)
        n_fund = seq.count("G" if rev else "C")
        pick = np.nonzero(rng.random(n_fund) < 0.8)[0]
        nums = np.diff(pick, prepend=-1) - 1
        tags = ["MM:Z:C+m?" + "".join(",%d" % x for x in nums) + ";", "ML:B:C" + "".join(",%d" % x for x in rng.integers(0, 256, len(pick))), "MN:i:%d" % L]
        recs.append(M.Rec("r%d" % i, 16 if rev else 0, int(starts[i]), 40, "%dM" % L, seq, tags))
    refs = [("chrT", clen)]
    f, fp = os.path.join(d, name + ".sam"), os.path.join(d, name + "_fp.sam")
    M.write_pair(refs, recs, T, f, fp)
    out = []
    for p in (f, fp):
        h = hostapi.BamFile(p)
        shutil.copyfile(h.staged_path(), p[:-4] + ".bam")
        h.close()
        os.remove(p)
        out.append(p[:-4] + ".bam")
    return out, sum(len(r.seq) for r in recs)


def timed(cmd, env=None):
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    dt = time.perf_counter() - t
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return dt


def blocks_of(path):
    h = hostapi.BamFile(path)
    t = h.bgzf_blocks()
    h.close()
    return open(path, "rb").read(), t["coff"], t["csize"], t["isize"], t["header_bytes"]


def decode_ms(eng, path, modtags, staged):
    """the decode kernels' time for one mth_bgzf_decode of the file: sum over k_decode_mm / k_mm_xm / k_decode of avg ms x launches"""
    os.environ["METHEOR_MM_STAGED"] = "1" if staged else "0"
    eng.decode_set_modtags(modtags, T)
    args = blocks_of(path)
    eng.bgzf_decode(*args)                                         # warm: allocations
    out = []
    for _ in range(reps):
        eng.timing_reset()
        eng.bgzf_decode(*args)
        t = eng.timing()
        out.append(sum(t[k][0] * t[k][1] for k in ("k_decode_mm", "k_mm_xm", "k_decode") if k in t))
    eng.decode_set_modtags(False)
    return out


def med_spread(ts):
    return "%.3f | %.3f .. %.3f" % (statistics.median(ts), min(ts), max(ts))


lines = ["# `--mm-tags`: MM / ML decode, both forms, against the XM route on the equivalent file", "",
         "`tools/bench_modtags.py --short %s --long %s --reps %d` on one MI355X.  `pdr -d 1 -p 1`, whole-process wall time, the runs of a"
         % (opt["--short"], opt["--long"], reps),
         "repetition in rotating order; decode = the decode kernels alone (`mth_timing_get`: `k_decode_mm`, or `k_mm_xm` + `k_decode`, or",
         "`k_decode` on F'), one `mth_bgzf_decode` of the file.  Median | min .. max over the repetitions.", ""]
eng = capi.Engine(0)
eng.timing_enable(True)
ok = True
for name, n, length in (("150 bp", int(opt["--short"]), 150), ("~5 kbp", int(opt["--long"]), 5000)):
    t0 = time.perf_counter()
    (f, fp), bases = make_input("in%d" % length, n, length, 3 + length)
    print("%s: %d records, %.1f Mbases, BAM %d MB / F' %d MB (generated in %.0f s)" % (name, n, bases / 1e6, os.path.getsize(f) >> 20, os.path.getsize(fp) >> 20,
                                                                                     time.perf_counter() - t0), flush=True)
    runs = [("`pdr --mm-tags`, `METHEOR_MM_STAGED=0` (direct: `k_decode_mm`)", f, ["--mm-tags"], {"METHEOR_MM_STAGED": "0"}),
            ("`pdr --mm-tags`, `METHEOR_MM_STAGED=1` (staged: `k_mm_xm` + `k_decode`)", f, ["--mm-tags"], {"METHEOR_MM_STAGED": "1"}),
            ("`pdr` on F' (XM route, the yardstick)", fp, [], {})]
    ts = [[] for _ in runs]
    for k in range(reps + 1):                                       # the first repetition warms the page cache and is dropped
        for i in [(k + j) % len(runs) for j in range(len(runs))]:
            _, inp, extra, env = runs[i]
            dt = timed([exe, "pdr", "-i", inp, "-o", os.path.join(d, "o%d.tsv" % i), "-d", "1", "-p", "1"] + extra, env)
            if k:
                ts[i].append(dt)
    outs = [open(os.path.join(d, "o%d.tsv" % i), "rb").read() for i in range(len(runs))]
    same = outs[0] == outs[1] == outs[2]
    ok &= same
    dec = [decode_ms(eng, f, True, False), decode_ms(eng, f, True, True), decode_ms(eng, fp, False, False)]
    lines += ["## %s records: %d records, %.1f Mbases; outputs of the three runs byte-identical: %s (%d rows)" % (name, n, bases / 1e6, same, outs[0].count(b"\n")), "",
              "| run | wall s: median | min .. max | decode ms: median | min .. max |", "|---|---|---|---|---|"]
    for (what, _, _, _), t, m in zip(runs, ts, dec):
        lines.append("| %s | %s | %s |" % (what, med_spread(t), med_spread(m)))
        print("%-76s wall %s s   decode %s ms" % (what, med_spread(t), med_spread(m)), flush=True)
    for unit, series in (("s of wall time", ts), ("ms of decode", dec)):
        md, ms = statistics.median(series[0]), statistics.median(series[1])
        spread = max(max(t) - min(t) for t in series[:2])
        lines += ["", "Staged faster than direct by more than the run-to-run spread (%.3f %s): %s (direct %.3f, staged %.3f)." % (spread, unit, ms < md - spread, md, ms)]
    lines.append("")
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
open(opt["--out"], "w").write("\n".join(lines) + "\n")
print("wrote " + opt["--out"])
shutil.rmtree(d)
sys.exit(0 if ok else 1)
