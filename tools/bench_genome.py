"""`metheor pdr -g genome.fa` on an XM-free BAM against the two commands it replaces (`metheor tag` to SAM text, then
`metheor pdr` on that), and against `pdr` on the BAM that already carries XM.  Whole-process wall times, alternating runs.

The contig is larger than the 256 MiB Infinity Cache on purpose (a human genome never fits it); random ACGT has a CG every
16 bp, six times a human genome's density -- more calls per read than real data, not fewer.

Usage (GPU box): python tools/bench_genome.py [reads] [contig bp] [reps] [--parent DIR] [--keep DIR]
  --parent DIR   directory with another build's `metheor` (the two-step side is run with it; default: this tree's)
  --keep DIR     leave the inputs there (xmfree.bam, tagged.bam, genome.fa) for profiler runs"""
import os, shutil, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metheor_amd import hostapi
from tests import tag_util

argv = [a for a in sys.argv[1:]]
opt = {}
for k in ("--parent", "--keep"):
    if k in argv:
        i = argv.index(k); opt[k] = argv[i + 1]; del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 2_000_000
L = int(argv[1]) if len(argv) > 1 else 320_000_000
reps = int(argv[2]) if len(argv) > 2 else 3
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
exe = os.path.join(root, "metheor_amd", "metheor")
parent = os.path.join(opt["--parent"], "metheor") if "--parent" in opt else exe
d = opt.get("--keep", "/dev/shm/bench_genome")
os.makedirs(d, exist_ok=True)
fa, sam, bam, tagged_sam, tagged_bam = (os.path.join(d, x) for x in ("genome.fa", "xmfree.sam", "xmfree.bam", "tagged.sam", "tagged.bam"))

t0 = time.perf_counter()
rng = np.random.default_rng(11)
contig = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
tag_util.write_fasta(fa, "chrT", contig.tobytes())
starts = np.sort(rng.integers(0, L - 150, size=n))
with open(sam, "w") as fh:
    fh.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrT\tLN:%d\n" % L)
    tail = "\t" + "I" * 150 + "\tNM:i:0\n"
    for b0 in range(0, n, 100_000):
        st = starts[b0:b0 + 100_000]
        seq = contig[st[:, None] + np.arange(150)[None, :]]
        conv = rng.random(seq.shape) < 0.7
        rev = ((np.arange(b0, b0 + len(st)) & 1) == 1)[:, None]
        seq[(seq == ord("G")) & conv & rev] = ord("A")
        seq[(seq == ord("C")) & conv & ~rev] = ord("T")
        rows = seq.tobytes()
        fh.write("".join("r%d\t%d\tchrT\t%d\t40\t150M\t*\t0\t0\t%s%s" % (b0 + i, 16 if (b0 + i) & 1 else 0, st[i] + 1, rows[150 * i:150 * i + 150].decode(), tail)
                         for i in range(len(st))))
del contig
f = hostapi.BamFile(sam)
shutil.copyfile(f.staged_path(), bam)
f.close()
os.remove(sam)
print("input: %d reads of 150 bp on a %d-bp contig, BAM %d MB, FASTA %d MB (generated in %.0f s)" % (n, L, os.path.getsize(bam) >> 20, os.path.getsize(fa) >> 20, time.perf_counter() - t0), flush=True)


def timed(cmd, env=None):
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    dt = time.perf_counter() - t
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return dt, r.stderr


def summary(name, ts):
    print("%-46s best %.3f s  median %.3f s  (%.2f M reads/s at best)  runs: %s" % (name, min(ts), statistics.median(ts), n / min(ts) / 1e6, " ".join("%.3f" % t for t in ts)), flush=True)


out = {k: os.path.join(d, k + ".tsv") for k in ("two", "g", "gs", "xm_parent", "xm_new")}
t_tag, t_pdr, t_g, t_gs = [], [], [], []
for k in range(reps):       # alternating: the two-step run with the parent's binary, then -g (direct), then -g (staged)
    a, _ = timed([parent, "tag", "-i", bam, "-o", tagged_sam, "-g", fa])
    b, _ = timed([parent, "pdr", "-i", tagged_sam, "-o", out["two"]])
    c, err_g = timed([exe, "pdr", "-i", bam, "-o", out["g"], "-g", fa], {"METHEOR_TIMING": "1"})
    e, _ = timed([exe, "pdr", "-i", bam, "-o", out["gs"], "-g", fa], {"METHEOR_GENOME_STAGED": "1"})
    t_tag.append(a); t_pdr.append(b); t_g.append(c); t_gs.append(e)
    print("pairing %d: tag %.3f s + pdr on its SAM %.3f s = %.3f s | pdr -g %.3f s | pdr -g (staged form) %.3f s | -g faster than tag alone: %s"
          % (k, a, b, a + b, c, e, c < a), flush=True)
same = open(out["two"], "rb").read() == open(out["g"], "rb").read() == open(out["gs"], "rb").read()
print("outputs of the timed runs byte-identical (two-step == -g == -g staged): %s, %d rows" % (same, sum(1 for _ in open(out["g"], "rb"))))
summary("parent: tag (BAM -> SAM text in /dev/shm)", t_tag)
summary("parent: pdr on that SAM", t_pdr)
summary("parent: the two together", [x + y for x, y in zip(t_tag, t_pdr)])
summary("pdr -g (k_decode_genome)", t_g)
summary("pdr -g, METHEOR_GENOME_STAGED=1", t_gs)
print("ratio two-step / -g at best: %.1f x; tag alone / -g: %.1f x" % ((min(t_tag) + min(t_pdr)) / min(t_g), min(t_tag) / min(t_g)))
print("phases of the last -g run:\n" + "\n".join(l for l in err_g.splitlines() if "timing" in l), flush=True)

# the same table from the input that already carries XM: what deriving the calls and loading the genome cost
f = hostapi.BamFile(tagged_sam)
shutil.copyfile(f.staged_path(), tagged_bam)
f.close()
os.remove(tagged_sam)
t_xp, t_xn, t_g2 = [], [], []
for k in range(reps):
    t_xp.append(timed([parent, "pdr", "-i", tagged_bam, "-o", out["xm_parent"]])[0])
    t_xn.append(timed([exe, "pdr", "-i", tagged_bam, "-o", out["xm_new"]])[0])
    t_g2.append(timed([exe, "pdr", "-i", bam, "-o", out["g"], "-g", fa])[0])
same2 = open(out["xm_parent"], "rb").read() == open(out["xm_new"], "rb").read() == open(out["g"], "rb").read()
print("tagged BAM %d MB; pdr on it, parent == new == pdr -g on the XM-free BAM: %s" % (os.path.getsize(tagged_bam) >> 20, same2))
summary("parent: pdr on the tagged BAM", t_xp)
summary("new: pdr on the tagged BAM", t_xn)
summary("new: pdr -g on the XM-free BAM", t_g2)
for p in out.values():
    if os.path.exists(p):
        os.remove(p)
if "--keep" not in opt:
    shutil.rmtree(d)
sys.exit(0 if same and same2 else 1)
