"""`metheor pdr -g genome.fa` on an XM-free BAM against the two commands it replaces (`metheor tag` to SAM text, then
`metheor pdr` on that), and against `pdr` on the BAM that already carries XM.  Whole-process wall times, alternating runs.

The contig is larger than the 256 MiB Infinity Cache on purpose (a human genome never fits it); random ACGT has a CG every
16 bp, six times a human genome's density -- more calls per read than real data, not fewer.

Usage (GPU box): python tools/bench_genome.py [reads] [contig bp] [reps] [--parent DIR] [--keep DIR] [--fasta-route R] [--routes-only]
  --parent DIR      directory with another build's `metheor` (the two-step side is run with it; default: this tree's)
  --keep DIR        leave the inputs there (xmfree.bam, tagged.bam, genome.fa) for profiler runs
  --fasta-route R   how this tree's `-g` runs read the FASTA: host (default: Fasta::fetch), device (METHEOR_GENOME_DEVICE=1: the
                    plain file packed by k_fasta_pack) or bgzf (genome.fa.gz + .fai, written here with Python's zlib)
  --routes-only     only the FASTA routes against each other and against the parent: parent `pdr -g g.fa`, new `pdr -g g.fa`,
                    new with METHEOR_GENOME_DEVICE=1, new `-g g.fa.gz`, alternating; wall times, genome phases, outputs compared"""
import os, shutil, statistics, struct, subprocess, sys, time, zlib
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metheor_amd import hostapi
from tests import tag_util

argv = [a for a in sys.argv[1:]]
opt = {}
for k in ("--parent", "--keep", "--fasta-route"):
    if k in argv:
        i = argv.index(k); opt[k] = argv[i + 1]; del argv[i:i + 2]
routes_only = "--routes-only" in argv
if routes_only:
    argv.remove("--routes-only")
route = opt.get("--fasta-route", "host")
assert route in ("host", "device", "bgzf"), route
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


def write_bgzf(src, dst):
    """src as BGZF (SAM spec 4.1): 65280-byte payloads, raw DEFLATE at zlib's default level, the 28-byte EOF block last"""
    with open(src, "rb") as fi, open(dst, "wb") as fo:
        while True:
            payload = fi.read(65280)
            if not payload:
                break
            co = zlib.compressobj(-1, zlib.DEFLATED, -15)
            comp = co.compress(payload) + co.flush()
            fo.write(struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(payload), len(payload)))
        fo.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    shutil.copyfile(src + ".fai", dst + ".fai")


fa_gz = fa + ".gz"
if route == "bgzf" or routes_only:
    write_bgzf(fa, fa_gz)
g_fa = fa_gz if route == "bgzf" else fa                    # what this tree's -g runs are given
g_env = {"METHEOR_GENOME_DEVICE": "1"} if route == "device" else {}
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


if routes_only:
    runs = [("parent: pdr -g g.fa", parent, fa, {}), ("new: pdr -g g.fa (host read)", exe, fa, {}),
            ("new: pdr -g g.fa, METHEOR_GENOME_DEVICE=1", exe, fa, {"METHEOR_GENOME_DEVICE": "1"}), ("new: pdr -g g.fa.gz", exe, fa_gz, {})]
    print("FASTA %d MB, bgzip copy %d MB" % (os.path.getsize(fa) >> 20, os.path.getsize(fa_gz) >> 20), flush=True)
    ts, errs, outs = [[] for _ in runs], [None] * len(runs), []
    for k in range(reps):
        for i in [(k + j) % len(runs) for j in range(len(runs))]:        # the order rotates: no run always follows the same neighbour
            name, binary, genome, env = runs[i]
            o = os.path.join(d, "route%d.tsv" % i)
            dt, errs[i] = timed([binary, "pdr", "-i", bam, "-o", o, "-g", genome], dict(env, METHEOR_TIMING="1"))
            ts[i].append(dt)
        print("pairing %d: %s | device beats host read: %s, bgzf beats host read: %s" % (k, " | ".join("%.3f" % t[-1] for t in ts), ts[2][-1] < ts[1][-1], ts[3][-1] < ts[1][-1]), flush=True)
    outs = [open(os.path.join(d, "route%d.tsv" % i), "rb").read() for i in range(len(runs))]
    same = all(o == outs[0] for o in outs)
    print("outputs of the four runs byte-identical: %s, %d rows" % (same, outs[0].count(b"\n")))
    for (name, _, _, _), t in zip(runs, ts):
        summary(name, t)
    for (name, _, _, _), e in zip(runs, errs):
        print("phases of the last run of [%s]:\n" % name + "\n".join(l for l in e.splitlines() if "genome" in l or "context" in l), flush=True)
    if "--keep" not in opt:
        shutil.rmtree(d)
    sys.exit(0 if same else 1)

out = {k: os.path.join(d, k + ".tsv") for k in ("two", "g", "gs", "xm_parent", "xm_new")}
t_tag, t_pdr, t_g, t_gs = [], [], [], []
for k in range(reps):       # alternating: the two-step run with the parent's binary, then -g (direct), then -g (staged)
    a, _ = timed([parent, "tag", "-i", bam, "-o", tagged_sam, "-g", fa])
    b, _ = timed([parent, "pdr", "-i", tagged_sam, "-o", out["two"]])
    c, err_g = timed([exe, "pdr", "-i", bam, "-o", out["g"], "-g", g_fa], dict(g_env, METHEOR_TIMING="1"))
    e, _ = timed([exe, "pdr", "-i", bam, "-o", out["gs"], "-g", g_fa], dict(g_env, METHEOR_GENOME_STAGED="1"))
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
    t_g2.append(timed([exe, "pdr", "-i", bam, "-o", out["g"], "-g", g_fa], g_env)[0])
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
