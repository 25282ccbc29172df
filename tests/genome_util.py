"""Inputs and expectations of the `--genome` tests (tests/test_genome_expected.py, tests/test_gpu_genome.py).

`metheor M -i in -g genome.fa` has to write what `metheor tag -i in -o tagged.sam -g genome.fa` followed by
`metheor M -i tagged.sam` writes.  The expectation is therefore built from the two existing oracle pieces, chained:
pyoracle.tag_xm per record -> bamio.Records(..., xms) -> pyoracle.Reads.decode -> the measures.  tag_xm returns None where
the reference panics (such records are dropped from inputs that are meant to run through); orc_decode takes an empty string
for a missing tag, so an empty XM is handed to it as b"." (no calls either way)."""
import numpy as np

from oracle import bamio, pyoracle

OPS = "MIDNSHP=X"
COMP_OK = set(b"ACGTNMRWSYKVHDB-")          # tag.rs:74-96: the characters the complement table holds


def make_contig(rng, length, lower):
    """random ACGT with CG written at length / 12 random places, a sprinkle of N and (lower) of lower case"""
    c = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length)
    at = rng.integers(0, length - 1, size=length // 12)
    c[at] = ord("C"); c[at + 1] = ord("G")
    c[rng.integers(0, length, size=length // 300)] = ord("N")
    if lower:
        lo = rng.random(length) < 0.1
        c[lo] = c[lo] | 0x20
    return bytes(c)


def is_rc(flag, paired):
    """tag.rs:136-144: is the read reverse-complemented before the context walk ?"""
    rev, first, last = bool(flag & 16), bool(flag & 64), bool(flag & 128)
    return (not ((not rev and first) or (rev and last))) if paired else rev


def cigar_string(ops):
    return "".join("%d%s" % (l, o) for l, o in ops)


def generate(seed, n=6000, length=30000):
    """bisulfite-like records on one generated contig (seeds 1, 2: single-end; 3, 4: paired) ->
    dict(contig, paired, recs=[(tid, pos, flag, mapq, packed cigar, seq bytes, cigar text)])"""
    rng = np.random.default_rng(seed)
    paired = seed >= 3
    contig = make_contig(rng, length, lower=bool(seed & 1))
    up = contig.upper()
    meth = rng.random(length) < 0.6                               # per position, fixed for all reads
    starts = np.sort(rng.integers(0, length - 400, size=n))
    recs = []
    for i in range(n):
        pos = int(starts[i])
        if paired:
            flag = 1 | 2 | int(rng.choice([64, 128])) | int(rng.choice([16, 32]))
        else:
            flag = 16 if rng.random() < 0.5 else 0
        rc = is_rc(flag, paired)
        if rng.random() < 0.75:
            ops = [(int(rng.integers(60, 150)), "M")]
        else:
            ops = []
            for _ in range(int(rng.integers(2, 6))):
                op = str(rng.choice(list("MMMID=XN")))
                if ops and ops[-1][1] == op:
                    continue
                ops.append((int(rng.integers(1, 9 if op in "IDN" else 40)), op))
            if not any(o in "M=X" for _, o in ops):
                ops.append((int(rng.integers(5, 40)), "M"))
            if rng.random() < 0.3:
                ops = [(int(rng.integers(1, 8)), "S")] + ops
            if rng.random() < 0.3:
                ops = ops + [(int(rng.integers(1, 8)), "S")]
            if rng.random() < 0.2:
                ops = [(3, "H")] + ops
        seq = bytearray()
        r = pos
        for l, o in ops:
            if o in "M=X":
                for p in range(r, r + l):
                    b = up[p]
                    if not rc and b == ord("C") and not (up[p + 1] == ord("G") and meth[p]):
                        b = ord("T")                               # C -> T unless a methylated CpG
                    if rc and b == ord("G") and not (p > 0 and up[p - 1] == ord("C") and meth[p - 1]):
                        b = ord("A")                               # the other strand: G -> A
                    seq.append(b)
                r += l
            elif o in "IS":
                seq += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=l))
            elif o in "DN":
                r += l
        err = np.flatnonzero(rng.random(len(seq)) < 0.01)
        for k in err:
            seq[k] = int(rng.choice(np.frombuffer(b"ACGTN", np.uint8)))
        mapq = int(rng.choice([0, 5, 30, 42]))
        recs.append((0, pos, flag, mapq, [(l << 4) | OPS.index(o) for l, o in ops], bytes(seq), cigar_string(ops)))
    return dict(contig=contig, paired=paired, recs=recs, name="g1")


def chain_xm(recs, contigs, paired):
    """pyoracle.tag_xm per record; None where the reference panics"""
    return [pyoracle.tag_xm(pos, flag, cig, seq, contigs[tid], is_paired_end=paired) if 0 <= tid < len(contigs) else None
            for tid, pos, flag, mapq, cig, seq, _ in recs]


def runnable(gen):
    """the generated input without the records `tag` panics on: (recs, xms), at most 1 % dropped"""
    xms = chain_xm(gen["recs"], [gen["contig"]], gen["paired"])
    keep = [k for k, x in enumerate(xms) if x is not None]
    assert len(gen["recs"]) - len(keep) <= len(gen["recs"]) // 100, "more than 1 % of the generated records panic"
    return [gen["recs"][k] for k in keep], [xms[k] for k in keep]


def sam_text(names_lens, recs, so="coordinate"):
    lines = ["@HD\tVN:1.6\tSO:" + so] + ["@SQ\tSN:%s\tLN:%d" % nl for nl in names_lens]
    for i, (tid, pos, flag, mapq, cig, seq, ctext) in enumerate(recs):
        lines.append("r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*" % (i, flag, names_lens[tid][0], pos + 1, mapq, ctext, seq.decode() if seq else "*"))
    return "\n".join(lines) + "\n"


def expected_reads(refs, recs, xms, cpg_set=None):
    """the chain's second half: Records with the derived strings -> the reference's decode"""
    rec = bamio.Records(refs, [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs],
                        [r[4] for r in recs], [x if x else b"." for x in xms])
    return pyoracle.Reads.decode(rec, cpg_set)


def decode_walk(pos, flag, cigar, xm):
    """readutil.rs:323-345 get_cpgs over one record: [(query offset, position, methylated)]"""
    fwd = flag in (0, 99, 147)
    out, q, r = [], 0, pos
    for c in cigar:
        op, ln = c & 15, c >> 4
        if op in (0, 7, 8):
            for k in range(ln):
                if q + k < len(xm) and xm[q + k] in b"zZ":
                    out.append((q + k, r + k if fwd else r + k - 1, xm[q + k] == ord("Z")))
            q += ln; r += ln
        elif op in (1, 4):
            q += ln
        elif op in (2, 3):
            r += ln
    return out


def plain_rule(pos, flag, cigar, seq, contig, paired):
    """The fast path of k_decode_genome in readable form.  A PLAIN record: every CIGAR operation is M, S or H and SEQ is at
    least as long as the M runs together (m bases).  Then tag.rs's column t is SEQ[t] against genome[pos + t], t < m, no gap
    anywhere, and the letter is Z / z exactly when
      read not reverse-complemented: genome[p] = C, genome[p + 1] = G, SEQ[t] = C (Z) / T (z)
      reverse-complemented:          genome[p] = G, genome[p - 1] = C, SEQ[t] = G (Z) / A (z)
    (p = pos + t; genome upper-cased, N outside the contig).  The decode reads letter q for the aligned base at query
    offset q.  That holds while the reference span holds A C G T N only; with anything else the record goes the way of every
    record that is not plain, the column walk.  -> the calls as decode_walk gives them, or None where tag.rs panics."""
    assert all((c & 15) in (0, 4, 5) for c in cigar)
    m = sum(c >> 4 for c in cigar if (c & 15) == 0)
    assert len(seq) >= m
    ln = len(contig)
    end = pos + (m if m else 1)
    if pos < 0 or end > ln or max(pos - 2, 0) > min(end + 2, ln):          # tag.rs:155-170
        return None
    ce = min(end + 2, ln)

    def gat(p):
        return ord("N") if p < 0 or p >= ce else ord(chr(contig[p]).upper())
    if any(gat(p) not in b"ACGTN" for p in range(pos - 2, end + 2)):        # an IUPAC code or a stray character after a C can cost
        xm = pyoracle.tag_xm(pos, flag, cigar, seq, contig, is_paired_end=paired)   # a letter (tag.rs:334-372 push none): not plain
        return None if xm is None else decode_walk(pos, flag, cigar, xm)
    rc = is_rc(flag, paired)
    if rc:                                                                   # tag.rs:19-25: every character is complemented
        if any(gat(p) not in COMP_OK for p in range(pos - 2, pos + m)) or any(seq[t] not in COMP_OK for t in range(m)):
            return None
    fwd = flag in (0, 99, 147)
    out, q, r = [], 0, pos
    for c in cigar:
        op, l = c & 15, c >> 4
        if op == 4:
            q += l
        if op != 0:
            continue
        for t in range(q, min(q + l, m)):
            p = pos + t
            if not rc and gat(p) == ord("C") and gat(p + 1) == ord("G") and seq[t] in b"CT":
                out.append((t, r + t - q if fwd else r + t - q - 1, seq[t] == ord("C")))
            if rc and gat(p) == ord("G") and gat(p - 1) == ord("C") and seq[t] in b"GA":
                out.append((t, r + t - q if fwd else r + t - q - 1, seq[t] == ord("G")))
        q += l; r += l
    return out


def random_plain_records(seed, n):
    """plain records around every edge: M of 1-119 with S and H at either end, starts at and next to both contig ends, a
    mixed-case genome with N, IUPAC letters and '=' in SEQ, single-end and paired flags incl. 99 / 147 / 83 / 163"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(130, 400))
        contig = bytes(rng.choice(list(b"ACGT") * 6 + list(b"CGCG") + list(b"Nacgtn"), size=ln).astype(np.uint8))
        m = int(rng.integers(1, 120))
        ops = [(m, "M")]
        if rng.random() < 0.3:
            ops = [(int(rng.integers(1, 9)), "S")] + ops
        if rng.random() < 0.3:
            ops = ops + [(int(rng.integers(1, 9)), "S")]
        if rng.random() < 0.15:
            ops = [(2, "H")] + ops
        if rng.random() < 0.15:
            ops = ops + [(2, "H")]
        where = rng.random()
        if where < 0.15:
            pos = int(rng.integers(0, 3))
        elif where < 0.35:
            pos = ln - m - int(rng.integers(-3, 3))          # ending next to, at, or past the contig's last base
        else:
            pos = int(rng.integers(0, ln - m + 1))
        paired = rng.random() < 0.5
        flag = int(rng.choice([99, 147, 83, 163, 65, 129, 81, 145])) if paired else int(rng.choice([0, 16]))
        qlen = sum(l for l, o in ops if o in "MS")
        alphabet = list(b"ACGT") * 8 + list(b"N") + (list(b"RYKM=") if rng.random() < 0.1 else [])
        seq = bytes(rng.choice(alphabet, size=qlen).astype(np.uint8))
        out.append((pos, flag, [(l << 4) | OPS.index(o) for l, o in ops], seq, contig, paired))
    return out
