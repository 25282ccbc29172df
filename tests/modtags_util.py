"""`--mm-tags` (mth_decode_set_modtags) test infrastructure: the rule X(record, T) restated in Python from its text
(include/metheor_hip.h; not from the kernel), a generator of SAM records with MM / ML / MN fields that counts the categories
it produced, the writer of F' (flag & 0x10, XM:Z fields out, XM:Z:X in) and a packer of raw BAM records."""
import re
import struct
from collections import Counter

import numpy as np

OPS = "MIDNSHP=X"
CODES = "=ACMGRSVTWYHKDBN"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
GRAMMAR = re.compile(r"(?:[ACGTUN][+-](?:[a-z]+|[0-9]+)[.?]?(?:,[0-9]{1,9})*;)*")
GROUP = re.compile(r"([ACGTUN])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]{1,9})*);")
PAIRED_FLAGS = (99, 147, 83, 163, 97, 65)


class ModTagError(ValueError):
    """the record is an error under the rule (ERRB_MODTAG)"""


class Rec:
    def __init__(self, name, flag, pos, mapq, cigar, seq, tags, tid=0):
        self.name, self.flag, self.pos, self.mapq, self.cigar, self.seq, self.tags, self.tid = name, flag, pos, mapq, cigar, seq, list(tags), tid

    def line(self, refs):
        rname = refs[self.tid][0] if self.tid >= 0 else "*"
        return "\t".join([self.name, str(self.flag), rname, str(self.pos + 1), str(self.mapq), self.cigar, "*", "0", "0", self.seq or "*", "*"] + self.tags)


def tag(tags, name, typ=None):
    """first field called `name` (of type `typ`) -> (type, value text) or None"""
    for t in tags:
        n, ty, v = t.split(":", 2)
        if n == name and (typ is None or ty == typ):
            return ty, v
    return None


def x_string(rec, T):
    """-> (X, contributes_nothing); raises ModTagError"""
    seq = "" if rec.seq in ("", "*") else rec.seq
    L = len(seq)
    dots = "." * L
    mn = tag(rec.tags, "MN", "i")
    if L == 0 or "H" in rec.cigar or (mn is not None and int(mn[1]) != L):
        return dots, True
    mm = tag(rec.tags, "MM", "Z")
    if mm is None:
        return dots, False
    ml = tag(rec.tags, "ML")
    probs = None
    if ml is not None:
        if ml[0] != "B" or not ml[1].startswith("C"):
            raise ModTagError("ML is not B:C")
        probs = [int(x) for x in ml[1].split(",")[1:]]
    if not GRAMMAR.fullmatch(mm[1]):
        raise ModTagError("grammar")
    chosen, owned = None, 0
    for base, strand, codes, mode, nums in GROUP.findall(mm[1]):
        k = 1 if codes[0].isdigit() else len(codes)
        d = [int(x) for x in nums.split(",")[1:]]
        if chosen is None and base == "C" and strand == "+" and not codes[0].isdigit() and "m" in codes:
            chosen = (owned, k, codes.index("m"), mode, d)
        owned += len(d) * k
    if probs is not None and len(probs) != owned:
        raise ModTagError("ML count")
    if chosen is None:
        return dots, False
    base_of_group, k, im, mode, d = chosen
    reverse = bool(rec.flag & 0x10)
    orig = "".join(COMP.get(c, "?") for c in reversed(seq)) if reverse else seq
    fund = [j for j, c in enumerate(orig) if c == "C"]
    listed = {}
    at = -1
    for i, skip in enumerate(d):
        at = skip if i == 0 else at + skip + 1
        if at >= len(fund):
            raise ModTagError("the list selects a C the read does not have")
        listed[fund[at]] = 255 if probs is None else probs[base_of_group + i * k + im]
    x = list(dots)
    for j in fund:
        if j + 1 >= L or orig[j + 1] != "G":
            continue
        q = L - 1 - j if reverse else j
        if j in listed:
            x[q] = "Z" if listed[j] >= T else "z"
        elif mode != "?":
            x[q] = "z"
    return "".join(x), False


def fprime(rec, T):
    x, _ = x_string(rec, T)
    return Rec(rec.name, rec.flag & 0x10, rec.pos, rec.mapq, rec.cigar, rec.seq, [t for t in rec.tags if not t.startswith("XM:Z:")] + ["XM:Z:" + x], rec.tid)


def sam_text(refs, recs, sorted_=True):
    head = "@HD\tVN:1.6\tSO:%s\n" % ("coordinate" if sorted_ else "unsorted") + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    return head + "".join(r.line(refs) + "\n" for r in recs)


def write_pair(refs, recs, T, path_f, path_fp, sorted_=True):
    open(path_f, "w").write(sam_text(refs, recs, sorted_))
    open(path_fp, "w").write(sam_text(refs, [fprime(r, T) for r in recs], sorted_))


# ---- raw BAM records -----------------------------------------------------------------------------------------------------
def cigar_ops(cigar):
    return [] if cigar == "*" else [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def pack_aux(tags):
    out = b""
    for t in tags:
        n, ty, v = t.split(":", 2)
        out += n.encode()
        if ty == "Z":
            out += b"Z" + v.encode() + b"\0"
        elif ty == "i":
            x = int(v)
            out += (b"C" + struct.pack("<B", x)) if 0 <= x < 256 else (b"S" + struct.pack("<H", x)) if 0 <= x < 65536 else (b"i" + struct.pack("<i", x))
        elif ty == "B":
            sub, items = v[0], [int(y) for y in v.split(",")[1:]]
            out += b"B" + sub.encode() + struct.pack("<I", len(items)) + struct.pack("<%d%s" % (len(items), {"C": "B", "c": "b", "S": "H", "s": "h", "I": "I", "i": "i"}[sub]), *items)
        elif ty == "A":
            out += b"A" + v.encode()
        else:
            raise ValueError(t)
    return out


def pack_record(rec, raw_aux=None):
    """the record as BAM bytes, block_size first; raw_aux: the aux bytes as given (crafted fields)"""
    seq = "" if rec.seq in ("", "*") else rec.seq
    name = rec.name.encode() + b"\0"
    cg = cigar_ops(rec.cigar)
    nib = [CODES.index(c) for c in seq] + [0]
    packed = bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(seq), 2))
    core = struct.pack("<iiBBHHHiiii", rec.tid, rec.pos, len(name), rec.mapq, 4680, len(cg), rec.flag, len(seq), -1, -1, 0)
    body = core + name + b"".join(struct.pack("<I", (n << 4) | OPS.index(o)) for n, o in cg) + packed + b"\xff" * len(seq)
    body += pack_aux(rec.tags) if raw_aux is None else raw_aux
    return struct.pack("<I", len(body)) + body


def pack_stream(recs):
    """-> (bytes, uint64 offsets [n + 1])"""
    parts = [pack_record(r) for r in recs]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(parts), off


# ---- the generator -------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33)


def make_contig(rng, n):
    c = rng.choice(list("ACGT"), n, p=[0.22, 0.28, 0.28, 0.22])
    for k in rng.integers(0, n - 1, n // 8):          # CpG-rich: calls on most reads
        c[k], c[k + 1] = "C", "G"
    return "".join(c)


def skips_of(chosen_idx):
    out, prev = [], -1
    for s in chosen_idx:
        out.append(s - prev - 1)
        prev = s
    return out


def generate(seed, n, long_reads=True, contig_len=40000, T=128):
    """-> dict(refs, recs (sorted by position), cats: Counter of the categories produced)"""
    rng = np.random.default_rng(seed)
    contig = make_contig(rng, contig_len)
    refs = [("c0", contig_len)]
    cats = Counter()
    recs = []
    starts = np.sort(rng.integers(500, contig_len - 4500, n))
    for i in range(n):
        pos = int(starts[i])
        u = rng.random()
        if long_reads and u < 0.005:
            L = int(rng.integers(2900, 3100)); cats["len~3000"] += 1
        elif u < 0.13:
            L = int(LENGTHS[int(rng.integers(0, len(LENGTHS)))]); cats["len%d" % L] += 1
        else:
            L = 150; cats["len150"] += 1
        reverse = rng.random() < 0.5
        cats["reverse" if reverse else "forward"] += 1
        if rng.random() < 0.3:
            flag = int(rng.choice([f for f in PAIRED_FLAGS if bool(f & 16) == reverse]))
            cats["flag%d" % flag] += 1
        else:
            flag = 16 if reverse else 0
        # CIGAR and SEQ
        ops = []
        if L == 0:
            ops = [(20, "M")]
        else:
            kind = rng.random()
            body = L
            lead = trail = 0
            if kind < 0.15 and L >= 8:
                lead, trail = int(rng.integers(0, 4)), int(rng.integers(1, 4))
                body = L - lead - trail
                cats["softclip"] += 1
            if lead:
                ops.append((lead, "S"))
            if 0.15 <= kind < 0.30 and body >= 12:
                a = int(rng.integers(3, body - 6)); k = int(rng.integers(1, 4))
                ops += [(a, "M"), (k, "I"), (body - a - k, "M")]; cats["insertion"] += 1
            elif 0.30 <= kind < 0.42 and body >= 12:
                a = int(rng.integers(3, body - 3)); k = int(rng.integers(1, 6))
                ops += [(a, "M"), (k, "D" if rng.random() < 0.7 else "N"), (body - a, "M")]; cats["deletion"] += 1
            elif 0.42 <= kind < 0.47 and body >= 6:
                a = int(rng.integers(1, body - 2))
                ops += [(a, "="), (1, "X"), (body - a - 1, "M")]
            else:
                ops.append((body, "M"))
            if trail:
                ops.append((trail, "S"))
            if rng.random() < 0.03:
                ops = [(5, "H")] + ops; cats["hardclip"] += 1
        seq, r = [], pos
        for ln, o in ops:
            if o in "M=X":
                seq.append(contig[r:r + ln]); r += ln
            elif o in "IS":
                seq.append("".join(rng.choice(list("ACGT"), ln)))
            elif o in "DN":
                r += ln
        seq = list("".join(seq)) if L else []
        assert len(seq) == L
        if L and rng.random() < 0.04:
            seq[int(rng.integers(0, L))] = "N"; cats["N"] += 1
        # an insertion right between a C and its G: the inserted bases start with the G
        ins = [j for j, (ln, o) in enumerate(ops) if o == "I"]
        if ins:
            k = ins[0]
            q = sum(ln for ln, o in ops[:k] if o in "MIS=X")
            if rng.random() < 0.7:
                seq[q - 1], seq[q] = "C", "G"
                cats["ins_between_CG"] += 1
        if L and not reverse and rng.random() < 0.06:
            seq[-1] = "C"
        if L and reverse and rng.random() < 0.06:
            seq[0] = "G"
        seq = "".join(seq)
        if L and not reverse and seq[-1] == "C":
            cats["C_last_forward"] += 1
        if L and reverse and seq[0] == "G":
            cats["G_first_reverse"] += 1
        cigar = "".join("%d%s" % x for x in ops)
        # the tags
        orig = "".join(COMP[c] for c in reversed(seq)) if reverse else seq
        fund = [j for j, c in enumerate(orig) if c == "C"]
        tags, probs, groups = [], [], []
        palette = [0, max(T - 1, 0), T, 255]

        def group(head, k, nums):
            groups.append(head + "".join(",%d" % x for x in nums) + ";")
            for _ in range(len(nums) * k):
                v = int(palette[int(rng.integers(0, 4))]) if rng.random() < 0.5 else int(rng.integers(0, 256))
                probs.append(v)
                if v in palette:
                    cats["ml%d" % v] += 1

        def foreign(kind):
            nums = [int(x) for x in rng.integers(0, 5, int(rng.integers(0, 4)))]
            if kind == "C-m":
                group("C-m" + str(rng.choice(["", ".", "?"])), 1, nums)
            elif kind == "N+m":
                group("N+m?", 1, nums)
            elif kind == "numeric":
                group("C+76792?", 1, nums)
            elif kind == "lead":
                head, k = [("A+a?", 1), ("G-gh.", 2), ("T+e", 1)][int(rng.integers(0, 3))]
                group(head, k, nums)
            else:
                group("T+fg.", 2, nums)
            cats["foreign_" + kind] += 1
        v = rng.random()
        if v < 0.06:
            cats["no_MM"] += 1
            if rng.random() < 0.3:
                tags.append("Mm:Z:C+m?,0;"); cats["old_spelling"] += 1
        else:
            if rng.random() < 0.15:
                foreign("lead")
            for kind in ("C-m", "N+m", "numeric"):
                if rng.random() < 0.06:
                    foreign(kind)
            if rng.random() < 0.04:
                group("C+h?", 1, [])
                cats["no_group_qualifies_yet"] += 1
            mode = str(rng.choice(["", ".", "?"]))
            cats["mode_" + (mode or "none")] += 1
            codes = str(rng.choice(["m", "m", "m", "hm", "mh"]))
            cats["codes_" + codes] += 1
            w = rng.random()
            dens = 1.0 if w < 0.1 else (0.0 if w < 0.15 else (0.05 if w < 0.35 else float(rng.random())))
            pick = [j for j in range(len(fund)) if rng.random() < dens]
            if fund and rng.random() < 0.15 and (not pick or pick[-1] != len(fund) - 1):
                pick.append(len(fund) - 1)
            if pick and pick[-1] == len(fund) - 1:
                cats["list_ends_on_last_C"] += 1
            nums = skips_of(pick)
            if any(x >= 10 for x in nums):
                cats["multi_digit"] += 1
            group("C+" + codes + mode, len(codes), nums)
            if rng.random() < 0.04:
                group("C+m?", 1, [0] if fund else []); cats["duplicate_group"] += 1
            if rng.random() < 0.15:
                foreign("trail")
            tags.append("MM:Z:" + "".join(groups))
            if rng.random() < 0.08:
                cats["no_ML"] += 1
            else:
                tags.append("ML:B:C" + "".join(",%d" % x for x in probs))
        m = rng.random()
        if m < 0.25:
            tags.append("MN:i:%d" % L); cats["MN_equal"] += 1
        elif m < 0.28:
            tags.append("MN:i:%d" % (L + 1 + int(rng.integers(0, 3)))); cats["MN_unequal"] += 1
        if rng.random() < 0.1:
            tags.insert(int(rng.integers(0, len(tags) + 1)), "XM:Z:" + "Z" * L); cats["stray_XM"] += 1
        if rng.random() < 0.2:
            tags.insert(0, "NM:i:%d" % int(rng.integers(0, 70000)))
        recs.append(Rec("r%d" % i, flag, pos, int(rng.integers(0, 61)) if rng.random() < 0.15 else int(rng.integers(10, 61)), cigar, seq, tags))
    return dict(refs=refs, recs=recs, cats=cats, contig=contig)


# every error the rule names, as SAM fields on SEQ ACGTCGCCGA (CIGAR 10M): (what, flag, tags)
ERROR_CASES = [
    ("ML of type Z", 0, ["MM:Z:C+m?,1,1;", "ML:Z:200,30"]),
    ("ML of type B:c", 0, ["MM:Z:C+m?,1,1;", "ML:B:c,100,30"]),
    ("ML of type B:S", 16, ["MM:Z:C+m?,0;", "ML:B:S,100"]),
    ("no semicolon at the end", 0, ["MM:Z:C+m?,1,1", "ML:B:C,200,30"]),
    ("text after the last semicolon", 0, ["MM:Z:C+m?,1,1;x", "ML:B:C,200,30"]),
    ("a base outside ACGTUN", 0, ["MM:Z:X+m?,1;C+m?,1,1;", "ML:B:C,1,200,30"]),
    ("a strand outside + -", 0, ["MM:Z:C*m?,1,1;", "ML:B:C,200,30"]),
    ("no code", 0, ["MM:Z:C+?,1,1;", "ML:B:C,200,30"]),
    ("letters and digits mixed in a code", 0, ["MM:Z:C+m5?,1,1;", "ML:B:C,200,30"]),
    ("an upper-case code", 0, ["MM:Z:C+M?,1,1;", "ML:B:C,200,30"]),
    ("an empty number", 0, ["MM:Z:C+m?,1,,1;", "ML:B:C,200,30"]),
    ("a number of ten digits", 0, ["MM:Z:C+m?,1000000000;"]),
    ("a negative number", 0, ["MM:Z:C+m?,-1;", "ML:B:C,200"]),
    ("two modes", 0, ["MM:Z:C+m?.,1,1;", "ML:B:C,200,30"]),
    ("a broken foreign group", 0, ["MM:Z:C+m?,1,1;A+a", "ML:B:C,200,30"]),
    ("no fifth C", 0, ["MM:Z:C+m?,1,1,0;"]),
    ("no fifth C, with ML", 0, ["MM:Z:C+m?,1,1,0;", "ML:B:C,200,30,9"]),
    ("the first number past the last C", 0, ["MM:Z:C+m?,4;"]),
    ("reverse: no fourth C", 16, ["MM:Z:C+m?,0,1,0,0;"]),
    ("ML too short", 0, ["MM:Z:C+m?,1,1;", "ML:B:C,200"]),
    ("ML too long", 0, ["MM:Z:C+m?,1,1;", "ML:B:C,200,30,1"]),
    ("ML short of a foreign group's entries", 0, ["MM:Z:A+a?,0;C+m?,1,1;", "ML:B:C,200,30"]),
    ("ML counted per code", 0, ["MM:Z:C+hm?,1,1;", "ML:B:C,200,30"]),
    ("ML with an empty MM", 0, ["MM:Z:", "ML:B:C,1"]),
]


def error_recs():
    return [(what, Rec("e%d" % k, flag, 99, 30, "10M", "ACGTCGCCGA", tags)) for k, (what, flag, tags) in enumerate(ERROR_CASES)]
