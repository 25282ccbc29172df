"""Inputs of the `tag` context-rule tests (tests/test_tag_hand_cases.py, tests/test_gpu_tag_cases.py): the hand-worked table
tests/golden/tag_hand_cases.json, a deterministic enumeration of short records over one small contig (and of longer plain
records over a second one), BAM packing, and the predicates that say which class of the table a record belongs to.

The predicates read the INPUTS only (CIGAR, SEQ, flag, contig): they rebuild the two gapped column strings of tag.rs:174-259
and look at where a reference C stands in them.  They never produce a letter; what a record's XM string is comes from the
table's `expect` (worked out by hand from tag.rs) or from the oracle, never from here."""
import json
import os
import re
import struct

import numpy as np

from oracle import pyoracle
from tests.genome_util import COMP_OK, OPS, is_rc

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "tag_hand_cases.json")
NIB = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
COMP = dict(zip("ACGTNMRWSYKVHDB-", "TGCANKYWSRMBDHV-"))                   # tag.rs:79-100

# ---- the contigs ----------------------------------------------------------------------------------------------------------
# 41 bases: CG at both ends, cg, Cg (twice), a CHG (CAG at 7), a CHH (CCA at 11), N, NN, one IUPAC letter (R, after a C and before a G)
SHORT = b"CGATcgTCAGTCCATNACgNNGTCRGACTGGCATTGCgACG"
# 96 bases with the same ingredients: CG at every phase of a 4-byte word and of a 16-byte load, runs of CG, CG at both ends
LONG = SHORT[:-2] + b"TTCGGCgTANCGCcGGTYCGATCGNNCCGTTAGCGCATCCGACGTTCGGACCGTAACGTCG"
assert len(SHORT) == 41 and len(LONG) >= 80
FLAGS = ((0, False), (16, False), (99, True), (147, True), (83, True), (163, True), (1, True))      # (flag, the file is paired)
PLAIN_M = (14, 15, 16, 17, 30, 31, 32, 33, 46)


def parse_cigar(text):
    return [(int(n) << 4) | OPS.index(o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def cigar_text(cigar):
    return "".join("%d%s" % (c >> 4, OPS[c & 15]) for c in cigar)


def ref_len(cigar):
    return sum(c >> 4 for c in cigar if (c & 15) in (0, 2, 3, 7, 8))


# ---- the enumeration --------------------------------------------------------------------------------------------------------
def shapes():
    """the CIGAR texts of the issue's list, in its order: 201 M / I / D / N shapes, the first 40 with a leading 2S and with a
    trailing 1S, five specials"""
    ac, bde = (1, 2, 3), (1, 2)
    out = ["%dM" % a for a in ac]
    for g in "IDN":
        out += ["%dM%d%s%dM" % (a, b, g, c) for a in ac for b in bde for c in ac]
    for g1, g2 in ("ID", "DI"):
        out += ["%dM%d%s%dM%d%s%dM" % (a, b, g1, c, d, g2, e) for a in ac for b in bde for c in ac for d in bde for e in bde]
    assert len(out) == 201
    out += ["2S" + s for s in out[:40]] + [s + "1S" for s in out[:40]]
    return out + ["2I", "1S2I1S", "3=2X", "2M1P2M", "2H3M"]


def seq_for(cigar, pos, contig, variant):
    """SEQ of a record: the reference bases under M / = / X (N past the contig's end), inserted and clipped runs start CG;
    variant 0: as is, 1: every C -> T and G -> A, 2: that conversion at odd offsets of SEQ only"""
    up, seq, r = contig.upper(), bytearray(), pos
    for c in cigar:
        op, l = c & 15, c >> 4
        if op in (0, 7, 8):
            seq += bytes(up[p] if 0 <= p < len(up) else ord("N") for p in range(r, r + l))
            r += l
        elif op in (1, 4):
            seq += (b"CG" + b"A" * l)[:l]
        elif op in (2, 3):
            r += l
    if variant:
        for k in range(len(seq)):
            if variant == 1 or (k & 1):
                seq[k] = {ord("C"): ord("T"), ord("G"): ord("A")}.get(seq[k], seq[k])
    return bytes(seq)


def _enumerate(contig, cigars):
    out, ln = [], len(contig)
    for text in cigars:
        cig = parse_cigar(text)
        rl = ref_len(cig)
        for pos in range(0, ln - rl + 3):
            for variant in (0, 1, 2):
                seq = seq_for(cig, pos, contig, variant)
                for flag, paired in FLAGS:
                    out.append((pos, flag, paired, cig, seq, text))
    return out


def enumerate_small():
    """[(pos, flag, paired, packed cigar, seq, cigar text)] on SHORT"""
    return _enumerate(SHORT, shapes())


def enumerate_plain():
    """the plain records that reach the vectorised genome search: M of 14 .. 46 with and without a leading 1S, on LONG"""
    return _enumerate(LONG, [p + "%dM" % m for m in PLAIN_M for p in ("", "1S")])


def oracle_xm(rec, contig, ln=None):
    """pyoracle's orc_tag_xm with the header LN given apart from the bases (LN <= the bases held); None where the reference panics"""
    pos, flag, paired, cig, seq = rec[:5]
    ln = len(contig) if ln is None else ln
    assert ln <= len(contig)
    return pyoracle.tag_xm(pos, flag, cig, seq, contig[:ln], is_paired_end=paired)


# ---- BAM bytes ------------------------------------------------------------------------------------------------------------
def bam_record(tid, pos, flag, cigar, seq, name=b"r", mapq=30):
    """one BAM record, block_size included; l_seq is len(seq) whatever the CIGAR says (as tests/test_gpu_tag.py::_bam_record)"""
    packed = bytearray((len(seq) + 1) // 2)
    for k, ch in enumerate(seq.decode()):
        packed[k >> 1] |= NIB[ch] << (0 if k & 1 else 4)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + b"\0" + struct.pack("<%dI" % len(cigar), *cigar) + bytes(packed) + b"\xff" * len(seq)
    return struct.pack("<i", len(body)) + body


def window(records):
    """[(tid, pos, flag, cigar, seq)] -> (raw bytes, uint64 offsets) as hostapi.BamFile.windows() gives them"""
    parts = [bam_record(*r) for r in records]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return b"".join(parts), off


# ---- the hand table -----------------------------------------------------------------------------------------------------------
def hand_cases():
    """the table with cigar parsed and seq / contig as bytes; `expect` is bytes, or None for "panic" """
    cases = json.load(open(TABLE))
    for c in cases:
        c["cig"] = parse_cigar(c["cigar"])
        seq = c["seq"].encode()
        c["seq_b"] = seq[:c["l_seq"]] if "l_seq" in c else seq
        c["contig_b"] = c["contig"].encode()
        c["ln_v"] = c.get("ln", len(c["contig"]))
        c["want"] = None if c["expect"] == "panic" else c["expect"].encode()
        c["rec"] = (c["pos"], c["flag"], bool(c["paired"]), c["cig"], c["seq_b"], c["cigar"])
    return cases


# ---- the predicates -----------------------------------------------------------------------------------------------------------
def columns(rec, contig, ln=None, raw=False):
    """tag.rs:154-259 -> (target read string, target reference string) in walk orientation, characters outside the complement
    table kept as they are under a reverse complement (raw: the strings before that choice, flanks included); None where the reference string cannot be cut (tag.rs:158-172)"""
    pos, flag, paired, cig, seq = rec[:5]
    ln = len(contig) if ln is None else ln
    end = pos + (ref_len(cig) or 1)
    cs, ce = max(pos - 2, 0), min(end + 2, ln)
    ps, pe = max(2 - pos, 0), max(end - ln + 2, 0)
    if pos < 0 or cs > ce or ce > len(contig) or pe > 2:
        return None
    ref = "N" * ps + contig[cs:ce].decode().upper() + "N" * pe
    if len(ref) < 2:
        return None
    sq = seq.decode().upper()
    R, G, uq, ug = "--", ref[:2], 0, 2
    for c in cig:
        op, l = c & 15, c >> 4
        if op == 0:
            R += sq[uq:uq + l]; G += ref[ug:ug + l]; uq += l; ug += l
        elif op == 1:
            R += sq[uq:uq + l]; G += "-" * l; uq += l
        elif op == 2:
            R += "-" * l; G += ref[ug:ug + l]; ug += l
    R += "--"; G += ref[-2:]
    if raw:
        return R, G
    if is_rc(flag, paired):
        return ("".join(COMP.get(x, x) for x in reversed(R[:-2])), "".join(COMP.get(x, x) for x in reversed(G[:-2])))
    return R[2:], G[2:]


def c_columns(rec, contig, ln=None):
    """every column the walk of tag.rs:262-267 looks a context up for: a read base that is neither - nor N over a reference C
    -> [(idx, exempt index, the gap condition of tag.rs:268-269, the context characters tag.rs collects)]"""
    rg = columns(rec, contig, ln)
    if rg is None:
        return []
    R, G = rg
    n, out = len(R), []
    for idx in range(max(n - 2, 0)):
        if R[idx] in "-N" or idx >= len(G) or G[idx] != "C":
            continue
        exempt = idx in (n - 3, n - 4)
        gap = "-" in R[idx + 1:idx + 3]
        if gap and not exempt:
            ctx = "C" + "".join(G[k] for k in range(idx + 1, n) if R[k] != "-" and k < len(G))[:2]
        else:
            ctx = G[idx:idx + 3]
        out.append((idx, exempt, gap, ctx))
    return out


def _ops(rec):
    return {OPS[c & 15] for c in rec[3]}


def _short(rec):
    return len(rec[4]) < sum(c >> 4 for c in rec[3] if (c & 15) in (0, 1))


def p_plain_m(rec, contig, ln=None):
    return _ops(rec) == {"M"} and len(rec[3]) == 1 and not _short(rec)


def p_orientation(rec, contig, ln=None):
    """a paired file's record whose reverse complement is not its 0x10 bit (tag.rs:15-18): mate 2 forward, mate 1 reverse, neither"""
    return rec[2] and is_rc(rec[1], True) != bool(rec[1] & 16)


def p_gap_lookahead(rec, contig, ln=None):
    """a reference C whose next two read columns hold a deleted base, away from the exempted indices: tag.rs:272-296 runs"""
    rg = columns(rec, contig, ln)
    return rg is not None and any(gap and not ex and "-" not in rg[1][i + 1:i + 3] for i, ex, gap, _ in c_columns(rec, contig, ln))


def p_insertion(rec, contig, ln=None):
    """a '-' reference column (an inserted base) within the two columns after a reference C"""
    rg = columns(rec, contig, ln)
    return rg is not None and any("-" in rg[1][i + 1:i + 3] for i, _, _, _ in c_columns(rec, contig, ln))


def p_exempt(rec, contig, ln=None):
    """a reference C in the last or the last-but-one column of the walk: the no-gap branch reads the flank (tag.rs:270, 332)"""
    return any(ex for _, ex, _, _ in c_columns(rec, contig, ln))


def p_runs_out(rec, contig, ln=None):
    """the look-ahead of tag.rs:281-292 leaves its loop by `break`: fewer than three characters collected"""
    return any(gap and not ex and len(ctx) < 3 for _, ex, gap, ctx in c_columns(rec, contig, ln))


def p_no_letter(rec, contig, ln=None):
    """a full three-character context without N or - that is no CG, CHG or CHH: an IUPAC code in it, nothing is pushed"""
    return any(len(ctx) == 3 and ctx[1] != "G" and not set(ctx) & set("N-") and set(ctx[1:]) - set("ACGT")
               and not (ctx[1] in "ATC" and ctx[2] in "ACGT") for _, _, _, ctx in c_columns(rec, contig, ln))


def p_ignored_ops(rec, contig, ln=None):
    return bool(_ops(rec) & set("SN=XHP")) or _ops(rec) == {"I"}


def p_complement(rec, contig, ln=None):
    """a character outside the complement table in SEQ or in the reference window (a panic only under a reverse complement)"""
    rg = columns(rec, contig, ln, raw=True)                 # what reverse_complement() would be handed: all but the last two columns
    return rg is not None and any(ord(x) not in COMP_OK for x in rg[0][:-2] + rg[1][:-2])


def p_short_seq(rec, contig, ln=None):
    return _short(rec)


CLASSES = {
    "plain_m": p_plain_m, "orientation": p_orientation, "gap_lookahead": p_gap_lookahead, "insertion": p_insertion,
    "exempt_index": p_exempt, "lookahead_runs_out": p_runs_out, "no_letter_pushed": p_no_letter, "ignored_ops": p_ignored_ops,
    "complement_panic": p_complement, "short_seq": p_short_seq,
}
# the enumeration writes SEQ from the contig (no '=') over a contig of table characters, with SEQ as long as the CIGAR says:
# these two classes are carried by the hand cases alone
NOT_ENUMERATED = ("complement_panic", "short_seq")
