"""Writers for the FASTA tests: FASTA text with a chosen line layout (+ .fai), a BGZF writer that cuts its payloads where the
caller says, and the shared cases of tests/test_fasta_inputs.py (CPU: the inputs are what they are meant to be) and
tests/test_gpu_fasta.py (the device route over them)."""
import struct
import zlib

import numpy as np

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def fasta_text(contigs, width=60, eol=b"\n", final_newline=True):
    """contigs: [(name, bases)] or [(name, bases, width)] -> (the file's bytes, .fai rows [(name, length, offset, line_bases,
    line_width)]).  A contig of length 0 is its header line alone; the last line of the file loses its line end when
    final_newline is False."""
    out = bytearray()
    rows = []
    for c in contigs:
        name, seq = c[0], bytes(c[1])
        w = c[2] if len(c) > 2 else width
        out += b">" + name.encode() + eol
        rows.append((name, len(seq), len(out), w, w + len(eol)))
        for i in range(0, len(seq), w):
            out += seq[i:i + w] + eol
    if not final_newline and out.endswith(eol):
        del out[len(out) - len(eol):]
    return bytes(out), rows


def fai_text(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\n" % r for r in rows)


def write_fasta(path, contigs, width=60, eol=b"\n", final_newline=True, with_fai=True):
    text, rows = fasta_text(contigs, width, eol, final_newline)
    with open(path, "wb") as fh:
        fh.write(text)
    if with_fai:
        with open(str(path) + ".fai", "w") as fh:
            fh.write(fai_text(rows))
    return text, rows


def bgzf_block(payload, level=6, fixed=False):
    """one BGZF block (SAM spec 4.1) of one raw-DEFLATE stream: level 0 gives stored blocks, fixed=True fixed-Huffman ones,
    level 6 over enough text dynamic ones"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_FIXED) if fixed else zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    assert len(payload) <= 65536 and len(comp) + 26 <= 65536
    head = struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25)
    return head + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


def bgzf_bytes(data, cuts, kinds=("dynamic",), empty_after=()):
    """data cut into payloads of the sizes `cuts` gives (the list is cycled; the last payload is what is left), block k compressed
    as kinds[k % len(kinds)] ('stored' | 'fixed' | 'dynamic'); an empty block follows every block whose number is in
    empty_after; the 28-byte EOF block ends the file.  -> (file bytes, [(payload start, payload end)] per data block)"""
    out = bytearray()
    spans = []
    pos = k = 0
    while pos < len(data):
        n = min(int(cuts[k % len(cuts)]), len(data) - pos)
        assert n > 0
        kind = kinds[k % len(kinds)]
        out += bgzf_block(data[pos:pos + n], level=0 if kind == "stored" else 6, fixed=kind == "fixed")
        spans.append((pos, pos + n))
        if k in empty_after:
            out += bgzf_block(b"")
        pos += n
        k += 1
    out += EOF_BLOCK
    return bytes(out), spans


def bgzf_table(blob):
    """the block table of a BGZF file as the engine takes it: payload offset, payload bytes, inflated bytes of every block that
    holds data -> (coff, csize, isize) numpy arrays"""
    coff, csize, isize = [], [], []
    o = 0
    while o < len(blob):
        assert blob[o:o + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", blob, o + 10)[0]
        assert blob[o + 12:o + 16] == b"BC\x02\x00"
        total = struct.unpack_from("<H", blob, o + 16)[0] + 1
        n = struct.unpack_from("<I", blob, o + total - 4)[0]
        if n:
            coff.append(o + 12 + xlen); csize.append(total - 12 - xlen - 8); isize.append(n)
        o += total
    return np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32)


def first_btype(blob, coff):
    """BTYPE of the first DEFLATE block of the payload at coff: 0 stored, 1 fixed, 2 dynamic (RFC 1951 3.2.3)"""
    return (blob[int(coff)] >> 1) & 3


def want_bases(seq, ln):
    """faidx_fetch_seq(name, 0, LN): the bases [0, LN] clipped to the sequence"""
    return bytes(seq[:max(0, ln + 1)])


# ---- the shared cases ----------------------------------------------------------------------------------------------------
def _rng_seq(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, np.uint8), size=n).tobytes() if n else b""


IUPAC = b"ACGTNacgtnRYKMSWBDHVrykmswbdhv"


def cases():
    """name -> dict(contigs: the FASTA's [(name, bases, width)], in file order; header: [(name, LN)] in tid order -- not the
    file's order, and not all of its contigs; eol, final_newline; cuts / kinds / empty_after: how the .fa.gz twin is cut).
    Contigs are at most a few tens of kb."""
    rng = np.random.default_rng(20)
    out = {}
    for w in (1, 15, 16, 17, 60, 61, 64):
        # lengths: 0, 1, an exact multiple of the width, one more than a multiple, odd ones (every later contig of the genome starts
        # at an unaligned address), and lower case / IUPAC letters, which are kept as they are
        lens = [("empty", 0), ("one", 1), ("mult", 7 * w), ("mult1", 9 * w + 1), ("odd", 1237 if w > 1 else 131), ("iupac", 333 if w > 1 else 77)]
        contigs = [(n, _rng_seq(rng, k, IUPAC if n == "iupac" else b"ACGT"), w) for n, k in lens]
        contigs.insert(2, ("decoy", _rng_seq(rng, 501 if w > 1 else 50), w))                    # not in the header
        header = [("odd", 1237 if w > 1 else 131), ("iupac", 400), ("empty", 0), ("mult1", 9 * w + 1), ("one", 1), ("mult", 3 * w)]   # iupac: LN past the sequence; mult: LN + 1 clips
        out["w%d" % w] = dict(contigs=contigs, header=header, eol=b"\n", final_newline=True, cuts=[997, 64, 1500], kinds=("dynamic", "stored", "fixed"), empty_after=(1,))
    big = _rng_seq(rng, 30011)
    out["single_line"] = dict(contigs=[("a", _rng_seq(rng, 4099), 4099), ("b", big, 30011)], header=[("b", 30011), ("a", 4099)], eol=b"\n", final_newline=True,
                              cuts=[9000], kinds=("dynamic",), empty_after=())
    out["crlf"] = dict(contigs=[("a", _rng_seq(rng, 2501), 60), ("b", _rng_seq(rng, 1999), 70)], header=[("a", 2501), ("b", 1000)], eol=b"\r\n", final_newline=True,
                       cuts=[61, 62, 63, 500], kinds=("fixed", "dynamic"), empty_after=(0, 3))
    out["no_final_newline"] = dict(contigs=[("a", _rng_seq(rng, 777), 60), ("b", _rng_seq(rng, 1201), 60)], header=[("a", 777), ("b", 1201)], eol=b"\n", final_newline=False,
                                   cuts=[400], kinds=("stored",), empty_after=())
    # about 30 kB of random ACGT lines at level 6: dynamic blocks; cut so that one block starts on a line feed, one on the first base
    # of a line, a '>' line is split across two blocks, and contig "long" covers more than three blocks
    contigs = [("short", _rng_seq(rng, 1000), 60), ("long", _rng_seq(rng, 29501), 60)]
    text, rows = fasta_text(contigs, 60)
    off_long = rows[1][2]
    hdr_long = off_long - len(b">long\n")
    cuts = [60 + len(b">short\n"),                          # block 1 starts on the line feed that ends the first line
            1,                                              # block 2 starts on the first base of the second line
            hdr_long + 3 - (60 + len(b">short\n") + 1),     # block 3 starts inside ">long"
            7000, 7000, 7000, 7000, 7000]
    out["block_edges"] = dict(contigs=contigs, header=[("long", 29501), ("short", 1000)], eol=b"\n", final_newline=True, cuts=cuts, kinds=("dynamic",), empty_after=(4,))
    return out


def build(case, d, name):
    """write case's .fa (+ .fai) and .fa.gz (+ .fai) under d -> dict(fa, gz, text, rows, blob, spans)"""
    fa, gz = str(d / (name + ".fa")), str(d / (name + ".fa.gz"))
    text, rows = write_fasta(fa, case["contigs"], eol=case["eol"], final_newline=case["final_newline"])
    blob, spans = bgzf_bytes(text, case["cuts"], case["kinds"], case["empty_after"])
    with open(gz, "wb") as fh:
        fh.write(blob)
    with open(gz + ".fai", "w") as fh:
        fh.write(fai_text(rows))
    return dict(fa=fa, gz=gz, text=text, rows=rows, blob=blob, spans=spans)
