"""Reading BGZF by hand, for the tests of the device's write side (`tag --output-format bam`, mth_bgzf_deflate): the framing of
every block is checked field by field, the payload is inflated with Python's zlib -- not with the project's inflater -- and the
DEFLATE block header can be taken apart far enough to see which code lengths a dynamic block declares."""
import heapq
import struct
import zlib

MAX_BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Block:
    __slots__ = ("off", "size", "payload", "raw", "btype")


def blocks(data, keep_eof=False):
    """-> [Block] of a BGZF stream; asserts magic 1f 8b 08 04, XLEN 6, BC/2/BSIZE, BSIZE + 1 = distance to the next block,
    ISIZE <= 0xff00, and CRC32 / ISIZE equal to what zlib computes from the inflated payload"""
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04", "gzip magic / CM / FLG.FEXTRA at %d" % p
        assert struct.unpack_from("<H", data, p + 10)[0] == 6, "XLEN at %d" % p
        assert data[p + 12:p + 16] == b"BC\x02\x00", "BC subfield at %d" % p
        size = struct.unpack_from("<H", data, p + 16)[0] + 1
        assert size >= 26 and p + size <= len(data), "BSIZE at %d" % p
        b = Block()
        b.off, b.size, b.payload = p, size, data[p + 18:p + size - 8]
        d = zlib.decompressobj(-15)
        b.raw = d.decompress(b.payload)
        assert d.eof and not d.unused_data, "payload of the block at %d is not exactly one DEFLATE stream" % p
        crc, isize = struct.unpack_from("<II", data, p + size - 8)
        assert isize == len(b.raw) and isize <= MAX_BLOCK, "ISIZE at %d" % p
        assert crc == zlib.crc32(b.raw), "CRC32 at %d" % p
        b.btype = (b.payload[0] >> 1) & 3
        assert b.payload[0] & 1, "BFINAL: one DEFLATE block per BGZF block"
        out.append(b)
        p += size
    if not keep_eof and out and data.endswith(EOF_BLOCK):
        out.pop()
    return out


def table(bl):
    """(coff, csize, isize) of the blocks, as Engine.bgzf_inflate / bgzf_decode take them"""
    return [b.off + 18 for b in bl], [len(b.payload) for b in bl], [len(b.raw) for b in bl]


def zlib1_size(raw):
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    return len(z.compress(raw) + z.flush())


class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def dynamic_header(payload):
    """the code lengths a BTYPE 10 block declares: (literal/length lengths [HLIT], distance lengths [HDIST], code-length-code
    lengths [19], the HLIT + HDIST code-length symbols as sent)"""
    b = _Bits(payload)
    assert b.get(1) == 1 and b.get(2) == 2
    hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = b.get(3)
    # canonical code of the code-length code
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    sent, lens = [], []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while True:
            c = (c << 1) | b.get(1); n += 1
            assert n <= 7
            if (n, c) in codes:
                break
        s = codes[(n, c)]
        sent.append(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.get(2))
        elif s == 17:
            lens += [0] * (3 + b.get(3))
        else:
            lens += [0] * (11 + b.get(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:], cl, sent


def huffman_depth(freqs):
    """depth of the deepest leaf of an (unlimited) Huffman tree over the non-zero frequencies; ties merge the shallower trees
    first, so the figure is the smallest depth a Huffman tree of these weights can have"""
    h = [(f, 0) for f in freqs if f > 0]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def kraft(lens):
    """sum of 2^-len over the used symbols, in units of 2^-15 (a complete code: 32768)"""
    return sum(1 << (15 - n) for n in lens if n)
