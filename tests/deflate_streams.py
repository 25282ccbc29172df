"""DEFLATE streams written bit by bit (RFC 1951), at the level a decoder sees them, and two corpora of them for the device inflater
(k_inflate, metheor_amd/csrc/mth_inflate.hip): VALID -- legal streams that zlib's deflate never writes but other encoders do, at the
smallest shapes at which a decoder can go wrong -- and INVALID -- one stream per rejection the kernel has.  tests/
test_deflate_streams.py holds every case against zlib's inflate on the CPU, tests/test_gpu_inflate_streams.py runs them on the device.

A member is a list of blocks: stored(bytes), fixed(tokens), dynamic(tokens, ll_lens, d_lens, header).  A token is a literal (an int),
a match M(length, distance[, lsym]) or, for the invalid corpus only, a raw symbol / raw bits.  build() returns the payload, the bytes
it encodes -- from executing the tokens here, not from a decoder -- and what it wrote per block (bit positions, code lengths, the
code-length symbols of a dynamic header with the index each starts at, literal runs, matches): the predicates of the cases read that.

Pure Python + numpy; imports nothing of the project."""
import bisect
import heapq
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32                       # 30 and 31 have codes and no meaning (RFC 1951 3.2.6)
LROOT, DROOT = 10, 9                     # direct-lookup bits of k_inflate's two tables
FAST_ROOM = 72                           # literal_run only runs while pos + 72 <= isize


# ---- tokens ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class M:
    """a match; lsym: the length symbol to write it with (258 is 285, or 284 + 31); unchecked: may reach before the member's start"""
    length: int
    dist: int
    lsym: int = None
    unchecked: bool = False


@dataclass(frozen=True)
class RawLL:
    """the code of a literal/length symbol and nothing else (invalid corpus)"""
    sym: int


@dataclass(frozen=True)
class RawD:
    """the code of a distance symbol and nothing else (invalid corpus)"""
    sym: int


@dataclass(frozen=True)
class RawBits:
    value: int
    n: int


def length_symbol(length, lsym=None):
    i = (28 if length == 258 else bisect.bisect_right(LBASE, length, 0, 28) - 1) if lsym is None else lsym - 257
    x = length - LBASE[i]
    assert 0 <= x < (1 << LEXTRA[i]), (length, lsym)
    return 257 + i, x, LEXTRA[i]


def dist_symbol(dist):
    i = bisect.bisect_right(DBASE, dist) - 1
    x = dist - DBASE[i]
    assert 1 <= dist <= 32768 and 0 <= x < (1 << DEXTRA[i]), dist
    return i, x, DEXTRA[i]


# ---- codes ----------------------------------------------------------------------------------------------------------------------
def canonical(lens):
    """RFC 1951 3.2.2; an over-subscribed set gets its codes cut to their length (only the invalid corpus has one)"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
    return codes


def kraft(lens):
    """-1 incomplete, 0 complete, 1 over-subscribed"""
    s = sum(1 << (15 - l) for l in lens if l)
    return (s > 1 << 15) - (s < 1 << 15)


def huff_lens(freq, n, limit):
    """Huffman code lengths of the symbols with freq > 0, none longer than `limit` (the weights are halved until it holds); a lone
    symbol gets one bit"""
    syms = [s for s in range(n) if freq.get(s, 0) > 0]
    lens = [0] * n
    if len(syms) == 1:
        lens[syms[0]] = 1
    if len(syms) < 2:
        return lens
    w = {s: freq[s] for s in syms}
    while True:
        heap = [(w[s], s, (s,)) for s in syms]
        heapq.heapify(heap)
        depth = dict.fromkeys(syms, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            for s in syms:
                lens[s] = depth[s]
            return lens
        w = {s: max(1, v // 2) for s, v in w.items()}


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):                         # a field: least significant bit first
        assert 0 <= v < (1 << n) or n == 0, (v, n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, l):                         # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % l)[::-1], 2), l)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


# ---- blocks ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Header:
    """how a dynamic block sends its code lengths.  hclen: "min" or 19.  rep16 / rep17 / rep18: where a run allows it, send it with
    that symbol and exactly that repeat count (None: never); zero16: a 16 may repeat the zero a 17 / 18 left; cross: the literal/length
    and the distance lengths are scanned as one sequence, so a repeat may run across HLIT; pad: HLIT 286 and HDIST 30, trailing zeros
    sent; cl_lens: the code-length code's own 19 lengths (else Huffman, <= 7); ops: the symbols themselves, (sym, extra value) or
    (-1, value, n bits), nothing derived (invalid corpus)"""
    hclen: object = "min"
    rep16: int = None
    rep17: int = None
    rep18: int = None
    zero16: bool = False
    cross: bool = False
    pad: bool = False
    cl_lens: list = None
    ops: list = None


@dataclass
class Stored:
    data: bytes
    final: bool = None
    nlen_field: int = None               # NLEN as written (invalid corpus)
    body: bytes = None                   # the bytes that actually follow LEN / NLEN (invalid corpus: fewer than LEN)


@dataclass
class Fixed:
    tokens: list
    final: bool = None
    eob: bool = True


@dataclass
class Dynamic:
    tokens: list
    ll_lens: object = None               # list, or {symbol: length}
    d_lens: object = None
    header: Header = field(default_factory=Header)
    final: bool = None
    eob: bool = True


@dataclass
class Raw:
    """BFINAL, then these (value, n bits) fields, BTYPE first (invalid corpus)"""
    fields: list
    final: bool = None


def stored(data, **kw):
    return Stored(bytes(data), **kw)


def fixed(tokens, **kw):
    return Fixed(list(tokens), **kw)


def dynamic(tokens, ll_lens=None, d_lens=None, header=None, **kw):
    return Dynamic(list(tokens), ll_lens, d_lens, header or Header(), **kw)


def _as_list(lens, n):
    if lens is None:
        return None
    if isinstance(lens, dict):
        out = [0] * (max(lens) + 1)
        for s, l in lens.items():
            out[s] = l
        lens = out
    return list(lens) + [0] * max(0, n - len(lens))


def _lower(tokens, eob):
    """tokens -> what is written: ("L" | "D", symbol, extra value, extra bits) and ("B", value, n)"""
    items = []
    for t in tokens:
        if isinstance(t, M):
            items.append(("L",) + length_symbol(t.length, t.lsym))
            items.append(("D",) + dist_symbol(t.dist))
        elif isinstance(t, RawLL):
            items.append(("L", t.sym, 0, 0))
        elif isinstance(t, RawD):
            items.append(("D", t.sym, 0, 0))
        elif isinstance(t, RawBits):
            items.append(("B", t.value, t.n, 0))
        else:
            items.append(("L", int(t), 0, 0))
    if eob:
        items.append(("L", 256, 0, 0))
    return items


def _execute(tokens, out, info, st):
    """what the tokens mean, appended to the member's bytes; a raw token, or a match that reaches too far, ends the meaning"""
    runs, matches, run0 = info["lit_runs"], info["matches"], None
    for t in tokens:
        if st["broken"]:
            break
        if isinstance(t, M):
            if run0 is not None:
                runs.append((run0, len(out) - run0))
                run0 = None
            if t.dist > len(out):
                assert t.unchecked, t
                st["broken"] = True
                break
            matches.append((len(out), t.length, t.dist, length_symbol(t.length, t.lsym)[0], dist_symbol(t.dist)[0]))
            if t.dist >= t.length:
                s = len(out) - t.dist
                out += out[s:s + t.length]
            else:
                seg = bytes(out[-t.dist:])
                out += (seg * (t.length // t.dist + 1))[:t.length]
        elif isinstance(t, (RawLL, RawD, RawBits)):
            st["broken"] = True
        else:
            if run0 is None:
                run0 = len(out)
            out.append(int(t))
    if run0 is not None:
        runs.append((run0, len(out) - run0))


def _rle_ops(seq, hlit, h):
    ops = []
    for a, b in ([(0, len(seq))] if h.cross else [(0, hlit), (hlit, len(seq))]):
        i = a
        while i < b:
            v, r = seq[i], 1
            while i + r < b and seq[i + r] == v:
                r += 1
            last = ops[-1][0] if ops else None
            if i > a and seq[i - 1] == v and h.rep16 and r >= h.rep16 and (v != 0 or (h.zero16 and last in (17, 18))):
                ops.append((16, h.rep16 - 3)); i += h.rep16
            elif v == 0 and h.rep18 and r >= h.rep18:
                ops.append((18, h.rep18 - 11)); i += h.rep18
            elif v == 0 and h.rep17 and r >= h.rep17:
                ops.append((17, h.rep17 - 3)); i += h.rep17
            else:
                ops.append((v, 0)); i += 1
    return ops


def _write_symbols(w, items, ll, d, info):
    llc, dc = canonical(ll), canonical(d)
    for kind, a, b, c in items:
        if kind == "B":
            w.bits(a, b)
            continue
        lens, codes, used = (ll, llc, info["used_ll"]) if kind == "L" else (d, dc, info["used_d"])
        assert a < len(lens) and lens[a], "%s symbol %d has no code" % (kind, a)
        w.code(codes[a], lens[a])
        w.bits(b, c)
        used.add(a)


@dataclass
class Member:
    payload: bytes
    data: bytes
    blocks: list                          # per block: what was written


def build(blocks):
    """-> Member(payload, the bytes it encodes, per-block info).  BFINAL: per block, or (None) set on the last one."""
    w, out, infos, st = BitWriter(), bytearray(), [], {"broken": False}
    for k, b in enumerate(blocks):
        final = (k == len(blocks) - 1) if b.final is None else b.final
        info = dict(kind=type(b).__name__.lower(), final=final, start_bit=w.bitpos, start_out=len(out), lit_runs=[], matches=[],
                    used_ll=set(), used_d=set())
        w.bits(int(final), 1)
        if isinstance(b, Raw):
            for v, n in b.fields:
                w.bits(v, n)
            info["fields"] = list(b.fields)
            st["broken"] = True
        elif isinstance(b, Stored):
            w.bits(0, 2)
            w.align()
            n = len(b.data)
            assert n <= 0xffff
            info.update(len=n, nlen=(~n & 0xffff) if b.nlen_field is None else b.nlen_field,
                        body=len(b.data if b.body is None else b.body))
            w.bits(n, 16)
            w.bits(info["nlen"], 16)
            w.raw(b.data if b.body is None else b.body)
            if not st["broken"]:
                out += b.data
            if info["nlen"] != (~n & 0xffff) or info["body"] != n:
                st["broken"] = True
        else:
            items = _lower(b.tokens, b.eob)
            if isinstance(b, Fixed):
                w.bits(1, 2)
                ll, d = FIXED_LL, FIXED_D
            else:
                w.bits(2, 2)
                fl, fd = {}, {}
                for kind, a, _, _ in items:
                    if kind != "B":
                        f = fl if kind == "L" else fd
                        f[a] = f.get(a, 0) + 1
                ll = _as_list(b.ll_lens, 257) or huff_lens(fl, 286, 15)
                d = _as_list(b.d_lens, 1) or huff_lens(fd, 30, 15)
                h = b.header
                hlit = 286 if h.pad else max(257, max((s + 1 for s, l in enumerate(ll) if l), default=0))
                hdist = 30 if h.pad else max(1, max((s + 1 for s, l in enumerate(d) if l), default=0))
                seq = (ll + [0] * 286)[:hlit] + (d + [0] * 30)[:hdist]
                ops = list(h.ops) if h.ops is not None else _rle_ops(seq, hlit, h)
                if h.cl_lens is not None:
                    cl = _as_list(h.cl_lens, 19)
                else:
                    fc = {}
                    for op in ops:
                        if op[0] >= 0:
                            fc[op[0]] = fc.get(op[0], 0) + 1
                    if len(fc) == 1:                       # zlib wants this code complete: a second one-bit code, unused
                        fc[0 if 0 not in fc else 1] = 1
                    cl = huff_lens(fc, 19, 7)
                hclen = 19 if h.hclen == 19 else max(4, max(i + 1 for i in range(19) if cl[CLEN_ORDER[i]]))
                w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
                for i in range(hclen):
                    w.bits(cl[CLEN_ORDER[i]], 3)
                clc, at, placed = canonical(cl), 0, []
                for op in ops:
                    if op[0] < 0:
                        w.bits(op[1], op[2])
                        st["broken"] = True
                        continue
                    assert cl[op[0]], "code-length symbol %d has no code" % op[0]
                    w.code(clc[op[0]], cl[op[0]])
                    n = 1
                    if op[0] == 16:
                        w.bits(op[1], 2); n = 3 + op[1]
                    elif op[0] == 17:
                        w.bits(op[1], 3); n = 3 + op[1]
                    elif op[0] == 18:
                        w.bits(op[1], 7); n = 11 + op[1]
                    placed.append((op[0], at, n))          # (symbol, index of the first length it sets, how many)
                    at += n
                if h.ops is None:
                    assert at == hlit + hdist
                info.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, ops=placed, ll_lens=ll, d_lens=d)
                if at != hlit + hdist or kraft(cl) > 0 or kraft(ll) > 0 or kraft(d) > 0 or not ll[256] or (placed and placed[0][0] == 16):
                    st["broken"] = True
            info["sym_bit"] = w.bitpos
            if not st["broken"]:
                _execute(b.tokens, out, info, st)
            _write_symbols(w, items, ll, d, info)
            if not b.eob:
                st["broken"] = True
        info["end_bit"], info["end_out"] = w.bitpos, len(out)
        infos.append(info)
    return Member(w.getvalue(), bytes(out), infos)


# ---- framing --------------------------------------------------------------------------------------------------------------------
def frame(members, slack=None):
    """members (anything with .payload and .data; .isize / .csize / .crc, where set, are what the table and the trailer declare),
    each followed by CRC32 + ISIZE and with slack[i] (0..3) bytes in front; by default the slack that puts member i's payload at a
    file offset = its .phase, or i, mod 4 -- every phase of the bit reader's seek -> (file bytes, coff, csize, isize, expected bytes)"""
    out, coff, csize, isize, want = bytearray(), [], [], [], []
    for i, m in enumerate(members):
        ph = getattr(m, "phase", None)
        s = slack[i] if slack is not None else ((i if ph is None else ph) - len(out)) % 4
        assert 0 <= s <= 3
        out += b"\xa5" * s
        n = len(m.data) if getattr(m, "isize", None) is None else m.isize
        crc = zlib.crc32(m.data) & 0xffffffff if getattr(m, "crc", None) is None else m.crc
        coff.append(len(out)); isize.append(n); want.append(m.data)
        csize.append(len(m.payload) if getattr(m, "csize", None) is None else m.csize)
        out += m.payload + struct.pack("<II", crc, n & 0xffffffff)
    return bytes(out), np.array(coff, np.uint64), np.array(csize, np.uint32), np.array(isize, np.uint32), b"".join(want)


def zlib_verdict(payload):
    """the reference: zlib's raw inflate -> dict(out, eof, unused, error)"""
    do = zlib.decompressobj(-15)
    try:
        out = do.decompress(payload)
        return dict(out=out, eof=do.eof, unused=do.unused_data, error=None)
    except zlib.error as e:
        return dict(out=None, eof=False, unused=b"", error=str(e))


# ---- the corpora ----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str
    what: str                              # what makes it the case, in words; pred states it over the stream
    payload: bytes
    data: bytes
    blocks: list
    pred: object
    phase: int = None
    # INVALID only
    isize: int = None                      # declared, where it is not len(data)
    csize: int = None
    crc: int = None
    last: bool = False                     # goes last in the file, so that reads past it meet the zero padding
    rejects: str = ""                      # the line of mth_inflate.hip that rejects it
    zlib_raises: bool = True               # else: wrong only against its table, and `verdict` is how zlib's view differs from it
    verdict: object = None


VALID, INVALID = [], []


def _valid(group, name, what, blocks, pred, phase=None):
    m = blocks if isinstance(blocks, Member) else build(blocks)
    VALID.append(Case(name, group, what, m.payload, m.data, m.blocks, pred, phase))


def _invalid(name, what, blocks, pred, rejects, **kw):
    m = blocks if isinstance(blocks, Member) else build(blocks)
    INVALID.append(Case(name, "invalid", what, m.payload, m.data, m.blocks, pred, rejects=rejects, **kw))


def _text(n, seed, alphabet=b"ACGTNacgt.,zZxh"):
    """n reproducible bytes over an alphabet, skewed so that code lengths differ"""
    x, out = 12345 + seed * 7919, bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        r = (x >> 8) % 64
        out.append(alphabet[min(len(alphabet) - 1, r.bit_length() * len(alphabet) // 7)] if r else alphabet[(x >> 16) % len(alphabet)])
    return bytes(out)


def _all_matches(c):
    return [m for b in c.blocks for m in b["matches"]]


def _kinds(c):
    return [b["kind"] for b in c.blocks]


def _fill():
    hello = list(b"hello, deflate")
    # ---- block structure --------------------------------------------------------------------------------------------------------
    _valid("structure", "stored then fixed", "a non-final stored block, then a final fixed one",
           [stored(b"stored bytes first"), fixed(hello + [M(6, 20)])],
           lambda c: _kinds(c) == ["stored", "fixed"] and [b["final"] for b in c.blocks] == [False, True])
    _valid("structure", "fixed then stored", "a non-final fixed block, then a final stored one",
           [fixed(hello), stored(b"stored bytes last")],
           lambda c: _kinds(c) == ["fixed", "stored"] and [b["final"] for b in c.blocks] == [False, True])
    for k in range(8):
        # a fixed block is 3 + 7 bits and 8 per literal below 144, 9 per literal from 144 on: j of those move its end by j bits
        j = (k - 2) % 8
        _valid("structure", "empty stored after bit %d" % k,
               "an empty stored block between two Huffman blocks, the first ending at bit %d of its byte" % k,
               [fixed(hello + [200 + i for i in range(j)]), stored(b""), dynamic(list(b"after the flush ") + [M(5, 20 + j), M(9, 3)])],
               lambda c, k=k: _kinds(c) == ["fixed", "stored", "dynamic"] and c.blocks[0]["end_bit"] % 8 == k and c.blocks[1]["len"] == 0
               and c.blocks[2]["matches"][0][0] - c.blocks[2]["matches"][0][2] < c.blocks[0]["end_out"])
    _valid("structure", "empty stored block last", "an empty stored block as the final block",
           [fixed(hello), stored(b"")], lambda c: c.blocks[-1]["kind"] == "stored" and c.blocks[-1]["len"] == 0 and c.blocks[-1]["final"])
    _valid("structure", "fixed block of end-of-block only", "a final fixed block that holds only the end-of-block code, after a stored block",
           [stored(b"all there is"), fixed([])],
           lambda c: c.blocks[1]["kind"] == "fixed" and c.blocks[1]["final"] and c.blocks[1]["end_bit"] - c.blocks[1]["start_bit"] == 10)
    _valid("structure", "empty member, fixed", "a member of nothing but a fixed block's end-of-block code: ISIZE 0",
           [fixed([])], lambda c: len(c.data) == 0 and len(c.payload) == 2)
    a, b, d = list(_text(40, 1, b"abcdefgh")), list(_text(30, 2, b"0123456789")), list(_text(5, 3, b"QRSTUVWXYZ"))
    _valid("structure", "three dynamic blocks", "three dynamic blocks with different codes; matches of the third reach into the first",
           [dynamic(a), dynamic(b + [M(4, 12)]), dynamic(d + [M(20, 70), M(33, 95), M(3, 1)])],
           lambda c: _kinds(c) == ["dynamic"] * 3 and len({tuple(x["ll_lens"]) for x in c.blocks}) == 3
           and sum(p - dist < c.blocks[0]["end_out"] for p, _, dist, _, _ in c.blocks[2]["matches"]) >= 2)
    _valid("structure", "matches across a stored block", "dynamic, stored, dynamic: matches of the last reach across the stored block",
           [dynamic(a), stored(bytes(b)), dynamic(d + [M(20, 70), M(40, 60)])],
           lambda c: _kinds(c) == ["dynamic", "stored", "dynamic"]
           and all(p - dist < c.blocks[0]["end_out"] for p, _, dist, _, _ in c.blocks[2]["matches"])
           and c.blocks[2]["matches"][1][0] - 60 + 40 > c.blocks[1]["start_out"])
    big = _text(65535, 4)
    _valid("structure", "stored 65535 + one literal", "a stored block of 65535 bytes, then a one-literal block: ISIZE 65536",
           [stored(big), fixed([33])], lambda c: c.blocks[0]["len"] == 65535 and len(c.data) == 65536 and c.blocks[1]["lit_runs"] == [(65535, 1)])
    for ph in range(4):
        _valid("structure", "payload at offset %d mod 4" % ph, "a member whose payload begins at a file offset = %d (mod 4)" % ph,
               [dynamic(hello + [M(4, 7)] + hello)], lambda c, ph=ph: c.phase == ph, phase=ph)

    # ---- inflated sizes ---------------------------------------------------------------------------------------------------------
    for n in (65279, 65280, 65281, 65498, 65535, 65536):
        data = (_text(3000, n) * 22)[:n]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = co.compress(data) + co.flush()
        VALID.append(Case("zlib, ISIZE %d" % n, "sizes", "zlib's stream of %d compressible bytes" % n, z, data, [],
                          lambda c, n=n: len(c.data) == n and len(c.payload) < n // 3))
        toks, pos, x = list(_text(300, n + 1)), 300, n
        while n - pos > 400:
            x = (x * 1103515245 + 12345) & 0x7fffffff
            ln, dist = 3 + (x >> 4) % 256, 1 + (x >> 12) % min(pos, 32768)
            toks.append(M(ln, dist)); pos += ln
            if (x >> 3) % 3 == 0:
                toks += list(_text(1 + x % 5, x)); pos += 1 + x % 5
        toks += list(_text(n - pos, n + 2))
        _valid("sizes", "built, ISIZE %d" % n, "one dynamic block of literals and matches that inflates to %d bytes" % n,
               [dynamic(toks)], lambda c, n=n: len(c.data) == n and len(c.blocks[0]["matches"]) > 100 and c.blocks[0]["lit_runs"][-1][1] > FAST_ROOM)

    # ---- long codes -------------------------------------------------------------------------------------------------------------
    # lengths 1, 2, ..., 14, 15, 15: complete, one symbol at every length on both sides of the direct table
    lits = list(b"etaoinshrdlu")                                     # lengths 1..12
    ll = {s: i + 1 for i, s in enumerate(lits)}
    ll.update({256: 13, 257: 14, ord("q"): 15, 285: 15})
    toks = lits * 3 + [M(3, 5), ord("q")] + lits + [M(258, 40), ord("q"), M(3, 1)] + lits[::-1] * 8
    _valid("long codes", "literal/length lengths 1..15", "a literal/length code with lengths 1, 2, ..., 14, 15, 15; every symbol used",
           [dynamic(toks, ll_lens=ll)],
           lambda c: sorted(l for l in c.blocks[0]["ll_lens"] if l) == list(range(1, 16)) + [15]
           and {c.blocks[0]["ll_lens"][s] for s in c.blocks[0]["used_ll"]} == set(range(1, 16))
           and len(c.blocks[0]["used_ll"]) == 16 and 1 < LROOT < 15)
    dl = [i + 1 for i in range(15)] + [15]                           # distance symbols 0..15
    toks = list(_text(300, 9))
    for k in range(3):
        for s in range(16):
            toks.append(M(3 + s + k, DBASE[s] + (k * 7) % (1 << DEXTRA[s])))
            toks += list(b"xy"[:k])
    _valid("long codes", "distance lengths 1..15", "a distance code with lengths 1, 2, ..., 14, 15, 15; every symbol used",
           [dynamic(toks, d_lens=dl)],
           lambda c: sorted(l for l in c.blocks[0]["d_lens"] if l) == list(range(1, 16)) + [15] and c.blocks[0]["used_d"] == set(range(16))
           and 1 < DROOT < 15)
    toks = list(range(256)) + [M(LBASE[i] + (1 << LEXTRA[i]) // 2, 1 + 7 * i, lsym=257 + i) for i in range(29)] + list(range(255, -1, -1))
    _valid("long codes", "all 286 symbols at 8-9 bits", "a literal/length code with all 286 symbols, 226 at 8 bits and 60 at 9; every symbol used",
           [dynamic(toks, ll_lens=[8] * 226 + [9] * 60)],
           lambda c: c.blocks[0]["hlit"] == 286 and all(l in (8, 9) for l in c.blocks[0]["ll_lens"]) and c.blocks[0]["used_ll"] == set(range(286)))
    cl = [0] * 19
    for s, l in ((18, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (6, 7)):
        cl[s] = l
    ll = {ord("a"): 1, ord("b"): 2, ord("c"): 3, ord("d"): 4, ord("e"): 5, 256: 6, 257: 6}
    _valid("long codes", "7-bit code-length codes", "a code-length code with lengths 1..7, 7; the 7-bit codes are used",
           [dynamic(list(b"abcdeabcaab") + [M(3, 2), M(3, 1)] + list(b"edcba"), ll_lens=ll, d_lens=[1, 1], header=Header(cl_lens=cl, rep18=11))],
           lambda c: max(c.blocks[0]["cl_lens"]) == 7 and {5, 6} <= {o[0] for o in c.blocks[0]["ops"]}
           and all(c.blocks[0]["cl_lens"][s] == 7 for s in (5, 6)))

    # ---- incomplete codes the decoder promises to accept ------------------------------------------------------------------------
    _valid("incomplete", "one distance code, used", "a distance code of one symbol of length 1, used",
           [dynamic(hello + [M(10, 1), 65, M(5, 1)])],
           lambda c: c.blocks[0]["d_lens"][:c.blocks[0]["hdist"]] == [1] and c.blocks[0]["used_d"] == {0} and kraft(c.blocks[0]["d_lens"]) < 0)
    _valid("incomplete", "no distance code", "no distance code at all (HDIST 1, length 0) in a literal-only block",
           [dynamic(hello * 3)], lambda c: c.blocks[0]["hdist"] == 1 and c.blocks[0]["d_lens"][0] == 0 and not c.blocks[0]["matches"])
    lone = lambda c, k: (sorted((s, l) for s, l in enumerate(c.blocks[k]["ll_lens"]) if l) == [(256, 1)] and c.blocks[k]["hdist"] == 1
                         and c.blocks[k]["d_lens"][0] == 0 and c.blocks[k]["end_out"] == c.blocks[k]["start_out"])
    _valid("incomplete", "lone end-of-block code", "a dynamic block whose only code is a one-bit end-of-block code: ISIZE 0",
           [dynamic([])], lambda c: lone(c, 0) and len(c.data) == 0)
    _valid("incomplete", "lone end-of-block code after data", "the same after a stored block",
           [stored(b"before"), dynamic([])], lambda c: lone(c, 1) and c.data == b"before")

    # ---- header encodings -------------------------------------------------------------------------------------------------------
    dense = list(range(256)) + [M(7, 100), M(30, 256)] + list(range(128))                  # long runs of equal lengths
    sparse = list(_text(60, 5, b"abcdefgh")) + [M(5, 9), M(12, 30)]                      # 97 and 151 zero lengths in a row
    ops_of = lambda c: {(s, n) for s, _, n in c.blocks[0]["ops"]}
    _valid("header", "HCLEN minimal", "HCLEN trimmed to its minimum", [dynamic(sparse, header=Header(rep18=138))],
           lambda c: c.blocks[0]["hclen"] < 19 and c.blocks[0]["cl_lens"][CLEN_ORDER[c.blocks[0]["hclen"] - 1]] != 0)
    _valid("header", "HCLEN 19", "HCLEN 19 with trailing zero lengths", [dynamic(sparse, header=Header(rep18=138, hclen=19))],
           lambda c: c.blocks[0]["hclen"] == 19 and c.blocks[0]["cl_lens"][15] == 0)
    for n in (3, 4, 5, 6):
        _valid("header", "16 x %d" % n, "symbol 16 with repeat count %d" % n, [dynamic(dense, header=Header(rep16=n))],
               lambda c, n=n: (16, n) in ops_of(c))
    for n in (3, 10):
        _valid("header", "17 x %d" % n, "symbol 17 with repeat count %d" % n, [dynamic(sparse, header=Header(rep17=n))],
               lambda c, n=n: (17, n) in ops_of(c))
    for n in (11, 138):
        _valid("header", "18 x %d" % n, "symbol 18 with repeat count %d" % n, [dynamic(sparse, header=Header(rep18=n))],
               lambda c, n=n: (18, n) in ops_of(c))
    after = lambda c, first: any(x[0] == first and y[0] == 16 for x, y in zip(c.blocks[0]["ops"], c.blocks[0]["ops"][1:]))
    _valid("header", "16 after 18", "symbol 16 directly after an 18 run (repeating zero)",
           [dynamic(sparse, header=Header(rep18=11, rep16=3, zero16=True))], lambda c: after(c, 18))
    _valid("header", "16 after 17", "symbol 16 directly after a 17 run (repeating zero)",
           [dynamic(sparse, header=Header(rep17=4, rep16=6, zero16=True))], lambda c: after(c, 17))
    crosses = lambda c, sym: any(s == sym and at < c.blocks[0]["hlit"] < at + n for s, at, n in c.blocks[0]["ops"])
    ll = {s: 3 for s in (65, 66, 67, 68, 253, 254, 255, 256)}
    _valid("header", "16 across HLIT", "a 16 run that starts before index HLIT and ends after it",
           [dynamic([65, 66, 253, 67, 254, 68, 255, 65], ll_lens=ll, d_lens=[3] * 8, header=Header(rep16=6, rep18=138, cross=True))],
           lambda c: crosses(c, 16))
    ll = {s: 3 for s in (65, 66, 67, 68, 69, 70, 256, 257)}
    _valid("header", "18 across HLIT", "an 18 run that starts before index HLIT (286, padded) and ends after it",
           [dynamic([65, 66, 67, 68, 69, 70] * 3 + [M(3, 5), M(3, 16), M(3, 9)], ll_lens=ll, d_lens=[0, 0, 0, 0, 2, 2, 2, 2],
                    header=Header(rep18=16, cross=True, pad=True))],
           lambda c: crosses(c, 18) and c.blocks[0]["hlit"] == 286)
    _valid("header", "HLIT 286, HDIST 30", "HLIT 286 and HDIST 30 with trailing zero lengths",
           [dynamic(sparse, header=Header(pad=True, rep17=10))],
           lambda c: c.blocks[0]["hlit"] == 286 and c.blocks[0]["hdist"] == 30 and c.blocks[0]["ll_lens"][285] == 0
           and c.blocks[0]["d_lens"][29:30] in ([0], []))

    # ---- symbols ----------------------------------------------------------------------------------------------------------------
    every = [M(n, 1 + (n * 5) % 19) for n in range(3, 259)] + [M(258, 7, lsym=284)]
    want = {(length_symbol(n)[0], n) for n in range(3, 259)} | {(284, 258)}
    for kind, mk in (("dynamic", dynamic), ("fixed", fixed)):
        _valid("symbols", "every length, " + kind, "every length 3..258 in a %s block, 258 both as symbol 285 and as 284 + 31" % kind,
               [mk(list(_text(20, 6)) + every)],
               lambda c, want=want: {(ls, ln) for _, ln, _, ls, _ in c.blocks[0]["matches"]} == want)
    hist = _text(32768, 7)
    far = [M(3, 32768)] + [M(3 + s % 5, dd) for s in range(30) for dd in (DBASE[s], DBASE[s] + (1 << DEXTRA[s]) - 1)]
    for kind, mk in (("dynamic", dynamic), ("fixed", fixed)):
        _valid("symbols", "every distance symbol, " + kind,
               "after 32768 stored bytes: distance 32768 = the position (the member's first byte), then every distance symbol at its smallest and largest distance",
               [stored(hist), mk(far)],
               lambda c: c.blocks[1]["matches"][0][:3] == (32768, 3, 32768)
               and {(ds, dist) for _, _, dist, _, ds in c.blocks[1]["matches"]} >= {(s, v) for s in range(30) for v in (DBASE[s], DBASE[s] + (1 << DEXTRA[s]) - 1)})
    _valid("symbols", "distance = position, small", "matches whose distance equals the position, from 1 up",
           [fixed([7, M(3, 1), M(4, 4), M(8, 8), 9, M(17, 17)])], lambda c: sum(p == dist for p, _, dist, _, _ in c.blocks[0]["matches"]) == 4)
    over = [(dd, ln) for dd in (1, 2, 3, 63, 64, 65) for ln in (dd + 1, 64, 65, 258) if ln >= 3] + [(2, 7), (3, 100), (63, 200), (64, 100), (65, 131)]
    toks = list(range(70))
    for i, (dd, ln) in enumerate(over):
        toks += [M(ln, dd), 100 + i, 200 - i]
    _valid("symbols", "overlapping copies", "overlapping copies: distance in {1, 2, 3, 63, 64, 65}, length in {distance + 1, 64, 65, 258} and lengths that are no multiple of the distance",
           [dynamic(toks)],
           lambda c, over=over: [(dist, ln) for _, ln, dist, _, _ in c.blocks[0]["matches"]] == over
           and all(any(ln > dd and (ln % dd or dd == 1) for d2, ln in over if d2 == dd) for dd in (1, 2, 3, 63, 64, 65)))

    # ---- the two loops' boundary ------------------------------------------------------------------------------------------------
    one_bit = lambda c: c.blocks[0]["ll_lens"][120] == 1 and not c.blocks[0]["matches"] and c.blocks[0]["lit_runs"] == [(0, len(c.data))]
    for n in list(range(1, 151)) + [65536]:
        _valid("loops", "one-bit literals, ISIZE %d" % n, "a literal-only member of %d one-bit literals" % n,
               [dynamic([120] * n, ll_lens={120: 1, 256: 1}, d_lens=[0])], lambda c, n=n: one_bit(c) and len(c.data) == n)
    for back in (73, 72, 71):
        n = 200 - back
        _valid("loops", "match at isize - %d" % back, "ISIZE 200: the literal run before the match ends at isize - %d" % back,
               [dynamic([120] * n + [M(3, 1)] + [120] * (200 - n - 3), ll_lens={120: 1, 256: 2, 257: 2}, d_lens=[1])],
               lambda c, n=n: len(c.data) == 200 and c.blocks[0]["lit_runs"][0] == (0, n) and c.blocks[0]["matches"][0][0] == n
               and c.blocks[0]["ll_lens"][120] == 1)
    toks = list(b"0123456789") + [M(4, 5)]
    for r in (1, 2, 3, 4) * 3:
        toks += list(b"abcd"[:r]) + [M(4, 5)]
    toks += list(_text(100, 8))
    _valid("loops", "short literal runs", "runs of 1, 2, 3 and 4 literals between matches, where the fast loop still runs",
           [dynamic(toks)],
           lambda c: {n for p, n in c.blocks[0]["lit_runs"][1:-1] if p + n + FAST_ROOM <= len(c.data)} == {1, 2, 3, 4}
           and len(c.blocks[0]["lit_runs"]) == 14)
    ll = {s: i + 1 for i, s in enumerate(b"abcdefghij")}
    ll.update({ord("k"): 11, 256: 11})
    _valid("loops", "11-bit literal in a run", "a literal with an 11-bit code in the middle of a run of short ones, where the fast loop runs",
           [dynamic(list(b"a" * 20 + b"k" + b"ab" * 10 + b"kk" + b"abcdefghij" * 12), ll_lens=ll, d_lens=[0])],
           lambda c: c.blocks[0]["ll_lens"][ord("k")] == 11 > LROOT and c.data[20:21] == b"k" and 21 + FAST_ROOM <= len(c.data)
           and c.blocks[0]["lit_runs"] == [(0, len(c.data))])

    # ---- INVALID ----------------------------------------------------------------------------------------------------------------
    # Each case names the line of mth_inflate.hip that refuses it (`rejects`), found by following the stream through k_inflate /
    # inflate_symbols / literal_run by hand.  What keeps every one of them inside its buffers, whatever it decodes on the way:
    #   stores -- k_inflate has four, each behind a bound on the member's own isize: the stored copy (pos + len <= isize), the general
    #   loop's literal (pos < isize), the match copy (pos + len <= isize) and literal_run, which is entered and refills only while
    #   pos + 72 <= isize and stores fewer than 72 literals between two such checks (it holds at most 63 bits, checks again once
    #   fewer than 32 are left, and a trip of three literals uses at least 3: at most 11 trips, 33 literals).  None lands at or
    #   past out0 + isize.
    #   loads -- the stored copy reads only after po + 4 + len <= coff + csize, inside the file bytes.  The bit reader is not bounded by
    #   csize: a member that does not end where it says reads on into the trailer and the next member (file bytes all), and behind the
    #   last member into the padding, which is zeros.  There a block header is 000 = stored with LEN = NLEN = 0: refused.  Inside a
    #   block every symbol either adds output (bounded by isize <= 65536: at most 15 bits a literal, 120 KiB, and matches yield more
    #   per bit), ends the block (then the header above) or is no code (refused); a dynamic header reads at most 316 lengths.  So no
    #   load leaves the 160 KiB of INF_FILE_PAD.  In this corpus only the cut payload gets there, for (900 - pos) one-bit literals.
    lead =fixed(hello, final=False)                                  # every case is well formed up to its fault
    tail = [(0, 16)]                                                  # bits behind a fault: never decoded
    _invalid("BTYPE 3", "a block of type 3", [lead, Raw([(3, 2)] + tail)], lambda c: c.blocks[1]["fields"][0] == (3, 2),
             "k_inflate: if (type == 3)")
    _invalid("stored, NLEN wrong", "a stored block whose NLEN is not the complement of LEN",
             [lead, stored(b"abc" * 10, nlen_field=(~30 & 0xffff) ^ 1)], lambda c: (c.blocks[1]["len"] ^ c.blocks[1]["nlen"]) != 0xffff,
             "k_inflate, stored: (len ^ nlen) != 0xffff")
    m = build([lead, stored(bytes(range(100)))])
    _invalid("stored, LEN over isize", "a stored block of 100 bytes where the table's isize leaves room for 99",
             m, lambda c: c.blocks[1]["start_out"] + c.blocks[1]["len"] == c.isize + 1, "k_inflate, stored: pos + len > isize",
             isize=len(m.data) - 1, zlib_raises=False, verdict=lambda c, r: r["eof"] and len(r["out"]) == c.isize + 1)
    _invalid("stored, LEN past csize", "a stored block with LEN 100 and 50 bytes of payload left",
             [lead, stored(bytes(range(100)), body=bytes(range(50)))], lambda c: c.blocks[1]["len"] == 100 and c.blocks[1]["body"] == 50,
             "k_inflate, stored: po + 4 + len > b.end", isize=len(hello) + 100, zlib_raises=False, verdict=lambda c, r: not r["eof"])
    for v in (30, 31):
        _invalid("HLIT %d" % (257 + v), "a dynamic header with HLIT %d" % (257 + v), [lead, Raw([(2, 2), (v, 5), (0, 5), (15, 4)] + tail)],
                 lambda c, v=v: c.blocks[1]["fields"][:2] == [(2, 2), (v, 5)], "k_inflate, dynamic: hlit > 286")
        _invalid("HDIST %d" % (1 + v), "a dynamic header with HDIST %d" % (1 + v), [lead, Raw([(2, 2), (0, 5), (v, 5), (15, 4)] + tail)],
                 lambda c, v=v: c.blocks[1]["fields"][:3] == [(2, 2), (0, 5), (v, 5)], "k_inflate, dynamic: hdist > 30")
    _invalid("code-length code over-subscribed", "three one-bit codes in the code-length code",
             [lead, dynamic([65, 66, 65], ll_lens={65: 1, 66: 2, 256: 2}, d_lens=[0], header=Header(cl_lens=[1, 1, 1]))],
             lambda c: kraft(c.blocks[1]["cl_lens"]) > 0 and kraft(c.blocks[1]["ll_lens"]) == 0, "k_inflate, dynamic: !huff_build(HC, ...)")
    _invalid("literal/length code over-subscribed", "three one-bit codes in the literal/length code",
             [lead, dynamic([65, 66, 65], ll_lens={65: 1, 66: 1, 256: 1}, d_lens=[0])],
             lambda c: kraft(c.blocks[1]["ll_lens"]) > 0 and kraft(c.blocks[1]["cl_lens"]) == 0, "k_inflate, dynamic: !huff_build(HL, ...)")
    _invalid("distance code over-subscribed", "three one-bit codes in the distance code",
             [lead, dynamic([65, 65, M(3, 1)], ll_lens={65: 1, 256: 2, 257: 2}, d_lens=[1, 1, 1])],
             lambda c: kraft(c.blocks[1]["d_lens"]) > 0 and kraft(c.blocks[1]["ll_lens"]) == 0 and kraft(c.blocks[1]["cl_lens"]) == 0,
             "k_inflate, dynamic: !huff_build(HD, ...)")
    ll = _as_list({65: 2, 66: 2, 67: 2, 256: 2}, 257)
    _invalid("16 first", "symbol 16 as the first code length",
             [lead, dynamic([65, 66], ll_lens=ll, d_lens=[0], header=Header(ops=[(16, 0)] + [(v, 0) for v in (ll + [0])[3:]]))],
             lambda c: c.blocks[1]["ops"][0] == (16, 0, 3) and sum(n for _, _, n in c.blocks[1]["ops"]) == 258, "k_inflate, dynamic: sym == 16, i == 0")
    ops = [(18, 65 - 11), (2, 0), (2, 0), (2, 0), (18, 127), (18, 50 - 11), (2, 0), (18, 0)]
    _invalid("repeat overruns the lengths", "an 18 run of 11 that starts at the last of HLIT + HDIST = 258 lengths",
             [lead, dynamic([65, 66], ll_lens=ll, d_lens=[0], header=Header(ops=ops))],
             lambda c: c.blocks[1]["ops"][-1] == (18, 257, 11) and c.blocks[1]["hlit"] + c.blocks[1]["hdist"] == 258, "k_inflate, dynamic: i + rep > total")
    _invalid("no end-of-block code", "a literal/length code without symbol 256",
             [lead, dynamic([65, 66, 67, 68], ll_lens={65: 2, 66: 2, 67: 2, 68: 2}, d_lens=[0], eob=False)],
             lambda c: c.blocks[1]["ll_lens"][256] == 0 and kraft(c.blocks[1]["ll_lens"]) == 0, "k_inflate, dynamic: s_lens[256] == 0")
    _invalid("no such literal/length code", "the lone one-bit end-of-block code 0, and a 1 bit",
             [lead, dynamic([RawBits(1, 1), RawBits(0, 15)], ll_lens={256: 1}, d_lens=[0], eob=False)],
             lambda c: kraft(c.blocks[1]["ll_lens"]) < 0 and canonical(c.blocks[1]["ll_lens"])[256] == 0,
             "inflate_symbols: sym < 0 (huff_decode walks 15 bits and finds no code)")
    _invalid("no such distance code", "one distance code of one bit, 0, and a 1 bit where a distance is due",
             [lead, dynamic(hello + [RawLL(257), RawBits(1, 1), RawBits(0, 15)], d_lens=[1])],
             lambda c: c.blocks[1]["d_lens"] == [1] and 257 in c.blocks[1]["used_ll"], "inflate_symbols: ds < 0")
    cl = [0] * 19
    cl[0], cl[2] = 1, 2
    _invalid("no such code-length code", "a code-length code of 0 and 10, and the bits 11",
             [lead, dynamic([65], ll_lens=ll, d_lens=[0], header=Header(cl_lens=cl, ops=[(0, 0)] * 10 + [(-1, 3, 2), (-1, 0, 15)]))],
             lambda c: kraft(c.blocks[1]["cl_lens"]) < 0 and canonical(c.blocks[1]["cl_lens"])[2] == 2, "k_inflate, dynamic: sym < 0 (code lengths)")
    for s in (286, 287):
        _invalid("fixed block, symbol %d" % s, "literal/length symbol %d in a fixed block" % s, [fixed(hello + [RawLL(s)], eob=False)],
                 lambda c, s=s: c.blocks[0]["used_ll"] >= {s}, "inflate_symbols: sym > 285")
    for s in (30, 31):
        _invalid("fixed block, distance symbol %d" % s, "distance symbol %d in a fixed block" % s,
                 [fixed(hello + [RawLL(257), RawD(s)], eob=False)], lambda c, s=s: c.blocks[0]["used_d"] == {s},
                 "inflate_symbols: ds < 0 (the fixed distance code is built from 30 lengths: 30 and 31 are no codes)")
    _invalid("distance 1 at position 0", "a match of distance 1 as the first symbol", [fixed([M(3, 1, unchecked=True)])],
             lambda c: len(c.data) == 0 and not c.blocks[0]["matches"], "inflate_symbols: dist > pos", isize=3)
    _invalid("distance position + 1", "a match of distance 15 at position 14", [fixed(hello + [M(3, len(hello) + 1, unchecked=True)])],
             lambda c: len(c.data) == 14 and not c.blocks[0]["matches"], "inflate_symbols: dist > pos", isize=17)
    m = build([dynamic(list(_text(300, 11)))])
    lit_only = lambda c: not _all_matches(c) and c.blocks[0]["lit_runs"] == [(0, 300)] and max(c.blocks[0]["ll_lens"]) <= LROOT
    _invalid("isize 1 too small, literals", "300 literals, isize 299", m, lambda c: lit_only(c) and c.isize == 299,
             "inflate_symbols: literal, pos >= isize (literal_run left at pos + 72 > isize)", isize=299, zlib_raises=False,
             verdict=lambda c, r: r["eof"] and len(r["out"]) == c.isize + 1)
    _invalid("isize 80 too small, literals", "300 literals, isize 220", m, lambda c: lit_only(c) and c.isize == 220 and c.isize > FAST_ROOM,
             "inflate_symbols: literal, pos >= isize (literal_run left at pos + 72 > isize)", isize=220, zlib_raises=False,
             verdict=lambda c, r: r["eof"] and len(r["out"]) == c.isize + 80)
    m = build([dynamic(list(_text(50, 12)) + [M(50, 10)])])
    _invalid("isize too small, match", "a member that ends in a match of 50, isize one short", m,
             lambda c: c.blocks[0]["matches"][-1][:2] == (50, 50) and c.isize == 99, "inflate_symbols: pos + len > isize", isize=99,
             zlib_raises=False, verdict=lambda c, r: r["eof"] and len(r["out"]) == c.isize + 1)
    _invalid("isize too large", "a whole member, isize 5 more than it holds", m, lambda c: c.isize == len(c.data) + 5,
             "k_inflate, end: pos != isize", isize=105, zlib_raises=False, verdict=lambda c, r: r["eof"] and len(r["out"]) == c.isize - 5)
    _invalid("csize one short", "a whole member, csize one byte less than its payload", m,
             lambda c: c.csize == len(c.payload) - 1 and c.blocks[-1]["end_bit"] > c.csize * 8, "k_inflate, end: b.cursor() > b.end", csize=len(m.payload) - 1,
             zlib_raises=False, verdict=lambda c, r: not r["eof"])
    # cut in half: the end-of-block code is fifteen 1 bits, the trailer's bits decode as literals, the zero padding as the one-bit one
    lits = list(b"etaoinshrdlucm")
    ll = {s: i + 1 for i, s in enumerate(lits)}
    ll.update({ord("q"): 15, 256: 15})
    m = build([dynamic(list(_text(900, 13, bytes(lits))), ll_lens=ll, d_lens=[0])])
    _invalid("payload cut in half, last in the file", "half a payload, its trailer, the end of the file: the reader meets the zero padding and reads literals from it",
             Member(m.payload[:len(m.payload) // 2], m.data, m.blocks), _cut_reaches_padding,
             "inflate_symbols: literal, pos >= isize (the padding's zero bits are one-bit literals)", last=True, zlib_raises=False,
             verdict=lambda c, r: not r["eof"] and len(r["out"]) < c.isize)
    m = build([dynamic(hello * 4 + [M(20, 14)])])
    _invalid("CRC wrong", "a whole member whose trailer holds another CRC32", m, lambda c: c.crc != zlib.crc32(c.data),
             "k_crc32: crc != want", crc=(zlib.crc32(m.data) ^ 1) & 0xffffffff, zlib_raises=False,
             verdict=lambda c, r: r["eof"] and r["out"] == c.data and zlib.crc32(r["out"]) != c.crc)
    for c in INVALID:
        if c.isize is None:
            c.isize = len(c.data)
        if c.csize is None:
            c.csize = len(c.payload)


def _cut_reaches_padding(c):
    """decode the cut payload, its trailer and zero bytes with the block's code: no end-of-block code and no unassigned pattern before
    isize literals are out, and by then the reader is in the padding"""
    b = c.blocks[0]
    code = {(l, k): s for s, (l, k) in enumerate(zip(b["ll_lens"], canonical(b["ll_lens"]))) if l}
    bits = c.payload + struct.pack("<II", zlib.crc32(c.data) & 0xffffffff, c.isize) + bytes(4096)
    at, n = b["sym_bit"], 0
    while n < c.isize:
        k = 0
        for l in range(1, 16):
            k = k << 1 | (bits[at >> 3] >> (at & 7) & 1)
            at += 1
            if (l, k) in code:
                break
        else:
            return False
        if code[(l, k)] >= 256:
            return False
        n += 1
    return at > (len(c.payload) + 8) * 8 and len(c.payload) * 8 > b["sym_bit"] + 100 and len(c.payload) < c.blocks[0]["end_bit"] // 8


_fill()
GROUPS = sorted({c.group for c in VALID})
