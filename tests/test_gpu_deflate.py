"""k_deflate through Engine.bgzf_deflate: one or two BGZF blocks per case -- the smallest shapes on which the encoder can go
wrong -- inflated with Python's zlib (tests/bgzf_util.py checks the framing of every block by hand).  Every case also pins
something of its own form, so that a case the encoder answers with a stored block cannot make another one pass vacuously."""
import numpy as np
import pytest

from tests import bgzf_util as B

pytestmark = pytest.mark.gpu
MAX = B.MAX_BLOCK


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def deflate(eng, data, cuts=None):
    """-> the blocks; their inflated bytes, concatenated, must be the input"""
    out = eng.bgzf_deflate(data, cuts)
    bl = B.blocks(out, keep_eof=True)
    assert b"".join(b.raw for b in bl) == bytes(data)
    for b in bl:
        assert len(b.payload) <= len(b.raw) + 5, "a payload is never larger than its input + 5 (the stored form)"
    return bl


# ---- the generated cases ---------------------------------------------------------------------------------------------------
def fibonacci_bytes():
    """22 byte values with the counts 1, 1, 2, 3, ... 17711 (46367 bytes), shuffled: a Huffman code of these weights is 21 deep"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    a = np.concatenate([np.full(c, 7 * i + 3, np.uint8) for i, c in enumerate(fib)])
    np.random.default_rng(5).shuffle(a)
    return a.tobytes(), fib


# literal/length code lengths -> number of symbols, found by search: 257 symbols (256 byte values and the end-of-block symbol),
# a complete code (sum of 2^-len = 1), and a histogram of lengths -- with the two 1-bit distance codes an encoder sends for a block
# without matches -- whose Huffman code is 8 deep: one more than the code-length code may be
SKEW_LENGTHS = {7: 124, 8: 3, 9: 1, 10: 4, 11: 6, 12: 25, 13: 8, 14: 34, 15: 52}


def skewed_code_length_bytes():
    """all 256 byte values, value v with the count 2^(15 - len(v)) (the end-of-block symbol takes one 15-bit place), in an order in
    which no three consecutive bytes occur twice: no match of the minimum length exists, the block is literals only and its
    Huffman lengths are exactly SKEW_LENGTHS"""
    assert sum(SKEW_LENGTHS.values()) == 257 and sum(c << (15 - k) for k, c in SKEW_LENGTHS.items()) == 32768
    lens = [k for k, c in sorted(SKEW_LENGTHS.items()) for _ in range(c)][:-1]        # (the last 15 is the end-of-block symbol's)
    rng = np.random.default_rng(9)
    values = rng.permutation(256)
    seq = np.concatenate([np.full(1 << (15 - k), v, np.int64) for v, k in zip(values, lens)])
    rng.shuffle(seq)
    seq = seq.tolist()
    seen = set()
    i = 2
    while i < len(seq):                                     # de Bruijn style: every window of three is new
        for _ in range(200):
            t = (seq[i - 2] << 16) | (seq[i - 1] << 8) | seq[i]
            if t not in seen:
                break
            j = int(rng.integers(i + 1, len(seq))) if i + 1 < len(seq) else i
            seq[i], seq[j] = seq[j], seq[i]
        seen.add(t)
        i += 1
    data = bytes(seq)
    triples = {data[k:k + 3] for k in range(len(data) - 2)}
    return data, len(triples) == len(data) - 2


DIST_RANGES = [(1, 1), (2, 2), (3, 3), (4, 4)] + [((1 << (e + 1)) + h * (1 << e) + 1, (1 << (e + 1)) + (h + 1) * (1 << e))
                                                   for e in range(1, 14) for h in (0, 1)]


def full_range_bytes():
    """all 256 byte values, a repeat of every length 3 .. 258, and a repeat at a distance inside each of the 30 distance-code
    ranges (1, 2, 3, 4, 5-6, 7-8, 9-12, ... 24577-32768): 25000 random bytes, then copy after copy (LZ77 semantics: a copy may
    overlap itself) with two fresh bytes between them"""
    assert len(DIST_RANGES) == 30 and DIST_RANGES[4] == (5, 6) and DIST_RANGES[-1] == (24577, 32768)
    rng = np.random.default_rng(21)
    buf = bytearray(np.random.default_rng(20).permutation(256).astype(np.uint8).tobytes() + rnd(22, 25000 - 256))
    plan = []
    for k, length in enumerate(range(3, 259)):
        lo, hi = DIST_RANGES[k % 30]
        d = int(rng.integers(lo, min(hi, len(buf)) + 1))
        plan.append((len(buf), length, d))
        for _ in range(length):
            buf.append(buf[-d])
        buf += bytes(rng.integers(0, 256, 2, dtype=np.uint8))
    assert len(buf) <= MAX
    return bytes(buf), plan


# ---- no possible match, a single literal, an empty distance code ---------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_shortest_inputs(eng, n):
    data = rnd(n, n)
    bl = deflate(eng, data, cuts=[0, n])
    assert len(bl) == 1
    # fixed Huffman costs 3 + 8n (or 9n) + 7 bits, stored n + 5 bytes, a dynamic header alone is 74 bits: the fixed form is the smallest
    assert bl[0].btype == 1 and len(bl[0].payload) <= (3 + 9 * n + 7 + 7) // 8
    assert eng.bgzf_deflate(b"") == b""                     # no block at all without a cut: the EOF block is the caller's


# ---- a run: an overlapping match at distance 1, at the maximum length ------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 258, 259, MAX])
def test_equal_bytes_are_not_stored(eng, n):
    bl = deflate(eng, b"\x07" * n)
    assert len(bl) == 1 and bl[0].btype != 0
    if n in (258, 259):
        # fixed form: one literal and one match (length 257: 13 bits, 258: 8 bits; distance 1: 5 bits) -- literals alone need 33 bytes
        assert bl[0].btype == 1 and len(bl[0].payload) <= 5
    if n == MAX:
        # literals alone cost at least a bit each (8160 bytes); one literal and 254 matches of at most 48 bits each under the
        # largest dynamic header there is (17 + 57 + 316 * 7 bits) stay far below that
        assert len(bl[0].payload) <= (3 + 17 + 57 + 316 * 7 + 15 + 48 * 254 + 15 + 7) // 8 < MAX // 8


def test_random_bytes_are_stored(eng):
    data = rnd(100, MAX)
    bl = deflate(eng, data)
    assert len(bl) == 1 and bl[0].btype == 0 and len(bl[0].payload) == MAX + 5 and bl[0].size == MAX + 5 + 26 <= 65536


def test_one_byte_over_a_block(eng):
    data = (b"the quick brown fox jumps over the lazy dog. " * 1500)[:MAX + 1]
    bl = deflate(eng, data)
    assert [len(b.raw) for b in bl] == [MAX, 1]
    assert bl[0].btype == 2 and bl[1].btype == 1 and len(bl[0].payload) < MAX // 20


def test_pattern_of_16_bytes(eng):
    data = rnd(7, 16) * 4000
    bl = deflate(eng, data)
    # 16 literals, then matches of 258 at distance 16: 250 tokens of at most 48 bits and the largest header
    assert len(bl) == 1 and bl[0].btype != 0 and len(bl[0].payload) <= (3 + 17 + 57 + 316 * 7 + 16 * 15 + 48 * 250 + 15 + 7) // 8


def test_period_32768_matches_at_the_maximum_distance(eng):
    data = (rnd(8, 32768) * 2)[:MAX]
    bl = deflate(eng, data)
    # the only repeats (beyond chance triples) lie exactly 32768 back; without them 65280 random bytes do not shrink at all
    assert bl[0].btype == 2 and len(bl[0].payload) < MAX * 3 // 4


def test_period_32769_has_nothing_to_match(eng):
    data = (rnd(8, 32769) * 2)[:MAX]
    bl = deflate(eng, data)
    assert bl[0].btype == 0 and len(bl[0].payload) == MAX + 5


def test_fibonacci_frequencies_give_complete_codes(eng):
    data, fib = fibonacci_bytes()
    # a Huffman code of the byte counts alone is 21 deep.  (What the encoder codes is its own histogram -- fewer literals where it
    # found matches, length symbols, the end of block -- so the limiting routine itself is pinned on the CPU, on exactly such
    # weights: tests/test_deflate_model.py.  Here: whatever it built, zlib accepts it as complete codes of at most 15 bits.)
    assert B.huffman_depth(fib) == 21
    bl = deflate(eng, data)
    assert len(bl) == 1 and bl[0].btype == 2
    ll, dd, cl, _ = B.dynamic_header(bl[0].payload)
    assert max(ll) <= 15 and B.kraft(ll) == 32768 and B.kraft(dd) == 32768       # complete, not over-subscribed
    assert sum(1 << (7 - n) for n in cl if n) == 128         # the code-length code is complete too
    assert len(bl[0].payload) < len(data) // 2               # 22 values of these weights: under 3 bits a byte even without matches


def test_skewed_code_lengths_need_the_7_bit_limit(eng):
    data, no_repeated_triple = skewed_code_length_bytes()
    assert no_repeated_triple and len(set(data)) == 256 and len(data) == 32767
    bl = deflate(eng, data)
    assert len(bl) == 1 and bl[0].btype == 2
    ll, dd, cl, sent = B.dynamic_header(bl[0].payload)
    assert len(ll) == 257 and all(ll) and dd == [1, 1]        # literals only: every byte value, the end of block, two 1-bit distance codes
    got = {k: ll.count(k) for k in set(ll)}
    assert got == SKEW_LENGTHS                               # the Huffman lengths of a dyadic distribution are its logarithms
    hist = [sent.count(s) for s in range(19)]
    assert B.huffman_depth(hist) > 7                         # an unlimited code-length code would be too deep ...
    assert max(cl) <= 7 and sum(1 << (7 - n) for n in cl if n) == 128      # ... the one sent is within 7 bits and complete
    # 32767 literals at their Huffman lengths (32768 * sum(len * 2^-len) bits less the end-of-block share) plus the header
    bits = sum(c * k * (1 << (15 - k)) for k, c in SKEW_LENGTHS.items())
    assert len(bl[0].payload) <= (bits + 17 + 57 + 259 * 7 + 7) // 8


def test_full_symbol_range(eng):
    data, plan = full_range_bytes()
    assert len(set(data)) == 256 and {p[1] for p in plan} == set(range(3, 259))
    assert all(any(lo <= d <= hi for _, _, d in plan) for lo, hi in DIST_RANGES)
    bl = deflate(eng, data)
    assert len(bl) == 1 and bl[0].btype == 2 and len(bl[0].payload) < len(data)
    # the copies are 33408 of the bytes; matched, they cost a small part of that
    assert len(bl[0].payload) < len(data) - 33408 // 2
    ll, dd, _, _ = B.dynamic_header(bl[0].payload)
    assert sum(1 for n in ll[257:] if n) >= 20 and sum(1 for n in dd if n) >= 20      # length and distance codes of every size are in use
    assert eng.bgzf_deflate(data) == eng.bgzf_deflate(data)


def test_cuts_of_any_size_and_determinism(eng):
    words = [rnd(300 + i, 2 + i % 7) for i in range(300)]
    pick = np.random.default_rng(4).integers(0, 300, 40000)
    data = b" ".join(words[int(i)] for i in pick)[:150000]
    cuts = [0, 1, 1 + MAX, 1 + MAX, 2 + MAX + 777, 100000, 150000]                    # (one empty block among them)
    first = eng.bgzf_deflate(data, cuts)
    bl = B.blocks(first, keep_eof=True)
    assert [len(b.raw) for b in bl] == [b - a for a, b in zip(cuts, cuts[1:])]
    assert b"".join(b.raw for b in bl) == data
    assert sum(len(b.payload) for b in bl) < len(data) * 0.6
    assert eng.bgzf_deflate(data, cuts) == first
    other = eng.bgzf_deflate(rnd(1, 5000))                    # another call in between does not leak into the next
    assert B.blocks(other, keep_eof=True)[0].raw == rnd(1, 5000)
    assert eng.bgzf_deflate(data, cuts) == first
    # the default cuts: every 0xff00 bytes
    bl = deflate(eng, data)
    assert [len(b.raw) for b in bl] == [MAX, MAX, 150000 - 2 * MAX]


def test_own_inflater_reads_it_back(eng):
    parts = [full_range_bytes()[0], fibonacci_bytes()[0], rnd(3, MAX), b"\x00" * 60000, b"abc"]
    cuts = [0]
    for p in parts:
        cuts.append(cuts[-1] + len(p))
    data = b"".join(parts)
    out = eng.bgzf_deflate(data, cuts)
    bl = B.blocks(out, keep_eof=True)
    assert [b.btype for b in bl] == [2, 2, 0, 2, 1]          # every form the encoder writes
    coff, csize, isize = B.table(bl)
    back = eng.bgzf_inflate(out, coff, csize, isize)
    assert back.tobytes() == data


def test_cuts_are_validated(eng):
    import metheor_amd
    with pytest.raises(metheor_amd.MthError):
        eng.bgzf_deflate(rnd(1, MAX + 1), cuts=[0, MAX + 1])          # a block above 0xff00 bytes
    with pytest.raises(metheor_amd.MthError):
        eng.bgzf_deflate(rnd(1, 100), cuts=[0, 60, 50, 100])          # not ascending
    with pytest.raises(metheor_amd.MthError):
        eng.bgzf_deflate(rnd(1, 100), cuts=[0, 50])                   # does not reach the end
