"""The format logic of k_deflate on the CPU.  metheor_amd/csrc/mth_deflate.hip writes the body of a block as phases between
barriers over LDS state; compiled with MTH_DEFLATE_HOST_MODEL a phase is a loop over the 256 lanes, so the very text the device
runs is exercised here: blocks against Python's zlib, and the code-length routine on weights that an unlimited Huffman code would
take beyond 15 (and, for the code-length code, beyond 7) bits."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bgzf_util as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#define MTH_DEFLATE_HOST_MODEL
#include "mth_deflate.hip"
#include <cstdio>
#include <cstring>
#include <vector>
#include <zlib.h>
using namespace mth;
static DfLds L;
// "block IN OUT": IN = cases (u32 n, n bytes), OUT = per case u32 size + the BGZF block.  "build": stdin = cases (n limit w[0..n)),
// stdout = the code lengths of each
int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "block")) {
        FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
        if (!f || !o) return 2;
        std::vector<uint32_t> slot(DF_SLOT / 4), tok(DF_MAX_IN);
        uint32_t n;
        while (fread(&n, 4, 1, f) == 1) {
            std::vector<uint8_t> src(n + 1);
            if (n && fread(src.data(), 1, n, f) != n) return 2;
            memset(slot.data(), 0xab, DF_SLOT);                  // the block zeroes what it writes into
            df_block(L, src.data(), n, slot.data(), tok.data(), (uint32_t)crc32(0, src.data(), n));
            const uint32_t total = 18 + L.pay_bytes + 8;
            fwrite(&total, 4, 1, o); fwrite(slot.data(), 1, total, o);
        }
        fclose(o);
        return 0;
    }
    unsigned n, limit;
    while (scanf("%u %u", &n, &limit) == 2) {
        static uint32_t hist[288];
        static uint8_t len[288];
        for (unsigned i = 0; i < n; ++i) if (scanf("%u", &hist[i]) != 1) return 2;
        df_build(L, hist, n, limit, len);
        for (unsigned i = 0; i < n; ++i) printf("%u ", len[i]);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_model")
    src = d / "deflate_model.cpp"
    src.write_text(DRIVER)
    out = d / "deflate_model"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(out), str(src), "-lz"])
    return str(out)


def model_blocks(exe, tmp_path, cases):
    inp, outp = tmp_path / "cases.bin", tmp_path / "blocks.bin"
    with open(inp, "wb") as f:
        for c in cases:
            f.write(struct.pack("<I", len(c)) + c)
    subprocess.check_call([exe, "block", str(inp), str(outp)])
    o, p, out = outp.read_bytes(), 0, []
    for c in cases:
        size, = struct.unpack_from("<I", o, p)
        bl = B.blocks(o[p + 4:p + 4 + size], keep_eof=True)
        assert len(bl) == 1 and bl[0].raw == c and len(bl[0].payload) <= len(c) + 5
        out.append(bl[0])
        p += 4 + size
    assert p == len(o)
    return out


def rnd(seed, n, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n, dtype=np.uint8).tobytes()


def test_model_blocks_inflate_with_zlib(exe, tmp_path):
    words = [rnd(50 + i, 2 + i % 9, 64) for i in range(200)]
    text = b" ".join(words[int(i)] for i in np.random.default_rng(2).integers(0, 200, 15000))[:B.MAX_BLOCK]
    cases = [b"", b"a", b"ab", b"abc", b"\x07" * 3, b"\x07" * 258, b"\x07" * 259, b"\x07" * B.MAX_BLOCK, rnd(1, B.MAX_BLOCK), rnd(2, 16) * 4000,
             (rnd(3, 32768) * 2)[:B.MAX_BLOCK], (rnd(3, 32769) * 2)[:B.MAX_BLOCK], text] + [text[:n] for n in (4, 255, 256, 257, 511, 513, 4097)] + \
            [rnd(4, 20000, 4), rnd(5, 30000, 2)]
    bl = model_blocks(exe, tmp_path, cases)
    assert [b.btype for b in bl[:4]] == [1, 1, 1, 1]
    assert bl[7].btype == 2 and len(bl[7].payload) < 2048 and bl[8].btype == 0 and bl[11].btype == 0
    assert bl[12].btype == 2 and len(bl[12].payload) < 1.25 * B.zlib1_size(text)      # (zlib level 1 chains its hash; this one keeps one candidate)


def lengths_of(exe, cases):
    text = "".join("%d %d %s\n" % (len(w), limit, " ".join(str(int(x)) for x in w)) for w, limit in cases)
    out = subprocess.run([exe, "build"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return [[int(x) for x in line.split()] for line in out]


def cost(w, lens):
    return sum(a * b for a, b in zip(w, lens))


def test_length_limiting_gives_complete_codes(exe):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(3)
    cases = []
    ll = [0] * 286
    for k, f in enumerate(fib[1:22]):                        # 21 byte values with the counts 1, 2, 3, 5 ... and the end-of-block symbol's 1:
        ll[7 * k + 3] = f                                    # the Fibonacci numbers, whose every merge is forced -- a tree 21 deep
    ll[256] = 1
    cases.append((ll, 15))
    cases.append(([int(x) for x in rng.permutation(fib[:19])], 7))            # the code-length code's 19 symbols
    cases.append(([0, 2, 0, 0, 0, 0, 0, 124, 3, 1, 4, 6, 25, 8, 34, 52, 0, 0, 0], 7))   # the histogram tests/test_gpu_deflate.py provokes
    cases.append(([1 << min(k, 20) for k in range(30)], 15))                   # distance code, powers of two
    cases.append(([0] * 286, 15))                                              # nothing used: two codes all the same
    cases.append(([0] * 5 + [9] + [0] * 24, 15))                               # one symbol used
    cases.append(([int(x) for x in rng.integers(0, 400, 286)], 15))            # nothing to limit: the Huffman code itself
    got = lengths_of(exe, cases)
    for (w, limit), lens in zip(cases, got):
        used = [n for n in lens if n]
        assert len(used) >= 2 and max(used) <= limit
        assert sum(1 << (limit - n) for n in used) == 1 << limit, "complete and not over-subscribed"
        assert all(n > 0 for n, f in zip(lens, w) if f), "every symbol that occurs has a code"
    assert B.huffman_depth(cases[0][0]) > 15 and B.huffman_depth(cases[1][0]) > 7 and B.huffman_depth(cases[2][0]) > 7
    # where nothing had to be limited the lengths are a Huffman code's: the cost is the optimum
    w, lens = cases[6][0], got[6]
    import heapq
    h = [(f, i, (i,)) for i, f in enumerate(w) if f]
    opt = [0] * 286
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for i in a[2] + b[2]:
            opt[i] += 1
        heapq.heappush(h, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    assert max(opt) <= 15 and cost(w, lens) == cost(w, opt)
    # and limiting costs little: within 3 % of the unlimited optimum on the Fibonacci weights
    w, lens = cases[0][0], got[0]
    h = [(f, i, (i,)) for i, f in enumerate(w) if f]
    opt = [0] * 286
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for i in a[2] + b[2]:
            opt[i] += 1
        heapq.heappush(h, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    assert cost(w, opt) <= cost(w, lens) <= 1.03 * cost(w, opt)
