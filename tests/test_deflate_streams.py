"""CPU: the two corpora of tests/deflate_streams.py against zlib's raw inflate.  Every VALID stream inflates to exactly the bytes its
tokens mean and holds the shape it is named for; every INVALID stream holds its fault, and zlib either refuses it or, where it is
wrong only against its block table (isize, csize, CRC trailer), sees it differ from the table in the stated way.  A case that
degenerates fails here, not on the device."""
import collections
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_streams as D

ids = lambda cases: ["%s: %s" % (c.group, c.name) for c in cases]


@pytest.mark.parametrize("c", D.VALID, ids=ids(D.VALID))
def test_valid_case(c):
    r = D.zlib_verdict(c.payload)
    assert r["error"] is None, r["error"]
    assert r["out"] == c.data
    assert r["eof"] and r["unused"] == b""
    assert len(c.data) <= 65536
    assert c.pred(c), c.what


@pytest.mark.parametrize("c", D.INVALID, ids=ids(D.INVALID))
def test_invalid_case(c):
    assert c.pred(c), c.what
    assert c.rejects
    r = D.zlib_verdict(c.payload[:c.csize])
    if c.zlib_raises:
        assert r["error"] is not None, "zlib accepts it"
    else:
        assert r["error"] is None, r["error"]
        assert c.verdict(c, r), c.what


def test_the_corpora_hold_what_they_list():
    n = collections.Counter(c.group for c in D.VALID)
    assert n == {"structure": 20, "sizes": 12, "long codes": 4, "incomplete": 4, "header": 15, "symbols": 6, "loops": 156}
    assert len(D.INVALID) == 30
    names = [c.name for c in D.VALID + D.INVALID]
    assert len(set(names)) == len(names)
    assert {len(c.data) for c in D.VALID if c.group == "sizes"} == {65279, 65280, 65281, 65498, 65535, 65536}
    assert {len(c.data) for c in D.VALID if c.name.startswith("one-bit literals")} == set(range(1, 151)) | {65536}
    # nine are wrong only against their table (isize x 5, csize x 2, truncation, CRC); zlib itself refuses the other 21
    assert sum(c.zlib_raises for c in D.INVALID) == 21
    assert len({c.rejects for c in D.INVALID}) >= 20


def test_frame():
    """payload + CRC32 + ISIZE per member, the payloads at every offset mod 4 -- by default, and where a case asks for one"""
    fb, coff, csize, isize, want = D.frame(D.VALID)
    assert want == b"".join(c.data for c in D.VALID)
    for i, c in enumerate(D.VALID):
        o, n = int(coff[i]), int(csize[i])
        assert fb[o:o + n] == c.payload and int(isize[i]) == len(c.data)
        assert struct.unpack_from("<II", fb, o + n) == (zlib.crc32(c.data), len(c.data))
        assert o % 4 == (i % 4 if c.phase is None else c.phase)
    assert {c.phase for c in D.VALID if c.phase is not None} == {0, 1, 2, 3}
    for g in D.GROUPS:
        assert {int(o) % 4 for o in D.frame([c for c in D.VALID if c.group == g])[1]} == {0, 1, 2, 3}, g
    # chosen slack, and what an INVALID case declares
    bad = next(c for c in D.INVALID if c.name == "csize one short")
    crc = next(c for c in D.INVALID if c.name == "CRC wrong")
    fb, coff, csize, isize, _ = D.frame([D.VALID[0], bad, crc], slack=[3, 0, 2])
    assert list(coff) == [3, 3 + len(D.VALID[0].payload) + 8, 3 + len(D.VALID[0].payload) + 8 + len(bad.payload) + 8 + 2]
    assert int(csize[1]) == len(bad.payload) - 1 and fb[int(coff[1]):int(coff[1]) + len(bad.payload)] == bad.payload
    assert struct.unpack_from("<I", fb, int(coff[2]) + int(csize[2]))[0] == crc.crc != zlib.crc32(crc.data)


def test_the_writer_against_zlibs_own_streams():
    """ordinary data through the writer: a greedy matcher's tokens -> a fixed and two dynamic blocks -> zlib reads the bytes back"""
    data = D._text(5000, 99) + bytes(range(256)) * 3 + b"\0" * 700
    toks, i = [], 0
    while i < len(data):                                      # a greedy matcher of its own: longest match among a few distances
        best = (0, 0)
        for dist in (1, 2, 3, 7, 64, 256, 700, 4999):
            if dist <= i:
                n = 0
                while n < 258 and i + n < len(data) and data[i + n] == data[i + n - dist]:
                    n += 1
                best = max(best, (n, dist))
        if best[0] >= 3:
            toks.append(D.M(*best)); i += best[0]
        else:
            toks.append(data[i]); i += 1
    assert sum(isinstance(t, D.M) for t in toks) > 50
    for blocks in ([D.fixed(toks)], [D.dynamic(toks)], [D.dynamic(toks, header=D.Header(rep16=3, rep17=3, rep18=11, hclen=19))]):
        m = D.build(blocks)
        assert m.data == data
        r = D.zlib_verdict(m.payload)
        assert r["error"] is None and r["out"] == data and r["eof"] and r["unused"] == b""


# ---- files cut where htsjdk cuts them (65498) and at the format's limit (65536) ---------------------------------------------------
FILE_CUTS = (65498, 65536)


def cut_file(d, cut):
    """3 000 irregular reads, written with incompressible sequences and re-cut every `cut` inflated bytes -> (records, Layout)"""
    import os
    from tests import irregular_util
    from tests import straddle_util as S
    rec = irregular_util.make_records(950, n_contigs=2, length=8_000, n_reads=1_500, density=0.03)[0]
    return rec, S.Layout(S.write_cut(os.path.join(d, "cut_%d.bam" % cut), rec, cut, realistic=True))


@pytest.mark.parametrize("cut", FILE_CUTS)
def test_cut_files_hold_full_blocks_that_records_straddle(tmp_path, cut):
    rec, lay = cut_file(str(tmp_path), cut)
    assert len(rec) == 3000 and len(lay.isize) >= 20
    assert int(np.sum(lay.isize == cut)) == len(lay.isize) - 1 and int(lay.isize.max()) == cut
    assert lay.blocks_cut_inside_a_record() >= 0.9
    assert int(lay.csize.max()) + 26 <= 65536                       # a legal BGZF block all the same
