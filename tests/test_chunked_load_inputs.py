"""CPU companion of tests/test_gpu_chunked_load.py: every generated input is what its GPU test claims it is -- chunk counts per
setting from the restated planner, which header case each huge-header file realises, by how much the CLI's reserve falls short on the
low-yield-first file, a random cut at a contig change, and the pieced tables' edges.  A GPU test that silently stopped reaching its
branch fails here first.  The restated rules themselves are held against the C++ text they restate."""
import gzip
import hashlib
import os
import re
import struct
import zlib

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import chunked_load_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("chunked_inputs"))


def test_the_restated_rules_still_match_the_sources():
    """the lines of load_chunks and inflate_blocks that chunked_load_util restates, as they stood when it was written"""
    cli = open(os.path.join(ROOT, "metheor_amd", "csrc", "host", "cli_main.cpp")).read()
    for text in ("size_t chunk_first = (size_t)512 << 20, chunk = (size_t)2 << 30, growth = 64;",
                 "for (size_t k = 0; k < chunks.size() && lim < chunk; ++k) lim = std::min(chunk, lim * growth);",
                 "while (b1 < bz.n_blocks && (b1 == b0 || bz.coff[b1] + bz.csize[b1] - bz.coff[b0] <= lim)) { ubytes += bz.isize[b1]; ++b1; }",
                 "bz.coff[b1 - 1] + bz.csize[b1 - 1] + 8 - bz.coff[b0]",
                 "const uint64_t first_byte = std::min<uint64_t>(hdr_left, c.ubytes);",
                 "if (c.b1 > c.b0 && hdr_left > c.ubytes && ci + 1 < chunks.size()) {",
                 "const double f = 1.03 * (double)total_u / (double)done_u;"):
        assert text in cli, text
    inf = open(os.path.join(ROOT, "metheor_amd", "csrc", "mth_inflate.hip")).read()
    for text in ("const bool pieced = !staged && piece_bytes && n_bytes >= 2 * (uint64_t)piece_bytes && nb >= 2;",
                 "if ((size_t)n_bytes - off - len < piece_bytes / 2) len = (size_t)n_bytes - off;",
                 "while (b1 < nb && (last || coff[b1] + (uint64_t)csize[b1] + 64u <= (uint64_t)off)) ++b1;"):
        assert text in inf, text


def test_layout_reads_a_file_as_gzip_does(d):
    p = U.one_contig(os.path.join(d, "one.bam"))
    lay = U.Layout(p)
    assert 100 < lay.n_blocks < 200
    assert int(lay.u1[-1]) == len(lay.raw) == len(gzip.decompress(open(p, "rb").read()))
    for b in (0, 1, lay.n_blocks // 2, lay.n_blocks - 1):
        fb, coff, csize, isize, first = lay.call(b, b + 1)
        raw = zlib.decompress(fb[int(coff[0]):int(coff[0]) + int(csize[0])].tobytes(), -15)
        assert raw == lay.raw[int(lay.u0[b]):int(lay.u1[b])]
        assert struct.unpack("<II", fb[-8:].tobytes()) == (zlib.crc32(raw) & 0xffffffff, len(raw))
    # slices of the one array: equal ranges are the same address, what mth_bgzf_stage matches on
    a, b = lay.call(3, 9)[0], lay.call(3, 9)[0]
    assert a.ctypes.data == b.ctypes.data == lay.arr.ctypes.data + int(lay.coff[3]) and np.ascontiguousarray(a, np.uint8) is a
    first_rec, n = lay.record_block_starts()
    assert n == 20_000 and (np.diff(first_rec[lay.first_data_block():]) > 0).all()      # whole records per block, no empty block


def test_plans(d):
    p, firsts = U.three_contigs(d)
    lay = U.Layout(p)
    first_rec, n = lay.record_block_starts()
    assert n == 9500
    cuts = [int(np.nonzero(first_rec == f)[0][0]) for f in firsts[1:]]            # a block opens with every contig's first record
    tid = pyoracle.Reads.decode(bamio.read_bam(p)).soa()["tid"]
    assert [int(tid[f]) for f in firsts] == [0, 1, 2] and [int(tid[f - 1]) for f in firsts[1:]] == [0, 1]
    # the header has blocks of its own: a first call of those alone is given first_byte == total
    fd = lay.first_data_block()
    assert fd >= 1 and int(lay.u1[fd - 1]) == lay.hbytes
    assert lay.call(0, fd)[4] == lay.hbytes and lay.call(fd, lay.n_blocks)[4] == 0
    # some cut of the random plans falls at a contig change (25 cuts over the file's blocks: seed 4 was chosen for it)
    r3 = U.plan_random(lay.n_blocks, 4, n_cuts=25)
    assert any(b0 in cuts for b0, _ in r3), (cuts, r3)
    for plan in (U.plan_every(lay.n_blocks, 1), U.plan_every(lay.n_blocks, 7), U.plan_random(lay.n_blocks, 2), r3, U.plan_with_empty_call(U.plan_every(lay.n_blocks, 30), 2)):
        assert plan[0][0] == 0 and plan[-1][1] == lay.n_blocks and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    e = U.plan_with_empty_call(U.plan_every(lay.n_blocks, 30), 2)
    assert e[2][0] == e[2][1] and U.expected_paths(lay, e, True) == (len(e) - 2, 2)
    assert U.expected_paths(lay, r3, True) == (len(r3) - 1, 1) and U.expected_paths(lay, r3, False) == (0, len(r3))


def test_low_yield_first_file_makes_the_cli_reserve_an_underestimate(d):
    p, second = U.low_yield_first(d)
    lay = U.Layout(p)
    soa = pyoracle.Reads.decode(bamio.read_bam(p)).soa()
    R, C = len(soa["tid"]), len(soa["cpg_pos"])
    assert int(soa["cpg_off"][second]) == 0 and R == 12_000 and C > 50_000
    first_rec, _ = lay.record_block_starts()
    cut = int(np.nonzero(first_rec == second)[0][0]) // 2
    assert cut >= 5
    n_first = int(first_rec[cut])
    r, c = U.cli_reserve(int(lay.u1[-1]), int(lay.u1[cut - 1]), n_first, 0)
    print("reserve", (r, c), "true", (R, C), "short by a factor of %.1f" % (C / c))
    assert r >= R and c == 4096 and C / c > 12                      # the call arrays have to grow (1.5x a time) six times and more


def test_swapped_pair_is_out_of_order_at_a_block_seam(d):
    p, i = U.swapped_pair(d)
    lay = U.Layout(p)
    soa = pyoracle.Reads.decode(bamio.read_bam(p)).soa()
    assert not U.in_order(soa) and soa["start"][i] > soa["start"][i + 1]
    bad = np.nonzero(soa["start"][1:] < soa["start"][:-1])[0]
    assert list(bad) == [i]                                          # the one place
    first_rec, _ = lay.record_block_starts()
    assert (first_rec == i + 1).sum() == 1                           # a block opens between the two


def test_cli_file_chunk_counts(d):
    p = os.path.join(d, "cli.bam")
    U.cli_bam(p)
    lay = U.Layout(p)
    n = {k: U.plan_chunks(lay.coff, lay.csize, lay.isize, env) for k, env in U.CLI_SETTINGS.items()}
    assert len(n["default"]) == 1 and len(n["chunk1"]) == len(n["chunk1-nostage"]) == 4 and len(n["first1"]) == 2 and len(n["first1-growth2"]) == 3
    assert [c["lim"] // U.MIB for c in n["first1-growth2"]] == [1, 2, 4] and [c["lim"] // U.MIB for c in n["first1"]] == [1, 64]
    assert all(c["nbytes"] <= c["lim"] + 8 for k in n for c in n[k])
    for k, env in U.CLI_SETTINGS.items():
        hows = U.chunk_paths(n[k], lay.hbytes, env, int(env.get("METHEOR_COPY_PIECE_MB", 0)))
        print(k, [(c["b1"] - c["b0"], c["nbytes"]) for c in n[k]], hows)
    pc = n["chunk3-pieced"]
    assert U.chunk_paths(pc, lay.hbytes, U.CLI_SETTINGS["chunk3-pieced"], 1) == ["pieced", "in line"] and pc[1]["nbytes"] < 2 * U.MIB
    pieces, launches = U.piece_plan(pc[0]["nbytes"], lay.coff[:pc[0]["b1"]] - lay.coff[0], lay.csize[:pc[0]["b1"]])
    assert len(pieces) == 3 and len(launches) == 3
    # the smallest read count (in steps of 500) that gives four chunks
    q = os.path.join(d, "cli_less.bam")
    U.cli_bam(q, U.CLI_READS - 500)
    less = U.Layout(q)
    assert len(U.plan_chunks(less.coff, less.csize, less.isize, U.CLI_SETTINGS["chunk1"])) == 3
    # the shuffled copy is cut into several chunks too, and is out of order
    s = U.Layout(U.shuffled_runs(p, os.path.join(d, "shuffled.bam")))
    assert len(U.plan_chunks(s.coff, s.csize, s.isize, U.CLI_SETTINGS["chunk1"])) >= 3
    assert s.record_block_starts()[1] == U.CLI_READS and hashlib.sha256(s.raw).digest() != hashlib.sha256(lay.raw).digest()


@pytest.mark.parametrize("case", list(U.HUGE))
def test_huge_header_cases(d, case):
    p, rec = U.huge_header_bam(d, case)
    lay = U.Layout(p)
    env = {"METHEOR_DEVICE_CHUNK_MB": "1"}
    chunks = U.plan_chunks(lay.coff, lay.csize, lay.isize, env)
    hows = U.chunk_paths(chunks, lay.hbytes, env)
    ends = np.cumsum([c["ubytes"] for c in chunks])
    print(case, lay.hbytes, [(c["b1"] - c["b0"], c["nbytes"], c["ubytes"]) for c in chunks], hows)
    assert len(rec) == 4500 and len(rec.refs) == U.HUGE[case][0]
    if case == "a":            # the header ends inside chunk 1
        assert hows == ["header only", "in line"] and ends[0] < lay.hbytes < ends[1]
    elif case == "c":          # it covers two whole chunks
        assert hows == ["header only", "header only", "in line"] and ends[1] < lay.hbytes < ends[2]
    else:                      # it ends with chunk 0's last byte; the next block is stored and too large to join
        assert hows == ["in line", "staged"] and ends[0] == lay.hbytes
        nxt = chunks[1]["b0"]
        assert int(lay.csize[nxt]) > int(lay.isize[nxt]) and int(lay.coff[nxt] + lay.csize[nxt] - lay.coff[0]) > U.MIB
        first_rec, n = lay.record_block_starts()
        whole = bool((np.diff(first_rec[lay.first_data_block():]) > 0).all()) and n == 4500
        o, straddles = lay.hbytes, 0                               # records whose first and last byte lie in different blocks
        while o < len(lay.raw):
            e = o + 4 + struct.unpack_from("<i", lay.raw, o)[0]
            straddles += int(np.searchsorted(lay.u0, o, side="right") != np.searchsorted(lay.u0, e - 1, side="right"))
            o = e
        assert (straddles > 20) if case == "b-cut" else (straddles == 0 and whole), (case, straddles)


def test_pieced_tables_hold_their_edges():
    t = U.pieced_tables()
    for name, (fb, coff, csize, isize, payloads) in t.items():
        assert U.is_pieced(len(fb), len(coff))
        for k in (0, len(coff) // 2, len(coff) - 1):
            assert zlib.decompress(fb[int(coff[k]):int(coff[k]) + int(csize[k])], -15) == payloads[k]
        end = coff.astype(np.int64) + csize.astype(np.int64)
        assert (end[:-1] + 8 <= coff.astype(np.int64)[1:]).all() and end[-1] + 8 <= len(fb)
    for name in ("mixed-2M", "mixed-3.6M"):
        fb, coff, csize, isize, _ = t[name]
        c0, c1 = coff.astype(np.int64), coff.astype(np.int64) + csize.astype(np.int64)
        assert ((c0 < U.MIB) & (c1 > U.MIB)).any(), name                  # a single block's payload spans a piece boundary
    pieces, launches = U.piece_plan(len(t["mixed-2M"][0]), t["mixed-2M"][1], t["mixed-2M"][2])
    assert len(pieces) == 2 and pieces[1] > U.MIB and len(launches) == 2    # the last piece is the merged one
    pieces, launches = U.piece_plan(len(t["mixed-3.6M"][0]), t["mixed-3.6M"][1], t["mixed-3.6M"][2])
    assert len(pieces) == 4 and pieces[3] >= U.MIB // 2 and len(launches) == 4
    # edge-equal: payload + 64 == the first piece's end.  `<` for `<=` would launch it a piece late: 3 launches instead of 4
    fb, coff, csize, _, _ = t["edge-equal"]
    assert int(coff[0]) + int(csize[0]) + 64 == U.MIB
    pieces, launches = U.piece_plan(len(fb), coff, csize)
    assert pieces == [U.MIB] * 3 and launches == [(0, 1), (1, 2), (2, 4)]
    # edge-slack: the payload has arrived with piece 2, its 64 bytes of slack have not.  Without the + 64: 3 launches instead of 2
    fb, coff, csize, _, _ = t["edge-slack"]
    assert 2 * U.MIB - 64 < int(coff[1]) + int(csize[1]) <= 2 * U.MIB
    pieces, launches = U.piece_plan(len(fb), coff, csize)
    assert pieces == [U.MIB] * 3 and launches == [(0, 1), (1, 3)]


def test_engine_has_the_three_methods_and_the_symbol():
    from metheor_amd import capi
    assert "mth_load_stats" in capi.SYMBOLS
    for m in ("bgzf_stage", "decode_reserve", "load_stats"):
        assert callable(getattr(capi.Engine, m))
    assert [f for f, _ in capi.mth_load_stats_t._fields_] == ["staged_calls", "inline_calls", "pieced_calls", "pieced_launches", "stage_misses", "decode_reallocs"]
    hdr = open(os.path.join(ROOT, "include", "metheor_hip.h")).read()
    m = re.search(r"typedef struct \{\s*uint64_t ([a-z_, ]+);\s*\} mth_load_stats_t;", hdr)
    assert m and [x.strip() for x in m.group(1).split(",")] == [f for f, _ in capi.mth_load_stats_t._fields_]
