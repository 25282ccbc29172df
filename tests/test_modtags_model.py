"""The per-record routine of `--mm-tags` on the CPU.  metheor_amd/csrc/mth_modtags_dev.h compiles under
MTH_MODTAGS_HOST_MODEL into a stand-alone program (its own main, g++ with the address and undefined-behaviour sanitizers),
so the very text the device runs is exercised here: raw BAM records in, X(record, T) or the error out, against the Python
restatement of the rule (tests/modtags_util.py) on the generated set, on every error case and on crafted aux fields."""
import os
import struct
import subprocess

import pytest

from tests import modtags_util as M

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#define MTH_MODTAGS_HOST_MODEL
#include "mth_modtags_dev.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace mth;
// IN: u32 threshold, then per record u32 n + n bytes (a BAM record, block_size first).  OUT: a line per record: "F" malformed
// record, "L" longer than 65535, "E" error, "S<X>" contributes nothing, "X<X>" otherwise
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t T, n;
    if (fread(&T, 4, 1, f) != 1) return 2;
    while (fread(&n, 4, 1, f) == 1) {
        std::vector<uint8_t> rec(n);                                   // exactly n bytes: the sanitizer sees any byte read past the record
        if (n && fread(rec.data(), 1, n, f) != n) return 2;
        uint32_t bs = 0;
        if (n >= 4) memcpy(&bs, rec.data(), 4);
        if (n < 36 || bs != n - 4) { fputs("F\n", o); continue; }
        const uint8_t *p = rec.data() + 4;
        const uint32_t len = n - 4, l_read_name = p[8];
        uint16_t n_cigar, flag;
        uint32_t l_seq;
        memcpy(&n_cigar, p + 12, 2); memcpy(&flag, p + 14, 2); memcpy(&l_seq, p + 16, 4);
        const uint64_t o_cigar = 32ull + l_read_name, o_seq = o_cigar + 4ull * n_cigar, o_aux = o_seq + ((uint64_t)l_seq + 1) / 2 + l_seq;
        if (o_aux > len) { fputs("F\n", o); continue; }
        if (l_seq > 65535u) { fputs("L\n", o); continue; }
        const bool reverse = flag & 16u;
        MmPlan P;
        mm_prepare(p, len, (uint32_t)o_cigar, n_cigar, (uint32_t)o_seq, l_seq, (uint32_t)o_aux, reverse, P);
        if (P.status == MM_ERROR) { fputs("E\n", o); continue; }
        std::string x(l_seq, '.');
        if (P.status == MM_CALLS) {
            MmWalk W;
            W.init(P, p + o_seq, l_seq, reverse, T);
            for (uint32_t q = 0; q < l_seq; ++q) { const uint32_t ch = W.step(q); x[q] = ch == 2 ? 'Z' : ch == 1 ? 'z' : '.'; }
        }
        fprintf(o, "%c%s\n", P.status == MM_NOTHING ? 'S' : 'X', x.c_str());
    }
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("modtags_model")
    src = d / "modtags_model.cpp"
    src.write_text(DRIVER)
    out = d / "modtags_model"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


def model(exe, tmp_path, raws, T):
    inp, outp = tmp_path / "recs.bin", tmp_path / "x.txt"
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", T))
        for r in raws:
            f.write(struct.pack("<I", len(r)) + r)
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = outp.read_text().split("\n")[:-1]
    assert len(lines) == len(raws)
    return lines


def expected(rec, T):
    try:
        x, nothing = M.x_string(rec, T)
    except M.ModTagError:
        return "E"
    return ("S" if nothing else "X") + x


@pytest.mark.parametrize("T", [0, 128, 255])
def test_the_generated_set_equals_the_restatement(exe, tmp_path, T):
    g = M.generate(11, 6000)
    got = model(exe, tmp_path, [M.pack_record(r) for r in g["recs"]], T)
    bad = [(r.name, r.flag, r.cigar, r.tags) for r, x in zip(g["recs"], got) if x != expected(r, T)]
    assert not bad, (len(bad), bad[:3])
    assert sum(x.count("Z") for x in got) > (0 if T == 255 else 20000) and sum(x[0] == "S" for x in got) > 100


def test_the_worked_examples(exe, tmp_path):
    seq = "ACGTCGCCGA"
    cases = [(0, "C+m?,1,1;", "200,30", "X....Z..z.."), (0, "C+m.,1,1;", "200,30", "X.z..Z..z.."), (0, "C+m,1,1;", "200,30", "X.z..Z..z.."),
             (0, "C+hm?,1,1;", "5,200,7,30", "X....Z..z.."), (0, "A+a?,0;C+m?,1,1;", "99,200,30", "X....Z..z.."), (0, "C+m?,1,1,0;", None, "E"),
             (16, "C+m?,0,1;", "10,250", "X..Z.....z.")]
    raws = [M.pack_record(M.Rec("r", flag, 99, 30, "10M", seq, ["MM:Z:" + mm] + (["ML:B:C," + ml] if ml else []))) for flag, mm, ml, _ in cases]
    assert model(exe, tmp_path, raws, 128) == [c[3] for c in cases]


def test_every_error_case_is_an_error(exe, tmp_path):
    cases = M.error_recs()
    got = model(exe, tmp_path, [M.pack_record(r) for _, r in cases], 128)
    assert [(w, x) for (w, _), x in zip(cases, got) if x != "E"] == []
    # the same fields behind a hard clip or an MN that differs contribute nothing instead: checked before MM / ML are looked at
    skipped = [M.Rec(r.name, r.flag, r.pos, r.mapq, "2H10M", r.seq, r.tags) for _, r in cases] + \
              [M.Rec(r.name, r.flag, r.pos, r.mapq, r.cigar, r.seq, r.tags + ["MN:i:11"]) for _, r in cases]
    assert set(model(exe, tmp_path, [M.pack_record(r) for r in skipped], 128)) == {"S.........."}


def test_crafted_aux_fields_end_as_errors_not_as_hangs(exe, tmp_path):
    r = M.Rec("r", 0, 99, 30, "10M", "ACGTCGCCGA", [])
    mm = b"MMZC+m?,1,1;\0"
    crafted = {
        # count * 4 wraps a 32-bit cursor back to the start of the field: the walk would never leave
        "count wraps the cursor": b"XBBI" + struct.pack("<I", 0x3ffffffe) + mm,
        "count past the record": b"XBBC" + struct.pack("<I", 1000) + mm,
        "count 2^32 - 1 of bytes": mm + b"MLBC" + struct.pack("<I", 0xffffffff),
        "B without its count": mm + b"XBBC\1",
        "unknown B subtype": b"XBBZ" + struct.pack("<I", 0) + mm,
        "unknown type": b"XBQ\0" + mm,
        "Z without its NUL": b"MMZC+m?,1,1;",
        "two bytes left over": mm + b"XY",
        "an integer cut short": mm + b"MNi\1\0",
    }
    got = model(exe, tmp_path, [M.pack_record(r, raw_aux=a) for a in crafted.values()], 128)
    assert dict(zip(crafted, got)) == {k: "E" for k in crafted}
    # field lengths that leave the record, and a read too long for 16-bit offsets
    raw = bytearray(M.pack_record(r, raw_aux=mm))
    struct.pack_into("<I", raw, 4 + 16, 1000)                         # l_seq
    long_read = M.pack_record(M.Rec("r", 0, 99, 30, "65536M", "A" * 65536, []))
    assert model(exe, tmp_path, [bytes(raw), long_read, M.pack_record(r, raw_aux=mm)], 128) == ["F", "L", "X....Z..Z.."]


def test_types_and_spellings_that_count_as_absent(exe, tmp_path):
    seq = "ACGTCGCCGA"
    recs = [M.Rec("r", 0, 99, 30, "10M", seq, ["Mm:Z:C+m?,1;", "Ml:B:C,200"]),                         # old spellings
            M.Rec("r", 0, 99, 30, "10M", seq, ["MM:i:5", "ML:Z:junk"]),                                 # MM not of type Z: ML is not looked at
            M.Rec("r", 0, 99, 30, "10M", seq, ["MM:i:5", "MM:Z:C+m.,1;", "ML:B:C,200"]),                # ... a later MM:Z counts
            M.Rec("r", 0, 99, 30, "10M", seq, ["MM:Z:C+m?,0;", "MM:Z:C+m?,1;", "ML:B:C,200", "ML:Z:x"]),   # the first of each
            M.Rec("r", 0, 99, 30, "10M", seq, ["MN:i:10", "MN:i:11", "MM:Z:C+m?,0;"])]
    want = ["X..........", "X..........", "X.z..Z..z..", "X.Z........", "X.Z........"]
    assert [expected(r, 128) for r in recs] == want
    assert model(exe, tmp_path, [M.pack_record(r) for r in recs], 128) == want
