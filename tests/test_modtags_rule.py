"""The rule of `--mm-tags` (mth_decode_set_modtags; include/metheor_hip.h): the worked examples, the error cases, the
generator's coverage, and the CPU oracle's decode of F' against a computation of the calls straight from the tags."""
import os
import re

import numpy as np
import pytest

from oracle import bamio, pyoracle
from tests import modtags_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = "ACGTCGCCGA"


def test_the_rule_is_in_the_header_and_the_library_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "metheor_hip.h")).read()
    assert re.search(r"int\s+mth_decode_set_modtags\(mth_ctx_t \*ctx, int enabled, uint32_t threshold\);", src)
    assert "MTH_NOTE_MODTAG_SKIPPED" in src and "flag & 0x10" in src
    from metheor_amd import capi
    assert "mth_decode_set_modtags" in capi.SYMBOLS and hasattr(capi.Engine, "decode_set_modtags")


def rec(flag, mm, ml):
    return M.Rec("r", flag, 99, 30, "10M", SEQ, ["MM:Z:" + mm] + (["ML:B:C," + ml] if ml else []))


def calls(r, T=128):
    """(1-based-free) reference positions of the calls of F', through the oracle: [(position, methylated)]"""
    s = decode_fprime([r], T)
    return [(int(w & 0x7fffffff), bool(w >> 31)) for w in s["cpg_pos"]]


def oracle_soa(path):
    rec = bamio.read_sam(str(path))
    rec.xms = [x if x else b"." for x in rec.xms]        # (the oracle's record block cannot hold an EMPTY tag: one dot, no call either)
    return pyoracle.Reads.decode(rec).soa()


def decode_fprime(recs, T):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fp.sam")
        open(p, "w").write(M.sam_text([("c0", 100000)], [M.fprime(r, T) for r in recs]))
        return oracle_soa(p)


@pytest.mark.parametrize("mm,ml,x", [
    ("C+m?,1,1;", "200,30", "....Z..z.."),
    ("C+m.,1,1;", "200,30", ".z..Z..z.."),
    ("C+m,1,1;", "200,30", ".z..Z..z.."),
    ("C+hm?,1,1;", "5,200,7,30", "....Z..z.."),
    ("A+a?,0;C+m?,1,1;", "99,200,30", "....Z..z.."),
])
def test_worked_examples_forward(mm, ml, x):
    assert [q for q, c in enumerate(SEQ) if c == "C"] == [1, 4, 6, 7]
    assert M.x_string(rec(0, mm, ml), 128) == (x, False)


def test_worked_example_calls():
    assert calls(rec(0, "C+m?,1,1;", "200,30")) == [(103, True), (106, False)]          # 0-based: the text's 104 and 107
    with pytest.raises(M.ModTagError):
        M.x_string(rec(0, "C+m?,1,1,0;", None), 128)                                      # no fifth C


def test_worked_example_reverse():
    assert "".join(M.COMP[c] for c in reversed(SEQ)) == "TCGGCGACGT"
    r = rec(16, "C+m?,0,1;", "10,250")
    assert M.x_string(r, 128) == ("..Z.....z.", False)
    # the first ML entry belongs to the LATER position; the calls are in ascending position; one below the aligned position
    assert calls(r) == [(100, True), (106, False)]                                        # 0-based: the text's 101 and 107
    fwd = {p for p, _ in calls(rec(0, "C+m.,0,0,0,0;", None))}
    rev = {p for p, _ in calls(rec(16, "C+m.,0,0,0;", None))}
    assert fwd == rev == {100, 103, 106}                                                  # both strands land on the top-strand C


def test_the_flag_rewrite():
    for flag in (0, 16) + M.PAIRED_FLAGS:
        f = M.fprime(rec(flag, "C+m?,0;", None), 128)
        assert f.flag == (flag & 0x10) and [t for t in f.tags if t.startswith("XM:Z:")] == ["XM:Z:" + M.x_string(rec(flag, "C+m?,0;", None), 128)[0]]
    withxm = M.Rec("r", 99, 99, 30, "10M", SEQ, ["XM:Z:ZZZZZZZZZZ", "MM:Z:C+m?,0;", "XM:Z:zzzzzzzzzz"])
    assert [t for t in M.fprime(withxm, 128).tags if t.startswith("XM")] == ["XM:Z:.Z........"]


@pytest.mark.parametrize("what,r", M.error_recs(), ids=[w for w, _ in M.error_recs()])
def test_every_error_case_raises(what, r):
    with pytest.raises(M.ModTagError):
        M.x_string(r, 128)


def test_records_that_contribute_nothing():
    tags = ["MM:Z:C+m.,0;"]
    assert M.x_string(M.Rec("r", 0, 99, 30, "20M", "*", tags), 128) == ("", True)
    assert M.x_string(M.Rec("r", 0, 99, 30, "3H10M", SEQ, tags), 128) == ("." * 10, True)
    assert M.x_string(M.Rec("r", 0, 99, 30, "10M", SEQ, tags + ["MN:i:12"]), 128) == ("." * 10, True)
    assert M.x_string(M.Rec("r", 0, 99, 30, "10M", SEQ, tags + ["MN:i:10"]), 128) == (".Z..z..z..", False)
    assert M.x_string(M.Rec("r", 0, 99, 30, "10M", SEQ, ["Mm:Z:C+m.,0;"]), 128) == ("." * 10, False)
    assert M.x_string(M.Rec("r", 0, 99, 30, "10M", SEQ, ["MM:Z:C-m.,0;N+m.,0;C+76792.,0;C+h.,0;"]), 128) == ("." * 10, False)
    assert M.x_string(M.Rec("r", 0, 99, 30, "10M", SEQ, ["MM:Z:"]), 128) == ("." * 10, False)


@pytest.fixture(scope="module")
def big():
    return M.generate(7, 20000)


NAMED = (["forward", "reverse"] + ["flag%d" % f for f in M.PAIRED_FLAGS] + ["len%d" % n for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 150)] +
         ["len~3000", "C_last_forward", "G_first_reverse", "softclip", "ins_between_CG", "deletion", "N", "hardclip", "list_ends_on_last_C",
          "multi_digit", "mode_.", "mode_?", "mode_none", "codes_hm", "codes_mh", "foreign_lead", "foreign_trail", "foreign_C-m", "foreign_N+m",
          "foreign_numeric", "no_ML", "MN_equal", "MN_unequal", "ml0", "ml127", "ml128", "ml255"])


def test_the_generator_produces_every_category(big):
    short = {k: big["cats"][k] for k in NAMED if big["cats"][k] < 50}
    assert not short, short
    # and what the counters claim is in the records
    recs = big["recs"]
    assert sum(1 for r in recs if "H" in r.cigar) == big["cats"]["hardclip"] >= 50
    assert sum(1 for r in recs if 2900 <= len(r.seq) < 3100) == big["cats"]["len~3000"]
    assert sum(1 for r in recs if r.seq == "") == big["cats"]["len0"]
    assert sum(1 for r in recs if M.tag(r.tags, "MM", "Z") and not M.tag(r.tags, "ML")) == big["cats"]["no_ML"]
    assert sum(1 for r in recs if any(re.search(r",\d\d", t) for t in r.tags if t.startswith("MM:Z:"))) >= big["cats"]["multi_digit"]
    n_err = 0
    for r in recs:
        try:
            M.x_string(r, 128)
        except M.ModTagError:
            n_err += 1
    assert n_err == 0                                                  # F' exists for every generated record


def direct_calls(r, T):
    """[(position, methylated, query offset)] in ascending query offset, worked out in STORED terms and by splitting the
    string -- another route than modtags_util.x_string, which follows the text through the original read"""
    seq = r.seq
    L = len(seq)
    mn = [t for t in r.tags if t.startswith("MN:i:")]
    if L == 0 or "H" in r.cigar or (mn and int(mn[0][5:]) != L):
        return []
    mm = [t[5:] for t in r.tags if t.startswith("MM:Z:")]
    if not mm:
        return []
    ml = [t for t in r.tags if t.startswith("ML:")]
    probs = [int(v) for v in ml[0].split(",")[1:]] if ml else None
    chosen, owned = None, 0
    for g in mm[0].split(";")[:-1]:
        head, *nums = g.split(",")
        code = head[2:].rstrip(".?")
        k = len(code) if code.isalpha() else 1
        if chosen is None and head[:2] == "C+" and code.isalpha() and "m" in code:
            chosen = (owned, k, code.find("m"), head[-1] == "?", [int(v) for v in nums])
        owned += k * len(nums)
    assert probs is None or len(probs) == owned
    if chosen is None:
        return []
    base, k, im, open_mode, nums = chosen
    reverse = bool(r.flag & 16)
    fund = [q for q in range(L) if seq[q] == "C"] if not reverse else [q for q in range(L - 1, -1, -1) if seq[q] == "G"]
    which = (np.cumsum(np.asarray(nums, np.int64) + 1) - 1).tolist() if nums else []
    prob = {fund[f]: (255 if probs is None else probs[base + i * k + im]) for i, f in enumerate(which)}
    ref, q, at = {}, 0, r.pos
    for n, o in M.cigar_ops(r.cigar):
        if o in "M=X":
            for j in range(n):
                ref[q + j] = at + j
            q += n; at += n
        elif o in "IS":
            q += n
        elif o in "DN":
            at += n
    out = []
    for q in sorted(fund):
        in_cpg = (q >= 1 and seq[q - 1] == "C") if reverse else seq[q + 1:q + 2] == "G"
        if not in_cpg or q not in ref or (q not in prob and open_mode):
            continue
        out.append((ref[q] - (1 if reverse else 0), q in prob and prob[q] >= T, q))
    return out


@pytest.mark.parametrize("T", [0, 128, 255])
def test_oracle_decode_of_fprime_equals_the_direct_computation(big, tmp_path, T):
    recs = big["recs"] if T == 128 else big["recs"][:4000]
    p = tmp_path / "fp.sam"
    p.write_text(M.sam_text(big["refs"], [M.fprime(r, T) for r in recs]))
    s = oracle_soa(p)
    assert len(s["tid"]) == len(recs)
    n_calls = 0
    for i, r in enumerate(recs):
        a, b = int(s["cpg_off"][i]), int(s["cpg_off"][i + 1])
        got = [(int(w & 0x7fffffff), bool(w >> 31), int(q)) for w, q in zip(s["cpg_pos"][a:b], s["cpg_rel"][a:b])]
        assert got == direct_calls(r, T), (r.name, r.flag, r.cigar, r.tags)
        assert bool(s["fwd"][i]) == (not r.flag & 16)
        n_calls += b - a
    assert n_calls > 50000
