"""GPU: BAMs whose records straddle BGZF blocks through the device load path (mth_bgzf_decode_straddle) -- the library call against
the oracle's decode on files cut at a byte count, the carry from call to call, decoy record headers that mislead the guess, records
that cover whole blocks; then the CLI: --region on such a file against the same command on its block-aligned copy, and whole-file
runs under METHEOR_DEVICE_STRADDLE=1 against the default route.  tests/test_straddle_inputs.py checks on the CPU that the inputs
hold these cases, and that the scheme modelled in Python settles on them.

Wall time of this file on an MI355X box: 21.5 s for its 32 tests (37 `metheor` runs among them; the slowest test 2.2 s)."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import straddle_util as S
from tests import test_irregular_paths as P
from tests import util
from tests.test_gpu_irregular_paths import MEASURES
from tests.test_host_decode import same_soa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
STREAM, DEVICE, STRADDLE = "  inflate + device record decode", "  device inflate + walk + decode", "  device inflate + straddle walk + decode"
ON = {"METHEOR_DEVICE_STRADDLE": "1"}


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("straddle"))


_made = {}


def made(d, name, rec_fn, cut, realistic=True):
    """(records, Layout, oracle SoA) of a file, written once per module"""
    key = (name, cut)
    if key not in _made:
        rec = rec_fn()
        lay = S.Layout(S.write_cut(os.path.join(d, "%s_%d.bam" % key), rec, cut, realistic=realistic))
        _made[key] = (rec, lay, pyoracle.Reads.decode(rec).soa())
    return _made[key]


def whole(eng, lay, **flags):
    return lay.call(eng, 0, len(lay.coff), lay.hbytes, last=True, **flags)[2]


# ---- the library ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", S.CUTS)
@pytest.mark.parametrize("name", ["weird", "irregular"])
def test_library_soa_equals_the_oracle(eng, d, name, cut):
    rec, lay, want = made(d, name, getattr(S, name), cut)
    info = whole(eng, lay)
    same_soa(eng.decoded_fetch(), want)
    assert info["rounds"] < S.MAX_ROUNDS and info["carry_bytes"] == 0, info
    if lay.wrong_guesses() == 0:
        assert info["repaired_blocks"] == 0 and info["rounds"] == 0
    # mth_bgzf_decode keeps refusing the file
    from metheor_amd import MthError
    with pytest.raises(MthError) as e:
        eng.bgzf_decode(lay.fb, lay.coff, lay.csize, lay.isize, lay.hbytes)
    assert e.value.status == -11
    eng.reset()


@pytest.mark.parametrize("n_calls", [2, 5, 9])
def test_carry_across_calls(eng, d, n_calls):
    """the 4 093-byte cut in 2, 5 and 9 calls, each cut before a block that starts inside a record: the SoA of one call, and every
    call leaves the bytes of its unfinished record"""
    rec, lay, want = made(d, "irregular", S.irregular, 4093)
    cuts = S.inside_cuts(lay, n_calls)
    infos = lay.in_calls(eng, cuts)
    same_soa(eng.decoded_fetch(), want)
    assert [i["carry_bytes"] for i in infos] == [lay.carry_after(c) for c in cuts] + [0]
    assert all(c > 0 for c in [i["carry_bytes"] for i in infos[:-1]])


def test_a_call_inside_one_record_and_the_ends_of_a_stream(eng, d):
    """the giant file: one call is a single block that begins and ends inside one record (nothing decoded, the carry grows by the
    block); a stream that stops inside a record is MTH_ERR_FORMAT under LAST and loses just that record under DROP_TAIL"""
    from metheor_amd import MthError
    rec, lay, want = made(d, "giant", S.RECIPES["giant"][0], 60000)
    b = S.block_inside_one_record(lay)
    infos = lay.in_calls(eng, [b, b + 1])
    same_soa(eng.decoded_fetch(), want)
    assert infos[1]["carry_bytes"] == infos[0]["carry_bytes"] + int(lay.isize[b]) == lay.carry_after(b + 1)
    # blocks [0, b + 1): the stream ends inside the giant record
    n_whole = int(np.searchsorted(lay.ends, int(lay.b1[b]), side="right"))
    assert 0 < n_whole < len(rec) and lay.starts[n_whole] < lay.b1[b] < lay.ends[n_whole]
    with pytest.raises(MthError) as e:
        lay.call(eng, 0, b + 1, lay.hbytes, last=True)
    assert e.value.status == -10
    eng.reset()
    n, _, info = lay.call(eng, 0, b + 1, lay.hbytes, drop_tail=True)
    assert n == n_whole and info["carry_bytes"] == 0
    same_soa(eng.decoded_fetch(), pyoracle.Reads.decode(rec.subset(range(n_whole))).soa())


@pytest.mark.parametrize("cut", [4093, 700])
def test_sparse_decoys_are_repaired(eng, d, cut):
    rec, lay, want = made(d, "sparse", S.RECIPES["sparse"][0], cut)
    info = whole(eng, lay)
    same_soa(eng.decoded_fetch(), want)
    assert info["repaired_blocks"] > 0 and 0 < info["rounds"] < S.MAX_ROUNDS, info


def test_dense_decoys_never_give_a_different_soa(eng, d):
    """decoys on every record, 700-byte blocks: the call gives up at the round bound (MTH_ERR_UNALIGNED) or is exact; after a reset the
    engine decodes the next file"""
    from metheor_amd import MthError
    rec, lay, want = made(d, "dense", S.RECIPES["dense"][0], 700)
    try:
        whole(eng, lay)
        same_soa(eng.decoded_fetch(), want)
    except MthError as e:
        assert e.status == -11, e
        assert eng.straddle_info["rounds"] == S.MAX_ROUNDS
    eng.reset()
    rec2, lay2, want2 = made(d, "irregular", S.irregular, 4093)
    whole(eng, lay2)
    same_soa(eng.decoded_fetch(), want2)


def test_giant_records(eng, d):
    rec, lay, want = made(d, "giant", S.RECIPES["giant"][0], 60000)
    info = whole(eng, lay)
    same_soa(eng.decoded_fetch(), want)
    assert info["repaired_blocks"] > 0 and 0 < info["rounds"] < S.MAX_ROUNDS, info      # blocks without a record start have no guess


def test_an_aligned_file_needs_no_round(eng, d):
    rec, lay, want = made(d, "irregular", S.irregular, 60000)
    ali = os.path.join(d, "aligned.bam")
    util.reblock_aligned(lay.path, ali)
    la = S.Layout(ali)
    eng.bgzf_decode(la.fb, la.coff, la.csize, la.isize, la.hbytes)
    ref = eng.decoded_fetch()
    info = whole(eng, la)
    same_soa(eng.decoded_fetch(), ref)
    same_soa(ref, want)
    assert info == dict(rounds=0, repaired_blocks=0, carry_bytes=0)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------
def run(env, *args):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, cwd=ROOT, timeout=600,
                          env=dict(os.environ, METHEOR_TIMING="1", METHEOR_SEED="2", **{k: str(v) for k, v in (env or {}).items()}))


def outputs(tmp_path, tag, env, sub, flags, bam, *more):
    """one run -> (result, output bytes with the input's path taken out, pairs table or None)"""
    o, pf = tmp_path / (tag + ".tsv"), tmp_path / (tag + ".pairs")
    r = run(env, sub, "-i", bam, "-o", o, *flags, *more, *(["-p", pf] if sub == "lpmd" else []))
    assert r.returncode == 0, (sub, tag, r.stderr)
    return r, o.read_bytes().replace(str(bam).encode(), b"<input>"), pf.read_bytes() if sub == "lpmd" else None


@pytest.fixture(scope="module")
def region(d):
    rd = os.path.join(d, "region")
    os.mkdir(rd)
    return S.region_inputs(rd)


@pytest.mark.parametrize("sub,flags", MEASURES, ids=[m[0] for m in MEASURES])
def test_region_on_a_straddling_file(region, tmp_path, sub, flags):
    """--region on the file cut every 4 093 bytes == the same command on its block-aligned copy, through the straddle walk; the
    region of test_irregular_paths.region_edges for every measure, and for pdr, lpmd and me the second one of test_straddle_inputs,
    which enters its first block at the index's record offset; pdr also against the oracle's rows the region owns"""
    rec, names, cut, ali = region
    for k, (t, b, e) in enumerate((P.region_edges(rec), S.SECOND_REGION)):
        if k == 1 and sub not in ("pdr", "me", "lpmd"):
            continue
        reg = "%s:%d-%d" % (names[t], b + 1, e)
        ra, out_a, pairs_a = outputs(tmp_path, "a%d" % k, {}, sub, flags, ali, "--region", reg)
        rc, out_c, pairs_c = outputs(tmp_path, "c%d" % k, {}, sub, flags, cut, "--region", reg)
        assert DEVICE in ra.stderr and STRADDLE not in ra.stderr, ra.stderr
        assert STRADDLE in rc.stderr and STREAM not in rc.stderr, rc.stderr
        assert out_c == out_a and pairs_c == pairs_a, (sub, k)
        assert len(out_c) > (10 if sub == "lpmd" else 1000)
        if sub == "pdr":
            want, _ = util.oracle_text(pyoracle.Reads.decode(rec), names, sub, seed=2, **util.oracle_kwargs(sub, flags))
            owned = "".join(l for l in want.splitlines(True) if l.split("\t")[0] == names[t] and b <= int(l.split("\t")[1]) < e)
            assert out_c.decode() == owned and len(owned) > 1000


def test_gpus_n_still_refuses_a_straddling_file(region, tmp_path):
    rec, names, cut, ali = region
    r = run(ON, "pdr", "-i", cut, "-o", tmp_path / "o.tsv", "--gpus", 2)
    assert r.returncode != 0 and "need the device load path" in r.stderr, r.stderr


@pytest.fixture(scope="module")
def chunked(d):
    p = S.write_cut(os.path.join(d, "chunked.bam"), S.chunked_records(), S.CHUNKED_CUT, realistic=True)
    return p


@pytest.mark.parametrize("sub,flags", MEASURES, ids=[m[0] for m in MEASURES])
def test_whole_file_under_the_switch(chunked, tmp_path, sub, flags):
    """METHEOR_DEVICE_STRADDLE=1 == the default route, which stays the host inflate; the run reports one library call per chunk: at
    least three, each but the last leaving the bytes of an unfinished record to the next"""
    env = {"METHEOR_DEVICE_CHUNK_MB": "1"}
    r0, out0, pairs0 = outputs(tmp_path, "off", env, sub, flags, chunked)
    r1, out1, pairs1 = outputs(tmp_path, "on", dict(env, **ON), sub, flags, chunked)
    assert STREAM in r0.stderr and STRADDLE not in r0.stderr, r0.stderr
    assert STRADDLE in r1.stderr and STREAM not in r1.stderr and "host decode" not in r1.stderr, r1.stderr
    assert out1 == out0 and pairs1 == pairs0 and len(out0) > (10 if sub == "lpmd" else 1000), sub
    calls = re.findall(r"^\[metheor straddle\] chunk (\d+) of (\d+): .* (\d+) bytes carried$", r1.stderr, re.M)
    assert len(calls) >= 3 and [int(c[0]) for c in calls] == list(range(1, len(calls) + 1)) and all(int(c[1]) == len(calls) for c in calls), r1.stderr
    assert all(int(c[2]) > 0 for c in calls[:-1]) and int(calls[-1][2]) == 0, calls


def test_file_order_replay_under_the_switch(tmp_path):
    """a flush-trap order cut every 4 093 bytes: pdr replays the file order from the straddle walk's stream as from the host's"""
    sh, bam = S.flush_trap_file(str(tmp_path))
    flags = ["-d", "1", "-p", "1"]
    r0, out0, _ = outputs(tmp_path, "off", {}, "pdr", flags, bam)
    r1, out1, _ = outputs(tmp_path, "on", ON, "pdr", flags, bam)
    assert "file-order replay" in r0.stderr and STREAM in r0.stderr
    assert "file-order replay" in r1.stderr and STRADDLE in r1.stderr and STREAM not in r1.stderr, r1.stderr
    want, _ = util.oracle_text(pyoracle.Reads.decode(sh), [n for n, _ in sh.refs], "pdr", min_depth=1, min_cpgs=1)
    assert out1 == out0 and out1.decode() == want and len(want) > 2000


def test_genome_calls_under_the_switch(tmp_path):
    """pdr -g on an untagged file cut every 4 093 bytes == on the file as the converter wrote it (whole records per block)"""
    ali, cut, fa = S.genome_files(str(tmp_path))
    flags = ["-d", "1", "-p", "1", "-g", fa]
    ra, out_a, _ = outputs(tmp_path, "a", {}, "pdr", flags, ali)
    rc, out_c, _ = outputs(tmp_path, "c", ON, "pdr", flags, cut)
    assert DEVICE in ra.stderr and STRADDLE in rc.stderr and STREAM not in rc.stderr, rc.stderr
    assert out_c == out_a and out_a.count(b"\n") >= 500
