"""GPU: the device inflater (k_inflate, mth_inflate.hip) on DEFLATE streams zlib's deflate never writes -- the VALID corpus of
tests/deflate_streams.py byte for byte against the bytes its tokens mean, with the hand-written literal loop and (in a child process,
METHEOR_INFLATE_ASM=0) with the general symbol loop alone; the INVALID corpus, one stream per rejection, each between two good
members: MTH_ERR_FORMAT and a usable engine after reset(); and files cut at 65498 and 65536 inflated bytes per block through
bgzf_inflate and the CLI.  tests/test_deflate_streams.py holds every case against zlib on the CPU.

Wall time of this file on an MI355X box: 7.8 s for its 45 tests; the child process 2.4 s, a CLI run 0.4 - 0.8 s, every other test
under 0.05 s."""
import os
import subprocess
import sys

import pytest

from oracle import pyoracle
from tests import deflate_streams as D
from tests import util
from tests.test_deflate_streams import FILE_CUTS, cut_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metheor_amd", "metheor")
STREAM, STRADDLE = "  inflate + device record decode", "  device inflate + straddle walk + decode"


@pytest.fixture(scope="module")
def eng():
    import metheor_amd
    e = metheor_amd.Engine(0)
    yield e
    e.close()


def inflate_cases(eng, cases):
    """the cases as one call; a difference names the case and the first differing byte"""
    fb, coff, csize, isize, want = D.frame(cases)
    got = eng.bgzf_inflate(fb, coff, csize, isize).tobytes()
    assert len(got) == len(want)
    o = 0
    for c in cases:
        g = got[o:o + len(c.data)]
        if g != c.data:
            bad = next(i for i in range(len(c.data)) if g[i] != c.data[i])
            raise AssertionError("%s: %s: first difference at byte %d of %d" % (c.group, c.name, bad, len(c.data)))
        o += len(c.data)


def test_valid_corpus_in_one_call(eng):
    inflate_cases(eng, D.VALID)


@pytest.mark.parametrize("group", D.GROUPS)
def test_valid_corpus_by_group(eng, group):
    cases = [c for c in D.VALID if c.group == group]
    assert cases
    inflate_cases(eng, cases)


CHILD = """
import metheor_amd
from tests import deflate_streams as D
eng = metheor_amd.Engine(0)
bad = []
for c in D.VALID:                      # one call per case: a refused one is named like a wrong one
    fb, coff, csize, isize, want = D.frame([c])
    try:
        if eng.bgzf_inflate(fb, coff, csize, isize).tobytes() != want:
            bad.append(c.name)
    except metheor_amd.MthError:
        bad.append(c.name + " (refused)")
        eng.reset()
fb, coff, csize, isize, want = D.frame(D.VALID)
if eng.bgzf_inflate(fb, coff, csize, isize).tobytes() != want:
    bad.append("the whole corpus in one call")
eng.close()
print("cases %d" % len(D.VALID))
print("mismatching %r" % (bad,))
"""


def test_valid_corpus_with_the_fast_literal_loop_off():
    """METHEOR_INFLATE_ASM is read once per process: a fresh child with the switch at 0 inflates the corpus with the general loop only"""
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, cwd=ROOT, timeout=120,
                       env=dict(os.environ, METHEOR_INFLATE_ASM="0"))
    assert r.returncode == 0, r.stderr
    assert "cases %d\n" % len(D.VALID) in r.stdout, r.stdout
    assert "mismatching []\n" in r.stdout, r.stdout


GOOD = [c for c in D.VALID if c.name in ("stored then fixed", "three dynamic blocks")]


@pytest.mark.parametrize("c", D.INVALID, ids=[c.name for c in D.INVALID])
def test_invalid_case_is_refused(eng, c):
    from metheor_amd import MthError
    assert len(GOOD) == 2
    fb, coff, csize, isize, _ = D.frame(GOOD + [c] if c.last else [GOOD[0], c, GOOD[1]])
    if c.last:
        assert int(coff[2]) + int(csize[2]) + 8 == len(fb)
    with pytest.raises(MthError) as e:
        eng.bgzf_inflate(fb, coff, csize, isize)
    assert e.value.status == -10
    eng.reset()
    inflate_cases(eng, GOOD)


# ---- files whose blocks inflate to 65498 and to 65536 bytes -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cuts"))
    return {cut: cut_file(d, cut) for cut in FILE_CUTS}


@pytest.mark.parametrize("cut", FILE_CUTS)
def test_file_cut_inflates_to_what_gzip_reads(eng, cuts, cut):
    rec, lay = cuts[cut]
    assert int(lay.isize.max()) == cut
    got = eng.bgzf_inflate(lay.fb, lay.coff, lay.csize, lay.isize).tobytes()
    assert len(got) == len(lay.raw)
    if got != lay.raw:
        bad = next(i for i in range(len(got)) if got[i] != lay.raw[i])
        raise AssertionError("first difference at byte %d of %d (block %d)" % (bad, len(got), bad // cut))


@pytest.mark.parametrize("sub,flags", [("pdr", ["-d", "1", "-p", "1"]), ("lpmd", ["-m", "1", "-M", "40"])], ids=["pdr", "lpmd"])
@pytest.mark.parametrize("cut", FILE_CUTS)
def test_file_cut_through_the_cli(cuts, tmp_path, cut, sub, flags):
    """the device load path (inflate, straddle walk, decode) on the file == the oracle's rows"""
    rec, lay = cuts[cut]
    o, pf = tmp_path / "o.tsv", tmp_path / "o.pairs"
    r = subprocess.run([EXE, sub, "-i", lay.path, "-o", str(o), *flags, *(["-p", str(pf)] if sub == "lpmd" else [])],
                       capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, METHEOR_TIMING="1", METHEOR_SEED="2", METHEOR_DEVICE_STRADDLE="1"))
    assert r.returncode == 0, r.stderr
    assert STRADDLE in r.stderr and STREAM not in r.stderr, r.stderr
    want, want_pairs = util.oracle_text(pyoracle.Reads.decode(rec), [n for n, _ in rec.refs], sub, input_name=lay.path,
                                        **util.oracle_kwargs(sub, flags))
    assert o.read_text() == want and len(want) > (10 if sub == "lpmd" else 1000)
    if sub == "lpmd":
        assert pf.read_text() == want_pairs and len(want_pairs) > 1000
