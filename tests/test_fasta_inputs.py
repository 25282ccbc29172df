"""The inputs of tests/test_gpu_fasta.py are what that file takes them to be (no GPU): the generated .fa.gz files hold their
plain twins, the .fai rows match the text, the host reader returns the Python sequences, the BGZF cuts land where the cases
say, and the new host calls refuse what they must."""
import gzip

import pytest

from metheor_amd import hostapi
from tests import fasta_util as fu

CASES = fu.cases()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_inputs")
    return {k: fu.build(c, d, k) for k, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_gz_holds_the_plain_twin_and_the_fai_matches_the_text(built, name):
    c, b = CASES[name], built[name]
    assert gzip.decompress(b["blob"]) == b["text"] == open(b["fa"], "rb").read()       # (gzip reads multi-member files)
    assert b["blob"].endswith(fu.EOF_BLOCK)
    eol = c["eol"]
    for (nm, seq, w), (rn, length, off, lb, lw) in zip(c["contigs"], b["rows"]):
        assert (rn, length, lb, lw) == (nm, len(seq), w, w + len(eol))
        assert b["text"][:off].endswith(b">" + nm.encode() + eol)
        # the bytes from the row's offset on, line ends taken out, are the sequence
        lines = (length + lb - 1) // lb
        raw = b["text"][off:off + length + lines * len(eol)]
        assert raw.replace(b"\r", b"").replace(b"\n", b"")[:length] == seq
        for i in (0, lb - 1, lb, length - 1):                                           # the gather's formula on single bases
            if 0 <= i < length:
                assert b["text"][off + (i // lb) * lw + i % lb] == seq[i]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_fetch_and_layout_of_the_plain_file(built, name):
    c, b = CASES[name], built[name]
    seqs = {x[0]: x[1] for x in c["contigs"]}
    rows = {r[0]: r for r in b["rows"]}
    fa = hostapi.Fasta(b["fa"])
    gz = hostapi.Fasta(b["gz"])
    assert not fa.compressed and gz.compressed
    m = gz.map()
    coff, csize, isize = fu.bgzf_table(b["blob"])
    assert m["compressed"] and m["stream_bytes"] == len(b["text"]) and bytes(m["file"]) == b["blob"]
    assert (m["coff"] == coff).all() and (m["csize"] == csize).all() and (m["isize"] == isize).all()
    pm = fa.map()
    assert not pm["compressed"] and pm["coff"] is None and pm["stream_bytes"] == len(b["text"]) and bytes(pm["file"]) == b["text"]
    for nm, ln in c["header"]:
        want = fu.want_bases(seqs[nm], ln)
        assert fa.fetch(nm, ln) == want
        for f in (fa, gz):
            r = f.layout(nm, ln)
            assert (r.src_off, r.n_bases, r.line_bases, r.line_width, r.name) == (rows[nm][2], len(want), rows[nm][3], rows[nm][4], nm.encode())
        with pytest.raises(hostapi.HostError) as e:
            gz.fetch(nm, ln)
        assert "read on the device" in str(e.value)
    fa.close(); gz.close()


def test_block_cuts_land_on_the_intended_boundaries(built):
    c, b = CASES["block_edges"], built["block_edges"]
    text, spans, rows = b["text"], b["spans"], {r[0]: r for r in b["rows"]}
    starts = [s for s, _ in spans]
    assert text[starts[1]:starts[1] + 1] == b"\n" and text[starts[1] - 1:starts[1]] != b"\n"          # a block that starts on a line feed
    assert text[starts[2] - 1:starts[2]] == b"\n" and text[starts[2]] in b"ACGT"                      # one that starts on the first base of a line
    hdr = text.index(b">long\n")
    assert hdr < starts[3] < hdr + len(b">long\n")                                                    # a header line split across two blocks
    off, length = rows["long"][2], rows["long"][1]
    end = off + length + (length + 59) // 60
    inside = [k for k, (s, e) in enumerate(spans) if s < end and e > off]
    assert len(inside) >= 4                                                                           # a contig over three blocks or more
    # and a contig that starts mid-block, after another one
    assert any(s < rows["long"][2] < e for s, e in spans)


def test_all_three_deflate_block_types_are_present(built):
    seen = set()
    for name in ("w60", "block_edges"):
        coff, _, _ = fu.bgzf_table(built[name]["blob"])
        seen |= {fu.first_btype(built[name]["blob"], o) for o in coff}
    assert seen == {0, 1, 2}, seen
    coff, _, _ = fu.bgzf_table(built["block_edges"]["blob"])
    assert sum(1 for o in coff if fu.first_btype(built["block_edges"]["blob"], o) == 2) >= 4          # ~30 kB of ACGT lines at level 6: dynamic


def test_empty_blocks_sit_mid_file(built):
    b = built["crlf"]
    blob = b["blob"]
    coff, _, _ = fu.bgzf_table(blob)
    empty = fu.bgzf_block(b"")
    at = blob.find(empty)
    assert 0 < at < int(coff[-1]) and blob.count(empty) >= 2


# ---- what the new host calls refuse ------------------------------------------------------------------------------------------
def test_plain_gzip_is_refused(tmp_path):
    p = tmp_path / "g.fa.gz"
    p.write_bytes(gzip.compress(b">c0\nACGT\n"))
    (tmp_path / "g.fa.gz.fai").write_text("c0\t4\t4\t4\t5\n")
    with pytest.raises(hostapi.HostError) as e:
        hostapi.Fasta(str(p))
    assert "bgzip" in str(e.value) and "not BGZF" in str(e.value)


def test_bgzf_without_fai_is_refused_and_names_the_index(tmp_path):
    p = tmp_path / "g.fa.gz"
    p.write_bytes(fu.bgzf_bytes(b">c0\nACGT\n", [100])[0])
    with pytest.raises(hostapi.HostError) as e:
        hostapi.Fasta(str(p))
    assert str(p) + ".fai" in str(e.value) and "samtools faidx" in str(e.value)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "bgzf"])
def test_missing_contig_gives_the_fetch_text(built, gz):
    f = hostapi.Fasta(built["w60"]["gz" if gz else "fa"])
    with pytest.raises(hostapi.HostError) as e:
        f.layout("nowhere", 10)
    assert str(e.value) == "sequence not in the FASTA: nowhere"
    f.close()


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "bgzf"])
def test_fai_past_the_end_of_the_stream_is_refused_on_the_host(tmp_path, gz):
    text, rows = fu.fasta_text([("c0", b"ACGT" * 50)], 60)
    p = tmp_path / ("g.fa.gz" if gz else "g.fa")
    p.write_bytes(fu.bgzf_bytes(text, [90])[0] if gz else text)
    name, length, off, lb, lw = rows[0]
    (tmp_path / (p.name + ".fai")).write_text(fu.fai_text([(name, length + 100, off, lb, lw)]))
    f = hostapi.Fasta(str(p))
    assert f.layout("c0", 150).n_bases == 151                                        # what is asked for lies inside the file
    with pytest.raises(hostapi.HostError) as e:
        f.layout("c0", 400)                                                             # min(LN + 1, 300) bases: past the end
    assert str(e.value) == "FASTA shorter than its index says: " + str(p)
    if not gz:
        with pytest.raises(hostapi.HostError) as e2:
            f.fetch("c0", 400)
        assert str(e2.value) == str(e.value)                                            # the fetch's own text
    f.close()
