"""The inputs of tests/test_gpu_straddle.py on the CPU (tests/straddle_util.py): each holds the case it is named for, and the scheme
of mth_bgzf_decode_straddle, modelled in Python over the same bytes, finds exactly the true record offsets on them."""
import os

import numpy as np
import pytest

from tests import straddle_util as S


@pytest.fixture(scope="module")
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp("straddle_inputs"))


@pytest.mark.parametrize("name", ["weird", "irregular"])
def test_cuts_land_inside_records_and_the_model_finds_the_offsets(d, name):
    rec = getattr(S, name)()
    for cut in S.CUTS:
        lay = S.Layout(S.write_cut(os.path.join(d, "%s_%d.bam" % (name, cut)), rec, cut, realistic=True))
        assert len(lay.b0) >= 10 and lay.blocks_cut_inside_a_record() >= 0.9, (cut, lay.blocks_cut_inside_a_record())
        m = S.model(lay)
        assert m["settled"] and m["rounds"] <= 2 and (m["offsets"] == lay.starts).all(), (cut, m["rounds"])
        assert (m["repaired_blocks"] == 0) == (lay.wrong_guesses() == 0)


@pytest.mark.parametrize("cut", [4093, 700])
def test_sparse_decoys_mislead_the_guess(d, cut):
    lay = S.Layout(S.write_cut(os.path.join(d, "sparse_%d.bam" % cut), S.RECIPES["sparse"][0](), cut, realistic=True))
    assert lay.blocks_cut_inside_a_record() >= 0.9
    g = lay.guesses()
    later = lay.b0 > lay.hbytes
    assert int(np.sum(later & (g >= 0) & ~np.isin(g, lay.starts))) >= 5          # guesses that are no record start at all
    m = S.model(lay)
    assert m["settled"] and 0 < m["rounds"] < S.MAX_ROUNDS and m["repaired_blocks"] > 0 and (m["offsets"] == lay.starts).all()


def test_dense_decoys_mislead_most_blocks(d):
    lay = S.Layout(S.write_cut(os.path.join(d, "dense_700.bam"), S.RECIPES["dense"][0](), 700, realistic=True))
    assert lay.blocks_cut_inside_a_record() >= 0.9
    assert lay.wrong_guesses() >= len(lay.b0) // 2
    m = S.model(lay)
    assert not m["settled"] or (m["offsets"] == lay.starts).all()


def test_giant_records_cover_whole_blocks(d):
    lay = S.Layout(S.write_cut(os.path.join(d, "giant.bam"), S.RECIPES["giant"][0](), 60000, realistic=True))
    assert lay.blocks_cut_inside_a_record() >= 0.9
    assert int((lay.first_start_in() < 0).sum()) >= 3 and S.block_inside_one_record(lay) is not None
    m = S.model(lay)
    assert m["settled"] and 2 <= m["rounds"] < S.MAX_ROUNDS and (m["offsets"] == lay.starts).all()


def test_chunked_file_has_a_record_across_every_chunk_boundary(d):
    lay = S.Layout(S.write_cut(os.path.join(d, "chunked.bam"), S.chunked_records(), S.CHUNKED_CUT, realistic=True))
    assert lay.blocks_cut_inside_a_record() >= 0.9
    edges = S.chunk_edges(lay)
    assert len(edges) >= 3, len(edges)
    for b in edges[1:]:
        assert lay.b0[b] not in lay.starts and lay.carry_after(b) > 0
    assert S.model(lay)["settled"]


def test_the_file_order_and_genome_files_are_cut_inside_records(d):
    for path in (S.flush_trap_file(d)[1], S.genome_files(d)[1]):
        lay = S.Layout(path)
        assert len(lay.b0) >= 100 and lay.blocks_cut_inside_a_record() >= 0.9, path


def test_region_plans_enter_inside_a_block_and_end_inside_a_record(d):
    """both regions of the CLI test: the index's first virtual offset has an in-block part, the last block the plan names ends inside
    a record; the second region's plan cannot start at the top of the file, so the in-block part is what the load enters at"""
    from metheor_amd import hostapi
    from oracle import bamio
    from tests import test_irregular_paths as P
    rec, names, cut, ali = S.region_inputs(d)
    lay = S.Layout(cut)
    assert lay.blocks_cut_inside_a_record() >= 0.9
    f = hostapi.BamFile(cut)
    refs = bamio.read_bai(cut + ".bai")
    for k, (t, b, e) in enumerate((P.region_edges(rec), S.SECOND_REGION)):
        vlo, _ = bamio.bai_query(refs, t, max(0, b - 65536), e + 1)
        assert vlo & 0xffff
        old, new = f.plan_region(t, b, e), f.plan_region(t, b, e, at_record=True)
        assert {x: old[x] for x in old if x != "first_byte"} == {x: new[x] for x in new if x != "first_byte"}
        if k == 0:
            assert new["block_beg"] == 0 and new["first_byte"] == old["first_byte"] == lay.hbytes
        else:
            assert new["block_beg"] > 0 and old["first_byte"] == 0 and new["first_byte"] == (vlo & 0xffff)
            assert int(lay.b0[new["block_beg"]]) + new["first_byte"] in lay.starts
        end = int(lay.b1[new["block_end"] - 1])
        assert end < lay.total and end not in lay.starts
    # the aligned copy's plans are what they were: first_byte 0 when the plan starts below the top of the file
    fa = hostapi.BamFile(ali)
    t, b, e = S.SECOND_REGION
    assert fa.plan_region(t, b, e)["first_byte"] == 0 and fa.plan_region(t, b, e)["block_beg"] > 0
