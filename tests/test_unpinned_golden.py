"""The C++ oracle against a SECOND, independent restatement of the reference: tests/golden/unpinned_cases.json.gz holds the
outputs of tools/gen_golden_unpinned.py, a Python transliteration written from /root/reference/src (not from oracle/) for the
branches no reference fixture reaches -- indels / clips / skips in reference_positions_full, the reverse-strand abspos - 1 rule and
the paired flags, several contigs, the flush / re-open / overwrite state machines of pdr, mhl, fdrp, qfdrp (sorted and unsorted
streams), window drops and NaN rows, the i32 wrap of lpmd.rs:11-12.  Integers, PDR / LPMD / PM / FDRP / qFDRP floats: bit for bit;
MHL (HashMap order in the reference, mhl.rs:50) and ME (libm log2f) within 1e-6."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import unpinned_util as U

DATA = U.load()
CASES = DATA["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_equals_the_transliteration(case):
    rec = U.records_of(case)
    reads = pyoracle.Reads.decode(rec)
    soa = reads.soa()
    # readutil.rs:24-53, 323-345
    for i, d in enumerate(case["decode"]):
        o0, o1 = int(soa["cpg_off"][i]), int(soa["cpg_off"][i + 1])
        assert (int(soa["start"][i]), int(soa["end"][i])) == (d["start"], d["end"]), i
        got = [[int(r), U.signed_pos(p), int(p >> 31)] for r, p in zip(soa["cpg_rel"][o0:o1], soa["cpg_pos"][o0:o1])]
        assert got == d["cpgs"], (i, case["records"][i])
    ex = case["expect"]
    for e in ex.get("pdr", []):
        t = reads.pdr(**e["params"])
        rows = e["rows"]
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [r[:2] for r in rows], e["params"]
        assert t.cnt.tolist() == [r[3:5] for r in rows]
        assert U.same_f32(t.val, U.from_bits([r[2] for r in rows]))
    for e in ex.get("lpmd", []):
        l = reads.lpmd(pairs=True, **e["params"])
        assert [l["n_concordant"], l["n_discordant"], l["n_read"], l["n_valid_read"]] == e["counts"]
        assert U.same_f32([l["lpmd"]], U.from_bits([e["lpmd_bits"]]))
        t = l["pairs"]
        assert [[int(a), int(p[0]), int(p[1])] for a, p in zip(t.tid, t.pos)] == [r[:3] for r in e["pairs"]]
        assert t.cnt.tolist() == [r[4:6] for r in e["pairs"]]
        assert U.same_f32(t.val, U.from_bits([r[3] for r in e["pairs"]]))
    for e in ex.get("mhl", []):
        t = reads.mhl(**e["params"])
        assert [[int(a), int(b)] for a, b in zip(t.tid, t.pos[:, 0])] == [r[:2] for r in e["rows"]], e["params"]
        assert U.same_f32(t.val, U.from_bits([r[2] for r in e["rows"]]), tol=1e-6)
    for e in ex.get("quartet", []):
        me, pm = reads.me(min_depth=0, **e["params"]), reads.pm(min_depth=0, **e["params"])
        key = lambda t: sorted(range(len(t)), key=lambda i: (int(t.tid[i]), *t.pos[i].tolist()))
        om, op = key(me), key(pm)
        assert [[int(me.tid[i]), *me.pos[i].tolist()] for i in om] == [r[:5] for r in e["rows"]]
        assert [me.cnt[i].tolist() for i in om] == [r[5] for r in e["rows"]] and [pm.cnt[i].tolist() for i in op] == [r[5] for r in e["rows"]]
        assert U.same_f32(me.val[om], U.from_bits([r[6] for r in e["rows"]]), tol=1e-6)
        assert U.same_f32(pm.val[op], U.from_bits([r[7] for r in e["rows"]]))
    for e in ex.get("fdrp", []):
        f, q = reads.fdrp(**e["params"]), reads.qfdrp(**e["params"])
        want = [r[:2] for r in e["rows"]]
        assert [[int(a), int(b)] for a, b in zip(f.tid, f.pos[:, 0])] == want and [[int(a), int(b)] for a, b in zip(q.tid, q.pos[:, 0])] == want
        assert U.same_f32(f.val, U.from_bits([r[2] for r in e["rows"]]))
        assert U.same_f32(q.val, U.from_bits([r[3] for r in e["rows"]]))


def test_lpmd_i32_wrap_of_the_product_formula():
    """lpmd.rs:11-12, 51-55 on wrapped i32 counters: the product's host-side mth_lpmd_from_counts (no device needed)"""
    import metheor_amd
    L = metheor_amd.lib()
    for nc, nd, bits in DATA["lpmd_from_counts"]:
        got = np.float32(L.mth_lpmd_from_counts(int(nc), int(nd)))
        assert U.same_f32([got], U.from_bits([bits])), (nc, nd)
