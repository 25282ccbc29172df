"""The two call_at_minus_one cases of tests/golden/unpinned_cases.json.gz (tools/gen_golden_unpinned.py) for the CPU and the GPU
tests of calls at position -1: a record at position 0 whose flag is outside {0, 99, 147} reports abspos - 1 for a call on its first
aligned base (readutil.rs:332-340), and the reference keeps -1 as an ordinary i32 key -- the first of its contig."""
import numpy as np

from oracle import pyoracle
from tests import unpinned_util as U

WORD = 0x7fffffff                       # position -1 in the 31 position bits of a decoded call word
SORTED, UNSORTED = "call_at_minus_one_sorted", "call_at_minus_one_unsorted"


def case(name):
    return next(c for c in U.load()["cases"] if c["name"] == name)


def records(name):
    return U.records_of(case(name))


def minus_one_records(rec):
    """indices of the records that call at position -1: at position 0, a shifted flag, a call on the first base"""
    return [i for i in range(len(rec)) if rec.pos[i] == 0 and int(rec.flag[i]) not in (0, 99, 147) and rec.xms[i][:1] in (b"z", b"Z")]


def seven_tables(rd, **kw):
    """the seven measures' tables of a pyoracle.Reads, at parameters that keep every row"""
    l = rd.lpmd(pairs=True)
    return dict(pdr=rd.pdr(min_depth=0, min_cpgs=0), mhl=rd.mhl(min_depth=0, min_cpgs=1), me=rd.me(min_depth=0), pm=rd.pm(min_depth=0),
                fdrp=rd.fdrp(min_depth=0, max_depth=64, min_overlap=10), qfdrp=rd.qfdrp(min_depth=0, max_depth=64, min_overlap=10),
                pairs=l["pairs"]), [l[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")] + [int(np.float32(l["lpmd"]).view(np.uint32))]


def same_table(a, b):
    return (a.tid.tolist() == b.tid.tolist() and a.pos.tolist() == b.pos.tolist() and a.cnt.tolist() == b.cnt.tolist() and
            U.same_f32(a.val, b.val))


def one_contig(rec, tid):
    """the records of contig `tid` alone, as contig 0 of a one-contig file"""
    sub = rec.subset([i for i in range(len(rec)) if rec.tid[i] == tid])
    sub.refs = [rec.refs[tid]]
    sub.tid = np.zeros(len(sub), np.int32)
    return sub


RES_SEEDS = (0, 2, 4, 10)               # reservoir seeds of the -D 3 runs: the draws at (tid, -1) differ between them (checked on the CPU)
RES = dict(min_depth=3, max_depth=3, min_overlap=10)


def reservoir_unsorted(rec):
    """the sorted case's records with each contig's position-0 reads moved, as one block, behind nine later reads of the contig: not
    coordinate-sorted (the file-order replay takes it), and site -1 still sees its four passing reads in a row -- more than -D 3"""
    idx = []
    for tid in sorted(set(rec.tid.tolist())):
        zero = [i for i in range(len(rec)) if rec.tid[i] == tid and rec.pos[i] == 0]
        rest = [i for i in range(len(rec)) if rec.tid[i] == tid and rec.pos[i] != 0]
        idx += rest[:9] + zero + rest[9:]
    return rec.subset(idx)


def rows_at_minus_one(rd, seed):
    """(tid, fdrp bits, qfdrp bits, stored reads) of the rows at -1 under the -D 3 parameters"""
    f, q = rd.fdrp(seed=seed, **RES), rd.qfdrp(seed=seed, **RES)
    return [(int(t), int(v.view(np.uint32)), int(w.view(np.uint32)), int(c)) for t, p, v, w, c in zip(f.tid, f.pos[:, 0], f.val, q.val, f.cnt[:, 0]) if p == -1]


def decode(rec):
    return pyoracle.Reads.decode(rec)
