"""Child process of tests/test_gpu_chunked_load.py::test_pieced_copy: METHEOR_COPY_PIECE_MB is read once per process, so the pieced
copy runs here, in a process started with the switch in its environment.  Inflates every table of chunked_load_util.pieced_tables
in one bgzf_inflate call each and prints one JSON line: per table the SHA-256 of the output and what load_stats counted for it."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import metheor_amd
    from tests import chunked_load_util as U
    eng = metheor_amd.Engine(0)
    out = {}
    for name, (fb, coff, csize, isize, _) in U.pieced_tables().items():
        before = eng.load_stats()
        got = eng.bgzf_inflate(fb, coff, csize, isize)
        after = eng.load_stats()
        out[name] = dict(sha256=hashlib.sha256(got.tobytes()).hexdigest(), **{k: after[k] - before[k] for k in after})
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
