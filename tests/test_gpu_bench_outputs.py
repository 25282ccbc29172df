"""A plain `bench.py` run on the device: the headline line only (the secondary legs belong to --full), and --dump-outputs writes
what the last timed step computed -- the PDR rows and LPMD totals of the seeded config-2 input, equal to the oracle's bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    from metheor_amd import synth
    from oracle import pyoracle
    n_reads, d = 5_000_000, tmp_path / "out"          # ~13x on the 58.6-Mbp contig: most sites reach the default min_depth 10
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", str(n_reads), "--preheat-seconds", "0",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["higher_is_better"] is True
    assert j["unit"] == "M reads/s" and j["dtype"] == "u32"
    assert not {"roofline", "cpu_baseline", "e2e", "all7", "soak", "two_contexts"} & set(j)
    got = {p.name[:-4]: np.load(p) for p in d.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    reads = pyoracle.Reads.from_soa(*synth.to_oracle_soa(synth.chr19_10m(n_reads=n_reads, seed=1234)))
    o, ol = reads.pdr(), reads.lpmd()
    assert len(o) == j["config"]["sites_emitted"] == len(got["pdr_pos"]) > 1000
    assert (got["pdr_tid"] == 0).all() and (got["pdr_pos"] == o.pos[:, 0]).all()
    assert (got["pdr_n_concordant"] == o.cnt[:, 0]).all() and (got["pdr_n_discordant"] == o.cnt[:, 1]).all()
    assert (got["pdr_value"].view(np.uint32) == o.val.view(np.uint32)).all()
    assert got["lpmd_counts"].tolist() == [ol[k] for k in ("n_concordant", "n_discordant", "n_read", "n_valid_read")]
    assert got["lpmd_counts"][2] == n_reads and got["lpmd_value"][0] == np.float32(ol["lpmd"])
