"""GPU: a plain bench.py run (no --full) on a small config-2 window: the
result line, --steps as the number of timed steps, and --dump-outputs -- the
verdicts of the last timed step, bit-exact against the oracle on the same
seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from comdb2_amd import hsc
from comdb2_amd.workloads import SEED_CONFIG2, config2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COMMITS, N_TXN = 20_000, 3_001  # (an odd batch: the last 64-set word is partial)


def test_plain_run_dumps_last_step_verdicts(oracle_mod, tmp_path):
    out = tmp_path / "dump"
    # 2 resident batches, 2 streams; warm-up step 0, timed steps 1 and 2: the
    # last one probes batch 0 again
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--n-commits", str(N_COMMITS), "--n-txn", str(N_TXN),
                        "--ring-gb", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "checks/s"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N_TXN / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # the legs of a --full run are absent
    assert d["cpu_baseline"] is None and d["probe_phase"] is None and "api" not in d
    assert d["roofline"]["traffic"] is None and d["roofline"]["l3_resident"] is None
    assert sorted(os.listdir(out)) == ["verdict.npy"]
    got = np.load(out / "verdict.npy")
    assert got.dtype == np.float32 and got.shape == (N_TXN,)

    c2 = config2(seed=SEED_CONFIG2, n_commits=N_COMMITS, n_txn=N_TXN)
    want, _, _ = oracle_mod.check(c2.log, c2.readsets)
    hv = hsc.Validator(-1)  # host only: the read sets the marshal decides by itself
    try:
        assert hv.register_group("t1", 0, 9) == 0
        hv.set_end(c2.params["end_lsn"])
        forced = hv.marshal(c2.readsets)["forced"]
    finally:
        hv.close()
    assert 0 < int((want != 0).sum()) < N_TXN  # both verdicts occur
    np.testing.assert_array_equal(np.maximum(got, forced) != 0, want != 0)
