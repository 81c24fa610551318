"""bench.py's plain run on one GPU: the headline alone (no verification, side legs or CPU baseline: those are --full),
`--steps` timed steps, and --dump-outputs writing what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"bench.py failed:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1
    assert j["unit"] == "op-triples/s" and j["higher_is_better"] is True and j["dtype"] == "u64"
    # value = 64 triples per step over the measured time per step
    assert abs(j["value"] - 64 / (j["ms_per_step"] * 1e-3)) / j["value"] < 0.02
    assert j["config"]["ciphertexts_moved_over_pcie_in_timed_region"] == {"ct_uploads": 0, "ct_downloads": 0}
    assert j["verified"] is None and j["cpu_baseline"] is None
    assert not {"raw_cabi", "execute_path", "dag", "dag_batch", "dag_configs"} & set(j)

    z = np.load(tmp_path / "z.npy")
    assert z.dtype == np.float64 and z.shape == (64, 1024)
    # the clear inputs are drawn as bench.py draws them (rank 0's seed, x_i then y_i, call after call): z_i = x_i * y_i
    rng = np.random.default_rng(0xE7A)
    want = []
    for _ in range(64):
        x, y = rng.uniform(-1, 1, 1024), rng.uniform(-1, 1, 1024)
        want.append(x * y)
    assert np.max(np.abs(z - np.array(want))) < 1e-3
