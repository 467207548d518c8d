"""bench.py's plain run (GPU): it prints the result line without the --full legs, times exactly
--steps steps, and --dump-outputs writes the last timed step's outputs, identical from run to run
(the clock-length prewarm is discarded before the warm-up steps)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")
LEGS = ("stages_ms", "inscan_certs", "exchange", "roofline", "fused_roofline", "c5_map_fuse", "dropin", "c5",
        "c5_dense", "c5_shard", "cpu_baseline")


def _bench(out_dir, prewarm_s):
    env = {k: v for k, v in os.environ.items() if k not in DIST_ENV}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--hyps", "3", "--n-az", "128", "--prewarm-s", str(prewarm_s), "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    a = _bench(tmp_path / "a", 0.02)
    b = _bench(tmp_path / "b", 0.0)  # another prewarm length (none at all): the same timed inputs
    for d in (a, b):
        assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0.0
        assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
        assert d["unit"] == "scans/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert not [k for k in LEGS if k in d]
    assert a["prewarm_steps"] > 0 and b["prewarm_steps"] == 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for want in ("belief_L.npy", "belief_X_anchor.npy", "combined_L.npy", "hyp_diag.npy", "iw_Psi_proc.npy",
                 "map_map.npy"):
        assert want in names
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x)), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "belief_L.npy").shape == (3, 22, 22)
    # 5 scans from the seeded initial state moved the beliefs: the dump is the state after the steps
    assert float(np.load(tmp_path / "a" / "belief_stamp.npy").max()) > 0.0
