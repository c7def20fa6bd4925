"""GPU: bench.py's command line at a small size (2^16 nodes, 3 timed steps).  A plain run prints the
headline line and nothing that takes a run of its own; --dump-outputs writes what the last timed
step returned, equal to the oracle's run of the same workload; --full still carries the extras."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 16
EXTRAS = ("secondary", "antientropy", "cpu_baseline")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nodes", str(N), *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    import bench
    import oracle_py as op

    out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["metric"] == "gossip node-updates/sec (nodes x rounds)" and out["unit"] == "node-updates/s"
    assert out["higher_is_better"] is True and out["dtype"] == "u64"
    rounds = out["config"]["rounds_to_converge"]
    assert out["value"] == pytest.approx(N * rounds / (out["ms_per_step"] * 1e-3))
    assert out["roofline"]["step_frac"]["rounds"] == 3 * rounds  # the engine timed 3 steps, no more
    assert out["verified"] is None and not any(k in out for k in EXTRAS) and "dense_only" not in out["roofline"]

    ora = op.OracleEngine(N, bench.RUMORS, bench.MODE, bench.FANOUT, bench.SEED_SECONDARY)
    ora.inject_random()
    want = ora.step(64, with_infected=False)
    assert want.converged and want.rounds == rounds
    stats = np.load(tmp_path / "round_stats.npy")
    assert stats.dtype == np.float64
    assert np.array_equal(stats, np.array([[s[k] for k in bench.STAT_KEYS] for s in want.stats], dtype=np.float64))
    limbs = np.load(tmp_path / "state_hash.npy")
    assert sum(int(x) << (16 * i) for i, x in enumerate(limbs)) == ora.state_hash()
    sample = np.load(tmp_path / "state_sample.npy")
    assert sample.shape == (bench.DUMP_SAMPLE_NODES, 1 + bench.RUMORS)
    state = ora.read_shard()[0]
    bits = (state[sample[:, 0].astype(np.int64), None] >> np.arange(bench.RUMORS, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(sample[:, 1:], bits.astype(np.float64))
    ora.close()


def test_full_run_keeps_the_extras():
    out = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert out["steps"] == 2 and "dense_only" in out["roofline"]
    assert out["secondary"]["nodes"] == 1 << 24 and out["secondary"]["value"] > 0
    assert "cpu_baseline" not in out and "antientropy" not in out  # switched off / only beside configs[3]
