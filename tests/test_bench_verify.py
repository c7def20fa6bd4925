"""CPU: bench.py's self-check.  A bench run of configs[3] (one GPU: with --full; N > 1:
always) compares its per-round stats and final state hash with the OpenMP oracle's run of the same
workload (tests/golden/cfg4_oracle.json), before and after the timed steps, so a multi-GPU line
cannot report a rate for a wrong dissemination."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_fixture_matches_the_bench_workload_only():
    fx = bench.load_fixture(bench.NODES_TOTAL, bench.SEED_TOTAL)
    assert fx is not None and fx["rounds"] == 15
    assert bench.load_fixture(bench.NODES_SECONDARY, bench.SEED_SECONDARY) is None
    assert bench.load_fixture(bench.NODES_TOTAL, bench.SEED_TOTAL + 1) is None


def test_check_run_accepts_the_oracle_run_and_names_a_difference():
    fx = bench.load_fixture(bench.NODES_TOTAL, bench.SEED_TOTAL)
    stats = copy.deepcopy(fx["stats"])
    for s in stats:
        s["state_hash"] = 0  # the bench's engines run without the per-round hash
    assert bench.check_run(stats, fx["final_state_hash"], fx) is None
    bad = copy.deepcopy(stats)
    bad[9]["full_nodes"] += 1
    assert "round 9: full_nodes" in bench.check_run(bad, fx["final_state_hash"], fx)
    assert "rounds" in bench.check_run(stats[:-1], fx["final_state_hash"], fx)
    assert "hash" in bench.check_run(stats, fx["final_state_hash"] ^ 1, fx)


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    """--dump-outputs, on the oracle (same Engine interface): per-round stats, the state hash as four
    16-bit limbs and a seeded sample of node states, float64, the same arrays on a second call."""
    import numpy as np
    import oracle_py as op

    n = 1 << 13
    ora = op.OracleEngine(n, bench.RUMORS, bench.MODE, bench.FANOUT, bench.SEED_SECONDARY)
    ora.inject_random()
    stats = ora.step(4, with_infected=False).stats  # mid-run: the sampled nodes hold some rumors, not all
    h = ora.state_hash()
    bench.dump_outputs(str(tmp_path / "a"), ora, stats, h)
    bench.dump_outputs(str(tmp_path / "b"), ora, stats, h)
    got = {name: np.load(tmp_path / "a" / f"{name}.npy") for name in ("round_stats", "state_hash", "state_sample")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["round_stats"].shape == (4, len(bench.STAT_KEYS))
    assert [[int(x) for x in row] for row in got["round_stats"]] == [[s[k] for k in bench.STAT_KEYS] for s in stats]
    assert sum(int(x) << (16 * i) for i, x in enumerate(got["state_hash"])) == h
    sample, state = got["state_sample"], ora.read_shard()[0]
    assert sample.shape == (bench.DUMP_SAMPLE_NODES, 1 + bench.RUMORS)
    ids = sample[:, 0].astype(np.int64)
    assert ids.min() >= 0 and ids.max() < n and len(set(ids.tolist())) > n // 4
    bits = (state[ids, None] >> np.arange(bench.RUMORS, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(sample[:, 1:], bits.astype(np.float64))
    assert 0 < sample[:, 1:].sum() < sample[:, 1:].size
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
    ora.close()
