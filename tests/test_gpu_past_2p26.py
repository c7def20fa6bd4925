"""GPU, the one-shard round paths past 2^26 nodes (more than 4096 destination tiles) against the
OpenMP oracle.

Past 4096 tiles the sender values no longer fit the emit's LDS beside the tile counters, so the
dense emit bins 16384-sender regions with 16-bit packed tile counters and writes each push packed
with its id (binned.hip: the one-shard big-region emit, peers kept in LDS, redrawn with faults),
and serve / apply run their per-XCD tile queues.
N = 2^26 + 4099: 4097 tiles, a ragged last region and a ragged last tile.  Every path must equal the
oracle bit for bit: per-round stats, per-rumor counts and the final state.  (Round 6 ran the same
cases on the 32768-sender layout it measured and dropped, profiles/r06_huge/.)
Reference: (*NodeState).Gossip, main.go:65-89, as rounds.
"""
import os

import numpy as np
import pytest

import oracle_py as op
from gossip_hip import Engine

pytestmark = pytest.mark.gpu

N = (1 << 26) + 4099
THREADS = min(16, os.cpu_count() or 1)
ROUNDS = 40
# auto: as planned (sparse and dense rounds); dense: every round on the dense pipeline; dense_filter:
# every round dense with the edge filter (empty / full peers' one-way edges dropped in the emit;
# past 2^25 nodes off by default, forced here)
PATHS = {"auto": {}, "dense": {"sparse_frac": -1.0},
         "dense_filter": {"sparse_frac": -1.0, "filter_frac": 0.3}}
CASES = {"pushpull-k2-R64": ("pushpull", 2, 64, 0x5EED0003, 0, 0),
         "push-k2-R5": ("push", 2, 5, 77, 0, 0),
         "pull-k1-R3": ("pull", 1, 3, 0x51, 0, 0),
         # edge loss: the emit's fault branch (FAULTS)
         "pushpull-k2-R7-loss": ("pushpull", 2, 7, 9, 1 << 30, 0)}


@pytest.fixture(scope="module")
def oracle_runs():
    cache = {}

    def get(case):
        if case not in cache:
            mode, k, r, seed, loss, parts = CASES[case]
            o = op.OracleEngine(N, r, mode, k, seed, flags=1, threads=THREADS, edge_loss=loss, partitions=parts)
            o.inject_random()
            res = o.step(ROUNDS)
            cache[case] = (res, o.read_shard())
            o.close()
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("path", list(PATHS))
def test_past_4096_tiles_equal_oracle(oracle_runs, case, path):
    mode, k, r, seed, loss, parts = CASES[case]
    ro, full = oracle_runs(case)
    e = Engine(N, r, mode, k, seed, flags=1, edge_loss=loss, partitions=parts, params=PATHS[path])
    e.inject_random()
    res = e.step(ROUNDS)
    assert res.converged == ro.converged and res.rounds == ro.rounds
    assert res.stats == ro.stats
    assert np.array_equal(res.infected, ro.infected)
    assert np.array_equal(e.read_shard(), full)
    e.close()
