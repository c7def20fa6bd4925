"""GPU, the big-region emit's write-out from on-chip ids against the OpenMP oracle.

Past kBigFromTiles destination tiles (N > 2^24) the dense emit sorts regions of up to 32768
records; each lane then holds the ids of records lane, lane + 1024, ... (at most 32) in registers
while the sender values take the staging room, and writes every field of a record in one loop
(csrc/binned.hip, bin_emit_kernel, BIG).  test_gpu_big_paths.py drives that path with full
regions; here are the shapes where the per-lane id count is irregular:

  pushpull-k1-R64   a region holds at most 16384 records: half the per-lane slots are empty
  pull-k2-R1        for many rounds almost every sender is empty: regions of 0 to a few hundred
                    records, totals that are no multiple of 1024, lanes without any id
  push-k2-R64-loss  the fault path (peers redrawn, also with k <= 2), records missing at random

Every round runs on the dense pipeline (sparse_frac -1) at N = 2^25 + 4099 (big regions, a ragged
last region) and must equal the oracle bit for bit: per-round stats, per-rumor counts and the
final state.  Reference: (*NodeState).Gossip, main.go:65-89, as rounds.
"""
import os

import numpy as np
import pytest

import oracle_py as op
from gossip_hip import Engine

pytestmark = pytest.mark.gpu

N = (1 << 25) + 4099
THREADS = min(16, os.cpu_count() or 1)
DENSE = {"sparse_frac": -1.0}
# mode, k, R, seed, edge_loss
CASES = {"pushpull-k1-R64": ("pushpull", 1, 64, 0x5EED0011, 0),
         "pull-k2-R1": ("pull", 2, 1, 0x5EED0012, 0),
         "push-k2-R64-loss": ("push", 2, 64, 0x5EED0013, 1 << 30)}


@pytest.mark.parametrize("case", list(CASES))
def test_emit_onchip_equals_oracle(case):
    mode, k, r, seed, loss = CASES[case]
    o = op.OracleEngine(N, r, mode, k, seed, flags=1, threads=THREADS, edge_loss=loss)
    o.inject_random()
    ro = o.step(200)
    full = o.read_shard()
    o.close()
    assert ro.converged  # the run covers the nearly empty and the nearly full rounds
    e = Engine(N, r, mode, k, seed, flags=1, edge_loss=loss, params=DENSE)
    e.inject_random()
    res = e.step(200)
    assert res.converged == ro.converged and res.rounds == ro.rounds
    assert res.stats == ro.stats
    assert np.array_equal(res.infected, ro.infected)
    assert np.array_equal(e.read_shard(), full)
    e.close()
