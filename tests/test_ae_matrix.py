"""CPU: the two references of the ANTIENTROPY matrix (ae_cases.py) against each other, and what the
C oracle does on the GPU tests' own runs.

The C oracle (oracle/gossip_oracle.c) is what test_gpu_ae_matrix.py and test_gpu_ae_states.py hold
the HIP engine to; numpy_ref.AntiEntropySim is the independent restatement of DESIGN.md §2.7.  No
golden holds a fanout above 3, so the oracle's churn word of k >= 4 (Philox({n, t, 1, 0}).x, not
{n, t, 0, 0}.w) is first held to the numpy form here, beside every row width.  The pinned round
counts show that the GPU cases do what they were chosen for: every run converges after each write,
the write after convergence takes several rounds to spread, two of them land on a dead node."""
import functools
import os

import numpy as np
import pytest

import ae_cases as ac
import numpy_ref as nr
import oracle_py as op
from gossip_hip.engine import StepResult

THREADS = min(16, os.cpu_count() or 1)
IDS = [f"K{K}-k{k}" for K, k in ac.MATRIX]


class NumpyEngine:
    """AntiEntropySim behind the calls of AbiEngine that ae_cases.run makes."""

    def __init__(self, n_nodes, K, mode, k, seed, flags=1, churn_fail=0, churn_recover=0):
        assert mode == "antientropy"
        self.n_nodes, self.n_rumors = n_nodes, K
        self.sim = nr.AntiEntropySim(n_nodes, K, k, seed, churn_fail, churn_recover)

    def inject_random(self):
        self.sim.inject_random()

    def inject(self, node, comp=0):
        self.sim.inject(node, comp)

    def step(self, max_rounds):
        out = self.sim.run(max_rounds)
        stats = [dict(round=s["round"], converged=s["converged"], full_nodes=s["full"], alive_nodes=s["alive"],
                      messages=s["messages"], state_hash=s["hash"]) for s in out]
        inf = np.array([s["infected"] for s in out], dtype=np.uint64).reshape(len(out), self.n_rumors)
        return StepResult(len(out), stats, inf)

    def read_rows(self):
        return self.sim.V.copy()

    def read_versions(self, node):
        return self.sim.V[node].copy(), bool(self.sim.alive[node])


def test_path_table_equals_the_parity_tests():
    """ae_cases.py restates the paths of test_gpu_antientropy.py that the matrix runs."""
    import test_gpu_antientropy as ta
    assert set(ac.PATHS) == set(ac.PATHS_BINNED) and set(ac.PATHS_OTHER) <= set(ac.PATHS_BINNED)
    for name, path in ac.PATHS.items():
        assert ta.PATHS[name] == path
    assert len(ac.MATRIX) == len(set(ac.MATRIX)) == 28 and set(ac.ROUNDS) == set(ac.MATRIX)
    assert all(set(ac.paths_of(K, k)) == set(ac.PATHS_BINNED if K <= 16 and k <= 3 else ac.PATHS_OTHER)
               for K, k in ac.MATRIX)
    assert sum(len(ac.paths_of(K, k)) for K, k in ac.MATRIX) == 185


@pytest.mark.parametrize("K,k", ac.MATRIX, ids=IDS)
def test_oracle_equals_numpy(K, k):
    """The matrix scenario at 1500 nodes (600 at fanout 64, where numpy's maximum.at is slow): every
    stat, every per-component count, every row, the sampled alive flags."""
    n = 600 if k == 64 else 1500
    args, kw = ac.engine_args(K, k, n)
    o = op.OracleEngine(*args, threads=THREADS, **kw)
    want = ac.run(NumpyEngine(*args, **kw))
    got = ac.run(o)
    o.close()
    ac.assert_same(got, want)
    assert got.stats[-1]["converged"] and got.steps[0] == 3


@functools.lru_cache(maxsize=None)
def _oracle(K, k):
    args, kw = ac.engine_args(K, k)
    o = op.OracleEngine(*args, threads=THREADS, **kw)
    r = ac.run(o)
    o.close()
    return r


@pytest.mark.parametrize("K,k", ac.MATRIX, ids=IDS)
def test_oracle_rounds_of_the_gpu_cases(K, k):
    """run() at the GPU tests' size: the second and third step converge in the pinned number of
    rounds; the write after convergence needs more than one round to spread (but at fanout 64)."""
    r = _oracle(K, k)
    first, second, third = r.steps
    assert first == 3 and (second, third) == ac.ROUNDS[(K, k)]
    assert r.stats[first + second - 1]["converged"] and r.stats[-1]["converged"]
    assert not any(s["converged"] for s in r.stats[first:first + second - 1] + r.stats[first + second:-1])
    assert [s["round"] for s in r.stats] == list(range(len(r.stats)))
    assert (third > 1) == ((K, k) != (3, 64))
    # every alive node ended on the target (dead ones keep what they had)
    last = r.stats[-1]
    assert 0 < last["full_nodes"] == last["alive_nodes"] <= int((r.rows == r.rows.max(axis=0)).all(axis=1).sum())


def test_oracle_dead_writes_of_the_gpu_cases():
    """What the last write meets, by the alive flag read before it (Run.dead_write) and the rounds
    after it.  (9, 2) and (3, 64): node N - 2 is dead at the write.  At (9, 2) it stays dead one more
    round and no alive node holds the new target in it; at (3, 64) the dead node had missed the write
    to node 3, so its own write only catches up with the target, and the run is converged again after
    one round.  (16, 4) and (16, 16): the node is alive at the call and dies in the churn of the very
    next round, before any exchange, for two rounds: nobody alive holds the new target in them."""
    assert [p for p in ac.MATRIX if _oracle(*p).dead_write] == ac.DEAD_AT_WRITE
    for p, rounds in ac.TARGET_HELD_BY_NOBODY.items():
        r = _oracle(*p)
        after = r.stats[r.steps[0] + r.steps[1]:]
        assert [s["full_nodes"] for s in after[:rounds]] == [0] * rounds and after[rounds]["full_nodes"] > 0
    for p in set(ac.MATRIX) - set(ac.TARGET_HELD_BY_NOBODY) - {(3, 64)}:
        r = _oracle(*p)
        assert r.stats[r.steps[0] + r.steps[1]]["full_nodes"] > 0
