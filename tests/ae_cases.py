"""ANTIENTROPY cases shared by test_ae_matrix.py (CPU), test_gpu_ae_matrix.py and
test_gpu_ae_states.py.  A plain module, not a conftest; it holds tables and helpers, no tests.

The kernels of csrc/antientropy.hip are instantiated per row width L = 2^ceil(log2 K) (1 .. 64) and,
for the binned dense round, per fanout k <= 3.  MATRIX walks every L, every ae_dense_apply<L, k>,
both ae_dense_apply_q variants beside configs[4]'s, the engines that cannot bin their dense rounds
(K > 16 or k > 3), and the fanouts at which the churn word changes its Philox stream (k >= 4), the
sparse emit's region shrinks (k = 5, 9) and the binned sparse scan gives way to the direct one (k = 17).
"""
from collections import namedtuple

import numpy as np

from gossip_hip import FLAG_AE_DIRECT_SCAN
from gossip_hip.engine import churn_threshold as ct

# three dense tiles of 2^14 nodes with a ragged last one, eleven sparse-scan tiles of 2^12
N = 41037
FAIL, RECOVER = ct(0.03), ct(0.25)

# (K, k): the binned dense round fits (K <= 16, k <= 3)
MATRIX_BINNED = [(1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (4, 2), (4, 3), (5, 1), (7, 3), (8, 1), (9, 2),
                 (15, 3), (16, 2), (16, 3)]
# K > 16: rows of 32 and 64 words, dense rounds as pull + atomicMax push + stats
MATRIX_WIDE = [(17, 1), (24, 2), (32, 3), (33, 1), (63, 2)]
# k >= 4: the churn word is Philox({n, t, 1, 0}).x, no first-peer shortcut, dense rounds not binned
MATRIX_FANOUT = [(2, 4), (7, 5), (16, 4), (9, 8), (13, 9), (16, 16), (17, 17), (3, 64)]
MATRIX = MATRIX_BINNED + MATRIX_WIDE + MATRIX_FANOUT

# the paths of test_gpu_antientropy.PATHS that the matrix runs, name -> (flags, params), restated so
# the CPU tests need not import a GPU test module; test_ae_matrix.py asserts the copies are equal
PATHS = {"auto": (0, {}), "dense": (0, {"ae_sparse": 0}),
         "dense_nofilter": (0, {"ae_sparse": 0, "ae_dense_filter": 0}),
         "dense_atomic": (0, {"ae_sparse": 0, "ae_dense_bin": 0}),
         "dense_ranges": (0, {"ae_sparse": 0, "ae_dense_cap": 256}),
         "sparse": (0, {"ae_sparse": 1}), "overflow": (0, {"ae_sparse": 1, "ae_cap": 64}),
         "sparse_direct": (FLAG_AE_DIRECT_SCAN, {"ae_sparse": 1})}
PATHS_BINNED = ["auto", "dense", "dense_nofilter", "dense_atomic", "dense_ranges", "sparse", "overflow",
                "sparse_direct"]
# engines with one dense form: the other dense knobs would repeat it
PATHS_OTHER = ["auto", "dense", "sparse", "overflow", "sparse_direct"]

# rounds the oracle takes in the second and the third step of run() at N nodes
ROUNDS = {(1, 2): (8, 12), (1, 3): (5, 9), (2, 1): (24, 25), (2, 2): (8, 10), (2, 3): (5, 8), (3, 1): (22, 25),
          (4, 2): (10, 11), (4, 3): (5, 8), (5, 1): (22, 26), (7, 3): (5, 9), (8, 1): (23, 23), (9, 2): (10, 12),
          (15, 3): (10, 8), (16, 2): (15, 13), (16, 3): (10, 8), (17, 1): (20, 28), (24, 2): (8, 13),
          (32, 3): (8, 8), (33, 1): (22, 25), (63, 2): (8, 13), (2, 4): (8, 7), (7, 5): (3, 6), (16, 4): (4, 9),
          (9, 8): (2, 5), (13, 9): (2, 5), (16, 16): (4, 6), (17, 17): (10, 4), (3, 64): (3, 1)}
# pairs whose last write lands on a dead node (the alive flag of N - 2 read before the write)
DEAD_AT_WRITE = [(9, 2), (3, 64)]
# pair -> rounds after the last write in which no alive node holds the new target: the written node
# is dead in them ((16, 4) and (16, 16): it dies in the churn of the round right after the write)
TARGET_HELD_BY_NOBODY = {(9, 2): 1, (16, 4): 2, (16, 16): 2}


def seed_of(K):
    return 0x5EED0100 + K


def paths_of(K, k):
    return PATHS_BINNED if (K, k) in MATRIX_BINNED else PATHS_OTHER


def samples(n_nodes=N):
    """Nodes on chunk (64) and tile (2^14) edges, and the last two."""
    return [n for n in (0, 63, 64, 16383, 16384, 32768, n_nodes - 2, n_nodes - 1) if n < n_nodes]


def engine_args(K, k, n_nodes=N, seed=None, fail=FAIL, recover=RECOVER):
    """(args, kwargs) of an Engine / OracleEngine of one case, with the state hash on."""
    return (n_nodes, K, "antientropy", k, seed_of(K) if seed is None else seed), \
        dict(flags=1, churn_fail=fail, churn_recover=recover)


Run = namedtuple("Run", "stats infected rows versions alive steps dead_write")


def snapshot(x, stats, infected, steps=(), dead_write=None):
    """A Run of the rounds collected so far and the state of x now (all rows, the sampled flags)."""
    vs = [x.read_versions(n) for n in samples(x.n_nodes)]
    inf = np.concatenate(infected) if infected else np.zeros((0, x.n_rumors), np.uint64)
    return Run(list(stats), inf, x.read_rows(), [v for v, _ in vs], [a for _, a in vs], tuple(steps), dead_write)


def run(x):
    """The matrix scenario on any engine of the ABI: random rows, three rounds, a write to the last
    component in the middle and one to node 3, to convergence, a write to the last node but one
    (every other node turns stale at once), to convergence again."""
    n, K = x.n_nodes, x.n_rumors
    x.inject_random()
    res = [x.step(3)]
    x.inject(n // 2, K - 1)
    x.inject(3, 0)
    res.append(x.step(400))
    dead = not x.read_versions(n - 2)[1]  # whether the last write lands on a dead node
    x.inject(n - 2, 0)
    res.append(x.step(400))
    stats = [s for r in res for s in r.stats]
    return snapshot(x, stats, [r.infected for r in res], [r.rounds for r in res], dead)


def assert_same(got, want):
    """Bit-exact equality of two Runs, round by round."""
    assert got.steps == want.steps and got.dead_write == want.dead_write
    assert len(got.stats) == len(want.stats)
    for a, b in zip(got.stats, want.stats):
        assert a == b
    assert np.array_equal(got.infected, want.infected)
    assert np.array_equal(got.rows, want.rows)
    assert got.alive == want.alive
    for a, b in zip(got.versions, want.versions):
        assert np.array_equal(a, b)
