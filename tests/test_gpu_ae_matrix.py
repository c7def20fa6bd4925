"""GPU: every row width, dense-apply variant and fanout class of the ANTIENTROPY kernels
(csrc/antientropy.hip) against the C oracle, bit for bit, on every round path of the engine.

ae_cases.MATRIX x the paths of the pair: K = 2, 3-4 and 17-32 are the row widths L = 2, 4, 32 that no
other test instantiates; (1, 2) .. (16, 3) are the ae_dense_apply<L, k> variants and the two
ae_dense_apply_q kernels (K = 16 with k = 2, 3) beside the one configs[4] runs; k >= 4 moves the churn
word to its own Philox stream, turns the first-peer shortcut off and keeps dense rounds off the
binned form; k = 17 and 64 take the direct sparse scan.  The scenario (ae_cases.run) writes once mid-run
and once after convergence, where the stale bits are valid and every other node turns stale at once.
test_ae_matrix.py holds the oracle to the numpy restatement on the same pairs and pins its rounds."""
import functools
import os

import pytest

import ae_cases as ac
import oracle_py as op
from gossip_hip import FLAG_TIMING, Engine

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
ITEMS = [(K, k, path) for K, k in ac.MATRIX for path in ac.paths_of(K, k)]


@functools.lru_cache(maxsize=None)
def _oracle(K, k):
    """The oracle's run of one pair and its final hash, computed once and shared by the paths (read only)."""
    args, kw = ac.engine_args(K, k)
    o = op.OracleEngine(*args, threads=THREADS, **kw)
    r = ac.run(o)
    h = o.state_hash()
    o.close()
    return r, h


def _engine(K, k, path, flags=0):
    args, kw = ac.engine_args(K, k)
    pf, params = ac.PATHS[path]
    kw["flags"] |= pf | flags
    return Engine(*args, params=params, **kw)


@pytest.mark.parametrize("K,k,path", ITEMS, ids=[f"K{K}-k{k}-{p}" for K, k, p in ITEMS])
def test_matrix_vs_oracle(K, k, path):
    want, h = _oracle(K, k)
    e = _engine(K, k, path)
    try:
        got = ac.run(e)
        ac.assert_same(got, want)
        assert e.state_hash() == h
    finally:
        e.close()


def _timed(K, k, params):
    """run() on a timed engine: (the Run, sparse rounds counted by timer 2)."""
    args, kw = ac.engine_args(K, k)
    kw["flags"] |= FLAG_TIMING
    e = Engine(*args, params=params, **kw)
    try:
        return ac.run(e), e.kernel_time(2)[1]
    finally:
        e.close()


@pytest.mark.parametrize("K,k", [(4, 2), (32, 3), (16, 16)])
def test_paths_run_what_they_name(K, k):
    """Timer 2 counts the sparse rounds (include/gossip.h gossip_kernel_time): path `sparse` ends
    with some, path `dense` with none.  A pipelined run of sparse rounds (engine.hip step_ae) counts
    a round only once it is known not to have overflowed its edge list; at (16, 16) every sparse
    round of the scenario does overflow the default list (16 exchanges per node, most with a stale
    end until the last round), so timer 2 stays at 0 there: that pair is checked with ae_ahead 1,
    where the timer brackets the scan of every sparse round, overflowed or not.
    test_fanout_sparse_rounds_with_room is the run in which those rounds finish sparse."""
    want, _ = _oracle(K, k)
    ahead = {"ae_ahead": 1} if (K, k) == (16, 16) else {}
    for path, sparse in (("sparse", True), ("dense", False)):
        got, launches = _timed(K, k, dict(ac.PATHS[path][1], **ahead))
        ac.assert_same(got, want)
        assert (launches > 0) == sparse, (path, launches)


@pytest.mark.parametrize("K,k", [p for p in ac.MATRIX_FANOUT if p[1] <= 16], ids=lambda v: str(v))
def test_fanout_sparse_rounds_with_room(K, k):
    """Fanouts 4 .. 16 on the binned sparse scan with an edge list that holds every exchange
    (ae_cap = k * N): no round overflows, so the exchanges listed from the emit's smaller regions
    (2^12, 2^11, 2^10 senders) are gathered and applied in place, not rerun dense as most are under
    path `sparse` (measured: 4 of 15 sparse rounds finish in place there at (2, 4), 2 of 9 at (7, 5),
    3 of 13 at (16, 4), 0 of 7 at (9, 8), 1 of 7 at (13, 9), 0 of 10 at (16, 16)).  Timer 2 of the
    pipelined run counts only sparse rounds that ran to their end."""
    want, _ = _oracle(K, k)
    got, launches = _timed(K, k, {"ae_sparse": 1, "ae_cap": k * ac.N})
    ac.assert_same(got, want)
    # every round is sparse but the first after each of the three writes (the stale bits are not valid)
    assert launches == sum(want.steps) - 3
