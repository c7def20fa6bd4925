"""CPU: lockstep_run over host (oracle) shards in one process equals one oracle engine in per-round
stats, every shard's final state and the plan kinds.  The copy comm of gossip_hip.sharded runs the
same round bodies as the per-rank driver, and the oracle hands out a send buffer outside its image,
so the gathers here copy every slot (a device engine's own slot is in place)."""
import numpy as np
import pytest

import oracle_py as op
from gossip_hip.engine import churn_threshold as ct
from gossip_hip.sharded import (CLASSCODED, DENSE, REP, REP_CLASSCODED, REP_GATHER, SPARSE, ANTIENTROPY,
                                lockstep_run)
from test_sharded_gloo import AE_CASES, CASES, PLAN_KINDS, PLANS, _faults, _grid

RANDOM_CASES = CASES[:5] + [("pushpull", 2, 5, 12, 3, None)]  # the last: an empty last shard at G = 5
REFS = {}


def _ref(case):
    """The one-engine run of a case: (stats, state), computed once."""
    if case not in REFS:
        mode, k, R, N, seed, _ = case
        ref = op.OracleEngine(N, R, mode.split("-")[0], k, seed, flags=1, **_faults(mode))
        ref.inject_random()
        REFS[case] = (ref.step(200).stats, ref.read_shard())
    return REFS[case]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("case", RANDOM_CASES, ids=[f"{c[0]}-N{c[3]}" for c in RANDOM_CASES])
@pytest.mark.parametrize("G", [2, 3, 5])
def test_host_lockstep_equals_one(G, case, plan):
    mode, k, R, N, seed, _ = case
    want, full = _ref(case)
    engines = [op.OracleEngine(N, R, mode.split("-")[0], k, seed, flags=1, shard_rank=r, shard_count=G,
                               **_faults(mode), params=PLANS[plan]) for r in range(G)]
    for e in engines:
        e.inject_random()
    stats, kinds = lockstep_run(engines, 200)
    assert stats == want
    for e in engines:
        assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])
    reps = {REP_GATHER, REP_CLASSCODED}
    if R > 64:
        assert set(kinds) == {DENSE}  # W > 1: the plain state all-gather only
    elif plan in PLAN_KINDS:
        assert set(kinds) == PLAN_KINDS[plan]
    elif plan == "replicated":  # the image gathered once (whole or class-coded), then stays whole
        assert kinds[0] in reps and set(kinds[1:]) == {REP}
    elif plan == "auto-replicated":  # every dense round replicated; after a sparse one, gathered again
        # (a few nodes, as under "auto" below: the cost model may plan no sparse round)
        assert (SPARSE in kinds or N < 1000) and set(kinds) & reps and set(kinds) <= {SPARSE, REP} | reps
        assert all(k in reps for i, k in enumerate(kinds)
                   if k in reps | {REP} and (i == 0 or kinds[i - 1] == SPARSE))
    elif plan == "auto" and N >= 1000:
        assert CLASSCODED in kinds and SPARSE in kinds
    elif plan == "auto":  # a few nodes: the link-aware cost model may keep every round dense
        assert set(kinds) <= {DENSE, SPARSE, CLASSCODED}


@pytest.mark.parametrize("G", [2, 3, 5])
def test_host_lockstep_flood_equals_one(G):
    """The 49-node grid with three injects: 200 rounds asked for, converged at round 12."""
    N = 49
    engines = [op.OracleEngine(N, 3, "flood", 0, 0, flags=1)]
    engines += [op.OracleEngine(N, 3, "flood", 0, 0, flags=1, shard_rank=r, shard_count=G) for r in range(G)]
    for e in engines:
        e.set_topology(_grid(N))
        e.inject(0, 0); e.inject(N - 1, 1); e.inject(N // 2, 2)
    ref, shards = engines[0], engines[1:]
    want = ref.step(200)
    stats, kinds = lockstep_run(shards, 200)
    assert stats == want.stats and len(stats) == 12 and stats[-1]["converged"]
    assert set(kinds) == {DENSE}  # FLOOD rounds are always dense
    full = ref.read_shard()
    for e in shards:
        assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])


AE_RUNS = AE_CASES + [(100, 8, 1, 5, 0.05, 0.3)]  # the last at G = 4: shards of 64, 36, 0 and 0 nodes


@pytest.mark.parametrize("case", AE_RUNS, ids=[f"N{c[0]}-K{c[1]}-k{c[2]}" for c in AE_RUNS])
def test_host_lockstep_antientropy_equals_one(case):
    """Rows and stats (round masked, as over gloo), with a client write after 4 rounds."""
    N, K, k, seed, fail, rec = case
    kw = dict(flags=1, churn_fail=ct(fail), churn_recover=ct(rec))

    def run(step, engines):
        for e in engines:
            e.inject_random()
        out = step(4)
        for e in engines:
            e.inject(N - 1, 0)
            e.inject(N // 3, K - 1)
        return out, step(300)

    ref = op.OracleEngine(N, K, "antientropy", k, seed, **kw)
    a, b = run(lambda n: ref.step(n).stats, [ref])
    want, rows = [dict(s, round=0) for s in a + b], ref.read_rows()
    assert b[-1]["converged"]
    for G in (2, 4):
        engines = [op.OracleEngine(N, K, "antientropy", k, seed, shard_rank=r, shard_count=G, **kw) for r in range(G)]
        (a, ka), (b, kb) = run(lambda n: lockstep_run(engines, n), engines)
        assert [dict(s, round=0) for s in a + b] == want and set(ka + kb) == {ANTIENTROPY}
        for e in engines:
            assert np.array_equal(e.read_rows(), rows[e.lo:e.hi])
