"""CPU, world 3 over gloo: the per-rank driver's trace (plan kind and link bytes of every round,
sharded_run(..., trace=)) equals tests/golden/shard_trace.json, recorded from the commit before the
round bodies were shared between the drivers (tests/golden/make_shard_trace.py); lockstep_run on
host shards plans the same kinds (the plan is a function of the global totals only)."""
import json
import os
import sys

import pytest
import torch.multiprocessing as mp

from test_sharded_gloo import AE_CASES, CASES, PLANS, _faults, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 3
AE = "antientropy"  # AE_CASES[1]; the other runs are CASES[0] under that plan of PLANS
RUNS = [(plan, direct) for plan in ("auto", "exchange", "classcoded", "replicated", AE) for direct in (None, True)]


def run_id(plan, direct):
    return f"{plan}-{'direct' if direct else 'staged'}"


def _engines(op, plan, ranks):
    """The shard engines of a run, injected: (engines, the injection that follows the first 4 rounds or None)"""
    if plan == AE:
        from gossip_hip.engine import churn_threshold as ct
        N, K, k, seed, fail, rec = AE_CASES[1]
        es = [op.OracleEngine(N, K, AE, k, seed, flags=1, shard_rank=r, shard_count=WORLD, churn_fail=ct(fail),
                              churn_recover=ct(rec)) for r in ranks]
        again = [(N - 1, 0), (N // 3, K - 1)]  # a client write mid-run: the global max vector is re-derived
    else:
        mode, k, R, N, seed, _ = CASES[0]
        es = [op.OracleEngine(N, R, mode, k, seed, flags=1, shard_rank=r, shard_count=WORLD, **_faults(mode),
                              params=PLANS[plan]) for r in ranks]
        again = None
    for e in es:
        e.inject_random()
    return es, again


def _worker(rank, port, root, plan, direct, q):
    sys.path[:0] = [os.path.join(root, "gossip-protocol_amd"), os.path.join(root, "oracle")]
    import torch.distributed as dist
    import oracle_py as op
    from gossip_hip.sharded import sharded_run
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    (e,), again = _engines(op, plan, [rank])
    trace = []
    if again:
        sharded_run(e, 4, direct=direct, trace=trace)
        for node, slot in again:
            e.inject(node, slot)
    sharded_run(e, 300, direct=direct, trace=trace)
    q.put((rank, [[t["kind"], t["link_bytes"]] for t in trace]))
    dist.destroy_process_group()


def record(root, plan, direct):
    """[kind, link_bytes] of every round, per rank, from the gossip_hip and oracle of the tree at root."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, root, plan, direct, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(WORLD))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return [got[r] for r in range(WORLD)]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "shard_trace.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("plan,direct", RUNS, ids=[run_id(*r) for r in RUNS])
def test_trace_equals_recorded(recorded, plan, direct):
    want = recorded[run_id(plan, direct)]
    assert record(ROOT, plan, direct) == want
    import oracle_py as op
    from gossip_hip.sharded import lockstep_run
    engines, again = _engines(op, plan, range(WORLD))
    kinds = []
    if again:
        kinds += lockstep_run(engines, 4)[1]
        for e in engines:
            for node, slot in again:
                e.inject(node, slot)
    kinds += lockstep_run(engines, 300)[1]
    for rank in want:
        assert kinds == [k for k, _ in rank]
