"""GPU: ANTIENTROPY under edge loss and partitions on every round path, one engine
and sharded, bit for bit per round against the numpy restatement (ae_faults_ref.py): stats,
per-component counts, hash, every row, the probed alive flags.  The restatement itself is held to
the frozen C oracle on the CPU (test_ae_faults_ref.py); the identity test here holds the engine to
the C oracle's faulty PUSHPULL directly.

Every reference is computed once per case and shared by the paths.  Guards keep a case from passing
vacuously: the reference lost at least one alive-alive edge in the first faulted round, a loss run
completed fewer exchanges in it than the fault-free run, and a standing partition kept the run from
converging.  Under a partition nobody holds the global max vector (full_nodes == 0) whenever K > 1;
with one component the global max is some node's own value, so its block fills up and only that
block: there the guard is 0 < full_nodes <= the largest block."""
import functools
import os

import numpy as np
import pytest

import ae_faults_ref as fr
import oracle_py as op
from gossip_hip import FLAG_AE_DIRECT_SCAN, Engine, GossipError
from gossip_hip.engine import Group, churn_threshold as ct, loss_threshold as lt

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
# the path table of test_gpu_antientropy.py: (flags, gossip_set_param knobs) per path
PATHS = {"auto": (0, {}), "dense": (0, {"ae_sparse": 0}), "sparse": (0, {"ae_sparse": 1}),
         "dense_atomic": (0, {"ae_sparse": 0, "ae_dense_bin": 0}),
         "dense_nofilter": (0, {"ae_sparse": 0, "ae_dense_filter": 0}),
         "dense_ranges": (0, {"ae_sparse": 0, "ae_dense_cap": 256}),
         "dense_fallback": (0, {"ae_sparse": 0, "ae_dense_cap": 16}),
         "overflow": (0, {"ae_sparse": 1, "ae_cap": 64}),
         "sparse_direct": (FLAG_AE_DIRECT_SCAN, {"ae_sparse": 1}),
         "auto_direct": (FLAG_AE_DIRECT_SCAN, {}),
         "auto_ahead1": (0, {"ae_ahead": 1}), "sparse_ahead3": (0, {"ae_sparse": 1, "ae_ahead": 3}),
         "overflow_ahead3": (0, {"ae_sparse": 1, "ae_cap": 64, "ae_ahead": 3})}
LOSS, PARTS = lt(0.3), 3


def test_path_table_is_the_parity_tests():
    import test_gpu_antientropy as ta
    assert PATHS == ta.PATHS


def _probe(N):
    return (0, 1, N // 3, N // 2, N - 1)


def _args(N, K, k, seed, fail, rec, **fa):
    return (N, K, "antientropy", k, seed), dict(flags=1, churn_fail=ct(fail), churn_recover=ct(rec), **fa)


def _engine(path, args, kw):
    pf, params = PATHS[path]
    kw = dict(kw, flags=kw["flags"] | pf)
    return Engine(*args, params=params, **kw)


@functools.lru_cache(maxsize=None)
def _reference(args, kwitems, script):
    """(run_script's result, lost alive-alive edges per round) of the restatement."""
    r = fr.RefEngine(*args, **dict(kwitems))
    out = fr.run_script(r, script, _probe(args[0]))
    return out, tuple(r.lost)


@functools.lru_cache(maxsize=None)
def _round0_messages_without_faults(args, kwitems):
    kw = {k: v for k, v in kwitems if k not in ("edge_loss", "partitions")}
    r = fr.RefEngine(*args, **kw)
    r.inject_random()
    return r.step(1).stats[0]["messages"]


def _want(args, kw, script):
    return _reference(args, tuple(sorted(kw.items())), script)


def _flat(out):
    return [s for o in out for s in o["stats"]]


def _guards(args, kw, want, lost, first=0, standing=None, from_start=True):
    """first: the first faulted round; standing: the rounds [a, b) a partition stood in; from_start:
    it stood from round 0 on (else rows may have met the global max before it: only no convergence)."""
    N, K = args[0], args[1]
    stats = _flat(want)
    assert lost[first] > 0
    if kw.get("edge_loss") and first == 0:
        assert stats[0]["messages"] < _round0_messages_without_faults(args, tuple(sorted(kw.items())))
    if standing:
        for s in stats[standing[0]:standing[1]]:
            assert not s["converged"]
            if not from_start:
                continue
            if K > 1:
                assert s["full_nodes"] == 0, s
            else:
                assert 0 < s["full_nodes"] <= -(-N // PARTS), s


def _check(path, args, kw, script, **guards):
    want, lost = _want(args, kw, script)
    _guards(args, kw, want, lost, **guards)
    e = _engine(path, args, kw)
    got = fr.run_script(e, script, _probe(args[0]))
    fr.assert_same(got, want)
    assert e.state_hash() == _flat(want)[-1]["state_hash"]
    e.close()
    return want


SHAPES = [(1 << 16, 16, 1, 0.01, 0.1), (50_001, 5, 2, 0.05, 0.3), (4099, 64, 3, 0.02, 0.2), (777, 1, 1, 0.0, 0.0)]


def _writes(N, K):
    return (("inject", N // 2, K - 1), ("inject", 3, 0))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("N,K,k,fail,rec", SHAPES)
def test_loss_paths(path, N, K, k, fail, rec):
    """edge_loss = 0.3 throughout: a few rounds, two client writes, then to convergence (the
    restatement takes 56, 24 and 15 rounds for the first three shapes, 11 for the last)."""
    args, kw = _args(N, K, k, 0x5EED0005 + K, fail, rec, edge_loss=LOSS)
    script = (("random",), ("step", 6)) + _writes(N, K) + (("step", 400),)
    want = _check(path, args, kw, script)
    assert want[-1]["stats"][-1]["converged"]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("N,K,k,fail,rec", SHAPES)
def test_partition_paths(path, N, K, k, fail, rec):
    """partitions = 3 for 40 rounds (block boundaries off the 64-node chunks and the dense tiles at
    50001 and 4099), the two writes after round 6, then the heal and the run to convergence."""
    args, kw = _args(N, K, k, 0x5EED0005 + K, fail, rec, partitions=PARTS)
    script = (("random",), ("step", 6)) + _writes(N, K) + (("step", 34), ("faults", 0, 0), ("step", 400))
    want = _check(path, args, kw, script, standing=(0, 40))
    assert len(_flat(want[:2])) == 40 and want[-1]["stats"][-1]["converged"]


# fanout classes and row widths the shapes above miss: k = 5 and 9 reach loss-draw counter words 1
# and 2 and the churn word's own stream; K = 2, 4, 32, 17 the row widths L = 2, 4, 32 and a ragged one
WIDE = [(20011, 2, 2), (20011, 4, 3), (20011, 32, 1), (4099, 17, 5), (20011, 16, 4), (130, 3, 9)]


@pytest.mark.parametrize("path", ["auto", "dense_atomic", "sparse"])
@pytest.mark.parametrize("N,K,k", WIDE)
def test_fanouts_and_widths(path, N, K, k):
    """Loss 0.25 together with partitions = 2 for 26 rounds; then the partition heals, the loss stays
    and the run converges."""
    loss = lt(0.25)
    args, kw = _args(N, K, k, 0x5EED0B00 + 16 * K + k, 0.03, 0.25, edge_loss=loss, partitions=2)
    script = (("random",), ("step", 6)) + _writes(N, K) + (("step", 20), ("faults", loss, 0), ("step", 400))
    want, lost = _want(args, kw, script)
    assert not any(s["converged"] for s in _flat(want[:2])) and len(_flat(want[:2])) == 26
    want = _check(path, args, kw, script)
    assert want[-1]["stats"][-1]["converged"]


@functools.lru_cache(maxsize=None)
def _oracle_pushpull(N, k, seed, loss, parts, rounds):
    o = op.OracleEngine(N, 1, "pushpull", k, seed, threads=THREADS, edge_loss=loss, partitions=parts)
    for n in (0, N // 3, N - 1):
        o.inject(n, 0)
    out = []
    for _ in range(rounds):
        r = o.step(1)
        out.append((r.stats[0]["full_nodes"], int(r.infected[0][0]), (o.read_shard()[0] & np.uint64(1)).astype(np.uint32)))
    o.close()
    return out


@pytest.mark.parametrize("path", ["auto", "sparse"])
@pytest.mark.parametrize("N,k,loss,parts", [(4099, 3, 0.25, 2), (1000, 9, 0.5, 4)])
def test_identity_against_the_oracles_pushpull(path, N, k, loss, parts):
    """K = 1, no churn, rows written by inject(n, 0) only: the faulty ANTIENTROPY engine is the C
    oracle's PUSHPULL with R = 1 and the same seed, N, k, edge_loss and partitions:
    V[n][0] = bit 0 of S[n], full_nodes and infected[0] equal, every round."""
    seed, rounds = 0x5EED0B00 + k, 60
    want = _oracle_pushpull(N, k, seed, lt(loss), parts, rounds)
    args, kw = _args(N, 1, k, seed, 0.0, 0.0, edge_loss=lt(loss), partitions=parts)
    e = _engine(path, args, kw)
    for n in (0, N // 3, N - 1):
        e.inject(n, 0)
    for t in range(rounds):
        r = e.step(1)
        full, inf, bits = want[t]
        assert r.stats[0]["full_nodes"] == full and int(r.infected[0][0]) == inf, t
        assert np.array_equal(e.read_rows()[:, 0], bits), t
    assert 3 < want[0][1] < want[-1][1]  # the writes spread
    e.close()


HEAL = (50_001, 5, 2, 0x5EED000A, 0.05, 0.3)


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_heal_midrun(path):
    """A partition with loss, then set_faults(0, 0): rows, alive bits and the round index stay."""
    N, K = HEAL[:2]
    args, kw = _args(*HEAL, edge_loss=LOSS, partitions=PARTS)
    script = (("random",), ("step", 6)) + _writes(N, K) + (("step", 20), ("faults", 0, 0), ("step", 400))
    want = _check(path, args, kw, script, standing=(0, 26))
    assert want[-1]["stats"][-1]["converged"] and want[-1]["stats"][0]["round"] == 26


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_faults_switched_on_later(path):
    """An engine created without faults takes them from gossip_set_faults in the next round."""
    args, kw = _args(*HEAL)
    script = (("random",), ("step", 3), ("faults", LOSS, PARTS), ("step", 20), ("faults", 0, 0), ("step", 400))
    want = _check(path, args, kw, script, first=3, standing=(3, 23), from_start=False)
    assert sum(_want(args, kw, script)[1][:3]) == 0 and want[-1]["stats"][-1]["converged"]


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_reset_then_second_run(path):
    """gossip_reset keeps the faults: the second run loses the same edges as a fresh engine."""
    args, kw = _args(*HEAL, edge_loss=LOSS)
    script = (("random",), ("step", 10), ("reset",), ("random",), ("step", 400))
    want = _check(path, args, kw, script)
    assert want[-1]["stats"][-1]["converged"] and want[-1]["stats"][:10] == want[0]["stats"]


# from test_gpu_ae_sharded.py's list: N, K, fanout, seed, fail, recover, G
SHARDED = [
    (50_001, 5, 2, 0x5EED000A, 0.05, 0.3, 3),
    (4099, 64, 3, 3, 0.02, 0.2, 2),
    (100, 8, 1, 5, 0.05, 0.3, 4),    # shards of 64, 36, 0 and 0 nodes
    (20011, 16, 4, 25, 0.03, 0.25, 2),
    (130, 3, 9, 26, 0.05, 0.3, 4),   # k > 8: the fill pass redraws the loss words
]


@pytest.mark.parametrize("case", SHARDED, ids=[f"N{c[0]}-K{c[1]}-k{c[2]}-G{c[6]}" for c in SHARDED])
def test_sharded_lockstep(case):
    """G shard engines in lockstep (gossip_ae_*) with loss 0.3 and partitions = 3, then a heal applied
    to every rank: equal to one engine and to the restatement, every round of kind 2."""
    N, K, k, seed, fail, rec, G = case
    args, kw = _args(N, K, k, seed, fail, rec, edge_loss=LOSS, partitions=PARTS)
    script = (("random",), ("step", 5)) + _writes(N, K) + (("step", 15), ("faults", 0, 0), ("step", 400))
    want = _check("auto", args, kw, script, standing=(0, 20) if K > 1 else None)
    assert want[-1]["stats"][-1]["converged"]
    engines = [Engine(*args, shard_rank=r, shard_count=G, **kw) for r in range(G)]
    got = fr.run_script(engines, script)
    fr.assert_same(got, want, keys=("stats", "rows"))
    assert all(g["kinds"] == [2] for g in got)
    for e in engines:
        e.close()


def test_group_with_faults_at_create():
    N, K, k, seed, fail, rec, G = SHARDED[0]
    args, kw = _args(N, K, k, seed, fail, rec, edge_loss=LOSS)
    script = (("random",), ("step", 400))
    want, lost = _want(args, kw, script)
    _guards(args, kw, want, lost)
    with Group(*args, n_shards=G, devices=[0] * G, **kw) as g:
        g.inject_random()
        got = g.step(400)
        assert got.stats == want[0]["stats"] and got.converged
        assert np.array_equal(got.infected, want[0]["infected"])
        for e in g.shards:
            assert np.array_equal(e.read_rows(), want[0]["rows"][e.lo:e.hi])


def test_stall_rounds_rejected():
    """ANTIENTROPY has no per-neighbour deadline: GOSSIP_ENOTSUP at create."""
    for kw in (dict(stall_rounds=1), dict(stall_rounds=2, edge_loss=LOSS)):
        with pytest.raises(GossipError) as ei:
            Engine(1000, 4, "antientropy", 1, 1, **kw)
        assert ei.value.code == -6 and "stall_rounds" in str(ei.value)
        with pytest.raises(GossipError):
            Group(1000, 4, "antientropy", 1, 1, n_shards=2, devices=[0] * 2, **kw)
