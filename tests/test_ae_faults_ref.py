"""CPU: ANTIENTROPY under edge loss and partitions, the numpy restatement
(ae_faults_ref.py) held to the frozen C oracle and to closed forms, and the ABI's create check.

The C oracle has no faulty ANTIENTROPY.  It has ANTIENTROPY without faults and PUSHPULL with them,
and the identity of §2.11 ties the two: with one component, no churn and rows written only by
inject(n, 0), versions are 0 or 1, max-merge is OR, and the faulty ANTIENTROPY engine is a PUSHPULL
engine of one rumor with the same seed, N, k, edge_loss and partitions (the loss draws are the same
stream-4 words).  `messages` differs by definition (completed exchanges against 2 per attempt)."""
import ctypes as C
import os

import numpy as np
import pytest

import ae_faults_ref as fr
import oracle_py as op
from gossip_hip import engine as eng_mod
from gossip_hip.engine import churn_threshold as ct, loss_threshold as lt

THREADS = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("N,K,k,fail,rec", [(777, 1, 1, 0.0, 0.0), (4099, 5, 2, 0.05, 0.3)])
def test_no_faults_equals_the_oracle(N, K, k, fail, rec):
    """edge_loss = 0, partitions <= 1: the restatement is the oracle's ANTIENTROPY, per round."""
    seed = 0x5EED0005 + K
    kw = dict(flags=1, churn_fail=ct(fail), churn_recover=ct(rec))
    r = fr.RefEngine(N, K, "antientropy", k, seed, **kw)
    o = op.OracleEngine(N, K, "antientropy", k, seed, threads=THREADS, **kw)
    for x in (r, o):
        x.inject_random()
    for rounds in (6, 400):  # a few rounds, two client writes, then to convergence
        a, b = r.step(rounds), o.step(rounds)
        assert a.rounds == b.rounds and a.stats == b.stats
        assert np.array_equal(a.infected, b.infected)
        assert np.array_equal(r.read_rows(), o.read_rows())
        if rounds == 6:
            for x in (r, o):
                x.inject(N // 2, K - 1)
                x.inject(3, 0)
    assert a.converged and sum(r.lost) == 0
    o.close()


IDENTITY = [(777, 1, 0.3, 0), (4099, 2, 0.0, 3), (4099, 3, 0.25, 2), (2050, 5, 0.4, 0), (1000, 9, 0.5, 4)]


@pytest.mark.parametrize("N,k,loss,parts", IDENTITY, ids=[f"N{c[0]}-k{c[1]}-P{c[3]}" for c in IDENTITY])
def test_identity_against_the_oracles_pushpull(N, k, loss, parts):
    """K = 1, no churn, rows from inject(n, 0) only: V[n][0] is bit 0 of the C oracle's PUSHPULL state
    with R = 1 and the same faults, every round up to 60; full_nodes and infected[0] are equal."""
    seed = 0x5EED0B00 + k
    fa = dict(edge_loss=lt(loss), partitions=parts)
    r = fr.RefEngine(N, 1, "antientropy", k, seed, **fa)
    o = op.OracleEngine(N, 1, "pushpull", k, seed, threads=THREADS, **fa)
    for x in (r, o):
        for n in (0, N // 3, N - 1):
            x.inject(n, 0)
    assert r.step(1).stats[0]["messages"] < N * k and r.lost[0] > 0  # the faults dropped something
    o.step(1)
    for t in range(1, 60):
        assert np.array_equal(r.read_rows()[:, 0].astype(np.uint64), o.read_shard()[0] & np.uint64(1)), t
        a, b = r.step(1), o.step(1)
        assert a.stats[0]["round"] == b.stats[0]["round"] == t
        assert a.stats[0]["full_nodes"] == b.stats[0]["full_nodes"], t
        assert int(a.infected[0][0]) == int(b.infected[0][0]), t
        assert a.stats[0]["converged"] == b.stats[0]["converged"]
    # the run converges iff every partition block holds one of the three writes
    blocks = {(n * parts) // N for n in (0, N // 3, N - 1)} if parts > 1 else {0}
    assert (a.stats[0]["converged"] == 1) == (len(blocks) == max(parts, 1))
    o.close()


@pytest.mark.parametrize("N,K,k", [(4099, 5, 2), (50001, 16, 1)])
def test_partition_closed_form_then_heal(N, K, k):
    """No churn, no loss, partitions = 3: every row reaches the componentwise max over the node's own
    block and stays there, nobody holds the global max vector, and after set_faults(0, 0) the run
    converges to it.  (Measured, seed 7: block maxima after 17 and 38 rounds, 3-4 rounds to heal.)"""
    P = 3
    r = fr.RefEngine(N, K, "antientropy", k, 7, partitions=P)
    r.inject_random()
    V0 = r.read_rows()
    block = (np.arange(N, dtype=np.int64) * P) // N
    want = np.stack([V0[block == b].max(axis=0) for b in range(P)])[block]
    reached = None
    for t in range(60):
        st = r.step(1).stats[0]
        assert st["full_nodes"] == 0 and st["converged"] == 0
        if np.array_equal(r.read_rows(), want):
            reached = reached if reached is not None else t + 1
        else:
            assert reached is None, t  # once there, the rows stay
        if reached is not None and t + 1 >= reached + 3:
            break
    assert reached is not None and r.lost[0] > 0
    r.set_faults(0, 0)
    res = r.step(100)
    assert res.converged and res.rounds < 100
    assert (r.read_rows() == V0.max(axis=0)[None, :]).all() and sum(r.lost[-res.rounds:]) == 0


def test_total_loss_moves_nothing():
    """edge_loss = 2^32 - 1 loses every edge (but a draw of exactly 2^32 - 1): no row moves."""
    N, K, k = 4099, 5, 2
    r = fr.RefEngine(N, K, "antientropy", k, 11, churn_fail=ct(0.05), churn_recover=ct(0.3), edge_loss=0xFFFFFFFF)
    r.inject_random()
    V0 = r.read_rows()
    res = r.step(5)
    assert res.rounds == 5 and [s["messages"] for s in res.stats] == [0] * 5
    assert np.array_equal(r.read_rows(), V0) and min(r.lost) > 0


def test_create_takes_antientropy_faults():
    """gossip_create no longer answers GOSSIP_ENOTSUP (-6) to a faulty ANTIENTROPY config: the fault
    check sits before the device check, so without a device the answer is GOSSIP_ENODEV (-5), with
    one GOSSIP_OK.  stall_rounds stays rejected: ANTIENTROPY has no per-neighbour deadline."""
    lib = eng_mod.load_library()
    for kw in (dict(edge_loss=lt(0.3)), dict(partitions=3), dict(edge_loss=1, partitions=2),
               dict(edge_loss=lt(0.3), shard_count=2)):
        cfg = eng_mod.make_config(100, 16, "antientropy", 1, 1, **kw)
        h = C.c_void_p()
        rc = lib.gossip_create(C.byref(cfg), C.byref(h))
        assert rc in (0, -5), (kw, rc)
        if rc == 0:
            lib.gossip_destroy(h)
    for kw in (dict(stall_rounds=1), dict(stall_rounds=1, edge_loss=lt(0.3))):
        cfg = eng_mod.make_config(100, 16, "antientropy", 1, 1, **kw)
        h = C.c_void_p()
        assert lib.gossip_create(C.byref(cfg), C.byref(h)) == -6
        assert b"stall_rounds" in lib.gossip_last_error(None)
