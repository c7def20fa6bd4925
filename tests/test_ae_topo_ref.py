"""CPU: ANTIENTROPY over the topology, the numpy restatement (ae_topo_ref.py) held
to what is already pinned and to closed forms, and the flag's value.

The C oracle has no topology ANTIENTROPY.  Two identities of §2.12 tie the restatement to it:
(a) on total_topology(N) row_n[i] = i + (i >= n), the uniform peer map, so the restatement is the
    oracle's ANTIENTROPY in every field (with faults: ae_faults_ref.AeFaultsSim, itself pinned);
(b) with one component, no churn and rows written only by inject(n, 0), max-merge is OR and the
    restatement is topo_ref.TopoSim's PUSHPULL with R = 1 on the same topology, seed, k and faults,
    in V[n][0], full_nodes and infected[0] (messages differ by definition)."""
import functools
import os
import re

import numpy as np
import pytest

import ae_faults_ref as fr
import ae_topo_ref as ar
import oracle_py as op
import topo_ref as tr
import topologies as tp
from conftest import ROOT
from gossip_hip import total_topology
from gossip_hip.engine import churn_threshold as ct, loss_threshold as lt

THREADS = min(16, os.cpu_count() or 1)
N = 257


@functools.lru_cache(maxsize=None)
def complete(n=N):
    return tr.csr_of_names(total_topology(n))


@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 9])
def test_complete_graph_equals_the_oracle(k, K):
    """Identity (a) without faults, with churn and inject_random: every round to convergence or 60."""
    seed = 0x5EED0C00 + 16 * K + k
    kw = dict(flags=1, churn_fail=ct(0.04), churn_recover=ct(0.3))
    r = ar.RefEngine(N, K, "antientropy", k, seed, topology=complete(), **kw)
    o = op.OracleEngine(N, K, "antientropy", k, seed, threads=THREADS, **kw)
    for x in (r, o):
        x.inject_random()
    a, b = r.step(60), o.step(60)
    assert a.rounds == b.rounds and a.rounds > 1
    assert a.stats == b.stats
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(r.read_rows(), o.read_rows())
    for n in (0, 1, N // 2, N - 1):
        assert r.read_versions(n)[1] == o.read_versions(n)[1]
    assert sum(r.selfs) == 0 and sum(r.lost) == 0  # the complete graph has no self-loop
    o.close()


FAULTS = {"loss": dict(edge_loss=lt(0.3)), "parts": dict(partitions=3), "both": dict(edge_loss=lt(0.25), partitions=2)}


@pytest.mark.parametrize("faults", FAULTS, ids=list(FAULTS))
@pytest.mark.parametrize("K,k", [(1, 1), (5, 2), (16, 5), (3, 9)])
def test_complete_graph_equals_the_faults_restatement(K, k, faults):
    """Identity (a) with faults against AeFaultsSim: stats, lost edges, rows, every round; then a heal."""
    seed = 0x5EED0D00 + 16 * K + k
    kw = dict(flags=1, churn_fail=ct(0.04), churn_recover=ct(0.3), **FAULTS[faults])
    r = ar.RefEngine(N, K, "antientropy", k, seed, topology=complete(), **kw)
    f = fr.RefEngine(N, K, "antientropy", k, seed, **kw)
    script = (("random",), ("step", 25), ("faults", 0, 0), ("step", 60))
    got, want = ar.run_script(r, script, (0, N - 1)), fr.run_script(f, script, (0, N - 1))
    fr.assert_same(got, want)
    assert r.lost == f.lost and r.lost[0] > 0


@functools.lru_cache(maxsize=None)
def ragged(n, seed=5):
    return tp.ragged(n, seed, max_deg=7, hub_every=97, hub_deg=40)


@pytest.mark.parametrize("faults", [{}, FAULTS["loss"], FAULTS["both"]], ids=["clean", "loss", "both"])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_one_component_equals_topo_pushpull(k, faults):
    """Identity (b) on a ragged topology (empty rows, self-loops, repeats, hubs), 40 rounds."""
    n, seed = 1201, 0x5EED0E00 + k
    topo = ragged(n)
    r = ar.RefEngine(n, 1, "antientropy", k, seed, topology=topo, **faults)
    s = tr.TopoSim(n, 1, "pushpull", k, seed, topo, **faults)
    for x in (0, n // 3, n - 1):
        r.inject(x, 0)
        s.inject(x, 0)
    for t in range(40):
        a, (b, inf) = r.step(1), s.round()
        assert np.array_equal(r.read_rows()[:, 0].astype(np.uint64), s.read_shard()[0] & np.uint64(1)), t
        assert a.stats[0]["round"] == b["round"] == t
        assert a.stats[0]["full_nodes"] == b["full_nodes"], t
        assert int(a.infected[0][0]) == int(inf[0]), t
    assert 3 < int(a.infected[0][0])  # the writes spread
    assert (sum(r.lost) > 0) == bool(faults)
    # what the complete graph never gives (a pair can repeat only with two draws per node)
    assert sum(r.selfs) > 0 and (sum(r.repeats) > 0) == (k > 1) and min(r.empty_alive) > 0


def ring(n):
    return np.arange(n + 1, dtype=np.uint32), ((np.arange(n) + 1) % n).astype(np.uint32)


def test_directed_ring_moves_one_hop_per_round_in_each_direction():
    """row_n = [n + 1], k = 1: every node exchanges with its successor each round, so a write at node
    5 reaches one more node on either side per round (the push forward, the pull backward)."""
    n = 41
    r = ar.RefEngine(n, 2, "antientropy", 1, 9, topology=ring(n))
    r.inject(5, 1)
    for t in range(19):
        st = r.step(1).stats[0]
        held = set(np.nonzero(r.read_rows()[:, 1])[0].tolist())
        assert held == {(5 + d) % n for d in range(-(t + 1), t + 2)}, t
        assert st["messages"] == n and st["full_nodes"] == 2 * (t + 1) + 1
    assert not st["converged"]
    assert r.step(1).stats[0]["converged"]  # 2 * 20 + 1 = 41 nodes
    assert sum(r.selfs) == 0 and sum(r.repeats) == 0


def test_empty_row_never_initiates_and_still_receives():
    """Node z has no row but sits in everybody's: it answers (both ends of an exchange merge), so its
    own write spreads and it learns the others'; messages counts the other nodes' exchanges only."""
    n, z, k = 33, 7, 2
    rows = [[] if u == z else [z, (u + 1) % n] for u in range(n)]
    rp = np.zeros(n + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    topo = (rp, np.array([v for r in rows for v in r], dtype=np.uint32))
    r = ar.RefEngine(n, 2, "antientropy", k, 3, topology=topo)
    r.inject(0, 0)
    r.inject(z, 1)
    res = r.step(40)
    assert res.converged and all(s["messages"] == k * (n - 1) for s in res.stats)
    assert r.empty_alive == [1] * res.rounds
    # nobody but z in z's row and nobody draws z: z's write never leaves, z never learns
    rows = [[] if u == z else [(u + 1) % n if (u + 1) % n != z else (u + 2) % n] for u in range(n)]
    rp[1:] = np.cumsum([len(x) for x in rows])
    topo = (rp, np.array([v for x in rows for v in x], dtype=np.uint32))
    r = ar.RefEngine(n, 2, "antientropy", k, 3, topology=topo)
    r.inject(0, 0)
    r.inject(z, 1)
    res = r.step(50)
    V = r.read_rows()
    assert not res.converged and res.rounds == 50
    assert int(V[z, 0]) == 0 and int((V[:, 1] != 0).sum()) == 1 and int((V[:, 0] != 0).sum()) == n - 1


def test_two_components_then_a_bridge():
    """Two rings that never meet: every row reaches its component's maximum and stays there,
    full_nodes < alive_nodes throughout, and one bridging edge (set_topology) makes it converge."""
    n, h, K = 64, 30, 3
    col = np.concatenate([(np.arange(h) + 1) % h, h + (np.arange(n - h) + 1) % (n - h)]).astype(np.uint32)
    topo = (np.arange(n + 1, dtype=np.uint32), col)
    r = ar.RefEngine(n, K, "antientropy", 2, 21, topology=topo)
    r.inject_random()
    V0 = r.read_rows()
    comp = (np.arange(n) >= h).astype(np.int64)
    want = np.stack([V0[comp == c].max(axis=0) for c in (0, 1)])[comp]
    assert not (want[0] == want[-1]).all()  # neither ring holds the global max vector
    reached = None
    for t in range(60):
        st = r.step(1).stats[0]
        assert st["full_nodes"] < st["alive_nodes"] and not st["converged"]
        if np.array_equal(r.read_rows(), want):
            reached = reached if reached is not None else t + 1
        else:
            assert reached is None, t
    assert reached is not None and reached <= 40
    rp = np.arange(n + 1, dtype=np.uint32)
    rp[1:] += 1  # node 0 gets a second entry: the first node of the other ring
    r.set_topology((rp, np.concatenate([[col[0], h], col[1:]]).astype(np.uint32)))
    res = r.step(100)
    assert res.converged and res.stats[0]["round"] == 60
    assert (r.read_rows() == V0.max(axis=0)[None, :]).all()


def test_row_index_is_the_host_probe():
    from gossip_hip import topo_peer_index
    nodes = np.array([0, 1, 77, 30010, 2**21 + 5, 2**32 - 2], dtype=np.uint64)
    for seed in (0, 0x5EED0003, 0xFEDCBA9876543210):
        for degree in (1, 2, 3, 300, 2**32 - 1):
            for t, j in ((0, 0), (1, 3), (23, 4), (7, 8)):
                want = tr.row_index(seed, np.full(nodes.size, degree, dtype=np.uint64), nodes, t, j)
                assert [topo_peer_index(seed, degree, int(n), t, j) for n in nodes] == [int(x) for x in want]
    # and the restatement's peers are the rows' entries at that index
    n, topo = 1201, ragged(1201)
    sim = ar.AeTopoSim(n, 1, 5, 0x5EED0003, topology=topo)
    sim.t = 4
    rp, col = tr.rows_as_sets(topo[0], topo[1], n)
    for j in range(5):
        p = sim.peers(j)
        for u in (0, 1, 98, 600, n - 1):
            d = int(rp[u + 1] - rp[u])
            assert int(p[u]) == (int(col[rp[u] + topo_peer_index(0x5EED0003, d, u, 4, j)]) if d else u)


def test_header_declares_the_flag():
    import gossip_hip
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    m = re.search(r"\bGOSSIP_FLAG_AE_TOPO_PEERS\s*=\s*1u\s*<<\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 7
    assert gossip_hip.FLAG_AE_TOPO_PEERS == 128
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u", hdr)


def test_create_checks_the_flag():
    """Item 8 of §2.12: the flag with another mode, or together with GOSSIP_FLAG_TOPO_PEERS, is
    GOSSIP_EINVAL (-1) before the device check; with ANTIENTROPY the answer is GOSSIP_OK or, without a
    device, GOSSIP_ENODEV (-5); stall_rounds stays GOSSIP_ENOTSUP (-6)."""
    import ctypes as C
    from gossip_hip import FLAG_AE_TOPO_PEERS, FLAG_TOPO_PEERS, engine as eng_mod
    lib = eng_mod.load_library()

    def create(mode, flags, **kw):
        cfg = eng_mod.make_config(100, 4, mode, 2, 1, flags, **kw)
        h = C.c_void_p()
        rc = lib.gossip_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            lib.gossip_destroy(h)
        return rc

    einval = eng_mod.GossipError(-1, "").code
    for mode in ("flood", "push", "pull", "pushpull"):
        assert create(mode, FLAG_AE_TOPO_PEERS) == einval, mode
        assert create(mode, FLAG_AE_TOPO_PEERS | FLAG_TOPO_PEERS) == einval, mode
    assert create("antientropy", FLAG_AE_TOPO_PEERS | FLAG_TOPO_PEERS) == einval
    assert create("antientropy", FLAG_AE_TOPO_PEERS) in (0, -5)
    assert create("antientropy", FLAG_AE_TOPO_PEERS, shard_count=2, edge_loss=lt(0.3)) in (0, -5)
    assert create("antientropy", FLAG_AE_TOPO_PEERS, stall_rounds=1) == -6
