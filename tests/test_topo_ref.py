"""CPU: the numpy restatement of random gossip over the topology (tests/topo_ref.py, DESIGN.md
§2.10) is tied to the C oracle by the identity of the complete graph — row_n = every node but
n, so row_n[i] = i + (i >= n), which is the uniform draw of §2.2 — and checked on topologies
whose runs have closed forms.  The host probe gossip_topo_peer_index and the flag's value are
held to it too (the library loads without a GPU)."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_py as op
import topo_ref as tr
from conftest import ROOT
from gossip_hip import loss_threshold, total_topology

N = 257
MODES = ("push", "pull", "pushpull")
FAULTS = {
    "clean": {},
    "loss": dict(edge_loss=loss_threshold(0.25)),
    "parts": dict(partitions=3),
    "loss-parts": dict(edge_loss=loss_threshold(0.25), partitions=3),
    "loss-parts-stall": dict(edge_loss=loss_threshold(0.25), partitions=3, stall_rounds=2),
}


@functools.lru_cache(maxsize=None)
def complete():
    return tr.csr_of_names(total_topology(N))


def injects(n, R):
    return [((431 * i) % n, i) for i in range(R)]


def test_complete_rows_are_the_uniform_peer_map():
    rp, col = complete()
    assert np.array_equal(np.diff(rp.astype(np.int64)), np.full(N, N - 1))
    i = np.arange(N - 1)
    for n in (0, 1, 100, N - 1):
        assert np.array_equal(col[rp[n]:rp[n + 1]], i + (i >= n))


@pytest.mark.parametrize("faults", FAULTS, ids=list(FAULTS))
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("mode", MODES)
def test_complete_topology_equals_the_oracle(mode, k, R, faults):
    kw = FAULTS[faults]
    seed = 0x5EED0000 + k
    sim = tr.TopoSim(N, R, mode, k, seed, complete(), **kw)
    ora = op.OracleEngine(N, R, mode, k, seed, flags=1, **kw)
    for n, r in injects(N, R):
        sim.inject(n, r)
        ora.inject(n, r)
    rounds = 200 if kw else 60
    b = ora.step(rounds)
    stats, infected, held = [], [], []
    while len(stats) < rounds and not (stats and stats[-1]["converged"]):
        held.append(int((sim.read_shard() != 0).any(axis=0).sum()))  # nodes holding something in S_t
        one = sim.step(1)
        stats += one.stats
        infected.append(one.infected[0])
    assert len(stats) == b.rounds and b.rounds > 2
    for sa, sb in zip(stats, b.stats):
        for f in ("round", "converged", "full_nodes", "alive_nodes", "state_hash"):
            assert sa[f] == sb[f], (f, sa, sb)
    assert np.array_equal(np.array(infected, dtype=np.uint64), b.infected)
    assert np.array_equal(sim.read_shard(), ora.read_shard())
    ora.close()
    # every node has a row: k exchanges each, PUSH only from the holders of S_t (stalled nodes: none)
    if not kw.get("stall_rounds"):
        want = [k * h for h in held] if mode == "push" else [k * N] * len(stats)
        assert [s["messages"] for s in stats] == want


def ring(n):
    return np.arange(n + 1, dtype=np.uint32), ((np.arange(n) + 1) % n).astype(np.uint32)


@pytest.mark.parametrize("k", [1, 3])
def test_directed_ring_push_moves_one_hop_per_round(k):
    """row_n = [n + 1]: every draw is that one neighbour, so the value walks the ring, one hop per
    round, and round t sends k messages from each of its t + 1 holders."""
    n = 41
    sim = tr.TopoSim(n, 1, "push", k, 9, ring(n))
    sim.inject(5, 0)
    res = sim.step(n + 5)
    assert res.rounds == n - 1 and res.stats[-1]["converged"]
    for t, st in enumerate(res.stats):
        assert int(res.infected[t][0]) == t + 2
        assert st["messages"] == k * (t + 1)
    sim = tr.TopoSim(n, 1, "push", k, 9, ring(n))
    sim.inject(5, 0)
    sim.step(7)
    held = np.nonzero(sim.read_shard()[0])[0]
    assert list(held) == list(range(5, 13))


def test_directed_ring_pull_never_moves_forward():
    """PULL reads S'[n] |= S[p_j(n)]: node n asks n + 1, so nothing ever travels along the edges
    (no node after the origin learns the value before it has gone all the way round against
    them), and every node initiates its k exchanges every round."""
    n, k = 41, 2
    sim = tr.TopoSim(n, 1, "pull", k, 9, ring(n))
    sim.inject(5, 0)
    res = sim.step(10)
    assert [int(x[0]) for x in res.infected] == list(range(2, 12))
    held = set(np.nonzero(sim.read_shard()[0])[0].tolist())
    assert held == {(5 - i) % n for i in range(11)} and not held & set(range(6, 30))
    assert all(st["messages"] == k * n for st in res.stats)


def test_empty_row_never_initiates_and_still_receives():
    """Node z has no row but sits in everybody's: it is pushed to, never pushes (its own value
    stays with it), pulls nothing, and is not counted in messages."""
    n, z, k = 33, 7, 2
    rows = [[] if u == z else [z, (u + 1) % n] for u in range(n)]
    rp = np.zeros(n + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    topo = (rp, np.array([v for r in rows for v in r], dtype=np.uint32))
    sim = tr.TopoSim(n, 2, "push", k, 3, topo)
    sim.inject(0, 0)
    sim.inject(z, 1)
    res = sim.step(40)
    S = sim.read_shard()[0]
    assert int(S[z]) == 3                               # received value 0
    assert [int(x[1]) for x in res.infected] == [1] * 40  # never sent value 1
    assert res.stats[0]["messages"] == k                # node 0 alone holds something and has a row
    sim = tr.TopoSim(n, 2, "push", k, 3, topo, stall_rounds=1, edge_loss=0xFFFFFFFF)
    sim.inject(0, 0)
    sim.step(2)
    assert int(sim.streak[z]) == 0 and int(sim.streak.sum()) == n - 1  # z has no exchange to lose
    sim = tr.TopoSim(n, 2, "pull", k, 3, topo)
    sim.inject(0, 0)
    sim.inject(z, 1)
    res = sim.step(12)
    assert int(sim.read_shard()[0][z]) == 2             # pulled nothing
    assert all(st["messages"] == k * (n - 1) for st in res.stats)
    assert int(res.infected[-1][1]) == n                # everybody else pulled value 1 from z


def test_stalled_nodes_send_no_messages():
    """Everything lost and D = 1: after round 0 every node with a row is stalled for good."""
    n, k = 64, 3
    sim = tr.TopoSim(n, 1, "pushpull", k, 1, ring(n), edge_loss=0xFFFFFFFF, stall_rounds=1)
    sim.inject(0, 0)
    res = sim.step(3)
    assert [st["messages"] for st in res.stats] == [k * n, 0, 0]
    assert [int(x[0]) for x in res.infected] == [1, 1, 1]


# --- the library's host probe and the flag (both new with GOSSIP_FLAG_TOPO_PEERS) -----------

def test_host_probe_matches_the_reference_index():
    from gossip_hip import topo_peer_index
    nodes = np.array([0, 1, 77, 30010, 2**21 + 5, 2**32 - 2], dtype=np.uint64)
    for seed in (0, 0x5EED0003, 0xFEDCBA9876543210):
        for degree in (1, 2, 3, 300, 2**32 - 1):
            for t in (0, 1, 23):
                for j in range(9):
                    want = tr.row_index(seed, np.full(nodes.size, degree, dtype=np.uint64), nodes, t, j)
                    got = [topo_peer_index(seed, degree, int(n), t, j) for n in nodes]
                    assert got == [int(x) for x in want], (seed, degree, t, j)
                    assert all(0 <= g < degree for g in got)
        assert topo_peer_index(seed, 0, 5, 1, 2) == 0
    # degree 2^32 - 1 is the draw itself but for its top value; degree 1 is always entry 0
    assert {topo_peer_index(7, 1, n, 3, j) for n in range(50) for j in range(9)} == {0}


def test_header_declares_the_flag():
    import gossip_hip
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    m = re.search(r"\bGOSSIP_FLAG_TOPO_PEERS\s*=\s*1u\s*<<\s*(\d+)", hdr)
    assert m and 1 << int(m.group(1)) == 64
    assert gossip_hip.FLAG_TOPO_PEERS == 64
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u", hdr)
