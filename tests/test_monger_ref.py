"""CPU: the numpy restatement of rumor mongering (tests/monger_ref.py) tied to what
is already pinned — with cool = 0 it is the C oracle's PUSH (uniform peers) and tests/topo_ref.py's
PUSH (row peers), bit for bit — and to what can be worked out on paper: invariants of every round,
closed forms on a directed ring, and the two variants under total loss."""
import numpy as np
import pytest

import monger_ref as mr
import numpy_ref as nr
import oracle_py as op
import topo_ref as tr
import topologies as tp

ALWAYS = 2 ** 32 - 1   # a coin or a loss draw below this: every word but 0xFFFFFFFF
LOSS = mr.threshold(0.3)
FAULTS = {"clean": {}, "loss": dict(edge_loss=LOSS), "parts": dict(partitions=3),
          "loss-parts": dict(edge_loss=LOSS, partitions=3)}


def injects(N, R):
    return [((431 * i + 7) % N, i) for i in range(R)]


# --- identity: cool = 0 is plain PUSH --------------------------------------------------------------

@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_cool_zero_is_the_oracles_push(k, R, faults):
    N, seed, rounds = 257, 0xC001 + k, 14
    o = op.OracleEngine(N, R, "push", k, seed, flags=1, **FAULTS[faults])
    m = mr.MongerSim(N, R, k, seed, **FAULTS[faults])
    for n, r in injects(N, R):
        o.inject(n, r)
        m.inject(n, r)
    for _ in range(rounds):   # (the oracle's step would stop at converged: one round at a time)
        want = o.step(1)
        holders = int((m.S != 0).any(axis=0).sum())
        st, inf, _ = m.round()
        assert np.array_equal(m.H, m.S)
        assert st["messages"] == k * holders
        assert dict(st, messages=0) == want.stats[0]
        assert [int(x) for x in want.infected[0]] == inf
        assert np.array_equal(o.read_shard(), m.S)
    o.close()


def ring(N):
    """row_n = {n + 1 mod N}."""
    return np.arange(N + 1, dtype=np.uint32), ((np.arange(N, dtype=np.int64) + 1) % N).astype(np.uint32)


@pytest.mark.parametrize("faults", ["clean", "loss-parts"])
@pytest.mark.parametrize("k,R", [(1, 3), (2, 70), (5, 3)])
def test_cool_zero_is_toposims_push(k, R, faults):
    """Row peers on a ragged topology: messages included."""
    N, seed = 3001, 21
    topo = tp.symmetrize(*tp.ragged(N, 7, hub_every=1024, hub_deg=40), N, every=2)
    t = tr.TopoSim(N, R, "push", k, seed, topology=topo, **FAULTS[faults])
    m = mr.MongerSim(N, R, k, seed, topo_peers=True, topology=topo, **FAULTS[faults])
    for n, r in injects(N, R):
        t.inject(n, r)
        m.inject(n, r)
    for _ in range(12):
        (a, ia), (b, ib, _) = t.round(), m.round()
        assert a == b and ia == ib and a["messages"] > 0
        assert np.array_equal(t.S, m.S) and np.array_equal(m.H, m.S)


# --- invariants ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("topo_peers", [False, True])
def test_invariants_every_round(topo_peers, blind):
    N, R, k = 3001, 70, 2
    m = mr.MongerSim(N, R, k, 5, topo_peers=topo_peers, topology=tp.ragged(N, 7, hub_every=1024, hub_deg=40),
                     edge_loss=LOSS)
    m.set_monger(0.5, blind)
    for n, r in injects(N, R):
        m.inject(n, r)
    quiet = False
    for _ in range(200):
        S0, H0 = m.S.copy(), m.H.copy()
        st, _, g = m.round()
        assert not (m.H & ~m.S).any()          # H ⊆ S
        assert not (S0 & ~m.S).any()           # S is monotone
        if quiet:                              # a quiescent state stays quiescent
            assert st["messages"] == 0 and np.array_equal(S0, m.S) and np.array_equal(H0, m.H)
            # what is still hot sits at nodes that cannot push: those with an empty row
            assert not m.H[:, m.deg > 0].any() if topo_peers else not m.H.any()
            break
        quiet = st["messages"] == 0
    assert quiet and st["full_nodes"] < N
    # a held, cooled rumor is not re-heated; a new one restarts the run
    held = int(np.nonzero(m.S[0] & np.uint64(1))[0][0])
    S0, H0 = m.S.copy(), m.H.copy()
    m.inject(held, 0)
    assert np.array_equal(S0, m.S) and np.array_equal(H0, m.H)
    assert m.step(5).rounds == 1
    lacks = int(np.nonzero(~m.S[0] & np.uint64(1))[0][0])
    if topo_peers:   # (a node that has a row, so that it can push)
        lacks = int(np.nonzero((~m.S[0] & np.uint64(1) != 0) & (m.deg > 0))[0][0])
    m.inject(lacks, 0)
    again = m.step(200)
    assert again.stats[0]["messages"] == k and again.rounds > 1 and again.stats[-1]["messages"] == 0


def test_reset_keeps_the_parameters():
    m = mr.MongerSim(101, 3, 2, 1)
    m.set_monger(0.25, True)
    m.inject(5, 1)
    m.step(3)
    m.reset()
    assert not m.S.any() and not m.H.any() and m.t == 0 and (m.cool, m.blind) == (1 << 30, True)


# --- closed forms on a directed ring ------------------------------------------------------------------

RING_N, RING_SEED = 97, 3


def ring_sim(blind, **faults):
    m = mr.MongerSim(RING_N, 1, 1, RING_SEED, topo_peers=True, topology=ring(RING_N), **faults)
    m.set_monger(ALWAYS, blind)
    m.inject(0, 0)
    return m


def test_ring_seed_makes_every_coin_hold():
    n = np.arange(RING_N)
    for t in range(RING_N + 2):
        assert (mr.coin_word(RING_SEED, n, t, 0) < np.uint32(ALWAYS)).all()


def test_ring_blind():
    """Every attempt cools: node t alone is hot in round t, pushes to t + 1 and goes quiet.  Everyone
    is full after N - 1 rounds; in round N - 1 the last node pushes to the origin (one message, nothing
    new) and cools; round N is the first that sends nothing."""
    m = ring_sim(True)
    for t in range(RING_N):
        assert list(np.nonzero(m.H[0])[0]) == [t]
        st, _, _ = m.round()
        assert st["messages"] == 1
        assert st["full_nodes"] == min(t + 2, RING_N) and st["converged"] == int(t >= RING_N - 2)
    assert not m.H.any()
    r = ring_sim(True).step(10 * RING_N)
    assert r.rounds == RING_N + 1 and [s["messages"] for s in r.stats] == [1] * RING_N + [0]
    assert [s["converged"] for s in r.stats].index(1) == RING_N - 2


def test_ring_feedback():
    """Node n's first push (round n) finds n + 1 without the rumor: delivered, nothing counted.  Its
    second (round n + 1) finds it there: counted, cooled.  So every node is hot for exactly two rounds —
    but the last one, whose first push already finds the origin holding the rumor: one round.  Round
    N - 1 has the last two nodes hot and cools both; round N is the first that sends nothing."""
    m = ring_sim(False)
    hot_rounds = np.zeros(RING_N, dtype=np.int64)
    msgs = []
    for t in range(RING_N + 1):
        hot_rounds += m.H[0] != 0
        msgs.append(m.round()[0]["messages"])
    assert list(hot_rounds) == [2] * (RING_N - 1) + [1]
    assert msgs == [1] + [2] * (RING_N - 1) + [0]
    r = ring_sim(False).step(10 * RING_N)
    assert r.rounds == RING_N + 1 and r.stats[-1]["messages"] == 0 and r.stats[-2]["messages"] == 2


# --- total loss -------------------------------------------------------------------------------------------

def test_blind_under_total_loss_cools_without_delivering():
    N, k = 257, 2
    m = mr.MongerSim(N, 1, k, 11, edge_loss=ALWAYS)
    for t in range(40):
        assert (nr.loss_draw(11, [9], t, 0) < np.uint32(ALWAYS)).all() and (nr.loss_draw(11, [9], t, 1) < np.uint32(ALWAYS)).all()
    m.set_monger(0.5, True)
    m.inject(9, 0)
    r = m.step(40)
    assert r.stats[-1]["messages"] == 0 and r.rounds < 40
    assert all(s["messages"] == k for s in r.stats[:-1])
    assert int(r.infected[-1][0]) == 1            # the residue is N - 1
    assert sum(g["lost"] for g in r.guards) == k * (r.rounds - 1) and sum(g["cooled"] for g in r.guards) == 1


def test_feedback_under_total_loss_never_cools():
    N, k = 257, 2
    m = mr.MongerSim(N, 1, k, 11, edge_loss=ALWAYS)
    m.set_monger(ALWAYS, False)
    m.inject(9, 0)
    r = m.step(40)
    assert r.rounds == 40 and all(s["messages"] == k for s in r.stats)
    assert int(r.infected[-1][0]) == 1 and m.H[0, 9] == 1
