"""CPU: the numpy restatement of mongering with connection limits and hunting
(tests/monger_conn_ref.py) tied to what is already pinned — without a limit, and
with a limit nothing can reach, it is the three unlimited restatements round for round — and to what
can be worked out on paper: invariants of every round, closed forms on a directed ring and on a hub,
and an instance of every guard the GPU tests rely on."""
import numpy as np
import pytest

import monger_conn_ref as mc
import monger_counter_ref as mcr
import monger_pull_ref as mp
import monger_pushpull_ref as mpp
import monger_ref as mr
import topologies as tp

ALWAYS = 2 ** 32 - 1
LOSS = mr.threshold(0.3)
FAULTS = {"clean": {}, "loss": dict(edge_loss=LOSS), "parts": dict(partitions=3)}
UNLIMITED = {"push": mcr.MongerCounterSim, "pull": mp.MongerPullSim, "pushpull": mpp.MongerPushPullSim}
ZERO = dict.fromkeys(mc.CONN_KEYS, 0)


def injects(N, R):
    return [((431 * i + 7) % N, i) for i in range(R)]


def ring(N, step=1):
    """Row n = {(n + step) % N}: in-degree 1."""
    return np.arange(N + 1, dtype=np.uint32), ((np.arange(N) + step) % N).astype(np.uint32)


def hub(N):
    """Every row = {0}."""
    return np.arange(N + 1, dtype=np.uint32), np.zeros(N, dtype=np.uint32)


def mid_topology(N):
    return tp.symmetrize(*tp.ragged(N, 7, hub_every=1024, hub_deg=40), N, every=2)


def pair(mode, N, R, k, seed, blind, limit=2, cool=0.5, **kw):
    """The unlimited restatement and the one under test, set up alike."""
    a = UNLIMITED[mode](N, R, k, seed, **kw)
    b = mc.MongerConnSim(mode, N, R, k, seed, **kw)
    for s in (a, b):
        s.set_monger(cool, blind)
        s.set_monger_limit(limit)
        for n, r in injects(N, R):
            s.inject(n, r)
    return a, b


def same_round(a, b):
    (sa, ia, _), (sb, ib, _) = a.round(), b.round()
    assert sa == sb and ia == ib
    assert np.array_equal(a.S, b.S) and np.array_equal(a.H, b.H) and np.array_equal(a.read_counts(), b.read_counts())


# --- identities (item 9) ----------------------------------------------------------------------------

@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("mode", mc.MODES)
def test_no_limit_is_the_unlimited_restatement(mode, k, R, faults, blind):
    a, b = pair(mode, 257, R, k, 0xC0DE + k, blind, **FAULTS[faults])
    for _ in range(10):
        same_round(a, b)
        assert b.connections() == ZERO


@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("mode", mc.MODES)
def test_a_limit_nothing_reaches_changes_nothing(mode, k, blind):
    """The directed ring has in-degree 1: at most k <= 8 = c edges reach a node, none is refused."""
    N, R = 257, 70
    a, b = pair(mode, N, R, k, 77, blind, topo_peers=True, topology=ring(N), edge_loss=LOSS)
    b.set_monger_connections(8, 3)
    for _ in range(10):
        same_round(a, b)
        c = b.connections()
        assert c["refused"] == 0 and c["hunts"] == 0 and c["accepted"] > 0 and c["attempts"] >= c["accepted"]


# --- invariants (asserted inside edges(): places per target, refusals only at full targets, the identities)

@pytest.mark.parametrize("c,h", [(1, 0), (1, 3), (2, 1), (3, 15)])
@pytest.mark.parametrize("topo_peers", [False, True])
@pytest.mark.parametrize("mode", mc.MODES)
def test_invariants_every_round(mode, topo_peers, c, h):
    N, R, k = 3001, 70, 5
    m = mc.MongerConnSim(mode, N, R, k, 5, topo_peers=topo_peers, topology=mid_topology(N), edge_loss=LOSS, partitions=2)
    m.set_monger(0.5, False)
    m.set_monger_limit(2)
    m.set_monger_connections(c, h)
    for n, r in injects(N, R):
        m.inject(n, r)
    for _ in range(8):
        init, peer, live, lost0, conn, g = m.edges()
        assert (np.bincount(peer[live], minlength=N) <= c).all()
        assert not (live & lost0).any() and not (live & ~init[None, :]).any()
        edges = k * int(init.sum())
        assert conn["attempts"] == edges + conn["hunts"]
        assert edges >= conn["accepted"] + conn["refused"] + g["lost"]     # (the rest: partitions at a hunt stage)
        assert edges == conn["accepted"] + conn["refused"] + g["lost"] + g["hunt_partition"]
        if h == 0:
            assert conn["hunts"] == 0 and g["hunt_accepted"] == 0
        st, _, _ = m.round()
        assert not (m.H & ~m.S).any()
        if mode == "push":
            assert st["messages"] == conn["attempts"]
        else:
            assert st["messages"] <= conn["accepted"]


# --- closed forms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["pull", "pushpull"])
def test_ring_two_edges_one_place_is_one_edge(mode):
    """k = 2, c = 1, h = 0 on the ring: both edges of n go to n + 1, which takes one; that is k = 1."""
    N, R = 257, 70
    a = UNLIMITED[mode](N, R, 1, 9, topo_peers=True, topology=ring(N))
    b = mc.MongerConnSim(mode, N, R, 2, 9, topo_peers=True, topology=ring(N))
    b.set_monger_connections(1, 0)
    for s in (a, b):
        s.set_monger(0.5, False)
        s.set_monger_limit(2)
        for n, r in injects(N, R):
            s.inject(n, r)
    for _ in range(12):
        (sa, ia, _), (sb, ib, g) = a.round(), b.round()
        assert sa == sb and ia == ib
        assert np.array_equal(a.S, b.S) and np.array_equal(a.H, b.H) and np.array_equal(a.C, b.C)
        assert b.connections() == dict(attempts=2 * N, accepted=N, refused=N, hunts=0) and g["split"] == N


def test_ring_push_two_edges_one_place():
    """Push under cool = 2^32 - 1 and feedback: the coin of either edge holds, so which of the two is
    accepted does not show in the state; twice the messages."""
    N, R = 257, 3
    a = mcr.MongerCounterSim(N, R, 1, 9, topo_peers=True, topology=ring(N))
    b = mc.MongerConnSim("push", N, R, 2, 9, topo_peers=True, topology=ring(N))
    b.set_monger_connections(1, 0)
    for s in (a, b):
        s.set_monger(ALWAYS, False)
        for n, r in injects(N, R):
            s.inject(n, r)
    for _ in range(12):
        (sa, ia, _), (sb, ib, _) = a.round(), b.round()
        assert dict(sa, messages=2 * sa["messages"]) == sb and ia == ib
        assert np.array_equal(a.S, b.S)


@pytest.mark.parametrize("c,h", [(1, 0), (3, 2), (8, 15)])
def test_hub_closed_form(c, h):
    """Every row = {0}, pull k = 1: N edges contend at node 0 in stage 0, the N - c refused ones in every
    hunt stage again (the hunt draws from the same row), and node 0 is full after stage 0."""
    N = 257
    m = mc.MongerConnSim("pull", N, 3, 1, 3, topo_peers=True, topology=hub(N))
    m.set_monger_connections(c, h)
    m.inject(0, 0)
    for _ in range(4):
        m.round()
        assert m.connections() == dict(attempts=N + (N - c) * h, accepted=c, refused=N - c, hunts=(N - c) * h)
    assert m.hot_nodes() <= 1 + 4 * c


def test_readout_follows_limit_and_reset():
    N = 257
    m = mc.MongerConnSim("pushpull", N, 3, 2, 3)
    m.inject(5, 1)
    assert m.connections() == ZERO
    m.set_monger_connections(1, 1)
    assert m.connections() == ZERO
    m.round()
    assert m.connections()["attempts"] >= 2 * N
    m.set_monger_connections(0, 0)
    assert m.connections() == ZERO
    m.round()
    m.set_monger_connections(2, 0)
    assert m.connections() == ZERO          # the last round ran without a limit
    m.round()
    assert m.connections()["attempts"] == 2 * N
    m.reset()
    assert m.connections() == ZERO and (m.c, m.h) == (2, 0)


# --- words -------------------------------------------------------------------------------------------

def test_conn_words_are_the_tag_six_stream():
    import numpy_ref as nr
    seed, n, t, s, j = 0xFEDCBA9876543210, 4097, 11, 15, 63
    pw, hw = mc.conn_words(seed, [n], t, s, j)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    assert int(pw[0]) == int(nr.philox4x32_10(n, t, 6 | (15 << 16), 15, k0, k1)[3])
    assert int(hw[0]) == int(nr.philox4x32_10(n, t, 6 | (15 << 16), 31, k0, k1)[3])
    assert int(pw[0]) != int(hw[0])


# --- every guard occurs --------------------------------------------------------------------------------

def guard_totals(mode, N, k, c, h, rounds=6, **kw):
    m = mc.MongerConnSim(mode, N, 3, k, 12, **kw)
    m.set_monger(0.5, False)
    m.set_monger_connections(c, h)
    for n, r in injects(N, 3):
        m.inject(n, r)
    tot = dict.fromkeys(mc.GUARDS, 0)
    for _ in range(rounds):
        _, _, g = m.round()
        for key in tot:
            tot[key] += g[key]
    return tot


def test_guard_instances():
    N = 3001
    a = guard_totals("pull", N, 5, 2, 2, topo_peers=True, topology=mid_topology(N), partitions=3, edge_loss=LOSS)
    for key in ("refusals", "hunt_accepted", "refused_last", "two_stage", "hunt_partition", "split", "lost"):
        assert a[key] > 0, (key, a)
    b = guard_totals("pushpull", N, 2, 2, 1)   # (a target's places fill over two stages only where it has two)
    for key in ("refusals", "hunt_accepted", "refused_last", "two_stage", "cooled"):
        assert b[key] > 0, (key, b)
