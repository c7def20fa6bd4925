"""CPU: the numpy restatement of rumor mongering with counters (tests/monger_counter_ref.py,
DESIGN.md §2.14) tied to what is already pinned — with limit = 1 it is tests/monger_ref.py's
MongerSim round for round — and to what can be worked out on paper: invariants of every round,
closed forms on a directed ring, the batched evaluation of item 7 and a limit lowered mid-run."""
import numpy as np
import pytest

import monger_counter_ref as mc
import monger_ref as mr
import topologies as tp

ALWAYS = 2 ** 32 - 1
LOSS = mr.threshold(0.3)
FAULTS = {"clean": {}, "loss": dict(edge_loss=LOSS), "parts": dict(partitions=3),
          "loss-parts": dict(edge_loss=LOSS, partitions=3)}


def injects(N, R):
    return [((431 * i + 7) % N, i) for i in range(R)]


def start(m, inj, cool, blind, limit=None):
    m.set_monger(cool, blind)
    if limit is not None:
        m.set_monger_limit(limit)
    for n, r in inj:
        m.inject(n, r)
    return m


# --- identity: limit = 1 is §2.13 -------------------------------------------------------------------------

@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_limit_one_is_mongersim(k, R, faults, blind):
    """Never set, and set to 2 and back to 1 (counts kept): both are MongerSim round for round."""
    N, seed = 257, 0xC001 + k
    want = start(mr.MongerSim(N, R, k, seed, **FAULTS[faults]), injects(N, R), 0.5, blind)
    never = start(mc.MongerCounterSim(N, R, k, seed, **FAULTS[faults]), injects(N, R), 0.5, blind)
    kept = start(mc.MongerCounterSim(N, R, k, seed, **FAULTS[faults]), injects(N, R), 0.5, blind, 2)
    kept.set_monger_limit(1)
    cooled = 0
    for _ in range(24):
        (a, ia, ga), (b, ib, gb), (c, ic, gc) = want.round(), never.round(), kept.round()
        assert a == b == c and ia == ib == ic
        assert ga["cooled"] == gb["cooled"] == gc["cooled"] and gb["kept"] == gc["kept"] == 0
        cooled += ga["cooled"]
        for m in (never, kept):
            assert np.array_equal(want.S, m.S) and np.array_equal(want.H, m.H)
    assert cooled > 0 and not never.C.any()
    # every cooled bit was counted at least once, nothing else was counted at all
    assert np.array_equal(kept.C > 0, mc.unpack(kept.S & ~kept.H, R))


# --- invariants ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("topo_peers", [False, True])
@pytest.mark.parametrize("limit", [2, 3])
def test_invariants_every_round(limit, topo_peers, blind):
    N, R, k = 3001, 70, 2
    m = mc.MongerCounterSim(N, R, k, 5, topo_peers=topo_peers, topology=tp.ragged(N, 7, hub_every=1024, hub_deg=40),
                            edge_loss=LOSS)
    start(m, injects(N, R), 0.5, blind, limit)
    tot = dict.fromkeys(mc.GUARDS, 0)
    for _ in range(300):
        S0, H0, C0 = m.S.copy(), m.H.copy(), m.C.copy()
        st, _, g = m.round()
        for name in mc.GUARDS:
            tot[name] += g[name]
        s, h, h0 = mc.unpack(m.S, R), mc.unpack(m.H, R), mc.unpack(H0, R)
        assert not (m.H & ~m.S).any() and not (S0 & ~m.S).any()   # H ⊆ S, S is monotone
        assert (m.C[h] < limit).all()                             # hot: not yet at the limit
        assert s[m.C > 0].all()                                   # counted: known
        assert (m.C >= C0).all() and (m.C[~h0] == C0[~h0]).all()  # counts grow, and only while hot
        assert (m.C[h0 & ~h] >= limit).all()                      # cooled in this round: at the limit
        assert not (h & ~h0 & (m.C > 0)).any()                    # hot since this round: count 0
        if st["messages"] == 0:
            break
    assert st["messages"] == 0 and st["full_nodes"] < N
    assert tot["cooled"] > 0 and tot["kept"] > 0 and tot["carry"] > 0 and tot["lost"] > 0
    # a held, cooled rumor is neither re-heated nor recounted
    held = int(np.nonzero(m.S[0] & ~m.H[0] & np.uint64(1))[0][0])
    S0, H0, C0 = m.S.copy(), m.H.copy(), m.C.copy()
    m.inject(held, 0)
    assert np.array_equal(S0, m.S) and np.array_equal(H0, m.H) and np.array_equal(C0, m.C) and C0[0, held] >= limit


def test_reset_keeps_the_limit_and_clears_the_counts():
    m = start(mc.MongerCounterSim(101, 3, 2, 1), [(5, 1)], ALWAYS, True, 3)
    m.step(2)
    assert m.C.any()
    m.reset()
    assert not m.S.any() and not m.H.any() and not m.C.any() and m.t == 0
    assert (m.cool, m.blind, m.limit, m.tracking) == (ALWAYS, True, 3, True)


# --- closed forms on a directed ring ------------------------------------------------------------------

RING_N, RING_SEED = 257, 3


def ring(N):
    """row_n = {n + 1 mod N}."""
    return np.arange(N + 1, dtype=np.uint32), ((np.arange(N, dtype=np.int64) + 1) % N).astype(np.uint32)


def ring_run(blind, m):
    sim = mc.MongerCounterSim(RING_N, 1, 1, RING_SEED, topo_peers=True, topology=ring(RING_N))
    start(sim, [(0, 0)], ALWAYS, blind, m)
    return sim, sim.step(10 * RING_N)


def test_ring_seed_makes_every_coin_hold():
    n = np.arange(RING_N)
    for t in range(RING_N + 16):
        assert (mr.coin_word(RING_SEED, n, t, 0) < np.uint32(ALWAYS)).all()


@pytest.mark.parametrize("m", [1, 2, 3, 15])
def test_ring_feedback(m):
    """Node n hears the rumor in round n - 1 and pushes from round n on.  Its first push finds n + 1
    without the rumor (nothing counted), each later one finds it there: m + 1 pushes, but the last
    node's first push already finds the origin informed, m pushes.  N (m + 1) - 1 messages; the last
    node's m-th push is round N - 1 + m - 1, so round N + m - 1 is the first that sends nothing."""
    sim, r = ring_run(False, m)
    assert r.rounds == RING_N + m and r.stats[-1]["messages"] == 0 and r.stats[-2]["messages"] > 0
    assert sum(s["messages"] for s in r.stats) == RING_N * (m + 1) - 1
    assert r.stats[-1]["full_nodes"] == RING_N and not sim.H.any()
    assert (sim.C == (m if m > 1 else 0)).all()   # (no count is kept before the first limit above 1)


@pytest.mark.parametrize("m", [1, 2, 3, 15])
def test_ring_blind(m):
    """Every attempt counts: each node pushes exactly m times, N m messages, the last node from round
    N - 1 to N + m - 2."""
    sim, r = ring_run(True, m)
    assert r.rounds == RING_N + m and r.stats[-1]["messages"] == 0 and r.stats[-2]["messages"] > 0
    assert sum(s["messages"] for s in r.stats) == RING_N * m
    assert r.stats[-1]["full_nodes"] == RING_N and not sim.H.any()
    assert (sim.C == (m if m > 1 else 0)).all()   # (no count is kept before the first limit above 1)


# --- item 7: cooling per batch of four edges is cooling per round --------------------------------------

@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("limit", [2, 3, 15])
def test_batched_evaluation_equals_the_whole_round(limit, blind):
    N, R, k = 1025, 70, 9
    whole = start(mc.MongerCounterSim(N, R, k, 31), injects(N, R), ALWAYS if blind else 0.5, blind, limit)
    batched = start(mc.MongerCounterSim(N, R, k, 31), injects(N, R), ALWAYS if blind else 0.5, blind, limit)
    tot = dict.fromkeys(mc.GUARDS, 0)
    for _ in range(40):
        (a, ia, ga), (b, ib, gb) = whole.round(), batched.round(batch=4)
        assert a == b and ia == ib and ga == gb
        assert np.array_equal(whole.S, batched.S) and np.array_equal(whole.H, batched.H)
        assert np.array_equal(whole.C, batched.C)
        for name in mc.GUARDS:
            tot[name] += ga[name]
        if a["messages"] == 0:
            break
    assert a["messages"] == 0 and tot["cooled"] > 0 and tot["carry"] > 0
    # blind, every coin holding: 9 counts per round, so a rumor cools in its first batch and is counted
    # on in the later ones (limits 2, 3), or passes 15 within its second round (limit 15)
    if blind:
        assert int(whole.C.max()) == (15 if limit == 15 else 9) and (tot["sat"] > 0) == (limit == 15)


# --- a lowered limit --------------------------------------------------------------------------------------

def test_lowered_limit_cools_at_the_next_counted_contact():
    m = start(mc.MongerCounterSim(257, 1, 1, 11), [(9, 0)], ALWAYS, True, 5)
    for t in range(2):
        assert (mr.coin_word(11, [9], t, 0) < np.uint32(ALWAYS)).all() and (mr.coin_word(11, [9], t + 3, 0) < np.uint32(ALWAYS)).all()
        m.round()
    assert m.C[0, 9] == 2 and m.H[0, 9] == 1
    m.set_monger_limit(2)              # the count is at the new limit already
    assert m.H[0, 9] == 1
    m.set_monger(0, True)              # no coin holds: contacts, none of them counted
    m.round()
    assert m.C[0, 9] == 2 and m.H[0, 9] == 1
    m.set_monger(ALWAYS, True)
    _, _, g = m.round()                # the next counted contact whose coin holds
    assert m.C[0, 9] == 3 and m.H[0, 9] == 0 and g["cooled"] >= 1
