"""CPU: the numpy restatement of push-pull rumor mongering (tests/monger_pushpull_ref.py, DESIGN.md
§2.16) tied to what is already pinned — with cool = 0 it is the C oracle's PUSHPULL (uniform peers)
and tests/topo_ref.py's PUSHPULL (row peers), bit for bit — and to what can be worked out on paper:
invariants of every round, closed forms on a directed ring, total loss, and the orderings of the
counter table (no table value is a gate).  It is neither the pull nor the push restatement: on one
seed it parts from both in the first round."""
import functools

import numpy as np
import pytest

import monger_counter_ref as mc
import monger_pull_ref as mp
import monger_pushpull_ref as mpp
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


def mid_topology(N):
    return tp.symmetrize(*tp.ragged(N, 7, hub_every=1024, hub_deg=40), N, every=2)


# --- identity (item 9): cool = 0 is plain PUSHPULL ---------------------------------------------------

@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_cool_zero_is_the_oracles_pushpull(k, R, faults):
    N, seed, rounds = 257, 0xC001 + k, 10
    o = op.OracleEngine(N, R, "pushpull", k, seed, flags=1, **FAULTS[faults])
    m = mpp.MongerPushPullSim(N, R, k, seed, **FAULTS[faults])
    for n, r in injects(N, R):
        o.inject(n, r)
        m.inject(n, r)
    for _ in range(rounds):   # (the oracle's step would stop at converged: one round at a time)
        want = o.step(1)
        st, inf, g = m.round()
        assert np.array_equal(m.H, m.S) and g["cooled"] == 0
        assert dict(st, messages=0) == want.stats[0]
        assert [int(x) for x in want.infected[0]] == inf
        assert np.array_equal(o.read_shard(), m.S)
    o.close()
    assert mpp.MongerPushPullSim(N, R, k, seed).step(3).rounds == 1   # nothing injected: nothing hot
    m.reset()
    m.inject(0, 0)
    assert m.step(40).rounds == 40                                    # H == S for ever: to max_rounds


@pytest.mark.parametrize("faults", ["clean", "loss-parts"])
@pytest.mark.parametrize("k,R", [(1, 3), (2, 70), (5, 3)])
def test_cool_zero_is_toposims_pushpull(k, R, faults):
    """Row peers on a ragged topology; the messages differ by design (TopoSim counts attempts)."""
    N, seed = 3001, 21
    topo = mid_topology(N)
    t = tr.TopoSim(N, R, "pushpull", k, seed, topology=topo, **FAULTS[faults])
    m = mpp.MongerPushPullSim(N, R, k, seed, topo_peers=True, topology=topo, **FAULTS[faults])
    for n, r in injects(N, R):
        t.inject(n, r)
        m.inject(n, r)
    sent = 0
    for _ in range(10):
        (a, ia), (b, ib, _) = t.round(), m.round()
        assert dict(a, messages=0) == dict(b, messages=0) and ia == ib
        assert b["messages"] <= a["messages"]
        sent += b["messages"]
        assert np.array_equal(t.S, m.S) and np.array_equal(m.H, m.S)
    assert sent > 0


# --- invariants ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("limit", [1, 3])
@pytest.mark.parametrize("blind", [False, True])
@pytest.mark.parametrize("topo_peers", [False, True])
def test_invariants_every_round(topo_peers, blind, limit):
    N, R, k = 3001, 70, 2
    m = mpp.MongerPushPullSim(N, R, k, 5, topo_peers=topo_peers, topology=mid_topology(N), edge_loss=LOSS)
    m.set_monger(0.5, blind)
    m.set_monger_limit(2)      # the counts are kept from the start, also with limit 1
    m.set_monger_limit(limit)
    for n, r in injects(N, R):
        m.inject(n, r)
    resets = 0
    for _ in range(300):
        S0, H0, C0 = m.S.copy(), m.H.copy(), m.C.copy()
        st, _, g = m.round()           # (need, less ⊆ H_t is asserted inside every round)
        resets += g["reset"]
        hot, known = mpp.unpack(m.H, R), mpp.unpack(m.S, R)
        assert not (hot & ~known).any()              # H ⊆ S
        assert not (S0 & ~m.S).any()                 # S is monotone
        assert (m.C[hot] < limit).all()              # hot: below the limit
        assert (m.C[known & ~hot] >= limit).all()    # cooled: at the limit (never re-heated, never reset)
        assert not m.C[~known].any()
        went = mpp.unpack(H0 & ~m.H, R)              # a rumor cools by a step of exactly one
        assert (m.C[went] == C0[went] + 1).all() and g["cooled"] == int(went.sum())
        step = m.C.astype(np.int64) - C0
        assert ((step == 1) | (step <= 0)).all() and (m.C[step < 0] == 0).all()
        if not m.H.any():
            break
    if topo_peers:   # what is still hot sits at nodes that take part in no exchange: no row, listed by nobody
        listed = np.zeros(N, dtype=bool)
        listed[m.col] = True
        alone = ~listed & (m.deg == 0)
        assert not m.H[:, ~alone].any()
    else:
        assert not m.H.any()
    assert blind or limit == 1 or resets > 0         # counts are not monotone: a needed rumor resets them
    if topo_peers:
        return
    # a held, cooled rumor is not re-heated; a new one restarts the run
    held = int(np.nonzero(m.S[0] & np.uint64(1))[0][0])
    S0, H0 = m.S.copy(), m.H.copy()
    m.inject(held, 0)
    assert np.array_equal(S0, m.S) and np.array_equal(H0, m.H)
    assert m.step(5).rounds == 1
    m.reset()
    m.inject(17, 0)
    assert m.hot_nodes() == 1 and m.step(300).rounds > 1 and not m.H.any()


def test_reset_keeps_the_parameters():
    m = mpp.MongerPushPullSim(101, 3, 2, 1)
    m.set_monger(0.25, True)
    m.set_monger_limit(3)
    m.inject(5, 1)
    m.step(3)
    assert m.C.any() or m.S.any()
    m.reset()
    assert not m.S.any() and not m.H.any() and not m.C.any() and m.t == 0
    assert (m.cool, m.blind, m.limit, m.tracking) == (1 << 30, True, 3, True)


# --- closed forms on a directed ring ------------------------------------------------------------------

RING_N, RING_SEED = 257, 3


def ring(N):
    """row_n = {n + 1 mod N}."""
    return np.arange(N + 1, dtype=np.uint32), ((np.arange(N, dtype=np.int64) + 1) % N).astype(np.uint32)


def ring_sim(blind, limit, N=RING_N, **faults):
    m = mpp.MongerPushPullSim(N, 1, 1, RING_SEED, topo_peers=True, topology=ring(N), **faults)
    m.set_monger(ALWAYS, blind)
    m.set_monger_limit(limit)
    m.inject(0, 0)
    return m


def test_ring_seed_makes_every_coin_hold():
    n = np.arange(RING_N)
    for t in range(RING_N // 2 + 20):
        assert (mr.coin_word(RING_SEED, n, t, 0) < np.uint32(ALWAYS)).all()


@pytest.mark.parametrize("N", [RING_N, 5])
@pytest.mark.parametrize("limit", [1, 2, 3, 15])
@pytest.mark.parametrize("blind", [False, True])
def test_ring(blind, limit, N):
    """Node x exchanges with x + 1 as initiator and with x - 1 as target: the rumor moves one hop in both
    directions per round, half the N - 1 + m rounds of the pull ring.  DESIGN.md §2.16 derives the
    values: (N - 1) / 2 + m rounds in both variants; (N - 1)(m + 2) + m - 2 messages with feedback,
    (N - 1)(m + 1) + m blind; everybody full."""
    half = (N - 1) // 2
    r = ring_sim(blind, limit, N).step(10 * N)
    msgs = sum(s["messages"] for s in r.stats)
    assert msgs == ((N - 1) * (limit + 1) + limit if blind else (N - 1) * (limit + 2) + limit - 2)
    assert r.rounds == half + limit and r.stats[-1]["full_nodes"] == N
    assert [s["converged"] for s in r.stats].index(1) == half - 1        # it runs on past converged
    m = ring_sim(blind, limit, N)
    for t in range(half):
        assert m.S[0, (t + 1) % N] == 0 and m.S[0, (N - t - 1) % N] == 0
        st, _, g = m.round()
        assert st["full_nodes"] == 2 * t + 3 and g["mutual"] == 0
        assert m.H[0, (t + 1) % N] == 1 and m.H[0, (N - t - 1) % N] == 1   # the newest holders are hot


@pytest.mark.parametrize("blind", [False, True])
def test_total_loss_cools_nothing(blind):
    """A lost exchange moves nothing and tells neither end anything, in both variants."""
    for t in range(40):
        assert (nr.loss_draw(RING_SEED, np.arange(RING_N), t, 0) < np.uint32(ALWAYS)).all()
    m = ring_sim(blind, 1, edge_loss=ALWAYS)
    r = m.step(40)
    assert r.rounds == 40 and all(s["messages"] == 0 for s in r.stats)
    assert int(r.infected[-1][0]) == 1 and m.H[0, 0] == 1 and m.hot_nodes() == 1     # the residue is N - 1
    assert sum(g["lost"] for g in r.guards) == 40 * RING_N and all(g["quiet"] for g in r.guards)


# --- the limit ---------------------------------------------------------------------------------------------

def run(N, R, k, seed, cool, blind, limits, rounds=300, **faults):
    m = mpp.MongerPushPullSim(N, R, k, seed, **faults)
    m.set_monger(cool, blind)
    for x in limits:
        m.set_monger_limit(x)
    for n, r in injects(N, R):
        m.inject(n, r)
    return m, m.step(rounds)


@pytest.mark.parametrize("blind", [False, True])
def test_limit_two_then_one_is_the_coin_alone(blind):
    """With the counts kept and limit 1 every counted rumor cools at once, as if no limit was ever set;
    every cooled rumor then reads a count of exactly 1."""
    a, ra = run(3001, 70, 2, 9, 0.5, blind, [])
    b, rb = run(3001, 70, 2, 9, 0.5, blind, [2, 1])
    assert ra.stats == rb.stats and np.array_equal(a.S, b.S) and np.array_equal(a.H, b.H)
    assert not a.C.any() and np.array_equal(b.C == 1, mpp.unpack(b.S & ~b.H, 70)) and int(b.C.max()) == 1


def test_a_lowered_limit_cools_at_the_next_counted_round():
    m = mpp.MongerPushPullSim(3001, 3, 2, 4)
    m.set_monger(ALWAYS, True)
    m.set_monger_limit(15)
    for n, r in injects(3001, 3):
        m.inject(n, r)
    m.step(9)
    hot = mpp.unpack(m.H, 3)
    high = hot & (m.C >= 2)
    assert high.sum() > 100
    m.set_monger_limit(2)
    H0, C0 = m.H.copy(), m.C.copy()
    _, _, g = m.round()
    still = mpp.unpack(m.H, 3) & high
    assert g["cooled"] > 0 and mpp.unpack(H0, 3)[high].all()
    assert (m.C[still] == C0[still]).all()          # not counted this round: still hot past the limit
    assert (m.C[high & ~still] == C0[high & ~still] + 1).all()


# --- neither pull nor push -----------------------------------------------------------------------------

def test_it_is_neither_the_pull_nor_the_push_restatement():
    N, R, k, seed = 3001, 3, 2, 9
    sims = [mpp.MongerPushPullSim(N, R, k, seed), mp.MongerPullSim(N, R, k, seed), mc.MongerCounterSim(N, R, k, seed)]
    out = []
    for m in sims:
        m.set_monger(0.5, False)
        m.set_monger_limit(2)
        for n, r in injects(N, R):
            m.inject(n, r)
        st = m.round()[0]
        out.append((st["full_nodes"], st["state_hash"], st["messages"]))
    (pp, pl, ps) = out
    assert pp[1] != pl[1] and pp[1] != ps[1]
    # what either one-way round learns the symmetric round learns too
    assert not (sims[1].S & ~sims[0].S).any() and not (sims[2].S & ~sims[0].S).any()


def test_residue_falls_and_traffic_rises_with_the_limit():
    """Push-pull, feedback, counter m.  Orderings only."""
    N = 1 << 14
    res, traffic = [], []
    for limit in (1, 2, 3):
        m = mpp.MongerPushPullSim(N, 1, 1, 0x5EED0003)
        m.set_monger(ALWAYS, False)
        m.set_monger_limit(limit)
        m.inject(0, 0)
        r = m.step(400)
        assert not m.H.any()
        res.append(N - int(r.infected[-1][0]))
        traffic.append(sum(s["messages"] for s in r.stats) / N)
    assert res[0] >= res[1] >= res[2] and res[0] > res[2] and traffic[0] < traffic[1] < traffic[2]


# --- the guards of the GPU cases -----------------------------------------------------------------------

N_G = 30011


@functools.lru_cache(maxsize=None)
def ragged():
    return tp.ragged(N_G, 7)


@pytest.mark.parametrize("blind", [False, True], ids=["feedback", "blind"])
@pytest.mark.parametrize("rows", [False, True], ids=["uniform", "rows"])
@pytest.mark.parametrize("R", [3, 130])
def test_guards_are_not_vacuous(R, rows, blind):
    """From the restatement alone, once per instantiation of the request kernel (one word / several x
    uniform / rows x feedback / blind): within the rounds a GPU case compares, the run cools bits,
    keeps counted bits hot, gains and loses hot bits in one word of one node, loses exchanges, sees a
    mutual gain and sees feedback reach nodes in each role alone; with feedback it also resets counts
    and has a rumor both needed and needless at one node in one round."""
    m = mpp.MongerPushPullSim(N_G, R, 2, 77, topo_peers=rows, topology=ragged() if rows else None, edge_loss=LOSS)
    m.set_monger(0.5, blind)
    m.set_monger_limit(2)
    for i in range(R):
        m.inject((431 * i) % N_G, i)
    res = m.step(12)
    tot = {name: sum(g[name] for g in res.guards) for name in mpp.GUARDS}
    for name in ("cooled", "kept", "gain_lose", "lost", "mutual", "init_only", "target_only") + \
            (() if blind else ("reset", "both")):
        assert tot[name] > 0, name
