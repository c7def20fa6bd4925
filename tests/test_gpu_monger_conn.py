"""GPU: mongering with connection limits and hunting (gossip_set_monger_connections)
against the numpy restatement tests/monger_conn_ref.py, bit for bit, one round per step: per round
full_nodes, messages, converged, the per-rumor counts, the state hash and connections(); at the end the
known and the hot bitsets, the count of every node and rumor, the number of hot nodes and the round
index.  tests/test_monger_conn_ref.py ties that restatement to the three unlimited ones, to invariants
and to closed forms.

The shapes: below a wave, a wave and a block (sizes.TINY) over sizes.tiny_topology, whose hub row and
ring put many edges on one target; many blocks with a ragged last wave (30011 nodes) with uniform
peers and over topologies.ragged (hub rows of 300 beside empty rows) for the three modes, feedback and
blind; the ends of the chain of minima (c = 1, 2, 3, 8) and of the stage field (h = 0, 1, 3, 15); every
fanout class (k = 1, 2, 5, 9); one and three words per node; loss and partitions on every instantiation;
and more nodes than one launch has lanes (2^21 + 4099).  test_guards_are_not_vacuous shows from the
restatement alone that the compared rounds refuse, hunt, accept at a later stage and refuse for good."""
import functools

import numpy as np
import pytest

import monger_conn_ref as mc
import sizes as sz
import topologies as tp
from gossip_hip import (FLAG_HASH, FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER_PUSHPULL, FLAG_TOPO_PEERS, Engine,
                        loss_threshold)
from gossip_hip.engine import GossipError

pytestmark = pytest.mark.gpu
N = 30011
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 nodes: the last 4099 are a second trip
ALWAYS = 2 ** 32 - 1
LOSS = loss_threshold(0.3)
CAP = 8                   # compared rounds
FLAG = {"push": FLAG_MONGER, "pull": FLAG_MONGER_PULL, "pushpull": FLAG_MONGER_PUSHPULL}
FAULTY = (("edge_loss", LOSS), ("partitions", 3))
ZERO = dict.fromkeys(mc.CONN_KEYS, 0)
EINVAL, ESTATE = -1, -4


@functools.lru_cache(maxsize=None)
def ragged():
    return tp.ragged(N, 7)   # hub rows of 300, empty rows, self-loops, repeated entries


def ring(n):
    return np.arange(n + 1, dtype=np.uint32), ((np.arange(n) + 1) % n).astype(np.uint32)


def injects(n, R):
    return tuple([((431 * i) % n, i) for i in range(R)] + [(n - 1, R - 1), (1, 0)])


def make(kind, mode, n, R, k, seed, topology=None, faults=()):
    rows = topology is not None
    if kind == "gpu":
        x = Engine(n, R, mode, k, seed, flags=FLAG_HASH | FLAG[mode] | (FLAG_TOPO_PEERS if rows else 0), **dict(faults))
    else:
        x = mc.MongerConnSim(mode, n, R, k, seed, topo_peers=rows, **dict(faults))
    if rows:
        x.set_topology(topology)
    return x


def setup(x, inj, cool, blind, limit, c, h):
    x.set_monger(cool, blind)
    if limit is not None:
        x.set_monger_limit(limit)
    x.set_monger_connections(c, h)
    for n, r in inj:
        x.inject(n, r)


def end_state(x):
    return x.read_shard(), x.read_hot(), x.read_counts(), x.hot_nodes(), x.round_index


def compare_rounds(e, r, rounds):
    """One round per step on both; stops with the restatement's stop rule.  Returns the guards' totals."""
    tot = dict.fromkeys(mc.GUARDS, 0)
    for _ in range(rounds):
        want, got = r.step(1), e.step(1)
        assert got.rounds == 1 and got.stats[0] == want.stats[0]
        assert np.array_equal(got.infected, want.infected)
        assert e.connections() == want.conns[0]
        for key in tot:
            tot[key] += want.guards[0][key]
        stop = want.stats[0]["messages"] == 0 if r.mode == "push" else r.hot_nodes() == 0
        if stop:
            break
    return tot


def same_end(e, r):
    (sa, ha, ca, na, ta), (sb, hb, cb, nb, tb) = end_state(e), end_state(r)
    assert ta == tb and na == nb
    assert np.array_equal(sa, sb) and np.array_equal(ha, hb)
    assert ca.dtype == np.uint8 and np.array_equal(ca, cb)


def run_case(mode, n, R, k, seed, topology, faults, cool, blind, limit, c, h, rounds=CAP, inj=None):
    r = make("ref", mode, n, R, k, seed, topology, faults)
    setup(r, inj or injects(n, R), cool, blind, limit, c, h)
    with make("gpu", mode, n, R, k, seed, topology, faults) as e:
        setup(e, inj or injects(n, R), cool, blind, limit, c, h)
        tot = compare_rounds(e, r, rounds)
        same_end(e, r)
    return tot


# --- the matrix: every request kernel with a limit (mode x peers x words x faults, push also x coin /
# counter form), with c, h, k, the variant and the coin rotating against all of them --------------------
CS, HS, KS = (1, 2, 3, 8), (0, 1, 3, 15), (1, 2, 5, 9)
COOLS, LIMITS = (0.5, ALWAYS, 0.25), (None, 2, 3)
PEERS = ("uniform", "ragged")


def matrix():
    """(mode, peers, R, k, c, h, faulty, cool, blind, limit, seed).  Push runs its coin form (no limit
    ever set: the engine holds no counters) and its counter form of every instantiation; pull and
    push-pull have one request kernel per instantiation whatever the rule.  The index shifts keep c,
    h and k from moving with the words or the faults (test_matrix_covers_the_issue)."""
    out, i = [], 0
    for mode in mc.MODES:
        for peers in PEERS:
            for R in (3, 130):
                for faulty in (False, True):
                    for limit in ((None, 2 + i // 4 % 2) if mode == "push" else (LIMITS[(i + i // 3) % 3],)):
                        out.append((mode, peers, R, KS[(3 * i + i // 4) % 4], CS[(i // 2 + i // 8) % 4], HS[(i + i // 8) % 4],
                                    faulty, COOLS[i % 3], bool((i + i // 4 + i // 16) % 2), limit, 900 + i))
                        i += 1
    return out


MATRIX = matrix()


def test_matrix_covers_the_issue():
    """Every request kernel with a limit is launched: mode x peers x words x faults, and for push each
    of them in the coin form and in the counter form.  Every mode with feedback and blind over both
    kinds of peers; every mode with every c, h and k; every c and every k with one and three words,
    clean and faulty, and with at least three of the h."""
    forms = {(m, p, R, f, lim is not None if m == "push" else None) for m, p, R, _, _, _, f, _, _, lim, _ in MATRIX}
    assert forms == {(m, p, R, f, cnt) for m in mc.MODES for p in PEERS for R in (3, 130) for f in (False, True)
                     for cnt in ((False, True) if m == "push" else (None,))}
    assert len(MATRIX) == len(forms) == 32
    assert {(m, p, b) for m, p, _, _, _, _, _, _, b, _, _ in MATRIX} == {(m, p, b) for m in mc.MODES for p in PEERS
                                                                        for b in (False, True)}
    for mode in mc.MODES:
        rows = [x for x in MATRIX if x[0] == mode]
        assert {x[4] for x in rows} == set(CS) and {x[5] for x in rows} == set(HS) and {x[3] for x in rows} == set(KS)
    every = {(R, f) for R in (3, 130) for f in (False, True)}
    for c in CS:
        assert {(x[2], x[6]) for x in MATRIX if x[4] == c} == every
        assert len({x[5] for x in MATRIX if x[4] == c}) >= 3 and len({x[3] for x in MATRIX if x[4] == c}) >= 3
    for k in KS:
        assert {(x[2], x[6]) for x in MATRIX if x[3] == k} == every


def case_args(case):
    mode, peers, R, k, c, h, faulty, cool, blind, limit, seed = case
    return dict(mode=mode, n=N, R=R, k=k, seed=seed, topology=ragged() if peers == "ragged" else None,
                faults=FAULTY if faulty else (), cool=cool, blind=blind, limit=limit, c=c, h=h)


@functools.lru_cache(maxsize=None)
def ref_run(case):
    """The restatement's run of a matrix case, computed once per session: per compared round the
    stats, the per-rumor counts, connections() and the guards; then the end state."""
    a = case_args(case)
    r = make("ref", a["mode"], N, a["R"], a["k"], a["seed"], a["topology"], a["faults"])
    setup(r, injects(N, a["R"]), a["cool"], a["blind"], a["limit"], a["c"], a["h"])
    rounds = []
    for _ in range(CAP if a["h"] < 15 else CAP // 2):   # (sixteen stages a round: half the rounds)
        want = r.step(1)
        rounds.append((want.stats[0], want.infected, want.conns[0], want.guards[0]))
        if want.stats[0]["messages"] == 0 if r.mode == "push" else r.hot_nodes() == 0:
            break
    return rounds, end_state(r)


@pytest.mark.parametrize("case", MATRIX, ids=lambda c: "-".join(str(x) for x in c[:7] + c[9:10]))
def test_engine_matches_restatement(case):
    a = case_args(case)
    rounds, (sb, hb, cb, nb, tb) = ref_run(case)
    with make("gpu", a["mode"], N, a["R"], a["k"], a["seed"], a["topology"], a["faults"]) as e:
        setup(e, injects(N, a["R"]), a["cool"], a["blind"], a["limit"], a["c"], a["h"])
        for st, inf, conn, _ in rounds:
            got = e.step(1)
            assert got.rounds == 1 and got.stats[0] == st
            assert np.array_equal(got.infected, inf)
            assert e.connections() == conn
        sa, ha, ca, na, ta = end_state(e)
    assert ta == tb and na == nb
    assert np.array_equal(sa, sb) and np.array_equal(ha, hb)
    assert ca.dtype == np.uint8 and np.array_equal(ca, cb)


def test_guards_are_not_vacuous():
    """From the restatement's runs alone (the ones the engine is compared with, all of them): for
    every c, the ends of the chain of minima included, the compared rounds refuse edges, accept hunted
    ones and refuse for good; over the matrix they fill a target over two stages, close an edge by a
    partition at a hunt stage, split the edges of one initiator at one target, lose edges and cool."""
    tot = dict.fromkeys(mc.GUARDS, 0)
    per_c = {c: dict.fromkeys(mc.GUARDS, 0) for c in CS}
    for case in MATRIX:
        for _, _, _, g in ref_run(case)[0]:
            for key, v in g.items():
                tot[key] += v
                per_c[case[4]][key] += v
    for key in ("refusals", "hunt_accepted", "refused_last", "two_stage", "hunt_partition", "split", "lost", "cooled"):
        assert tot[key] > 0, (key, tot)
    for c in CS:
        for key in ("refusals", "hunt_accepted", "refused_last"):
            assert per_c[c][key] > 0, (c, key, per_c[c])
    for c in CS[1:]:   # (a target's places fill over two stages only where it has two)
        assert per_c[c]["two_stage"] > 0, (c, per_c[c])


# --- tiny sizes: partial waves, and a hub row with a ring around it ------------------------------------

@pytest.mark.parametrize("n", sz.TINY)
def test_tiny_sizes(n):
    i = sz.TINY.index(n)
    for a, mode in enumerate(mc.MODES):
        R = (3, 70)[(i + a) % 2]
        run_case(mode, n, R, KS[(i + a) % 4], 50 + i, sz.tiny_topology(n), FAULTY if (i + a) % 3 == 0 else (),
                 COOLS[(i + a) % 3], bool((i + a) % 2), LIMITS[a], CS[(i + a) % 4], HS[(i + 2 * a) % 4], rounds=8,
                 inj=sz.tiny_injects(n, R))


# --- more nodes than one launch has lanes ---------------------------------------------------------------

@pytest.mark.parametrize("mode", mc.MODES)
def test_past_one_launch(mode):
    inj = tuple((x, x % 3) for x in sz.boundary_nodes(NBIG)) + ((NBIG - 1, 0),)
    tot = run_case(mode, NBIG, 3, 2, 77, None, (), 0.5, False, None, 1, 1, rounds=2, inj=inj)
    if mode != "push":   # (push: only the few dozen hot nodes initiate, and 2^21 targets are never full)
        assert tot["refusals"] > 0 and tot["hunt_accepted"] > 0 and tot["refused_last"] > 0


# --- changes between steps ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", mc.MODES)
def test_changes_between_steps(mode):
    """c set, lowered, set to 0 and back; inject, reset and a new topology between steps."""
    R, k = 70, 5
    r = make("ref", mode, N, R, k, 31, ragged())
    with make("gpu", mode, N, R, k, 31, ragged()) as e:
        for x in (r, e):
            setup(x, injects(N, R), 0.5, False, 2, 3, 1)
        assert e.connections() == ZERO
        compare_rounds(e, r, 2)
        for c, h in ((1, 3), (0, 0), (8, 15), (2, 0)):
            for x in (r, e):
                x.set_monger_connections(c, h)
            assert e.connections() == r.connections()
            compare_rounds(e, r, 2)
            assert e.connections() == r.connections()
        for x in (r, e):
            x.inject(4098, 5)
            x.inject(N - 2, 69)
        compare_rounds(e, r, 2)
        other = tp.symmetrize(*tp.ragged(N, 11), N, every=2)
        for x in (r, e):
            x.set_topology(other)
        compare_rounds(e, r, 2)
        same_end(e, r)
        for x in (r, e):
            x.reset()
        assert e.connections() == ZERO
        for x in (r, e):
            for n, rr in injects(N, R)[:9]:
                x.inject(n, rr)
        compare_rounds(e, r, 3)
        same_end(e, r)


# --- the two equalities with the unlimited engine ---------------------------------------------------------

def unlimited_run(mode, topology, k, set_zero, rounds=8):
    R = 70
    with make("gpu", mode, N, R, k, 41, topology) as e:
        e.set_monger(0.5, False)
        e.set_monger_limit(2)
        if set_zero:
            e.set_monger_connections(2, 3)
            e.set_monger_connections(0, 0)
        for n, r in injects(N, R):
            e.inject(n, r)
        st = [e.step(1).stats[0] for _ in range(rounds)]
        return st, end_state(e)


@pytest.mark.parametrize("mode", mc.MODES)
def test_limit_zero_is_the_engine_that_never_set_one(mode):
    (sa, ea), (sb, eb) = unlimited_run(mode, ragged(), 5, False), unlimited_run(mode, ragged(), 5, True)
    assert sa == sb and ea[3:] == eb[3:]
    for x, y in zip(ea[:3], eb[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("mode", mc.MODES)
def test_round_that_refuses_nothing_is_the_unlimited_round(mode):
    """The directed ring has in-degree 1: with k = 8 <= c = 8 nothing is refused."""
    R, k = 70, 8
    sa, ea = unlimited_run(mode, ring(N), k, False)
    with make("gpu", mode, N, R, k, 41, ring(N)) as e:
        e.set_monger(0.5, False)
        e.set_monger_limit(2)
        e.set_monger_connections(8, 3)
        for n, r in injects(N, R):
            e.inject(n, r)
        sb = []
        for _ in range(8):
            sb.append(e.step(1).stats[0])
            c = e.connections()
            assert c["refused"] == 0 and c["hunts"] == 0 and c["accepted"] == c["attempts"] > 0
        eb = end_state(e)
    assert sa == sb and ea[3:] == eb[3:]
    for x, y in zip(ea[:3], eb[:3]):
        assert np.array_equal(x, y)


# --- refusals ---------------------------------------------------------------------------------------------------

def test_refusals():
    with Engine(1000, 3, "push", 2, 1) as e:
        for call in (lambda: e.set_monger_connections(1, 0), e.connections):
            with pytest.raises(GossipError) as ei:
                call()
            assert ei.value.code == ESTATE
    with make("gpu", "pull", 1000, 3, 2, 1) as e:
        for c, h in ((9, 0), (1, 16), (0, 1), (2 ** 32 - 1, 0)):
            with pytest.raises(GossipError) as ei:
                e.set_monger_connections(c, h)
            assert ei.value.code == EINVAL
        e.set_monger_connections(8, 15)
        e.set_monger_connections(0, 0)
        assert e.connections() == ZERO
