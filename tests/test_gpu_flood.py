"""GPU: FLOOD (the reference's own algorithm, (*NodeState).Gossip, main.go:65-89) against the C
oracle, bit for bit, on ragged topologies (tests/topologies.py) at the sizes where its kernels
can go wrong: many blocks and full waves (30011 nodes), rows of 300 entries (loss-draw counter
words up to 74, long in-neighbour scans), more lanes than one launch has (2^21 + 4099 nodes,
2,100,770 walks: the second trip of the stride loops), two words per node, shards of uneven size
driven in lockstep and by the library, and state changes between steps.  Each run compares the
per-round stats (messages, full, hash, converged), the per-value counts and the final state.
tests/test_topologies.py holds the oracle itself to two independent restatements on the same rows."""
import functools
import os

import numpy as np
import pytest

import oracle_py as op
import topologies as tp
from gossip_hip import Engine, Group, loss_threshold
from gossip_hip.engine import GossipError
from gossip_hip.sharded import lockstep_run

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
N = 30011
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 nodes: the last 4099 are a second trip
NMID = 3001
INJ3 = [(0, 0), (N - 1, 1), (12345, 2)]


def injects(n, R):
    return [((431 * i) % n, i) for i in range(R)]


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":
        return tp.ragged(N, 7)
    if name == "ragged_sym":
        return tp.symmetrize(*tp.ragged(N, 7), N)
    if name == "ragged_half":   # odd nodes hear from nodes they do not send to, and from nodes they do
        return tp.symmetrize(*tp.ragged(N, 7), N, every=2)
    if name == "ragged_sym_sets":
        return tp.dedupe(*topo("ragged_sym"), N)
    if name == "banded_sym":
        return tp.symmetrize(*tp.banded(N, 7), N)
    if name == "big":
        return tp.symmetrize(*tp.ragged(NBIG, 11, max_deg=5, hub_every=65537, hub_deg=70), NBIG)
    if name == "mid_ragged":   # hubs at 1, 1025, 2049 with rows of 40 (+ their in-edges)
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID)
    if name == "mid_banded":
        return tp.symmetrize(*tp.banded(NMID, 7, hub_every=1024, hub_deg=40), NMID)
    if name == "mid_half":
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID, every=2)
    raise KeyError(name)


def nodes_of(name):
    return topo(name)[0].size - 1


_ORACLE = {}


def oracle(name, R, inj, rounds=256, seed=0, **faults):
    """(step result, final state) of the oracle on topo(name), computed once per session."""
    key = (name, R, tuple(inj), rounds, seed, tuple(sorted(faults.items())))
    if key not in _ORACLE:
        o = op.OracleEngine(nodes_of(name), R, "flood", 0, seed, flags=1, threads=THREADS, **faults)
        o.set_topology(topo(name))
        for n, r in inj:
            o.inject(n, r)
        _ORACLE[key] = (o.step(rounds), o.read_shard())
        o.close()
    return _ORACLE[key]


def total(res):
    return sum(s["messages"] for s in res.stats)


def gpu_run(name, R, inj, rounds=256, seed=0, **faults):
    e = Engine(nodes_of(name), R, "flood", 0, seed, flags=1, **faults)
    e.set_topology(topo(name))
    for n, r in inj:
        e.inject(n, r)
    res = e.step(rounds)
    shard = e.read_shard()
    e.close()
    return res, shard


def same(got, want):
    (a, sa), (b, sb) = got, want
    assert a.rounds == b.rounds
    assert a.stats == b.stats
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)


# --- plain FLOOD, one engine ------------------------------------------------------------------

# topology, values, rounds, total messages, nodes holding each value at the end
PLAIN = [("ragged", 3, 15, 362538, 29468), ("ragged_sym", 3, 9, 648153, 29956),
         ("ragged_sym", 70, 10, 15123570, 29956), ("banded_sym", 3, 12, 615105, 29951),
         # several values of one word reach a node in one round, from senders in its row and others:
         # the skip goes to each value's own first sender (any sender: 493,959 and 11,269,678 messages)
         ("ragged_half", 3, 11, 495122, 29890), ("ragged_half", 70, 12, 11386127, 29890)]


@pytest.mark.parametrize("name,R,rounds,msgs,reached", PLAIN, ids=[f"{c[0]}-R{c[1]}" for c in PLAIN])
def test_plain_flood(name, R, rounds, msgs, reached):
    inj = INJ3 if R == 3 else injects(N, R)
    want = oracle(name, R, inj)
    assert (want[0].rounds, total(want[0])) == (rounds, msgs)
    last = [int(x) for x in want[0].infected[-1]]
    if name == "ragged_half" and R == 70:   # 69 values; the one injected at a node with an empty row stays there
        assert sorted(last) == [1] + [reached] * 69
    else:
        assert last == [reached] * R
    same(gpu_run(name, R, inj), want)


def test_plain_flood_past_one_grid():
    """2^21 + 4099 nodes: the round, frontier, stats and hash kernels all take a second trip of
    their stride loops, and the nodes of that trip take part (3978 of them end with both values)."""
    inj = [(5, 0), (NBIG - 1, 1)]
    want = oracle("big", 2, inj)
    assert topo("big")[1].size == 8407880
    assert (want[0].rounds, total(want[0])) == (18, 12727422)
    assert [int(x) for x in want[0].infected[-1]] == [2040453] * 2
    got = gpu_run("big", 2, inj)
    same(got, want)
    assert int((got[1][0, -4099:] == 3).sum()) == 3978


def test_walk_kernel_without_losses_equals_plain_flood():
    """With nothing lost every walk finishes in its first round: plain FLOOD, on rows without
    repeated entries (the walks send to each entry, plain FLOOD reads rows as sets)."""
    want = oracle("ragged_sym", 3, INJ3)
    got = gpu_run("ragged_sym_sets", 3, INJ3, stall_rounds=1)
    same(got, want)
    same(got, oracle("ragged_sym_sets", 3, INJ3, stall_rounds=1))


# --- the walks of FLOOD with faults, one engine --------------------------------------------------

# deadline D, partitions, loss, total messages over 40 rounds
WALKS = [(1, 0, 0.1, 40810391), (0, 3, 0.2, 8566333), (3, 2, 0.3, 14688160), (2, 4, 0.0, 6381275)]


@pytest.mark.parametrize("D,parts,loss,msgs", WALKS, ids=[f"D{c[0]}-P{c[1]}-loss{c[2]}" for c in WALKS])
def test_walks_70_values(D, parts, loss, msgs):
    """70 x 30011 = 2,100,770 walks (a second trip of the walk kernels' stride loops), two words
    per node, hub rows of 300 entries and more (draw counter words up to 74)."""
    kw = dict(seed=5, edge_loss=loss_threshold(loss), partitions=parts, stall_rounds=D)
    want = oracle("banded_sym", 70, injects(N, 70), 40, **kw)
    assert (want[0].rounds, total(want[0])) == (40, msgs)
    if D == 1:
        assert want[0].stats[-1]["full_nodes"] == 27793
    same(gpu_run("banded_sym", 70, injects(N, 70), 40, **kw), want)


def test_walks_heavy_loss_200_rounds():
    """No deadline, half the messages lost: every reachable node is full long before round 200,
    while the hubs' walks are still going down their rows, one delivered entry at a time."""
    kw = dict(seed=5, edge_loss=loss_threshold(0.5))
    want = oracle("banded_sym", 5, injects(N, 5), 200, **kw)
    assert (want[0].rounds, total(want[0])) == (200, 2134946)
    assert want[0].stats[-1]["full_nodes"] == 29951 and want[0].stats[-1]["messages"] > 0
    same(gpu_run("banded_sym", 5, injects(N, 5), 200, **kw), want)


# --- sharded, all shards on one GPU ------------------------------------------------------------

@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("R", [3, 70])
def test_sharded_flood(R, G, driver):
    """Shards of 10004, 10004, 10003 nodes (G = 3) or 15006, 15005 (G = 2): the gathered frontier
    image is [G][W][Nl] with W = 2 at R = 70 and a short last shard."""
    inj = INJ3 if R == 3 else injects(N, R)
    want, full = oracle("ragged_sym", R, inj)
    if driver == "lockstep":
        shards = [Engine(N, R, "flood", 0, 0, flags=1, shard_rank=r, shard_count=G) for r in range(G)]
        for e in shards:
            e.set_topology(topo("ragged_sym"))
            for n, r in inj:
                e.inject(n, r)
        stats, _ = lockstep_run(shards, want.rounds)  # (it stops on convergence only)
        assert stats == want.stats
        owner = None
    else:
        owner = Group(N, R, "flood", 0, 0, flags=1, n_shards=G, devices=[0] * G)
        assert owner.transport == 2
        shards = owner.shards
        for e in shards:
            e.set_topology(topo("ragged_sym"))
        for n, r in inj:
            owner.inject(n, r)
        got = owner.step(256)
        assert got.rounds == want.rounds and got.stats == want.stats
        assert np.array_equal(got.infected, want.infected)
    assert [e.hi - e.lo for e in shards] == ([10004, 10004, 10003] if G == 3 else [15006, 15005])
    for e in shards:
        assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])
    for e in shards:
        e.close()
    if owner:
        owner.close()


def test_sharded_flood_rejects_faults():
    """FLOOD retries keep their walks on one shard."""
    for kw in (dict(edge_loss=1), dict(partitions=2), dict(stall_rounds=1)):
        with pytest.raises(GossipError) as ei:
            Engine(N, 3, "flood", 0, 0, shard_rank=1, shard_count=3, **kw)
        assert ei.value.code == -6  # GOSSIP_ENOTSUP
        with pytest.raises(GossipError):
            Group(N, 3, "flood", 0, 0, n_shards=3, devices=[0] * 3, **kw)


# --- state changes between steps ---------------------------------------------------------------

def both(script, R, seed=0, **faults):
    """Runs script(engine) -> list of step results on the GPU and on the oracle; everything equal."""
    runs = []
    for x in (Engine(NMID, R, "flood", 0, seed, flags=1, **faults),
              op.OracleEngine(NMID, R, "flood", 0, seed, flags=1, **faults)):
        steps = script(x)
        runs.append((steps, x.read_shard()))
        x.close()
    (a, sa), (b, sb) = runs
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra.rounds == rb.rounds and ra.stats == rb.stats
        assert np.array_equal(ra.infected, rb.infected)
    assert np.array_equal(sa, sb)
    return a


def start(x, name, inj):
    x.set_topology(topo(name))
    for n, r in inj:
        x.inject(n, r)


def test_plain_inject_between_steps():
    """A new value, and one its node already holds (no second forward, main.go:113)."""
    def script(x):
        start(x, "mid_half", [(0, 0), (NMID - 1, 1)])
        out = [x.step(3)]
        x.inject(1500, 2)
        x.inject(0, 0)
        out.append(x.step(3))
        x.inject(1025, 3)   # a hub
        x.inject(1500, 2)
        out.append(x.step(100))
        return out
    steps = both(script, 4)
    assert steps[-1].stats[-1]["messages"] == 0 and steps[-1].infected[-1].min() > 2900


def test_plain_new_topology_between_steps():
    """The values learned in the last round are forwarded over the new rows; their skip masks
    still name the first senders of the old ones."""
    def script(x):
        start(x, "mid_ragged", [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(3)]
        x.set_topology(topo("mid_banded"))
        out.append(x.step(100))
        return out
    steps = both(script, 3)
    assert steps[0].rounds == 3 and steps[1].stats[-1]["messages"] == 0


def test_plain_reset_and_rerun():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]

    def script(x):
        start(x, "mid_ragged", inj)
        out = [x.step(4)]       # stop mid-run: S_{t-1}, the skip masks and the frontier are live
        x.reset()
        for n, r in inj:
            x.inject(n, r)
        out.append(x.step(100))
        x.reset()
        for n, r in inj:
            x.inject(n, r)
        out.append(x.step(100))
        return out
    steps = both(script, 3)
    assert steps[1].stats == steps[2].stats and steps[1].stats[:4] == steps[0].stats
    assert np.array_equal(steps[1].infected, steps[2].infected)


def test_plain_single_steps_equal_one_step():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]
    whole = oracle("mid_ragged", 3, inj, 100)[0]

    def script(x):
        start(x, "mid_ragged", inj)
        return [x.step(1) for _ in range(whole.rounds + 2)]
    ones = both(script, 3)
    assert [s.stats[0] for s in ones[:whole.rounds]] == whole.stats
    assert np.array_equal(np.concatenate([s.infected for s in ones[:whole.rounds]]), whole.infected)
    assert all(s.rounds == 1 and s.stats[0]["messages"] == 0 for s in ones[whole.rounds:])


def test_plain_step_after_quiescence_then_inject():
    def script(x):
        start(x, "mid_ragged", [(0, 0), (NMID - 1, 1)])
        out = [x.step(100), x.step(3)]   # the second: nothing left to forward
        x.inject(2049, 2)
        out += [x.step(100), x.step(2)]
        return out
    steps = both(script, 3)
    assert steps[0].stats[-1]["messages"] == 0 and steps[0].rounds > 3
    assert steps[1].rounds == 1 and steps[1].stats[0]["messages"] == 0
    assert steps[2].rounds > 3 and steps[2].infected[-1][2] > 2900


WALK_FAULTS = dict(seed=5, edge_loss=loss_threshold(0.1), stall_rounds=1)


def test_walks_heal_partition():
    def script(x):
        start(x, "mid_banded", injects(NMID, 5))
        out = [x.step(15)]
        x.set_faults(loss_threshold(0.1), 0)
        out.append(x.step(300))
        return out
    steps = both(script, 5, seed=5, edge_loss=loss_threshold(0.1), partitions=3, stall_rounds=0)
    assert steps[0].rounds == 15 and steps[1].stats[-1]["messages"] == 0
    assert steps[1].stats[-1]["full_nodes"] > steps[0].stats[-1]["full_nodes"]


def test_walks_reset_and_rerun():
    def script(x):
        start(x, "mid_ragged", injects(NMID, 5))
        out = [x.step(6)]
        x.reset()
        for n, r in injects(NMID, 5):
            x.inject(n, r)
        out.append(x.step(12))
        return out
    steps = both(script, 5, **WALK_FAULTS)
    assert steps[1].stats[:6] == steps[0].stats


def test_walks_inject_at_a_node_with_a_stuck_walk():
    """D = 1 and three partition blocks: node u's walk of value 0 is stuck for good on its first
    neighbour across the cut.  A second value injected at u later starts a walk of its own, from
    the top of the row."""
    rp, col = topo("mid_banded")
    block = lambda n: n * 3 // NMID
    u = next(v for v in range(NMID) if block(v) == 0 and rp[v + 1] - rp[v] >= 6 and
             any(block(int(w)) != 0 for w in col[rp[v]:rp[v + 1] - 2]))

    def script(x):
        start(x, "mid_banded", [(u, 0), (NMID - 1, 1)])
        out = [x.step(8)]
        x.inject(u, 2)
        x.inject(u, 0)   # held: its walk goes on where it is
        out.append(x.step(30))
        return out
    steps = both(script, 3, partitions=3, **WALK_FAULTS)
    assert all(s["messages"] > 0 for s in steps[1].stats)   # stuck walks retry every round
    assert steps[1].infected[-1][2] > 1
