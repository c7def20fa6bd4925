"""GPU: random gossip over the topology (GOSSIP_FLAG_TOPO_PEERS) against the
numpy restatement tests/topo_ref.py, bit for bit: per round full_nodes, messages, converged, the
per-value counts and the state hash, and the whole state at the end.  tests/test_topo_ref.py ties
that restatement to the C oracle.  The sizes are those at which the kernel can go wrong: many
blocks and ragged last waves (30011 nodes), hub rows of 300 entries beside empty rows, self-loops
and repeated entries, every fanout class (the unrolled block of four, a second and a third Philox
block), one and three words per node with a ragged last word, more senders than one launch has
lanes (2^21 + 4099: a second trip of the stride loop), and shards of uneven size."""
import functools

import numpy as np
import pytest

import oracle_py as op
import topo_ref as tr
import topologies as tp
from gossip_hip import FLAG_HASH, FLAG_TOPO_PEERS, Engine, Group, loss_threshold, total_topology
from gossip_hip.engine import GossipError
from gossip_hip.sharded import DENSE, lockstep_run

pytestmark = pytest.mark.gpu
FLAGS = FLAG_HASH | FLAG_TOPO_PEERS
N = 30011
NMID = 3001
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 senders: the last 4099 are a second trip
NFULL = 1025
MODES = ("push", "pull", "pushpull")


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":
        return tp.ragged(N, 7)
    if name == "ragged_half":   # hub rows of 300 and more, empty rows, self-loops, repeated entries
        return tp.symmetrize(*tp.ragged(N, 7), N, every=2)
    if name == "banded":
        return tp.banded(N, 7)
    if name == "big":
        return tp.ragged(NBIG, 11, max_deg=5, hub_every=65537, hub_deg=70)
    if name == "mid_ragged":
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID, every=2)
    if name == "mid_banded":
        return tp.banded(NMID, 7, hub_every=1024, hub_deg=40)
    if name == "complete":
        return tr.csr_of_names(total_topology(NFULL))
    raise KeyError(name)


def nodes_of(name):
    return topo(name)[0].size - 1


def injects(name, R):
    """Every value somewhere, and one each at a hub, at a node with an empty row and at the last node."""
    n = nodes_of(name)
    deg = np.diff(topo(name)[0].astype(np.int64))
    hub, empty = int(np.argmax(deg)), int(np.nonzero(deg == 0)[0][3])
    assert deg[hub] >= 40 and deg[empty] == 0
    return tuple([((431 * i) % n, i) for i in range(R)] + [(hub, 0), (empty, R // 2), (n - 1, R - 1)])


def run(x, name, inj, rounds):
    x.set_topology(topo(name))
    for n, r in inj:
        x.inject(n, r)
    return x.step(rounds), x.read_shard()


@functools.lru_cache(maxsize=None)
def ref(name, R, mode, k, seed, inj, rounds, faults=()):
    """(step result, final state) of the restatement, computed once per session."""
    return run(tr.TopoSim(nodes_of(name), R, mode, k, seed, **dict(faults)), name, inj, rounds)


def gpu(name, R, mode, k, seed, inj, rounds, faults=()):
    with Engine(nodes_of(name), R, mode, k, seed, flags=FLAGS, **dict(faults)) as e:
        return run(e, name, inj, rounds)


def same(got, want):
    (a, sa), (b, sb) = got, want
    assert a.rounds == b.rounds
    for x, y in zip(a.stats, b.stats):
        assert x == y
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)


# --- ragged topologies, one engine -------------------------------------------------------------

@pytest.mark.parametrize("R", [3, 130])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ragged", "ragged_half"])
def test_ragged(name, mode, k, R):
    """24 rounds (nodes nobody points at and nodes with no row: it never converges)."""
    case = (name, R, mode, k, 0x5EED0000 + k, injects(name, R), 24)
    want = ref(*case)
    assert want[0].rounds == 24 and not want[0].stats[-1]["converged"]
    # (a value injected at a node with no row stays there under PULL: the counts' minimum may be 1)
    assert want[0].stats[-1]["messages"] > 0 and int(want[0].infected[-1].max()) > 1000
    same(gpu(*case), want)


def test_ragged_rows_are_what_the_cases_need():
    for name in ("ragged", "ragged_half"):
        rp, col = (a.astype(np.int64) for a in topo(name))
        deg = np.diff(rp)
        src = np.repeat(np.arange(N), deg)
        assert deg.max() >= 300 and (deg == 0).sum() > 100 and (src == col).any()
        assert np.unique(src * N + col).size < col.size   # repeated entries: dropped by the engine


# --- the complete graph: the uniform draw, hence the C oracle -----------------------------------

@pytest.mark.parametrize("mode,k,R", [("pushpull", 2, 3), ("pull", 5, 70)])
def test_complete_topology_equals_the_oracle(mode, k, R):
    """row_n[i] = i + (i >= n) is peer_from_word: everything but messages equals the unflagged run."""
    inj = [((431 * i) % NFULL, i) for i in range(R)]
    o = op.OracleEngine(NFULL, R, mode, k, 77, flags=1)
    for n, r in inj:
        o.inject(n, r)
    want, full = o.step(100), o.read_shard()
    o.close()
    got, shard = gpu("complete", R, mode, k, 77, tuple(inj), 100)
    assert got.rounds == want.rounds and got.converged
    for a, b in zip(got.stats, want.stats):
        assert b["messages"] == 0 and a["messages"] == k * NFULL
        assert dict(a, messages=0) == b
    assert np.array_equal(got.infected, want.infected)
    assert np.array_equal(shard, full)


# --- faults --------------------------------------------------------------------------------------

LOSS = loss_threshold(0.25)
FAULTS = {
    "loss": (("edge_loss", LOSS),),
    "parts": (("partitions", 3),),
    "loss-parts": (("edge_loss", LOSS), ("partitions", 3)),
    "stall1": (("edge_loss", LOSS), ("partitions", 3), ("stall_rounds", 1)),
    "stall2": (("edge_loss", LOSS), ("stall_rounds", 2)),
}


@pytest.mark.parametrize("mode,k,R", [("pushpull", 2, 3), ("push", 5, 130), ("pull", 4, 3)])
@pytest.mark.parametrize("faults", FAULTS, ids=list(FAULTS))
def test_faults(faults, mode, k, R):
    case = ("banded", R, mode, k, 5, injects("banded", R), 24, FAULTS[faults])
    want = ref(*case)
    clean = ref(*case[:-1])
    assert want[0].rounds == 24
    assert [int(x) for x in want[0].infected[-1]] != [int(x) for x in clean[0].infected[-1]]
    if "stall" in faults:   # stalled nodes initiate nothing: fewer messages than without the deadline
        assert want[0].stats[-1]["messages"] < ref(*case[:-1], FAULTS["loss"])[0].stats[-1]["messages"]
    same(gpu(*case), want)


def test_heal_partition_between_steps():
    def script(x):
        out = [run(x, "banded", injects("banded", 3), 10)[0]]
        x.set_faults(LOSS, 0)
        out.append(x.step(14))
        return out, x.read_shard()
    kw = dict(edge_loss=LOSS, partitions=3, stall_rounds=2)
    with Engine(N, 3, "pushpull", 2, 5, flags=FLAGS, **kw) as e:
        got = script(e)
    want = script(tr.TopoSim(N, 3, "pushpull", 2, 5, **kw))
    for a, b in zip(got[0], want[0]):
        same((a, got[1]), (b, want[1]))
    # the values cross the old cuts only after the heal: further than in a run that kept them
    cut = ref("banded", 3, "pushpull", 2, 5, injects("banded", 3), 24, tuple(kw.items()))
    assert cut[0].stats[:10] == want[0][0].stats
    assert all(int(a) > int(b) for a, b in zip(want[0][1].infected[-1], cut[0].infected[-1]))


# --- more senders than one launch has lanes -------------------------------------------------------

def test_past_one_grid():
    """2^21 + 4099 senders at 8192 blocks of 256: the last 4099 are the stride loop's second trip,
    and they take part (they pull, push and are counted)."""
    inj = tuple([((1021 * i) % NBIG, i % 3) for i in range(4096)] + [(NBIG - 1, 1), (NBIG - 4099, 2)])
    case = ("big", 3, "pushpull", 2, 11, inj, 6)
    want = ref(*case)
    got = gpu(*case)
    same(got, want)
    tail0 = {n for n, _ in inj if n >= 1 << 21}
    changed = np.nonzero(got[1][0, 1 << 21:])[0]
    assert changed.size > 1000 > len(tail0)
    deg = np.diff(topo("big")[0].astype(np.int64))
    assert want[0].stats[0]["messages"] == 2 * int((deg > 0).sum())


# --- sharded, all shards on one GPU ---------------------------------------------------------------

SHARDED = [("pushpull", 2, 3, 2), ("pushpull", 2, 3, 3), ("push", 4, 70, 3), ("pull", 5, 3, 3)]


@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("mode,k,R,G", SHARDED, ids=[f"{c[0]}-k{c[1]}-R{c[2]}-G{c[3]}" for c in SHARDED])
def test_sharded(mode, k, R, G, driver):
    """Shards of 10004, 10004, 10003 nodes (G = 3) or 15006, 15005 (G = 2); every round is a state
    all-gather round, and every shard holds the whole topology."""
    inj = injects("ragged_half", R)
    case = ("ragged_half", R, mode, k, 3, inj, 12)
    want = ref(*case)
    one = gpu(*case)
    same(one, want)
    owner = None
    if driver == "lockstep":
        shards = [Engine(N, R, mode, k, 3, flags=FLAGS, shard_rank=r, shard_count=G) for r in range(G)]
        for e in shards:
            e.set_topology(topo("ragged_half"))
            for n, r in inj:
                e.inject(n, r)
        stats, kinds = lockstep_run(shards, 12)
        assert kinds == [DENSE] * 12
        assert stats == one[0].stats
    else:
        owner = Group(N, R, mode, k, 3, flags=FLAGS, n_shards=G, devices=[0] * G)
        assert owner.transport == 2
        shards = owner.shards
        for e in shards:
            e.set_topology(topo("ragged_half"))
        for n, r in inj:
            owner.inject(n, r)
        got = owner.step(12)
        assert got.rounds == 12 and got.stats == one[0].stats
        assert np.array_equal(got.infected, one[0].infected)
    assert [e.hi - e.lo for e in shards] == ([10004, 10004, 10003] if G == 3 else [15006, 15005])
    for e in shards:
        assert np.array_equal(e.read_shard(), one[1][:, e.lo:e.hi])
    for e in shards:
        e.close()
    if owner:
        owner.close()


def test_sharded_faults_and_stall():
    """The streaks of all N nodes live on every shard and are updated through the rows."""
    kw = (("edge_loss", LOSS), ("partitions", 3), ("stall_rounds", 2))
    inj = injects("banded", 3)
    want = ref("banded", 3, "pushpull", 2, 5, inj, 24, kw)
    shards = [Engine(N, 3, "pushpull", 2, 5, flags=FLAGS, shard_rank=r, shard_count=3, **dict(kw)) for r in range(3)]
    for e in shards:
        e.set_topology(topo("banded"))
        for n, r in inj:
            e.inject(n, r)
    stats, _ = lockstep_run(shards, 24)
    assert stats == want[0].stats
    for e in shards:
        assert np.array_equal(e.read_shard(), want[1][:, e.lo:e.hi])
        e.close()


# --- state changes between steps ------------------------------------------------------------------

def both(script, R, mode, k, seed=0, **faults):
    """Runs script(x) -> list of step results on the GPU and on the restatement; everything equal."""
    runs = []
    for x in (Engine(NMID, R, mode, k, seed, flags=FLAGS, **faults), tr.TopoSim(NMID, R, mode, k, seed, **faults)):
        steps = script(x)
        runs.append((steps, x.read_shard()))
        if hasattr(x, "close"):
            x.close()
    (a, sa), (b, sb) = runs
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        same((ra, sa), (rb, sb))
    return a


def test_inject_between_steps():
    def script(x):
        out = [run(x, "mid_ragged", [(0, 0), (NMID - 1, 1)], 3)[0]]
        x.inject(1500, 2)
        x.inject(0, 0)      # held already
        out.append(x.step(3))
        x.inject(1025, 3)   # a hub
        out.append(x.step(6))
        return out
    steps = both(script, 4, "pushpull", 2, seed=9)
    assert int(steps[-1].infected[-1][3]) > 1 and int(steps[1].infected[0][2]) > 1


def test_new_topology_between_steps():
    """The next round draws from the new rows; state, round index and streaks stay."""
    def script(x):
        out = [run(x, "mid_ragged", [(0, 0), (NMID - 1, 1), (1234, 2)], 4)[0]]
        x.set_topology(topo("mid_banded"))
        out.append(x.step(8))
        return out
    steps = both(script, 3, "pushpull", 5, seed=9, edge_loss=LOSS, stall_rounds=2)
    assert steps[1].stats[0]["round"] == 4
    # and it differs from a run that kept the old rows
    keep = ref("mid_ragged", 3, "pushpull", 5, 9, ((0, 0), (NMID - 1, 1), (1234, 2)), 12,
               (("edge_loss", LOSS), ("stall_rounds", 2)))
    assert keep[0].stats[4:] != steps[1].stats


def test_reset_and_rerun():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]

    def script(x):
        out = [run(x, "mid_ragged", inj, 5)[0]]
        x.reset()           # clears the state, the round index and the streaks; the rows stay
        for n, r in inj:
            x.inject(n, r)
        out.append(x.step(9))
        return out
    steps = both(script, 3, "push", 4, seed=9, edge_loss=LOSS, stall_rounds=1)
    assert steps[1].stats[:5] == steps[0].stats


def test_single_steps_equal_one_step():
    inj = ((0, 0), (NMID - 1, 1), (1234, 2))
    whole = ref("mid_ragged", 3, "pull", 2, 9, inj, 10)

    def script(x):
        x.set_topology(topo("mid_ragged"))
        for n, r in inj:
            x.inject(n, r)
        return [x.step(1) for _ in range(10)]
    ones = both(script, 3, "pull", 2, seed=9)
    assert [s.stats[0] for s in ones] == whole[0].stats


# --- errors, and engines without the flag ------------------------------------------------------------

def test_step_without_topology():
    with Engine(N, 3, "pushpull", 2, 0, flags=FLAGS) as e:
        e.inject(0, 0)
        with pytest.raises(GossipError) as ei:
            e.step(1)
        assert ei.value.code == -4 and "topology" in str(ei.value)   # GOSSIP_ESTATE
        e.set_topology(topo("ragged"))
        assert e.step(1).rounds == 1
    shards = [Engine(N, 3, "pushpull", 2, 0, flags=FLAGS, shard_rank=r, shard_count=2) for r in range(2)]
    with pytest.raises(GossipError) as ei:
        lockstep_run(shards, 1)
    assert ei.value.code == -4
    for e in shards:
        e.close()


@pytest.mark.parametrize("mode", ["flood", "antientropy"])
def test_flag_needs_a_random_mode(mode):
    with pytest.raises(GossipError) as ei:
        Engine(N, 3, mode, 2, 0, flags=FLAGS)
    assert ei.value.code == -1   # GOSSIP_EINVAL
    with pytest.raises(GossipError):
        Group(N, 3, mode, 2, 0, flags=FLAGS, n_shards=2, devices=[0, 0])


def test_unflagged_engine_ignores_its_topology():
    """Without the flag nothing changes: a push engine that was handed a topology still draws its
    peers over all N nodes (the oracle's uniform run) and reports no messages."""
    inj = [(0, 0), (N - 1, 1), (12345, 2)]
    o = op.OracleEngine(N, 3, "push", 2, 4, flags=1)
    for n, r in inj:
        o.inject(n, r)
    want, full = o.step(12), o.read_shard()
    o.close()
    with Engine(N, 3, "push", 2, 4, flags=FLAG_HASH) as e:
        got, shard = run(e, "ragged", inj, 12)
    assert got.stats == want.stats and all(s["messages"] == 0 for s in got.stats)
    assert np.array_equal(got.infected, want.infected) and np.array_equal(shard, full)
    assert not np.array_equal(shard, ref("ragged", 3, "push", 2, 4, tuple(inj), 12)[1])
