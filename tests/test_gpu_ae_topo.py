"""GPU: ANTIENTROPY over the topology (GOSSIP_FLAG_AE_TOPO_PEERS) on every round
path that draws a peer through a row, one engine and sharded, bit for bit per round against the
numpy restatement (ae_topo_ref.py): stats, per-component counts, hash, every row, the probed alive
flags.  test_ae_topo_ref.py holds that restatement to the C oracle on the CPU; the complete-graph
test here holds the engine to the C oracle directly.

Shapes: 30011 nodes (469 chunks, the last of 59 nodes) on `ragged` and its half-symmetrized form
(hub rows of 300, empty rows, self-loops, repeated entries) and on a connected form that converges,
so the late sparse rounds run; every lane class of the row phase (K = 1, 3, 5, 16, 33, 64) and every
fanout class (k <= 3 shares the churn word, 4 fills the Philox block, 5 opens the second, 9 the third
and the sharded redraw); 2^21 + 4099 nodes for the second trip of the chunk loop.

Every reference is computed once per case and shared by the paths.  Guards keep a case from passing
vacuously: see _guards and the counters read from the engine's timers (timer 2 counts the sparse
rounds tried, timer 0 the dense rounds, so tried + dense - rounds = overflowed and rerun)."""
import functools
import os

import numpy as np
import pytest

import ae_faults_ref as fr
import ae_topo_ref as ar
import oracle_py as op
import topo_ref as tr
import topologies as tp
from gossip_hip import (FLAG_AE_DIRECT_SCAN, FLAG_AE_TOPO_PEERS, FLAG_HASH, FLAG_TIMING, FLAG_TOPO_PEERS, Engine,
                        GossipError, Group, grid_topology, total_topology)
from gossip_hip.engine import churn_threshold as ct, loss_threshold as lt

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
FLAGS = FLAG_HASH | FLAG_TIMING | FLAG_AE_TOPO_PEERS
N = 30011
NBIG = (1 << 21) + 4099   # chunk_grid caps at 8192 blocks of 4 waves = 2^21 nodes: the rest is a second trip
NFULL = 1025
NSMALL = 130              # G = 4: Nl = 64, shards of 64, 64, 2 and 0 nodes
NGRID = 1024
LOSS, PARTS = lt(0.3), 3
FAIL, REC = 0.03, 0.25


def _with_ring(rp, col, n):
    """Every row gets (u + 1) % n appended: with the listings back, one component."""
    rp = rp.astype(np.int64)
    col2 = np.insert(col.astype(np.int64), rp[1:], (np.arange(n) + 1) % n)
    return (rp + np.arange(n + 1)).astype(np.uint32), col2.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":
        return tp.ragged(N, 7)
    if name == "ragged_half":
        return tp.symmetrize(*tp.ragged(N, 7), N, every=2)
    if name == "connected":   # fully symmetrized over a ring: it converges
        return tp.symmetrize(*_with_ring(*tp.ragged(N, 7), N), N)
    if name == "banded":      # a second topology for the state changes
        return tp.banded(N, 7)
    if name == "big":
        return tp.ragged(NBIG, 11, max_deg=5, hub_every=65537, hub_deg=70)
    if name == "small":
        return tp.symmetrize(*tp.ragged(NSMALL, 3, max_deg=5, hub_every=50, hub_deg=20), NSMALL, every=2)
    if name == "complete":
        return tr.csr_of_names(total_topology(NFULL))
    if name == "grid":
        return tr.csr_of_names(grid_topology(NGRID))
    raise KeyError(name)


def nodes_of(name):
    return topo(name)[0].size - 1


def test_topologies_are_what_the_cases_need():
    for name in ("ragged", "ragged_half"):
        rp, col = (a.astype(np.int64) for a in topo(name))
        deg = np.diff(rp)
        src = np.repeat(np.arange(N), deg)
        assert deg.max() >= 300 and (deg == 0).sum() > 100 and (src == col).any()
        assert np.unique(src * N + col).size < col.size   # repeated entries: dropped by the engine
    assert N % 64 == 59 and (np.diff(topo("connected")[0].astype(np.int64)) > 0).all()
    assert (np.diff(topo("small")[0].astype(np.int64)) == 0).any()


# --- scripts, references, engines ------------------------------------------------------------------

def _resolve(script):
    return tuple(("topology", topo(op_[1])) if op_[0] == "topology" else op_ for op_ in script)


def _probe(n):
    return (0, 1, n // 3, n // 2, n - 1)


def _args(n, K, k, seed, fail=FAIL, rec=REC, **fa):
    return (n, K, "antientropy", k, seed), dict(flags=1, churn_fail=ct(fail), churn_recover=ct(rec), **fa)


@functools.lru_cache(maxsize=None)
def _reference(args, kwitems, script):
    """(run_script's result, the restatement's per-round guard figures), once per session."""
    r = ar.RefEngine(*args, **dict(kwitems))
    out = ar.run_script(r, _resolve(script), _probe(args[0]))
    return out, dict(lost=tuple(r.lost), selfs=tuple(r.selfs), repeats=tuple(r.repeats), empty=tuple(r.empty_alive))


def _want(args, kw, script):
    return _reference(args, tuple(sorted(kw.items())), script)


def _flat(out):
    return [s for o in out for s in o["stats"]]


PATHS = {"auto": {}, "dense": {"ae_sparse": 0}, "sparse": {"ae_sparse": 1}, "overflow": {"ae_sparse": 1, "ae_cap": 64},
         # knobs of the binned paths and of the pipeline: accepted, and they move nothing here
         "knobs": {"ae_dense_bin": 1, "ae_dense_cap": 16, "ae_dense_filter": 0, "ae_ahead": 3}}


def _params(path, args):
    p = dict(PATHS[path])
    if path == "sparse":  # room for every exchange (the default list holds max(N / 8, 65536) edges)
        p["ae_cap"] = 2 * args[0] * args[3]
    return p


def _engine(path, args, kw, extra_flags=0):
    return Engine(*args, params=_params(path, args), **dict(kw, flags=FLAGS | extra_flags))


def _counters(e, rounds):
    """(dense rounds, sparse rounds that held, sparse rounds that overflowed and were rerun dense)."""
    dense, tried = e.kernel_time(0)[1], e.kernel_time(2)[1]
    over = dense + tried - rounds
    return dense, tried - over, over


def _check(path, args, kw, script, lost_from=None, ragged=False):
    """lost_from: the first faulted round (its alive-alive edges must include a lost one); ragged: a
    30011-node ragged case (a self-exchange, a repeated pair where k > 1, an alive node with no row)."""
    want, fig = _want(args, kw, script)
    rounds = len(_flat(want))
    if lost_from is not None:
        assert fig["lost"][lost_from] > 0 and sum(fig["lost"][:lost_from]) == 0
    if ragged:
        assert sum(fig["selfs"]) > 0 and min(fig["empty"]) > 0
        assert args[3] == 1 or sum(fig["repeats"]) > 0
    e = _engine(path, args, kw)
    got = ar.run_script(e, _resolve(script), _probe(args[0]))
    fr.assert_same(got, want)
    assert e.state_hash() == _flat(want)[-1]["state_hash"]
    dense, sparse, over = _counters(e, rounds)
    e.close()
    assert dense + sparse == rounds and dense >= 1  # (the first round has no stale bits yet: dense)
    if path == "dense":
        assert sparse == 0 and over == 0
    if path == "sparse":
        assert sparse >= 1
    if path == "overflow":
        assert over >= 1
    return want, (dense, sparse, over)


def _writes(n, K):
    return (("inject", n // 2, K - 1), ("inject", 3, 0))


# --- ragged topologies: every lane class and fanout class on every path -----------------------------

SHAPES = [(1, 1), (3, 2), (5, 3), (16, 4), (33, 9), (64, 5)]


@pytest.mark.parametrize("path", ["auto", "dense", "sparse"])
@pytest.mark.parametrize("K,k", SHAPES)
@pytest.mark.parametrize("name", ["ragged", "ragged_half"])
def test_ragged(name, K, k, path):
    """12 rounds with churn and two client writes (nodes nobody points at: it never converges)."""
    args, kw = _args(N, K, k, 0x5EED0F00 + 16 * K + k)
    script = (("topology", name), ("random",), ("step", 5)) + _writes(N, K) + (("step", 7),)
    want, _ = _check(path, args, kw, script, ragged=True)
    assert len(_flat(want)) == 12 and not _flat(want)[-1]["converged"]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("K,k", [(5, 2), (16, 1), (3, 9)])
def test_connected_converges(K, k, path):
    """To convergence (the restatement: 23, 31 and 13 rounds): the late rounds run sparse on `auto`,
    the 64-edge list overflows and the round is rerun dense, the ignored knobs move nothing."""
    args, kw = _args(N, K, k, 0x5EED0F00 + K)
    script = (("topology", "connected"), ("random",), ("step", 400))
    want, cnt = _check(path, args, kw, script)
    assert _flat(want)[-1]["converged"] and 10 < len(_flat(want)) < 60
    if path == "auto":
        assert cnt[1] >= 1  # a sparse round ran and held
    if path == "knobs":     # the same rounds on the same paths as without the knobs
        e = _engine("auto", args, kw)
        e.set_topology(topo("connected"))
        e.inject_random()
        assert e.step(400).rounds == len(_flat(want))
        assert _counters(e, len(_flat(want))) == cnt
        e.close()


# --- faults ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "dense", "sparse"])
@pytest.mark.parametrize("name,K,k", [("connected", 5, 2), ("connected", 16, 4), ("ragged_half", 3, 9)])
def test_loss(name, K, k, path):
    """edge_loss = 0.3 throughout, to convergence (connected: 28 and 18 rounds) or 24 rounds."""
    args, kw = _args(N, K, k, 0x5EED0F00 + K, edge_loss=LOSS)
    script = (("topology", name), ("random",), ("step", 6)) + _writes(N, K) + (("step", 400 if name == "connected" else 18),)
    want, _ = _check(path, args, kw, script, lost_from=0, ragged=name != "connected")
    assert _flat(want)[-1]["converged"] == (name == "connected")


@pytest.mark.parametrize("path", ["auto", "sparse"])
@pytest.mark.parametrize("name,K,k", [("connected", 5, 2), ("ragged_half", 16, 1)])
def test_partition_then_heal(name, K, k, path):
    """partitions = 3 for 40 rounds (block boundaries off the 64-node chunks), then the heal."""
    args, kw = _args(N, K, k, 0x5EED0F00 + K, partitions=PARTS)
    script = (("topology", name), ("random",), ("step", 6)) + _writes(N, K) + (("step", 34), ("faults", 0, 0), ("step", 60))
    want, _ = _check(path, args, kw, script, lost_from=0, ragged=name != "connected")
    assert len(_flat(want[:2])) == 40 and not any(s["converged"] or s["full_nodes"] for s in _flat(want[:2]))
    assert _flat(want)[-1]["converged"] == (name == "connected")


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_faults_switched_on_later(path):
    args, kw = _args(N, 5, 2, 0x5EED0F05)
    script = (("topology", "connected"), ("random",), ("step", 3), ("faults", LOSS, PARTS), ("step", 20), ("faults", 0, 0),
              ("step", 400))
    want, _ = _check(path, args, kw, script, lost_from=3)
    assert _flat(want)[-1]["converged"] and not any(s["converged"] for s in _flat(want)[:23])


# --- the complete graph: the uniform draw, hence the C oracle ---------------------------------------

@pytest.mark.parametrize("path", ["auto", "sparse"])
@pytest.mark.parametrize("K,k", [(5, 2), (16, 5)])
def test_complete_graph_equals_the_oracle(K, k, path):
    """Identity (a): row_n[i] = i + (i >= n) is peer_from_word, so the flagged engine is the C
    oracle's ANTIENTROPY in every field, messages included."""
    args, kw = _args(NFULL, K, k, 0x5EED0A00 + K)
    o = op.OracleEngine(*args, threads=THREADS, **kw)
    e = _engine(path, args, kw)
    e.set_topology(topo("complete"))
    for x in (e, o):
        x.inject_random()
    a, b = e.step(100), o.step(100)
    assert a.rounds == b.rounds and a.converged and a.stats == b.stats
    assert np.array_equal(a.infected, b.infected) and np.array_equal(e.read_rows(), o.read_rows())
    for n in _probe(NFULL):
        assert e.read_versions(n)[1] == o.read_versions(n)[1]
    for x in (e, o):
        x.close()


# --- past one launch's chunks ------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["dense", "sparse"])
def test_second_trip_of_the_chunk_loop(path):
    args, kw = _args(NBIG, 1, 2, 0x5EED0B16)
    want, _ = _check(path, args, kw, (("topology", "big"), ("random",), ("step", 3)))
    assert len(_flat(want)) == 3


# --- state changes between steps ----------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_state_changes_between_steps(path):
    """A new topology takes effect in the next round (rows, alive and stale bits, round index stay);
    inject raises the target; reset keeps the topology and the faults."""
    K, k = 5, 2
    args, kw = _args(N, K, k, 0x5EED0F55, edge_loss=lt(0.1))
    script = (("topology", "ragged_half"), ("random",), ("step", 8), ("topology", "connected"), ("step", 12)) + \
        _writes(N, K) + (("topology", "banded"), ("step", 5), ("topology", "connected"), ("step", 400), ("reset",),
                         ("random",), ("step", 400))
    want, _ = _check(path, args, kw, script, lost_from=0)
    assert [o["stats"][0]["round"] for o in want[:4]] == [0, 8, 20, 25] and want[3]["stats"][-1]["converged"]
    assert want[4]["stats"][0]["round"] == 0 and want[4]["stats"][-1]["converged"]


# --- errors and the unflagged engine ------------------------------------------------------------------

def test_step_without_a_topology_is_estate():
    with Engine(1000, 4, "antientropy", 2, 1, flags=FLAGS) as e:
        e.inject_random()
        with pytest.raises(GossipError) as ei:
            e.step(1)
        assert ei.value.code == -4 and "topology" in str(ei.value)
        e.set_topology(tp.ragged(1000, 3))
        assert e.step(2).rounds == 2
    engines = [Engine(1000, 4, "antientropy", 2, 1, flags=FLAGS, shard_rank=r, shard_count=2) for r in range(2)]
    for e in engines:  # every rank fails in the plan, before any collective
        e.inject_random()
        with pytest.raises(GossipError) as ei:
            e.sharded_plan()
        assert ei.value.code == -4
        with pytest.raises(GossipError):
            e.exchange_buffers()
        e.close()
    with Group(1000, 4, "antientropy", 2, 1, flags=FLAGS, n_shards=2, devices=[0, 0]) as g:
        g.inject_random()
        with pytest.raises(GossipError) as ei:
            g.step(1)
        assert ei.value.code == -4
        for e in g.shards:
            e.set_topology(tp.ragged(1000, 3))
        assert g.step(2).rounds == 2


def test_create_rules():
    for mode in ("flood", "push", "pull", "pushpull"):
        for flags in (FLAG_AE_TOPO_PEERS, FLAG_AE_TOPO_PEERS | FLAG_TOPO_PEERS):
            with pytest.raises(GossipError) as ei:
                Engine(1000, 4, mode, 2, 1, flags=flags)
            assert ei.value.code == -1
    for make in (lambda **kw: Engine(1000, 4, "antientropy", 2, 1, **kw),
                 lambda **kw: Group(1000, 4, "antientropy", 2, 1, n_shards=2, devices=[0, 0], **kw)):
        with pytest.raises(GossipError) as ei:
            make(flags=FLAG_AE_TOPO_PEERS | FLAG_TOPO_PEERS)
        assert ei.value.code == -1
        with pytest.raises(GossipError) as ei:
            make(flags=FLAG_AE_TOPO_PEERS, stall_rounds=1)
        assert ei.value.code == -6


@pytest.mark.parametrize("extra", [0, FLAG_AE_DIRECT_SCAN])
def test_unflagged_engine_ignores_its_topology(extra):
    """Without the flag nothing changes, bit for bit, whatever topology the engine was handed."""
    args, kw = _args(N, 5, 2, 0x5EED0F77, edge_loss=lt(0.1))
    out = []
    for with_topo in (False, True):
        with Engine(*args, **dict(kw, flags=FLAG_HASH | extra)) as e:
            if with_topo:
                e.set_topology(topo("ragged_half"))
            e.inject_random()
            r = e.step(400)
            out.append((r.stats, r.infected.copy(), e.read_rows()))
    assert out[0][0] == out[1][0] and out[0][0][-1]["converged"]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# --- sharded -------------------------------------------------------------------------------------------

# topology, K, fanout, G, faults
SHARDED = [
    ("ragged_half", 5, 2, 3, dict(edge_loss=LOSS, partitions=PARTS)),
    ("connected", 16, 4, 2, dict(edge_loss=LOSS, partitions=PARTS)),
    ("connected", 3, 9, 4, dict(edge_loss=LOSS)),           # k > 8: the fill pass redraws
    ("ragged_half", 64, 3, 4, {}),                           # 7552, 7552, 7552 and 7355 nodes
    ("small", 3, 9, 4, dict(edge_loss=LOSS, partitions=2)),  # 64, 64, 2 and 0 nodes
    ("small", 8, 1, 2, {}),
]


def _sharded_script(name, n, K):
    return (("topology", name), ("random",), ("step", 5)) + _writes(n, K) + (("step", 15), ("faults", 0, 0), ("step", 30))


@pytest.mark.parametrize("case", SHARDED, ids=[f"{c[0]}-K{c[1]}-k{c[2]}-G{c[3]}" for c in SHARDED])
def test_sharded_lockstep(case):
    """G shard engines in lockstep (gossip_ae_*), faults healed on every rank after 20 rounds: equal
    to the restatement (which the one-engine tests hold the single engine to), every round of kind 2."""
    name, K, k, G, fa = case
    n = nodes_of(name)
    args, kw = _args(n, K, k, 0x5EED0F00 + 16 * K + G, **fa)
    script = _sharded_script(name, n, K)
    want, fig = _want(args, kw, script)
    if fa:
        assert fig["lost"][0] > 0
    assert sum(fig["selfs"]) > 0 and min(fig["empty"]) > 0 or name == "connected"
    engines = [Engine(*args, shard_rank=r, shard_count=G, **dict(kw, flags=FLAGS)) for r in range(G)]
    assert engines[-1].hi - engines[-1].lo < engines[0].hi - engines[0].lo
    got = ar.run_script(engines, _resolve(script))
    fr.assert_same(got, want, keys=("stats", "rows"))
    assert all(g["kinds"] == [2] for g in got)
    for e in engines:
        e.close()


@pytest.mark.parametrize("case", SHARDED[:3] + SHARDED[4:5], ids=[f"{c[0]}-K{c[1]}-k{c[2]}-G{c[3]}" for c in SHARDED[:3] + SHARDED[4:5]])
def test_group(case):
    """The library-driven rounds (gossip_group_step) over G shards on one device."""
    name, K, k, G, fa = case
    n = nodes_of(name)
    args, kw = _args(n, K, k, 0x5EED0F00 + 16 * K + G, **fa)
    script = (("topology", name), ("random",), ("step", 20))
    want, fig = _want(args, kw, script)
    assert fig["lost"][0] > 0
    with Group(*args, n_shards=G, devices=[0] * G, **dict(kw, flags=FLAGS)) as g:
        for e in g.shards:
            e.set_topology(topo(name))
        g.inject_random()
        got = g.step(20)
        assert got.stats == want[0]["stats"]
        assert np.array_equal(got.infected, want[0]["infected"])
        for e in g.shards:
            assert np.array_equal(e.read_rows(), want[0]["rows"][e.lo:e.hi])


# --- the scenario the mode exists for --------------------------------------------------------------------

GRID_SPLIT, GRID_HEAL = 48, 40  # the restatement: the halves hold their maxima after 41 rounds, 22 to heal


@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_grid_partition_diverge_heal(path):
    """A 32 x 32 grid split into its top and bottom halves (contiguous id blocks, each connected):
    writes on either side spread through their own half only; after the heal every row reaches the
    global maximum over the grid's own edges."""
    K, k = 3, 2
    args, kw = _args(NGRID, K, k, 0x5EED1002, fail=0.0, rec=0.0, partitions=2)
    writes = tuple(("inject", n, c) for n, c in ((5, 0), (5, 0), (300, 1), (700, 1), (700, 1), (1000, 2)))
    script = (("topology", "grid"),) + writes + (("step", GRID_SPLIT), ("faults", 0, 0), ("step", GRID_HEAL))
    want, fig = _want(args, kw, script)
    rows = want[0]["rows"]
    top, bottom = np.array([2, 1, 0], dtype=np.uint32), np.array([0, 2, 1], dtype=np.uint32)
    assert (rows[:NGRID // 2] == top).all() and (rows[NGRID // 2:] == bottom).all()
    assert not any(s["converged"] for s in want[0]["stats"]) and len(want[0]["stats"]) == GRID_SPLIT
    assert want[1]["stats"][-1]["converged"] and (want[1]["rows"] == np.array([2, 2, 1], dtype=np.uint32)).all()
    assert len(want[1]["stats"]) < GRID_HEAL
    _check(path, args, kw, script, lost_from=0)
