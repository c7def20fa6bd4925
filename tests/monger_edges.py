"""The three mongering engines at the scalar and shape edges their own files leave out: full-width
seeds, fanout 61 .. 64, 64 and 4096 rumors, a limit of 15 reached count by count, node counts on and
beside the 2^21 lanes of one launch, the ends of the partition and loss ranges, and rounds past 2^8.
Shared by test_monger_edge_tables.py (CPU) and test_gpu_monger_edges.py.  A plain module, not a
conftest; it holds tables and helpers, no tests, in the style of sizes.py and values.py.

An engine is a key of ENGINES: (flag, mode, restatement).  A case is a Case tuple; `script` turns it
into the ops that `run` plays on the HIP engine and on the restatement alike, and `ref` is the
restatement's run, computed once per session.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import monger_counter_ref as mc
import monger_pull_ref as mp
import monger_pushpull_ref as mpp
import numpy_ref as nr
import sizes as sz
import topologies as tp
import values as va
from gossip_hip import (FLAG_HASH, FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER_PUSHPULL, FLAG_TOPO_PEERS, Engine,
                        loss_threshold as lt)

ENGINES = {"push": (FLAG_MONGER, "push", mc.MongerCounterSim),
           "pull": (FLAG_MONGER_PULL, "pull", mp.MongerPullSim),
           "pushpull": (FLAG_MONGER_PUSHPULL, "pushpull", mpp.MongerPushPullSim)}
ALWAYS = va.A
LOW = 0xFFFFFFFF
NSMALL = 257              # a block of 256 lanes and one node; sizes.tiny_topology
NMID = va.NMID            # 3001: twelve blocks, a ragged last wave
GRID_EDGE = 1 << 21       # 8192 blocks x 256 lanes: the nodes one launch of the sender kernels covers
DENSE = 64                # holders below GRID_EDGE in the GRID cases: the last wave of the first trip

# faults: the sorted items of the fault arguments; inj: a key of `injects`
Case = namedtuple("Case", "table engine peers N R k seed cool blind limit faults rounds inj")


def case_id(c):
    cool = "always" if c.cool == ALWAYS else str(c.cool)
    faults = "".join(f"-{name}{value:#x}" for name, value in c.faults)
    return (f"{c.engine}-{c.peers}-N{c.N}-R{c.R}-k{c.k}-seed{c.seed >> 56:02x}-cool{cool}-"
            f"{'blind' if c.blind else 'feedback'}-limit{c.limit}{faults}")


# --- the tables --------------------------------------------------------------------------------------
# SEEDS: per engine and seed one uniform and one row-peers case; R and k alternate so that both the one-word
# and the several-word kernels of an engine see every seed, with one batch of edges and with two
SEED_FAULTS = (("edge_loss", lt(0.2)),)
SEEDS = []
for _e, _engine in enumerate(ENGINES):
    for _j, _seed in enumerate(va.SEEDS):
        for _p, _peers in enumerate(("uniform", "rows")):
            SEEDS.append(Case("SEEDS", _engine, _peers, NMID, (3, 65)[(_j + _p) % 2], (2, 5)[(_e + _j + _p) % 2], _seed,
                              0.5, False, 2, SEED_FAULTS, 12, "spread"))

# MAXIMA: (N, R, k, cool, blind, limit, faults, rounds)
LOSSY = (("edge_loss", lt(0.9)),)
MAX_SHAPES = [
    (NSMALL, 4096, 2, 0.5, False, 15, (), 40),      # W = 64, every bit of every word a rumor; counts climb to 15
    (NMID, 3, 64, 0.5, False, 3, LOSSY, 16),        # sixteen full batches; the loss keeps the spread alive
    (NMID, 65, 63, ALWAYS, True, 2, LOSSY + (("partitions", 3),), 12),   # a last batch of three; one bit in word 1
    (NMID, 64, 8, 0.25, False, 15, (), 60),         # bit 63 a rumor, two full batches; counts climb to 15
    (NMID, 4033, 61, ALWAYS, True, 3, (), 6),       # W = 64 with one bit in the last word; a last batch of one
    (NSMALL, 4096, 64, 0.5, False, 2, (), 8),       # the joint corner
]
MAXIMA = []
for _e, _engine in enumerate(ENGINES):
    for _i, _shape in enumerate(MAX_SHAPES):
        for _p, _peers in enumerate(("uniform", "rows")):
            MAXIMA.append(Case("MAXIMA", _engine, _peers, *_shape[:3], va.SEEDS[(_e + _i + _p) % 3], *_shape[3:], "spread"))

# GRID: on and beside the lanes of one launch.  The seeds are full width and rotate so that the pull case of
# 2^21 + 1 nodes runs under SEEDS[0]: there some node pulls from node 2^21 in both rounds, so its counts reach
# the limit (under SEEDS[2] nobody draws it in round 1); test_gpu_monger_edges.py asserts grid_guards
GRID_SIZES = [(GRID_EDGE - 1, 65), (GRID_EDGE, 3), (GRID_EDGE + 1, 65)]
GRID = [Case("GRID", _engine, "uniform", _n, _r, 2, va.SEEDS[(_e + _i + 1) % 3], ALWAYS, True, 2, (), 2, "grid")
        for _e, _engine in enumerate(("pull", "pushpull")) for _i, (_n, _r) in enumerate(GRID_SIZES)]

PARTS = [Case("PARTS", _engine, "uniform", NMID, 3, 2, va.PAIR_SEED[NMID], 0.5, False, 2, (("partitions", _P),), 12, "pair")
         for _engine in ("pull", "pushpull") for _P in va.PARTS(NMID)]
LOSS = [Case("LOSS", _engine, "uniform", NMID, 3, 2, va.PAIR_SEED[NMID], 0.5, False, 2, (("edge_loss", _l),), 12, "pair")
        for _engine in ("pull", "pushpull") for _l in va.LOSS]

# LATE: 300 rounds in which nothing cools, then cooling by draws at t >= 300 alone (`script`)
LATE_ROUNDS = (va.LONG[0], 200)
LATE = [Case("LATE", _engine, "uniform", va.NLONG, 130, 2, va.SEEDS[_e], 0.5, False, 3, (), sum(LATE_ROUNDS), "spread")
        for _e, _engine in enumerate(ENGINES)]

TABLES = {"SEEDS": SEEDS, "MAXIMA": MAXIMA, "GRID": GRID, "PARTS": PARTS, "LOSS": LOSS, "LATE": LATE}


# --- topologies, injects, scripts ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rows(N):
    """The rows of the row-peers cases: sizes.tiny_topology at 257 nodes (a hub that lists everyone, every
    third row empty), at 3001 the ragged rows with hubs of 40, half of the listings returned."""
    if N == NSMALL:
        return sz.tiny_topology(N)
    return tp.symmetrize(*tp.ragged(N, 7, hub_every=1024, hub_deg=40), N, every=2)


def spread(c):
    """Every rumor somewhere and one at the last node; over the rows also one at a hub and one at a node
    with an empty row."""
    out = [((431 * i) % c.N, i) for i in range(c.R)] + [(c.N - 1, c.R - 1)]
    if c.peers == "rows":
        deg = np.diff(rows(c.N)[0].astype(np.int64))
        out += [(int(np.argmax(deg)), 0), (int(np.nonzero(deg == 0)[0][3]), c.R // 2)]
    return out


def grid_nodes(N):
    """The nodes of a GRID case beside the edge: the 64 below it, and above it the first and the last."""
    return sorted(set(range(GRID_EDGE - DENSE, min(GRID_EDGE, N))) | {n for n in (GRID_EDGE, N - 1) if GRID_EDGE <= n < N})


def grid_injects(c):
    """4096 spread holders; two rumors below the last at every node of grid_nodes, and the last rumor (at
    R = 65 the one bit of the last word) at the peer that node draws first in round 0: whatever the seed,
    these nodes learn in round 0 a rumor that the second round finds hot."""
    out = [((1021 * i) % c.N, i % c.R) for i in range(4096)]
    near = grid_nodes(c.N)
    first = nr.peers(c.seed, c.N, 0, 1, nodes=near)[:, 0]
    for i, (n, p) in enumerate(zip(near, first)):
        out += [(n, i % (c.R - 1)), (n, (i + 1) % (c.R - 1)), (int(p), c.R - 1)]
    return out


@functools.lru_cache(maxsize=None)
def injects(c):
    if c.inj == "grid":
        return tuple(grid_injects(c))
    if c.inj == "pair":     # node 0 draws node 1 in slot 0 of round 0 (values.PAIR_SEED): both ends hold something
        return tuple(spread(c) + [(0, 0), (1, 1)])
    return tuple(spread(c))


def script(c):
    """The ops `run` plays: ("monger", cool, blind), ("limit", m), ("inject", n, r), ("step", rounds)."""
    inj = tuple(("inject", n, r) for n, r in injects(c))
    if c.table == "LATE":
        return (("monger", 0.0, False),) + inj + (("step", LATE_ROUNDS[0]), ("monger", c.cool, c.blind), ("limit", c.limit),
                                                 ("step", LATE_ROUNDS[1]))
    return (("monger", c.cool, c.blind), ("limit", c.limit)) + inj + (("step", c.rounds),)


# --- make, run, ref, same ------------------------------------------------------------------------------

def make(kind, engine, N, R, k, seed, peers="uniform", faults=()):
    """The HIP engine (kind "gpu") or the restatement ("ref") of `engine`, the rows set where it draws from them."""
    flag, mode, sim = ENGINES[engine]
    if kind == "gpu":
        x = Engine(N, R, mode, k, seed, flags=FLAG_HASH | flag | (FLAG_TOPO_PEERS if peers == "rows" else 0), **dict(faults))
    else:
        x = sim(N, R, k, seed, topo_peers=peers == "rows", **dict(faults))
    if peers == "rows":
        x.set_topology(rows(N))
    return x


def make_case(kind, c):
    return make(kind, c.engine, c.N, c.R, c.k, c.seed, c.peers, c.faults)


def run(x, c):
    """Plays script(c) on x: the step results, and at the end the known and the hot bitsets, the counts,
    the number of hot nodes, the round index and the state hash."""
    steps = []
    for op in script(c):
        if op[0] == "step":
            steps.append(x.step(op[1]))
        else:
            getattr(x, {"monger": "set_monger", "limit": "set_monger_limit", "inject": "inject"}[op[0]])(*op[1:])
    S, H = x.read_shard(), x.read_hot()
    return SimpleNamespace(steps=steps, shard=S, hot=H, counts=x.read_counts(),
                           hot_nodes=x.hot_nodes() if hasattr(x, "hot_nodes") else int((H != 0).any(axis=0).sum()),
                           round_index=x.round_index, state_hash=x.state_hash() if hasattr(x, "state_hash") else nr.state_hash(S))


def watch_climb(x, log):
    """Makes x.round append to log the number of (node, rumor) whose count went 14 -> 15 in the round and
    whose rumor cooled in it."""
    inner = x.round

    def watched():
        c0, h0 = x.C.copy(), x.H.copy()
        out = inner()
        left = mp.unpack(h0 & ~x.H, x.R)
        log.append(int(((c0 == 14) & (x.C == 15) & left).sum()))
        return out
    x.round = watched


@functools.lru_cache(maxsize=None)
def ref(c):
    """The restatement's run of a case, computed once per session and never changed; with a limit of 15 also
    .climbed, per round (watch_climb)."""
    x = make_case("ref", c)
    climbed = []
    if c.limit == 15:
        watch_climb(x, climbed)
    out = run(x, c)
    out.climbed = climbed
    return out


def hot_after_round_0(c):
    """The restatement's hot bitset after the first round of script(c) alone."""
    x = make_case("ref", c)
    for op in script(c):
        if op[0] == "step":
            x.step(1)
            return x.read_hot()
        getattr(x, {"monger": "set_monger", "limit": "set_monger_limit", "inject": "inject"}[op[0]])(*op[1:])


def gpu(c):
    with make_case("gpu", c) as e:
        return run(e, c)


def same(got, want):
    """Bit for bit: per step the rounds, every round's stats (state_hash and messages among them) and
    per-rumor counts; at the end both bitsets, every count, the hot nodes, the round index, the hash."""
    assert len(got.steps) == len(want.steps)
    for i, (a, b) in enumerate(zip(got.steps, want.steps)):
        assert a.rounds == b.rounds, (i, a.rounds, b.rounds)
        assert len(a.stats) == len(b.stats) == a.rounds == len(a.infected) == len(b.infected), i
        for x, y in zip(a.stats, b.stats):
            assert x == y, (i, x, y)
        assert np.array_equal(a.infected, b.infected), i
    assert got.round_index == want.round_index and got.state_hash == want.state_hash
    assert np.array_equal(got.shard, want.shard)
    assert np.array_equal(got.hot, want.hot)
    assert got.counts.dtype == np.uint8 and got.counts.shape == want.counts.shape and np.array_equal(got.counts, want.counts)
    assert got.hot_nodes == want.hot_nodes == int((want.hot != 0).any(axis=0).sum())


def guard(res, name, step=None):
    """The total of one guard of the restatement over a run's rounds, or over those of one step."""
    steps = res.steps if step is None else [res.steps[step]]
    return sum(g[name] for s in steps for g in s.guards)


def held(res, R):
    """bool [R][N]: the known, the hot and the cooled rumors of a run's end state."""
    S, H = mp.unpack(res.shard, R), mp.unpack(res.hot, R)
    return S, H, S & ~H


def grid_regions(N):
    """The 64 nodes below the edge of one launch, and the second trip where there is one."""
    return [slice(GRID_EDGE - DENSE, min(GRID_EDGE, N))] + ([slice(GRID_EDGE, N)] if N > GRID_EDGE else [])


def grid_guards(c, res):
    """Per region of grid_regions: (cooled rumors, hot rumors with a count of 1, hot rumors, hot bits in the
    last word).  All must be above 0 (the last where R = 65) for the case to show that the region's lanes
    ran both passes of both rounds."""
    S, H, cooled = held(res, c.R)
    out = []
    for reg in grid_regions(c.N):
        out.append((int(cooled[:, reg].sum()), int((H[:, reg] & (res.counts[:, reg] == 1)).sum()), int(H[:, reg].sum()),
                    int(np.count_nonzero(res.hot[-1, reg]))))
    return out
