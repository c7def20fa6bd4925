"""Shard lengths on, one below and one above the units of the sharded kernels, the states built for them
and the cases run at them; shared by test_shard_size_tables.py (CPU, oracle host shards) and
test_gpu_shard_sizes.py.  A plain module in the style of sizes.py: tables, builders and the bodies the
two files share, no tests.

A sharded kernel has two index spaces, the local id (own bitmaps, `(nown + 63) >> 6` words) and the
global id (the gathered rare bitmap, the summaries, `p >> 6`); they line up only where lo = rank * Nl
is a multiple of the unit.  The other sharded files run at node counts whose shard edges are ragged in
every unit at once; these put Nl = ceil(N / G) on each unit and beside it.

A builder is `build(engine, R, G) -> number of inject calls`: it only calls `engine.inject`, so the
same call builds the one oracle engine, the oracle shards and the HIP shards.
"""
import functools

import numpy as np

import shard_cases as sc
import sizes as sz
from gossip_hip import loss_threshold
from gossip_hip.sharded import (CLASSCODED, DENSE, EXCHANGE, REP, REP_CLASSCODED, REP_GATHER, SPARSE, _CopyComm,
                                _round)
from shard_cases import SLOTS, SLOTS_CC
from states import SEED

# --- size tables -----------------------------------------------------------------------------------
# Nl = u - 1, u, u + 1 for
#   64     one bitmap word: word_valid(w, nown), setbits_kernel's segmented OR, the p >> 6 words of grb and
#          gpre (csrc/sharded.hip); the 64-row blocks of sharded ANTIENTROPY (csrc/engine.hip)
#   256    kCcUnroll = 4 bitmap words per wave step of cc_expand_kernel (csrc/sharded.hip); one 256-lane
#          block (csrc/sender.h, csrc/ae_sharded.hip)
#   1024   kScanThreads (csrc/sharded.hip)
#   2048   kScanThreads x kScanUnroll = 2: one scan step, scan_per_block and msg_cap
#   4096   ts(k) for k = 3, 4: own_regions / own_tiles of the state all-gather round (csrc/binned.hip)
#   8192   ts(k) for k = 1, 2
#   16384  kTileD: make_sb_geom's own tiles nt_d, make_xd_geom; the p_local | slot << 14 items (csrc/binned.hip)
#   32768  kRwWords = 512 words: the staged chunk of the scan (csrc/sharded.hip)
UNITS = (64, 256, 1024, 2048, 4096, 8192, 16384, 32768)
GS = (2, 3, 5, 4)


def _rotation():
    """(Nl, G, short) with G over GS and short over 0, 1, G - 1"""
    out = []
    for i, Nl in enumerate(u + d for u in UNITS for d in (-1, 0, 1)):
        G = GS[i % 4]
        out.append((Nl, G, (0, 1, G - 1)[i % 3]))
    return out


ROTATION = _rotation()
# The rotation ties short to Nl - u (both follow i % 3): u - 1 always has a full last shard, u one that is
# one node short, u + 1 one that is G - 1 short.  EXTRA gives every one of u - 1, u, u + 1 the other kind,
# at a bitmap word, a sender tile and the destination tile, and adds
#   (32768, 2, 0)  Nl = 2 x kTileD: two own tiles per shard, the edge on a tile
#   (16384, 3, 0)  the edges on tiles 1 and 2
EXTRA = [
    (32768, 2, 0), (16384, 3, 0),
    (63, 3, 2), (4095, 4, 1), (16383, 3, 1),      # u - 1 with a short last shard
    (64, 2, 0), (4096, 4, 0),                      # u with a full one (and the two above)
    (65, 4, 0), (4097, 2, 0), (16385, 3, 0),      # u + 1 with a full one
]
SHARD_SIZES = ROTATION + EXTRA


def nodes_of(entry):
    Nl, G, short = entry
    return G * Nl - short


def entry_id(entry):
    return f"Nl{entry[0]}-G{entry[1]}-N{nodes_of(entry)}"


for _e in SHARD_SIZES:
    assert 0 <= _e[2] < _e[1] and -(-nodes_of(_e) // _e[1]) == _e[0], _e
assert len(set(SHARD_SIZES)) == len(SHARD_SIZES)


def entries_at(*Nls):
    """the first entry of each of the given shard lengths (the rotation's)"""
    return [next(e for e in SHARD_SIZES if e[0] == Nl) for Nl in Nls]


WIRE_ENTRIES = entries_at(63, 64, 65, 16383, 16384, 16385)
ORDERED_ENTRIES = entries_at(63, 64, 65, 16383, 16385)
FAULT_ENTRIES = entries_at(16383, 16385, 4095, 4097)
TINY_ENTRIES = [e for e in SHARD_SIZES if nodes_of(e) <= 1100]
CAROUSEL_CPU = [e for e in SHARD_SIZES if nodes_of(e) <= 32769]
# shard_holes costs about 3 N inject calls per engine: the entries of Nl = 4096 (12287 and 16384 nodes)
HOLES_ENTRIES = [e for e in SHARD_SIZES if e[0] == 4096]

# ANTIENTROPY rounds Nl up to whole 64-row blocks: (N, G) -> the rows every shard owns
AE_SHARD_SIZES = {
    (127, 2): [64, 63],
    (128, 2): [64, 64],
    (129, 2): [128, 1],
    (129, 3): [64, 64, 1],
    (257, 3): [128, 128, 1],
    (511, 2): [256, 255],
    (512, 2): [256, 256],
    (513, 2): [320, 193],
    (4097, 2): [2112, 1985],
    (8192, 2): [4096, 4096],
    (12289, 3): [4160, 4160, 3969],
}
AE_ALIGNED_AT = [(128, 2), (512, 2), (8192, 2)]


def ae_pairs(N, G):
    """The (K, k) pairs run at one entry: sizes.AE_PAIRS in rotation, and sizes.AE_ALIGNED (a wide row, a
    fanout past the binned dense round) where every shard is whole blocks."""
    i = list(AE_SHARD_SIZES).index((N, G))
    return [sz.AE_PAIRS[i % 3]] + (sz.AE_ALIGNED if (N, G) in AE_ALIGNED_AT else [])


AE_ITEMS = [(N, G, K, k) for N, G in AE_SHARD_SIZES for K, k in ae_pairs(N, G)]

# kSmallIndex = 2^16 (csrc/sharded.hip): at most that many rare nodes over all shards and values are found
# by binary search in the owner's list; one more and the per-word ranks and the summary pass run.  Three
# shards of 65537 nodes, node 3 i holds the one rumor for i < rare: the rare nodes spread over every shard.
INDEX_N, INDEX_G, INDEX_R = 3 * 65537, 3, 1
INDEX_RARE = (65536, 65537)
K_SMALL_INDEX = 1 << 16


# --- builders ----------------------------------------------------------------------------------------

def shard_nodes(N, G):
    """0, N - 2, N - 1, two nodes on either side of every shard edge, and sizes.boundary_nodes(N); sorted."""
    Nl = -(-N // G)
    out = {0, N - 2, N - 1} | set(sz.boundary_nodes(N))
    for r in range(1, G):
        out.update(r * Nl + d for d in (-2, -1, 0, 1))
    return sorted(x for x in out if 0 <= x < N)


def shard_edges(engine, R, G):
    """The sharded twin of sizes.edges_at: rumor i % R at the i-th node of shard_nodes and every rumor at
    N - 1, so the first sparse rounds have their whole rare set on shard edges and unit edges."""
    N = engine.n_nodes
    calls = 0
    for i, n in enumerate(shard_nodes(N, G)):
        engine.inject(n, i % R)
        calls += 1
    for r in range(R):
        engine.inject(N - 1, r)
    return calls + R


def shard_holes(engine, R, G):
    """sizes.holes_at with shard_nodes empty: full-majority from the start, the not-full rare lists come
    from shard edges.  About 3 N calls: for N <= 16385."""
    N = engine.n_nodes
    empty = set(shard_nodes(N, G))
    calls = 0
    for n in range(N):
        if n in empty:
            continue
        for r in range(R):
            if n % 97 == 5 and r == n % R:
                continue
            engine.inject(n, r)
            calls += 1
    return calls


def index_state(engine, rare, complement=False):
    """node 3 i holds the rumor for i < rare; complement: every node but those"""
    held = set(range(0, 3 * rare, 3))
    for n in (sorted(set(range(engine.n_nodes)) - held) if complement else sorted(held)):
        engine.inject(n, 0)


BUILDERS = {"edges": shard_edges, "holes": shard_holes}

# --- runs (tests/shard_cases.py: (name, mode, k, edge_loss, partitions)) ---------------------------------
R3 = 3
MODES = sz.MODES
# shard_edges leaves every rumor in each of the three partitions, so these runs converge, later
LOSS, PARTS = loss_threshold(0.25), 3


def run_of(entry, mode, k, builder="edges", loss=0, parts=0, R=R3):
    """The run of one entry; its name says N, G, R and the builder."""
    Nl, G, _ = entry
    N = nodes_of(entry)
    name = sc.register(f"{builder}-N{N}-G{G}-R{R}", N, R, functools.partial(BUILDERS[builder], R=R, G=G))
    return (name, mode, k, loss, parts)


def index_run(rare, mode, k, complement=False):
    name = sc.register(f"index{'-full' if complement else ''}-{rare}", INDEX_N, INDEX_R,
                       functools.partial(index_state, rare=rare, complement=complement))
    return (name, mode, k, 0, 0)


# the three runs test_shard_size_tables.py holds every entry to
TABLE_RUNS = (("push", 3), ("pull", 1), ("pushpull", 2))

# A sparse message addressed to the last node of a shard (p + 1 a multiple of Nl) from another shard is
# what an owner computed one node off gets wrong.  It is a chance event: G = 2 has one such node, a run
# that also pulls heals a misdelivered push in the same round, and under SEED the table runs of four
# G = 2 entries never deliver one that matters.  EDGE_RUN, PUSH with fanout 1 (the longest runs), is added
# on the sparse plan at every entry; at 8190 and 8194 nodes it needs another seed to push onto that node
# from the other shard while it still lacks something (test_shard_size_tables.py asserts the push).
EDGE_RUN = ("push", 1)
EDGE_SEED = {(4095, 2, 0): SEED + 1, (4097, 2, 0): SEED + 1}


def edge_seed(entry):
    return EDGE_SEED.get(entry, SEED)


def last_node_pushes(entry, mode, k, seed=SEED):
    """The rounds of a run in which a sparse round sends a message from another shard to the last node of
    a shard that is not the last: restated from S_t and the peers of oracle/numpy_ref.py."""
    Nl, G, _ = entry
    N = nodes_of(entry)
    states, _ = sc.reference(run_of(entry, mode, k), seed)
    fm = sc.full_mask(R3)
    n = np.arange(N, dtype=np.int64)
    rounds = []
    for t, S in enumerate(states[:-1]):
        maj = sc.rare_is_not_full(S, N, R3)
        rare = (S != fm) if maj else (S != 0)
        P, live = sc._edges(seed, N, k, 0, 0, t)
        for target in (q * Nl - 1 for q in range(1, G)):
            v = S[target] if rare[target] else (fm if maj else np.uint64(0))
            sent = (P == target) & live & ((n // Nl != target // Nl) & (rare | rare[target]) & ((S & ~v) != 0))[:, None]
            if sent.any():
                rounds.append(t)
    return sorted(set(rounds))


# forced plans: name -> (knobs, the first round's kind); the later rounds are of the same kind, REP after
# either way into replication
PLANS = {
    "sparse": (SLOTS[0][1], SPARSE), "sparse_alld": (SLOTS[6][1], SPARSE), "dense": (SLOTS[1][1], DENSE),
    "classcoded": (SLOTS[5][1], CLASSCODED), "exchange": (SLOTS[4][1], EXCHANGE),
    "exchange_unfiltered": (SLOTS[7][1], EXCHANGE), "replicated": (SLOTS[2][1], REP_GATHER),
    "replicated_cc": (SLOTS_CC[2][1], REP_CLASSCODED),
}
# GOSSIP_FLAG_SHARD_DIRECT: the same knobs on the direct kernels (HIP only: the oracle has one form)
DIRECT_PLANS = {"dense_direct": "dense", "classcoded_direct": "classcoded"}
GPU_PLANS = list(PLANS) + list(DIRECT_PLANS)
K_ROTATION = (1, 3, 2, 4)


def plan_kinds(plan, rounds):
    kind = PLANS[DIRECT_PLANS.get(plan, plan)][1]
    return [kind] + [REP if kind in (REP_GATHER, REP_CLASSCODED) else kind] * (rounds - 1)


def forced_case(entry, plan):
    """(mode, k) of one entry on one plan: the modes rotate so that an entry runs all three across its plans,
    the fanouts over K_ROTATION, in which neighbours are of different ts classes (8192 for k <= 2, 4096
    for k <= 4), so that the all-gather plans (dense, class-coded, replicated), which are neighbours in
    GPU_PLANS, meet both classes of own_regions at every entry."""
    i, j = SHARD_SIZES.index(entry), GPU_PLANS.index(plan)
    return MODES[(i + j) % 3], K_ROTATION[(i + j) % 4]


def carousel_case(entry):
    """(mode, k): k = 1 or 2, so that the smallest entries run the six rounds that reach every kind"""
    i = SHARD_SIZES.index(entry)
    return MODES[i % 3], 1 + i % 2


# --- bodies shared by the CPU file (factory = op.OracleEngine) and the GPU file (Engine) ---------------------

MASK64 = (1 << 64) - 1


def assert_final_hash(engines, want_hash):
    """the shards' own hashes add up (mod 2^64) to the one engine's"""
    assert sum(e.state_hash() for e in engines) & MASK64 == want_hash


def body_forced(factory, run, G, plan, driver=None, flags=0, rounds=None, seed=SEED):
    """One forced plan from the built state to convergence (or `rounds` rounds): per-round stats with the
    hash, per-rumor counts where the driver has them, the kind of every round, every shard's final slice
    and the final state hash against one oracle engine."""
    states, want = sc.reference(run, seed)
    infected = sc.reference_infected(run, seed)
    T = min(len(want), rounds or len(want))
    knobs = PLANS[DIRECT_PLANS.get(plan, plan)][0]
    d = sc.open_driver(driver, factory, run, G, flags=flags, params=knobs, seed=seed)
    try:
        kinds = []
        for i in range(T):
            got, kind = d.round()
            kinds.append(kind)
            assert got == want[i], (i, kinds)
            sc.assert_infected(d, infected[i])
        assert kinds == plan_kinds(plan, T)
        sc.assert_shards_hold(d.engines, states[T])
        assert_final_hash(d.engines, want[T - 1]["state_hash"])
    finally:
        d.close()
    return kinds


def body_sparse_wire(factory, run, G):
    """The forced sparse plan over the recording comm: every round's rare counts, rare lists and messages
    against the numpy restatement from S_t alone.  A rare node listed past a short last shard's end
    changes no state bit and shows only here.  (A PULL run costs the restatement no peer draws.)"""
    states, want = sc.reference(run)
    knobs = PLANS["sparse"][0]
    d = sc.open_driver(None, factory, run, G, params=knobs, recording=True)
    try:
        for i, w in enumerate(want):
            got, kind = d.round()
            assert got == w and kind == SPARSE, i
            sc.check_round_wire(kind, d.comm.take(), states[i], run, G, i, knobs)
    finally:
        d.close()


def body_auto(factory, run, G, driver=None):
    """The planner's own choice: stats, per-rumor counts, final slices and hash."""
    states, want = sc.reference(run)
    infected = sc.reference_infected(run)
    d = sc.open_driver(driver, factory, run, G)
    try:
        for i, w in enumerate(want):
            got, _ = d.round()
            assert got == w, i
            sc.assert_infected(d, infected[i])
        sc.assert_shards_hold(d.engines, states[-1])
        assert_final_hash(d.engines, want[-1]["state_hash"])
    finally:
        d.close()


def body_carousel(factory, run, G, offset, driver=None):
    """shard_cases.body_carousel with every shard compared after every round."""
    states, want = sc.reference(run)
    infected = sc.reference_infected(run)
    d = sc.open_driver(driver, factory, run, G)

    def after(i, kind, knobs):
        sc.assert_infected(d, infected[i])
        sc.assert_shards_hold(d.engines, states[i + 1])

    try:
        stats, kinds = sc.carousel(d, SLOTS, offset, len(want), after_round=after)
        assert stats == list(want)
        assert kinds == sc.expected_kinds(SLOTS, offset, len(want))
        assert_final_hash(d.engines, want[-1]["state_hash"])
    finally:
        d.close()
    return kinds


# --- multi-word and topology shards: image_base(n, Nl, W) of csrc/sender.h ---------------------------------
WIDE_R = 130


def multiword_reference(factory, N, mode, k, rounds=64):
    ref = factory(N, WIDE_R, mode, k, SEED, flags=1)
    shard_edges(ref, WIDE_R, 1)
    res = ref.step(rounds)
    out = res.stats, ref.read_shard(), res.infected
    ref.close()
    return out


def body_multiword(factory, entry, mode, k, want, driver=None):
    """R = 130 (three words per node) from shard_edges: every round the plain state all-gather over the
    [G][W][Nl] image."""
    Nl, G, _ = entry
    N = nodes_of(entry)
    stats, full, infected = want
    d = (driver or sc.LockstepDriver)(factory, N, WIDE_R, mode, k, SEED, G, flags=1)
    try:
        for e in d.engines:
            shard_edges(e, WIDE_R, 1)
        for i, w in enumerate(stats):
            got, kind = d.round()
            assert got == w and kind == DENSE, i
            sc.assert_infected(d, infected[i])
        for e in d.engines:
            assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])
    finally:
        d.close()


TOPO_ROUNDS = 24       # the nodes with an empty row pull nothing, so PULL never converges


def topo_cases(entry):
    """(mode, R, k) of GOSSIP_FLAG_TOPO_PEERS over sizes.tiny_topology at one entry: all three modes, one
    and three words per node in turn, k over sizes.MONGER_K."""
    i = SHARD_SIZES.index(entry)
    return [(mode, (3, WIDE_R)[(i + j) % 2], sz.MONGER_K[(i + j) % 3]) for j, mode in enumerate(MODES)]


def topo_run(x, N, R):
    x.set_topology(sz.tiny_topology(N))
    for n, r in sz.tiny_injects(N, R):
        x.inject(n, r)


# --- sharded ANTIENTROPY through ae_cases.run --------------------------------------------------------------

class _KeepComm(_CopyComm):
    """the copy comm, keeping the last summed partials (the round's: its per-component counts)"""

    def sum(self, L, stem, each=None):
        self.total = super().sum(L, stem, each=each)
        return self.total


class _Step:
    def __init__(self, stats, infected):
        self.stats, self.infected, self.rounds = stats, infected, len(stats)


class AeShards:
    """G ANTIENTROPY shards behind the one-engine calls ae_cases.run makes.  group: a gossip_hip.Group
    (its own step), else the engines run sharded._round in lockstep over the copy comm, every round of
    kind 2."""

    def __init__(self, engines, group=None):
        self.engines, self.group = engines, group
        self.n_nodes, self.n_rumors = engines[0].n_nodes, engines[0].n_rumors
        self.comm = None if group else _KeepComm(engines)

    def inject_random(self):
        for e in self.engines:
            e.inject_random()

    def inject(self, node, comp):
        for e in self.engines:
            e.inject(node, comp)

    def step(self, rounds):
        if self.group:
            return self.group.step(rounds)
        stats, infected = [], []
        for _ in range(rounds):
            kinds = []
            _, st = _round(self.engines, self.comm, kinds)
            assert kinds == [2] and all(s == st[0] for s in st)
            stats.append(st[0])
            infected.append(np.array(self.comm.total[4:4 + self.n_rumors], dtype=np.uint64))
            if st[0]["converged"]:
                break
        return _Step(stats, np.stack(infected) if infected else np.zeros((0, self.n_rumors), np.uint64))

    def read_versions(self, node):
        (owner,) = [e for e in self.engines if e.lo <= node < e.hi]
        return owner.read_versions(node)

    def read_rows(self):
        return np.concatenate([e.read_rows() for e in self.engines])
