"""GPU: HIP shards on one device at shard lengths on, one below and one above the units of the sharded
kernels (tests/shard_sizes.py), bit for bit against one C oracle engine, never against another HIP
engine: per-round stats with FLAG_HASH, the kind of every round, per-rumor counts where the driver hands
them out, every shard's read_shard slice and the shards' summed state hash.

The states put their holders on the shard edges (shard_edges) or leave exactly those empty
(shard_holes).  tests/test_shard_size_tables.py shows from oracle shards and the numpy restatements
alone that every case converges, runs the kinds asserted here and meets the guards (rare lists on every
rank, messages across every shard edge both ways, both majorities, a mixed node in a ragged last bitmap
word, exchange items to every owner).  References are computed once per run and shared read-only."""
import functools

import numpy as np
import pytest

import ae_cases as ac
import oracle_py as op
import shard_cases as sc
import shard_sizes as ss
import topo_ref as tr
from gossip_hip import FLAG_HASH, FLAG_SHARD_DIRECT, FLAG_TOPO_PEERS, Engine
from gossip_hip.engine import Group
from gossip_hip.sharded import DENSE
from shard_cases import GroupDriver, OrderedDevDriver
from states import SEED

pytestmark = pytest.mark.gpu
IDS = [ss.entry_id(e) for e in ss.SHARD_SIZES]
DRIVERS = {"lockstep": (Engine, None), "group": (None, GroupDriver), "ordered": (Engine, OrderedDevDriver)}


def ids(entries):
    return [ss.entry_id(e) for e in entries]


def flags_of(plan):
    return FLAG_SHARD_DIRECT if plan in ss.DIRECT_PLANS else 0


# --- a. forced plans, the lockstep driver ----------------------------------------------------------------

@pytest.mark.parametrize("plan", ss.GPU_PLANS)
@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_forced_plan(entry, plan):
    mode, k = ss.forced_case(entry, plan)
    ss.body_forced(Engine, ss.run_of(entry, mode, k), entry[1], plan, flags=flags_of(plan))


@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_sparse_edge_run(entry, driver):
    """PUSH with fanout 1: a sparse message from another shard reaches the last node of a shard while it
    lacks what the sender holds (asserted on the CPU), so an owner one node off loses a rumor."""
    factory, drv = DRIVERS[driver]
    ss.body_forced(factory, ss.run_of(entry, *ss.EDGE_RUN), entry[1], "sparse", driver=drv, seed=ss.edge_seed(entry))


@pytest.mark.parametrize("plan", ["dense", "exchange", "sparse"])
@pytest.mark.parametrize("entry", ss.FAULT_ENTRIES, ids=ids(ss.FAULT_ENTRIES))
def test_forced_plan_with_faults(entry, plan):
    """k = 3 with loss 0.25 and three partitions: the redrawn-peer emit forms."""
    ss.body_forced(Engine, ss.run_of(entry, "pushpull", 3, loss=ss.LOSS, parts=ss.PARTS), entry[1], plan)


# --- b. the other drivers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_group_auto(entry):
    mode, k = ss.carousel_case(entry)
    ss.body_auto(None, ss.run_of(entry, mode, k), entry[1], driver=GroupDriver)


@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_group_carousel(entry, offset):
    mode, k = ss.carousel_case(entry)
    ss.body_carousel(None, ss.run_of(entry, mode, k), entry[1], offset, driver=GroupDriver)


@pytest.mark.parametrize("plan", ss.GPU_PLANS)
@pytest.mark.parametrize("entry", ss.ORDERED_ENTRIES, ids=ids(ss.ORDERED_ENTRIES))
def test_ordered_forced_plan(entry, plan):
    mode, k = ss.forced_case(entry, plan)
    ss.body_forced(Engine, ss.run_of(entry, mode, k), entry[1], plan, driver=OrderedDevDriver, flags=flags_of(plan))


@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("entry", ss.ORDERED_ENTRIES, ids=ids(ss.ORDERED_ENTRIES))
def test_ordered_carousel(entry, offset):
    mode, k = ss.carousel_case(entry)
    ss.body_carousel(Engine, ss.run_of(entry, mode, k), entry[1], offset, driver=OrderedDevDriver)


# --- c. the wire -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("entry", ss.WIRE_ENTRIES, ids=ids(ss.WIRE_ENTRIES))
def test_wire_products_equal_numpy(entry, offset):
    """Class-coded slots with their tail bits, prefix words and padding, rare lists and messages as sorted
    multisets per (sender, owner), exchange items and replies: word for word."""
    mode, k = ss.carousel_case(entry)
    sc.body_carousel_wire(Engine, ss.run_of(entry, mode, k), entry[1], offset)


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_sparse_wire_equals_numpy(entry):
    """Every rank's rare list in every round of the PULL run, on every entry: a not-full node listed
    past a short last shard's end changes no state bit and shows only on the wire."""
    ss.body_sparse_wire(Engine, ss.run_of(entry, *ss.TABLE_RUNS[1]), entry[1])


# --- d. shard_holes: full-majority from round 0, the rare nodes on the shard edges --------------------------------

HOLES_ITEMS = [(e, p, d) for e in ss.HOLES_ENTRIES for p in ("sparse", "classcoded", "exchange", "replicated")
               for d in ("lockstep", "group")]


@pytest.mark.parametrize("entry,plan,driver", HOLES_ITEMS, ids=[f"{ss.entry_id(e)}-{p}-{d}" for e, p, d in HOLES_ITEMS])
def test_holes(entry, plan, driver):
    factory, drv = DRIVERS[driver]
    mode, k = ss.TABLE_RUNS[ss.GPU_PLANS.index(plan) % 3]
    ss.body_forced(factory, ss.run_of(entry, mode, k, "holes"), entry[1], plan, driver=drv)


# --- e. the index threshold ----------------------------------------------------------------------------------------

INDEX_ITEMS = [(rare, mode, k, plan, d) for rare in ss.INDEX_RARE for mode, k in (("push", 1), ("pushpull", 2))
               for plan in ("sparse", "sparse_alld") for d in ("lockstep", "group")]


@pytest.mark.parametrize("rare,mode,k,plan,driver", INDEX_ITEMS, ids=["-".join(str(x) for x in it) for it in INDEX_ITEMS])
def test_index_edge(rare, mode, k, plan, driver):
    """The global rare count on either side of kSmallIndex in round 0; the push run goes above it, flips
    the majority and comes back under it with not-full as the rare class."""
    factory, drv = DRIVERS[driver]
    ss.body_forced(factory, ss.index_run(rare, mode, k), ss.INDEX_G, plan, driver=drv)


@pytest.mark.parametrize("rare", ss.INDEX_RARE)
def test_index_edge_full_majority_twin(rare):
    """Every node but 3 i holds the rumor: not-full is the rare class from round 0, on either side of
    kSmallIndex."""
    ss.body_forced(Engine, ss.index_run(rare, "push", 1, complement=True), ss.INDEX_G, "sparse")


# --- f. image_base: multi-word shards and GOSSIP_FLAG_TOPO_PEERS at the tiny entries ----------------------------------

multiword_reference = functools.lru_cache(maxsize=None)(functools.partial(ss.multiword_reference, op.OracleEngine))


@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("entry", ss.TINY_ENTRIES, ids=ids(ss.TINY_ENTRIES))
def test_multiword(entry, driver):
    factory, drv = DRIVERS[driver]
    i = ss.SHARD_SIZES.index(entry)
    for mode, k in (("push", 1 + i % 3), ("pull", 1 + (i + 1) % 3)):
        ss.body_multiword(factory, entry, mode, k, multiword_reference(ss.nodes_of(entry), mode, k), driver=drv)


@functools.lru_cache(maxsize=None)
def topo_reference(N, R, mode, k):
    x = tr.TopoSim(N, R, mode, k, SEED)
    ss.topo_run(x, N, R)
    res = x.step(ss.TOPO_ROUNDS)
    return res, x.read_shard()


@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("entry", ss.TINY_ENTRIES, ids=ids(ss.TINY_ENTRIES))
def test_topo_peers(entry, driver):
    Nl, G, _ = entry
    N = ss.nodes_of(entry)
    factory, drv = DRIVERS[driver]
    for mode, R, k in ss.topo_cases(entry):
        want, full = topo_reference(N, R, mode, k)
        infected = want.infected
        d = (drv or sc.LockstepDriver)(factory, N, R, mode, k, SEED, G, flags=FLAG_HASH | FLAG_TOPO_PEERS)
        try:
            for e in d.engines:
                ss.topo_run(e, N, R)
            for i, w in enumerate(want.stats):
                if drv is GroupDriver:      # (no planner over the topology: the plan string stays empty)
                    res = d.group.step(1)
                    got, kind = res.stats[0], DENSE
                    assert np.array_equal(res.infected[0], infected[i])
                else:
                    got, kind = d.round()
                assert got == w and kind == DENSE, (mode, R, k, i)
            for e in d.engines:
                assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi]), (mode, R, k)
        finally:
            d.close()


# --- g. ANTIENTROPY: Nl rounded up to whole 64-row blocks ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ae_reference(N, K, k):
    args, kw = ac.engine_args(K, k, n_nodes=N)
    o = op.OracleEngine(*args, **kw)
    r = ac.run(o)
    h = o.state_hash()
    o.close()
    return r, h


@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("N,G,K,k", ss.AE_ITEMS, ids=[f"N{i[0]}-G{i[1]}-K{i[2]}-k{i[3]}" for i in ss.AE_ITEMS])
def test_antientropy(N, G, K, k, driver):
    want, h = ae_reference(N, K, k)
    args, kw = ac.engine_args(K, k, n_nodes=N)
    if driver == "group":
        owner = Group(*args, n_shards=G, devices=[0] * G, transport=2, **kw)
        shards = owner.shards
    else:
        owner = None
        shards = [Engine(*args, shard_rank=r, shard_count=G, **kw) for r in range(G)]
    try:
        assert [e.hi - e.lo for e in shards] == ss.AE_SHARD_SIZES[(N, G)]
        got = ac.run(ss.AeShards(shards, owner))
        ac.assert_same(got, want)
        assert got.stats[-1]["state_hash"] == h
    finally:
        if owner:
            owner.close()
        else:
            sc.close_all(shards)
