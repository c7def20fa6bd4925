"""CPU only: the tables and builders of tests/shard_sizes.py, and the preconditions
test_gpu_shard_sizes.py relies on, shown on oracle host shards, one oracle engine and the numpy
restatements alone, so that no GPU case is vacuous.

Oracle shards run every entry through the sharded round bodies (gossip_hip.sharded._round) on every
forced plan and equal one oracle engine: a disagreement here is an oracle bug.  The guards are taken
from shard_cases.ref_wire: round 0 of a sparse plan has a rare list on every rank and messages across
every shard edge in both directions, a sparse run sees both majorities, a class-coded run has a mixed
node in a ragged last bitmap word, round 0 of an exchange plan sends items to every owner.  Two more
came from mutants of the oracle's shard code: every entry's rare lists against numpy
in every round, and a PUSH run that pushes onto the last node of a shard from another shard."""
import functools

import numpy as np
import pytest

import ae_cases as ac
import oracle_py as op
import shard_cases as sc
import shard_sizes as ss
import sizes as sz
import topo_ref as tr
from gossip_hip.sharded import CLASSCODED, EXCHANGE, SPARSE
from states import SEED

IDS = [ss.entry_id(e) for e in ss.SHARD_SIZES]


def ids(entries):
    return [ss.entry_id(e) for e in entries]


# --- the tables themselves -------------------------------------------------------------------------

def test_rotation_is_the_table_of_the_units():
    units = (64, 256, 1024, 2048, 4096, 8192, 16384, 32768)
    assert ss.UNITS == units and [e[0] for e in ss.ROTATION] == [u + d for u in units for d in (-1, 0, 1)]
    assert [(ss.nodes_of(e), e[1]) for e in ss.ROTATION] == [
        (126, 2), (191, 3), (321, 5), (1020, 4), (511, 2), (769, 3), (5115, 5), (4095, 4), (2049, 2), (6141, 3),
        (10239, 5), (8193, 4), (8190, 2), (12287, 3), (20481, 5), (32764, 4), (16383, 2), (24577, 3), (81915, 5),
        (65535, 4), (32769, 2), (98301, 3), (163839, 5), (131073, 4)]
    assert ss.SHARD_SIZES[:24] == ss.ROTATION and (32768, 2, 0) in ss.EXTRA and (16384, 3, 0) in ss.EXTRA


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_entry_geometry(entry):
    """N = G Nl - short with ceil(N / G) = Nl: the last shard alone is short, by `short` nodes, and the
    oracle's shards own exactly that."""
    Nl, G, short = entry
    N = ss.nodes_of(entry)
    assert 0 <= short < G and -(-N // G) == Nl
    assert sc.shard_geometry(N, G) == (Nl, [r * Nl for r in range(G)], [Nl] * (G - 1) + [Nl - short])
    shards = [op.OracleEngine(N, 3, "push", 1, SEED, shard_rank=r, shard_count=G) for r in range(G)]
    assert [(e.lo, e.hi) for e in shards] == [(r * Nl, min(N, (r + 1) * Nl)) for r in range(G)]
    sc.close_all(shards)


def test_every_offset_has_a_full_and_a_short_last_shard():
    """Nl = u - 1, u and u + 1 each with a full last shard and with a short one, each kind at a bitmap
    word and at a tile of csrc/binned.hip; every G at every kind."""
    for d in (-1, 0, 1):
        at = [e for e in ss.SHARD_SIZES if any(e[0] == u + d for u in ss.UNITS)]
        for short in (False, True):
            units = {e[0] - d for e in at if bool(e[2]) == short}
            assert 64 in units and units & {4096, 8192, 16384}, (d, short, units)
    assert {e[1] for e in ss.SHARD_SIZES if e[2]} == {e[1] for e in ss.SHARD_SIZES if not e[2]} == {2, 3, 4, 5}
    # a ragged last word (nown % 64 != 0) with the earlier shards whole words, and the reverse
    assert any(e[0] % 64 == 0 and e[2] for e in ss.SHARD_SIZES)
    assert any(e[0] % 64 and (e[0] - e[2]) % 64 == 0 for e in ss.SHARD_SIZES)


def test_subsets():
    assert [e[0] for e in ss.WIRE_ENTRIES] == [63, 64, 65, 16383, 16384, 16385]
    assert [e[0] for e in ss.FAULT_ENTRIES] == [16383, 16385, 4095, 4097]
    assert sorted(ss.nodes_of(e) for e in ss.TINY_ENTRIES) == [126, 128, 187, 191, 260, 321, 511, 769, 1020]
    assert [(ss.nodes_of(e), e[1]) for e in ss.HOLES_ENTRIES] == [(12287, 3), (16384, 4)]
    assert all(ss.nodes_of(e) <= 32769 for e in ss.CAROUSEL_CPU) and len(ss.CAROUSEL_CPU) == 25


def test_forced_cases_rotate_modes_and_fanouts():
    for e in ss.SHARD_SIZES:
        cases = [ss.forced_case(e, p) for p in ss.GPU_PLANS]
        assert {m for m, _ in cases} == set(ss.MODES)
        assert {k for _, k in cases} == {1, 2, 3, 4}
        for plans in (("sparse", "sparse_alld"), ("exchange", "exchange_unfiltered")):
            assert len({ss.forced_case(e, p)[0] for p in plans}) == 2
        # both ts classes of own_regions on the binned all-gather plans
        ks = {ss.forced_case(e, p)[1] for p in ("dense", "classcoded", "replicated", "replicated_cc")}
        assert min(ks) <= 2 and max(ks) >= 3


# --- the builders ------------------------------------------------------------------------------------

def test_shard_nodes():
    assert ss.shard_nodes(126, 2) == [0, 61, 62, 63, 64, 124, 125]
    assert ss.shard_nodes(191, 3) == [0, 62, 63, 64, 65, 126, 127, 128, 129, 189, 190]
    for e in ss.SHARD_SIZES:
        Nl, G, _ = e
        N = ss.nodes_of(e)
        b = ss.shard_nodes(N, G)
        assert b == sorted(set(b)) and b[0] == 0 and b[-1] == N - 1 and len(b) <= 64
        assert set(sz.boundary_nodes(N)) <= set(b)
        for r in range(1, G):
            assert {r * Nl - 2, r * Nl - 1, r * Nl, r * Nl + 1} & set(range(N)) <= set(b)
        # every shard has a node of the set, also the shortest last one
        _, los, nown = sc.shard_geometry(N, G)
        assert all(any(lo <= x < lo + c for x in b) for lo, c in zip(los, nown))


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_shard_edges_puts_a_rumor_on_every_edge_node(entry):
    N, G = ss.nodes_of(entry), entry[1]
    o = op.OracleEngine(N, 3, "push", 1, SEED, flags=1)
    calls = ss.shard_edges(o, 3, G)
    w = o.read_shard()[0]
    b = ss.shard_nodes(N, G)
    assert calls == len(b) + 3 <= 67
    assert (w[b] != 0).all() and int(w[N - 1]) == 7 and int((w != 0).sum()) == len(b)
    o.close()


@pytest.mark.parametrize("entry", ss.HOLES_ENTRIES, ids=ids(ss.HOLES_ENTRIES))
def test_shard_holes_is_nearly_full_with_empty_edges(entry):
    N, G = ss.nodes_of(entry), entry[1]
    assert N <= 16385
    o = op.OracleEngine(N, 3, "push", 1, SEED, flags=1)
    calls = ss.shard_holes(o, 3, G)
    w = o.read_shard()[0]
    b = ss.shard_nodes(N, G)
    n = np.arange(N, dtype=np.uint64)
    want = np.where(n % 97 == 5, np.uint64(7) & ~(np.uint64(1) << (n % 3)), np.uint64(7))
    want[b] = 0
    assert np.array_equal(w, want) and calls == sum(bin(int(x)).count("1") for x in want) <= 49200
    assert sc.rare_is_not_full(w, N, 3)      # not-full is the rare class from round 0
    o.close()


# --- every entry on every forced plan: oracle shards against one oracle engine -----------------------------

def runs_of(entry, plan):
    """the three table runs, and whatever test_gpu_shard_sizes.py runs on this plan and its direct twin"""
    cases = list(ss.TABLE_RUNS) + [ss.forced_case(entry, p) for p in ss.GPU_PLANS if ss.DIRECT_PLANS.get(p, p) == plan]
    return [ss.run_of(entry, mode, k) for mode, k in dict.fromkeys(cases)]


@pytest.mark.parametrize("plan", list(ss.PLANS))
@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_forced_plan_equals_one_engine(entry, plan):
    """Converges within 64 rounds, every round of the forced kind (kind 5 or 7, then 6, when replicated)."""
    for run in runs_of(entry, plan):
        _, want = sc.reference(run)
        assert want[-1]["converged"] and len(want) <= 40, (run, len(want))
        kinds = ss.body_forced(op.OracleEngine, run, entry[1], plan)
        assert set(kinds) == {{"replicated": 5, "replicated_cc": 7}.get(plan, kinds[0]), kinds[-1]}
        assert kinds[-1] == {SPARSE: 1, 0: 0, CLASSCODED: 4, EXCHANGE: 3}.get(ss.PLANS[plan][1], 6)


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_edge_run_pushes_onto_the_last_node_of_a_shard(entry):
    """PUSH with fanout 1 on the sparse plan: some round sends a message from another shard to the last
    node of a shard (p + 1 a multiple of Nl) while it lacks what the sender holds, so an owner computed as
    (p + 1) / Nl loses a rumor there."""
    seed = ss.edge_seed(entry)
    assert ss.last_node_pushes(entry, *ss.EDGE_RUN, seed=seed)
    assert (seed != SEED) == (entry in ss.EDGE_SEED)
    assert not (entry in ss.EDGE_SEED and ss.last_node_pushes(entry, *ss.EDGE_RUN))      # SEED does not do there
    _, want = sc.reference(ss.run_of(entry, *ss.EDGE_RUN), seed)
    assert want[-1]["converged"] and len(want) <= 40
    ss.body_forced(op.OracleEngine, ss.run_of(entry, *ss.EDGE_RUN), entry[1], "sparse", seed=seed)


def crosses(groups, G):
    """the shard edges (q | q + 1) a set of (sender, owner) groups crosses upwards and downwards"""
    up = {q for s, o in groups for q in range(G - 1) if s <= q < o}
    down = {q for s, o in groups for q in range(G - 1) if o <= q < s}
    return up, down


# Round 0 from shard_edges has about 4 G + 30 holders; a pushing round sends k messages from each.  No
# entry needed pinning: every edge is crossed both ways on every one.
NOT_CROSSED = {}
# Round 0 of a filtered exchange plan in PULL drops the pulls from empty peers; what is left are the pulls
# that hit one of the holders, about 7 of 126 edges at fanout 1 on the two smallest G = 2 entries, and
# under SEED all of them hit shard 1.  The unfiltered plan sends to both owners there too.
FILTERED_OWNERS = {((63, 2, 0), "pull"): {1}, ((64, 2, 0), "pull"): {1}}


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_guards(entry):
    Nl, G, short = entry
    N = ss.nodes_of(entry)
    _, los, nown = sc.shard_geometry(N, G)
    fm = sc.full_mask(3)
    for mode, k in ss.TABLE_RUNS:
        run = ss.run_of(entry, mode, k)
        states, want = sc.reference(run)
        S0 = states[0]
        # sparse, round 0: a rare list on every rank; messages across every shard edge, both ways
        w = sc.ref_wire(SPARSE, S0, N, G, 3, mode, k, SEED, 0)
        assert min(w["rare_counts"]) > 0
        assert all(r != q for r, q in w["msgs"])
        if mode != "pull":
            up, down = crosses(w["msgs"], G)
            missing = (set(range(G - 1)) - up, set(range(G - 1)) - down)
            assert missing == NOT_CROSSED.get((entry, mode), (set(), set())), (mode, missing)
        else:
            assert not w["msgs"]
        # a sparse run: rounds of each majority
        maj = {sc.rare_is_not_full(S, N, 3) for S in states[:-1]}
        assert maj == {False, True}, mode
        # a class-coded run: a mixed node in the last bitmap word of a shard whose nown % 64 != 0
        ragged = [q for q in range(G) if nown[q] % 64]
        assert bool(ragged) == bool(Nl % 64 or short)
        if ragged:
            def last_word_mixed(S):
                return any(((x != 0) & (x != fm)).any() for q in ragged
                           for x in [S[los[q] + nown[q] // 64 * 64:los[q] + nown[q]]])
            assert any(last_word_mixed(S) for S in states[:-1]), mode
        # exchange, round 0: items to every owner
        x = sc.ref_wire(EXCHANGE, S0, N, G, 3, mode, k, SEED, 0)
        assert {q for _, q in x["items"]} == FILTERED_OWNERS.get((entry, mode), set(range(G))), mode
        x = sc.ref_wire(EXCHANGE, S0, N, G, 3, mode, k, SEED, 0, xd_filter_frac=1.0)
        assert {q for _, q in x["items"]} == set(range(G)), mode


@pytest.mark.parametrize("entry", ss.HOLES_ENTRIES, ids=ids(ss.HOLES_ENTRIES))
def test_holes_runs(entry):
    """Full-majority from round 0 on every plan the GPU file runs them on."""
    N, G = ss.nodes_of(entry), entry[1]
    for mode, k in ss.TABLE_RUNS:
        run = ss.run_of(entry, mode, k, "holes")
        states, want = sc.reference(run)
        assert want[-1]["converged"] and all(sc.rare_is_not_full(S, N, 3) for S in states[:-1])
        w = sc.ref_wire(SPARSE, states[0], N, G, 3, mode, k, SEED, 0)
        assert min(w["rare_counts"]) > 0 and sum(w["rare_counts"]) < N // 50
        for plan in ("sparse", "classcoded", "exchange", "replicated"):
            ss.body_forced(op.OracleEngine, run, G, plan)


@pytest.mark.parametrize("entry", ss.FAULT_ENTRIES, ids=ids(ss.FAULT_ENTRIES))
def test_fault_runs_lose_edges_that_matter(entry):
    run = ss.run_of(entry, "pushpull", 3, loss=ss.LOSS, parts=ss.PARTS)
    clean = ss.run_of(entry, "pushpull", 3)
    _, want = sc.reference(run)
    _, unfaulted = sc.reference(clean)
    assert want[-1]["converged"] and unfaulted[-1]["converged"] and 2 * len(unfaulted) < len(want) <= 24
    # edges lost in round 0 already
    assert want[0] != unfaulted[0] and want[0]["full_nodes"] <= unfaulted[0]["full_nodes"]
    for plan in ("dense", "exchange", "sparse"):
        ss.body_forced(op.OracleEngine, run, entry[1], plan)


# --- the carousel and the wire ---------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("entry", ss.CAROUSEL_CPU, ids=ids(ss.CAROUSEL_CPU))
def test_carousel_equals_one_engine(entry, offset):
    mode, k = ss.carousel_case(entry)
    ss.body_carousel(op.OracleEngine, ss.run_of(entry, mode, k), entry[1], offset)


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_carousel_runs_reach_every_kind(entry):
    mode, k = ss.carousel_case(entry)
    _, want = sc.reference(ss.run_of(entry, mode, k))
    assert want[-1]["converged"]
    seen = set()
    for offset in (0, 3, 5):
        seen |= set(sc.expected_kinds(sc.SLOTS, offset, len(want)))
    assert seen == sc.ALL_KINDS


@pytest.mark.parametrize("entry", ss.SHARD_SIZES, ids=IDS)
def test_sparse_wire_equals_numpy(entry):
    """The rare lists of every rank in every round of the PULL run (rounds of both majorities: test_guards),
    on every entry: a last shard that lists not-full nodes past its end fails here alone."""
    ss.body_sparse_wire(op.OracleEngine, ss.run_of(entry, *ss.TABLE_RUNS[1]), entry[1])


@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("entry", ss.WIRE_ENTRIES, ids=ids(ss.WIRE_ENTRIES))
def test_carousel_wire_equals_numpy(entry, offset):
    mode, k = ss.carousel_case(entry)
    sc.body_carousel_wire(op.OracleEngine, ss.run_of(entry, mode, k), entry[1], offset)


# --- the index threshold ----------------------------------------------------------------------------------

def planner_rare(S):
    """the rare count plan_choose_sparse sees: min(not full, nonzero) over all shards"""
    return min(int((S != 1).sum()), int((S != 0).sum()))


@pytest.mark.parametrize("rare", ss.INDEX_RARE)
def test_index_edge_states(rare):
    assert ss.INDEX_N == 196611 and ss.INDEX_RARE == (ss.K_SMALL_INDEX, ss.K_SMALL_INDEX + 1)
    push, pushpull = ss.index_run(rare, "push", 1), ss.index_run(rare, "pushpull", 2)
    states, want = sc.reference(push)
    assert int((states[0] != 0).sum()) == rare and planner_rare(states[0]) == rare
    # every shard holds rare nodes
    _, los, nown = sc.shard_geometry(ss.INDEX_N, ss.INDEX_G)
    assert all(states[0][lo:lo + c].any() for lo, c in zip(los, nown))
    counts = [planner_rare(S) for S in states[:-1]]
    assert want[-1]["converged"] and len(want) == 15
    assert counts[1] > ss.K_SMALL_INDEX and any(c <= ss.K_SMALL_INDEX for c in counts[2:])
    assert {sc.rare_is_not_full(S, ss.INDEX_N, 1) for S in states[:-1]} == {False, True}
    assert len(sc.reference(pushpull)[1]) == 3
    for plan in ("sparse", "sparse_alld"):
        ss.body_forced(op.OracleEngine, push, ss.INDEX_G, plan)
        ss.body_forced(op.OracleEngine, pushpull, ss.INDEX_G, plan)


@pytest.mark.parametrize("rare", ss.INDEX_RARE)
def test_index_edge_full_majority_twin(rare):
    run = ss.index_run(rare, "push", 1, complement=True)
    states, want = sc.reference(run)
    assert int((states[0] == 0).sum()) == rare == planner_rare(states[0])
    assert sc.rare_is_not_full(states[0], ss.INDEX_N, 1) and want[-1]["converged"]
    ss.body_forced(op.OracleEngine, run, ss.INDEX_G, "sparse")


# --- multi-word and topology shards at the tiny entries ---------------------------------------------------

@pytest.mark.parametrize("entry", ss.TINY_ENTRIES, ids=ids(ss.TINY_ENTRIES))
def test_multiword_shards_equal_one_engine(entry):
    i = ss.SHARD_SIZES.index(entry)
    for mode, k in (("push", 1 + i % 3), ("pull", 1 + (i + 1) % 3)):
        want = ss.multiword_reference(op.OracleEngine, ss.nodes_of(entry), mode, k)
        assert want[0][-1]["converged"] and len(want[0]) > 2
        ss.body_multiword(op.OracleEngine, entry, mode, k, want)


@pytest.mark.parametrize("entry", ss.TINY_ENTRIES, ids=ids(ss.TINY_ENTRIES))
def test_topo_cases_move_rumors(entry):
    N = ss.nodes_of(entry)
    for mode, R, k in ss.topo_cases(entry):
        x = tr.TopoSim(N, R, mode, k, SEED, topology=sz.tiny_topology(N))
        for n, r in sz.tiny_injects(N, R):
            x.inject(n, r)
        before = int(np.count_nonzero(x.read_shard()))
        res = x.step(ss.TOPO_ROUNDS)
        assert res.stats[0]["messages"] > 0 and int(np.count_nonzero(x.read_shard())) > before


# --- ANTIENTROPY ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ae_reference(N, K, k):
    args, kw = ac.engine_args(K, k, n_nodes=N)
    o = op.OracleEngine(*args, **kw)
    r = ac.run(o)
    h = o.state_hash()
    o.close()
    return r, h


def test_ae_table():
    assert list(ss.AE_SHARD_SIZES) == [(127, 2), (128, 2), (129, 2), (129, 3), (257, 3), (511, 2), (512, 2), (513, 2),
                                       (4097, 2), (8192, 2), (12289, 3)]
    for (N, G), owned in ss.AE_SHARD_SIZES.items():
        Nl = -(-(-(-N // G)) // 64) * 64      # ceil(N / G) rounded up to whole 64-row blocks
        assert owned == [max(0, min(N, (r + 1) * Nl) - r * Nl) for r in range(G)] and sum(owned) == N
    assert {tuple(ss.ae_pairs(N, G)[:1]) for N, G in ss.AE_SHARD_SIZES} == {(p,) for p in sz.AE_PAIRS}
    assert [(N, G) for N, G in ss.AE_SHARD_SIZES if len(ss.ae_pairs(N, G)) == 3] == [(128, 2), (512, 2), (8192, 2)]
    # nown on and off the 256-lane block of csrc/ae_sharded.hip, and a last shard of one row
    flat = [c for owned in ss.AE_SHARD_SIZES.values() for c in owned]
    assert {1, 63, 64, 255, 256, 4096} <= set(flat) and any(c % 256 for c in flat)


@pytest.mark.parametrize("N,G,K,k", ss.AE_ITEMS, ids=[f"N{i[0]}-G{i[1]}-K{i[2]}-k{i[3]}" for i in ss.AE_ITEMS])
def test_ae_shards_equal_one_engine(N, G, K, k):
    want, h = ae_reference(N, K, k)
    a, b, c = want.steps
    assert a <= 3 and b < 400 and c < 400 and want.stats[a + b - 1]["converged"] and want.stats[-1]["converged"]
    assert want.stats[-1]["state_hash"] == h
    args, kw = ac.engine_args(K, k, n_nodes=N)
    shards = [op.OracleEngine(*args, shard_rank=r, shard_count=G, **kw) for r in range(G)]
    try:
        assert [e.hi - e.lo for e in shards] == ss.AE_SHARD_SIZES[(N, G)]
        ac.assert_same(ac.run(ss.AeShards(shards)), want)
    finally:
        sc.close_all(shards)
