"""CPU only: the tables of tests/monger_edges.py, and the preconditions test_gpu_monger_edges.py relies on,
shown on the restatements alone, so that no GPU case is vacuous.

The pull and the push-pull restatements are held to the C oracle at full-width seeds (cool = 0 is the
unflagged engine), a full-width seed gives another run than its low word alone and the coin itself reads
key1, and every table meets its guards: messages in round 0, cooled and kept bits, rumors with a needed
and a needless contact in one round, counts that climb 8, 9, .. 15 and cool there, lost edges at fanout 64,
gains and losses in one word at fanout 63, the last bit of a word and of the 64th word spreading, partition
counts at and past N freezing the run, loss 1 losing nothing and loss 2^32 - 2 everything, and a second step
that cools by draws at t >= 300 alone.  The GRID restatements take seconds each and are not run here:
test_gpu_monger_edges.py asserts their guards from the run it needs anyway."""
import numpy as np
import pytest

import monger_edges as me
import monger_pull_ref as mp
import monger_pushpull_ref as mpp
import monger_ref as mr
import numpy_ref as nr
import oracle_py as op
import values as va
from gossip_hip import loss_threshold as lt

A = va.A
FEEDBACK = ("pull", "pushpull")   # the engines whose restatements report reset, both and gain_lose


def ids(cases):
    return [me.case_id(c) for c in cases]


# --- the tables themselves ------------------------------------------------------------------------------

def test_tables_cover_what_they_claim():
    assert set(me.ENGINES) == {"push", "pull", "pushpull"}
    assert [me.ENGINES[e][1] for e in me.ENGINES] == list(me.ENGINES)
    assert me.ENGINES["push"][2].__name__ == "MongerCounterSim" and me.ENGINES["pull"][2] is mp.MongerPullSim
    assert me.ENGINES["pushpull"][2] is mpp.MongerPushPullSim
    for name, cases in me.TABLES.items():
        assert len(set(cases)) == len(cases) == len(set(ids(cases))) and all(c.table == name for c in cases)
    # SEEDS: every engine x every seed x {one word, several} and x {uniform, rows}, one batch of edges and two
    assert len(me.SEEDS) == 18
    assert {(c.engine, c.seed, c.R) for c in me.SEEDS} == {(e, s, R) for e in me.ENGINES for s in va.SEEDS for R in (3, 65)}
    assert {(c.engine, c.seed, c.peers) for c in me.SEEDS} == {(e, s, p) for e in me.ENGINES for s in va.SEEDS
                                                               for p in ("uniform", "rows")}
    assert {(c.engine, c.k) for c in me.SEEDS} == {(e, k) for e in me.ENGINES for k in (2, 5)}
    assert all(c.seed >> 32 and c.N == me.NMID and c.limit == 2 and not c.blind and c.faults == (("edge_loss", lt(0.2)),)
               for c in me.SEEDS)
    # MAXIMA: all four request instantiations of every engine, every shape over both kinds of peers
    assert {(c.engine, c.R <= 64, c.peers) for c in me.MAXIMA} == {(e, one, p) for e in me.ENGINES for one in (False, True)
                                                                   for p in ("uniform", "rows")}
    for e in me.ENGINES:
        for p in ("uniform", "rows"):
            mine = [c for c in me.MAXIMA if c.engine == e and c.peers == p]
            assert [(c.N, c.R, c.k, c.cool, c.blind, c.limit, c.faults, c.rounds) for c in mine] == me.MAX_SHAPES
        assert {c.seed for c in me.MAXIMA if c.engine == e} == set(va.SEEDS)
    assert {c.k for c in me.MAXIMA} == {2, 8, 61, 63, 64} and {c.R for c in me.MAXIMA} == {3, 64, 65, 4033, 4096}
    assert {c.limit for c in me.MAXIMA} == {2, 3, 15} and (257, 4096, 64) in {(c.N, c.R, c.k) for c in me.MAXIMA}
    assert {(c.k + 3) // 4 for c in me.MAXIMA} == {1, 2, 16} and {c.k % 4 for c in me.MAXIMA if c.k > 8} == {0, 1, 3}
    # GRID, PARTS, LOSS: the two engines of monger_close.h; LATE: all three
    assert [(c.N, c.R) for c in me.GRID if c.engine == "pull"] == [(2 ** 21 - 1, 65), (2 ** 21, 3), (2 ** 21 + 1, 65)]
    assert {c.engine for c in me.GRID} == set(FEEDBACK) and all(c.seed >> 32 and c.rounds == 2 and c.k == 2 for c in me.GRID)
    for e in FEEDBACK:
        assert [dict(c.faults)["partitions"] for c in me.PARTS if c.engine == e] == va.PARTS(me.NMID) == \
            [5, 7, 3000, 3001, 3002, 2 ** 31, 2 ** 32 - 1]
        assert [dict(c.faults)["edge_loss"] for c in me.LOSS if c.engine == e] == va.LOSS
    assert all(c.seed == va.PAIR_SEED[me.NMID] and {(0, 0), (1, 1)} <= set(me.injects(c)) for c in me.PARTS + me.LOSS)
    assert nr.peers(va.PAIR_SEED[me.NMID], me.NMID, 0, 2, nodes=[0])[0, 0] == 1
    assert [c.engine for c in me.LATE] == list(me.ENGINES) and me.LATE_ROUNDS == (300, 200)
    assert all(c.N == va.NLONG == 130 and c.R == 130 and c.seed >> 32 for c in me.LATE)


def test_injects_stay_in_range():
    for cases in me.TABLES.values():
        for c in cases:
            if c.table == "GRID" and c != me.GRID[-1]:
                continue                 # (one GRID case: its peers cost a Philox pass each)
            inj = me.injects(c)
            assert all(0 <= n < c.N and 0 <= r < c.R for n, r in inj)
            assert {r for _, r in inj} >= {0, c.R - 1}
    c = me.GRID[-1]
    near = me.grid_nodes(c.N)
    assert near == list(range(2 ** 21 - 64, 2 ** 21 + 1)) and me.grid_nodes(2 ** 21 - 1)[-1] == 2 ** 21 - 2
    assert me.grid_nodes(2 ** 21) == list(range(2 ** 21 - 64, 2 ** 21))
    held = {n: {r for m, r in me.injects(c) if m == n} for n in near}
    assert all(len(v) >= 2 and c.R - 1 not in v for v in held.values())


# --- the restatements against the C oracle at full-width seeds -------------------------------------------

@pytest.mark.parametrize("faults", [{}, dict(edge_loss=lt(0.2), partitions=3)], ids=["clean", "loss-parts"])
@pytest.mark.parametrize("engine", FEEDBACK)
@pytest.mark.parametrize("seed", va.SEEDS, ids=[f"{s:#x}" for s in va.SEEDS])
def test_cool_zero_is_the_oracle_at_full_width_seeds(seed, engine, faults):
    """cool = 0: H == S for ever, and S is the unflagged engine's, round by round; the messages differ by
    design."""
    N, R, k, rounds = 1025, 65 if faults else 3, 5 if faults else 2, 14
    inj = [((431 * i) % N, i) for i in range(R)]
    o = op.OracleEngine(N, R, engine, k, seed, flags=1, **faults)
    m = me.ENGINES[engine][2](N, R, k, seed, **faults)
    for n, r in inj:
        o.inject(n, r)
        m.inject(n, r)
    moved = 0
    for t in range(rounds):      # (the oracle's step would stop at converged: one round at a time)
        want = o.step(1)
        st, inf, g = m.round()
        assert np.array_equal(m.H, m.S) and g["cooled"] == 0
        assert dict(st, messages=0) == want.stats[0], t
        assert [int(x) for x in want.infected[0]] == [int(x) for x in inf], t
        moved += st["messages"]
    assert np.array_equal(o.read_shard(), m.S) and moved > 0
    o.close()


# --- key1 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", me.SEEDS, ids=ids(me.SEEDS))
def test_the_low_word_alone_gives_another_run(c):
    """Before anything saturates: the per-rumor counts after round 0, or the hot bitsets at the end."""
    full, low = me.ref(c), me.ref(c._replace(seed=c.seed & me.LOW))
    assert not np.array_equal(full.steps[0].infected[0], low.steps[0].infected[0]) or not np.array_equal(full.hot, low.hot)
    assert full.steps[0].stats[1]["state_hash"] != low.steps[0].stats[1]["state_hash"]


# what a coin that mishandles key1 is keyed with: (key0, 0) is the slip no seed below 2^32 shows (there it is
# the right key); (key0, key0) differs from the right key at every seed whose two words differ
WRONG_KEYS = {"dropped": lambda s: s & me.LOW, "key0-twice": lambda s: (s & me.LOW) * 0x100000001}
COIN_ITEMS = [(c, how) for c in me.SEEDS for how in WRONG_KEYS if WRONG_KEYS[how](c.seed) != c.seed]


@pytest.mark.parametrize("c,how", COIN_ITEMS, ids=[f"{how}-{me.case_id(c)}" for c, how in COIN_ITEMS])
def test_the_coin_itself_reads_key1(c, how, monkeypatch):
    """The same peers and losses under a coin with a wrong key: another hot bitset at the end of the compared
    rounds (other counts where the run ends with nobody hot), so a close pass that drops key1 or passes
    key0 twice cannot match.  (Under the all-ones seed the latter could: every seed is run under the former.)"""
    assert {x.seed for x, h in COIN_ITEMS if h == "dropped"} == set(va.SEEDS)
    want = me.ref(c)
    coin = mr.coin_word
    monkeypatch.setattr(mr, "coin_word", lambda seed, nodes, t, j: coin(WRONG_KEYS[how](seed), nodes, t, j))
    got = me.run(me.make_case("ref", c), c)
    assert got.steps[0].stats[0] == want.steps[0].stats[0]            # S_1 hangs on the peers alone
    assert not np.array_equal(got.hot, want.hot) or not np.array_equal(got.counts, want.counts)


# --- guards per table ----------------------------------------------------------------------------------------

def report(table, totals):
    """One line per table for the log (pytest -s): what the guards measured."""
    print(f"\n{table}: " + ", ".join(f"{k} {v}" for k, v in totals.items()))


def push_counts_past(c):
    """The PUSH cases in which nothing is counted and kept hot; the test pins kept == 0 there.  PUSH counts every
    edge of a round.  Blind under a coin that always holds, every hot rumor of a sender is counted k times, and
    k >= limit: it cools in the round that first counts it.  The other case is measured, not derived: the joint
    corner over the rows of sizes.tiny_topology, where a sender's 64 edges (feedback, coin 1/2, limit 2) fall on
    its two neighbours, 32 each, so a rumor a neighbour holds is counted about 16 times and never once."""
    if c.engine != "push":
        return False
    return (c.blind and c.cool == me.ALWAYS and c.k >= c.limit) or (c.N, c.R, c.k, c.peers) == (me.NSMALL, 4096, 64, "rows")


@pytest.mark.parametrize("c", me.SEEDS + me.MAXIMA, ids=ids(me.SEEDS + me.MAXIMA))
def test_seeds_and_maxima_guards(c):
    """One case per id: the restatement's run of a MAXIMA case takes up to a few seconds (the tests below
    find it in the cache)."""
    res = me.ref(c)
    assert res.steps[0].stats[0]["messages"] > 0
    assert me.guard(res, "cooled") > 0
    assert c.limit > 1 and res.counts.any()
    if push_counts_past(c):
        assert me.guard(res, "kept") == 0
    else:
        assert me.guard(res, "kept") > 0
    if c.engine in FEEDBACK and not c.blind:
        assert me.guard(res, "both") > 0


@pytest.mark.parametrize("table", ["SEEDS", "MAXIMA"])
def test_seeds_and_maxima_totals(table):
    """Per engine every guard its restatement reports is met somewhere in the table."""
    totals = {}
    for c in me.TABLES[table]:
        res = me.ref(c)
        for name in res.steps[0].guards[0]:
            totals[(c.engine, name)] = totals.get((c.engine, name), 0) + me.guard(res, name)
    for e in me.ENGINES:
        for name in ("cooled", "kept", "lost") + (("reset", "both", "gain_lose") if e in FEEDBACK else ("carry", "and_or")):
            assert totals[(e, name)] > 0, (e, name)
    report(table, {f"{e}.{name}": v for (e, name), v in totals.items()})


@pytest.mark.parametrize("peers", ["uniform", "rows"])
@pytest.mark.parametrize("engine", list(me.ENGINES))
def test_maxima_counts_climb_to_15(engine, peers):
    """Over the two limit-15 cases of an engine and a kind of peers the end counts take every value from 8 to 15
    (every carry out of the three low planes is behind them), and rumors cool in the round their count goes
    14 -> 15.  PUSH under uniform peers is the exception: both runs end inside the compared rounds with every
    held rumor cooled, so every end count is 15 (pinned below); the climb is then shown by `climbed` alone, and
    the values below 15 by PUSH over the rows."""
    cases = [c for c in me.MAXIMA if c.engine == engine and c.limit == 15 and c.peers == peers]
    assert {(c.R, c.k) for c in cases} == {(4096, 2), (64, 8)} and len(cases) == 2
    values, climbed = set(), 0
    for c in cases:
        res = me.ref(c)
        values |= {int(v) for v in np.unique(res.counts)}
        assert len(res.climbed) == res.steps[0].rounds and sum(res.climbed) > 0, c
        climbed += sum(res.climbed)
        S, H, cooled = me.held(res, c.R)
        assert (res.counts[cooled] == 15).all() and (res.counts[H] < 15).all()
    if (engine, peers) == ("push", "uniform"):
        assert values == {15} and all(me.ref(c).hot_nodes == 0 and me.ref(c).steps[0].rounds < c.rounds for c in cases)
    else:
        assert values >= set(range(8, 16))
    if engine in FEEDBACK:
        assert sum(me.guard(me.ref(c), "reset") for c in cases) > 0
    report(f"MAXIMA limit 15 {engine} {peers}", dict(values=sorted(values), cooled_at_15=climbed))


def test_maxima_fanouts():
    totals = {}
    for c in me.MAXIMA:
        res = me.ref(c)
        rounds = res.steps[0].rounds
        if c.k == 64 and c.faults:          # sixteen full batches under loss 0.9
            assert me.guard(res, "lost") > 0 and rounds >= 8, c
            totals[f"{c.engine}.k64.lost"] = totals.get(f"{c.engine}.k64.lost", 0) + me.guard(res, "lost")
        elif c.k == 64:                     # the joint corner: the one-step-per-round engines go to the cap
            assert rounds == 8 if c.engine in FEEDBACK else rounds >= 3, c
        if c.k == 63:
            name = "gain_lose" if c.engine in FEEDBACK else "and_or"
            assert me.guard(res, name) > 0 and me.guard(res, "lost") > 0, c
            totals[f"{c.engine}.k63.{name}"] = totals.get(f"{c.engine}.k63.{name}", 0) + me.guard(res, name)
    report("MAXIMA fanouts", totals)


LAST_BITS = [c for c in me.MAXIMA if c.R in (64, 4033, 4096)]


@pytest.mark.parametrize("c", LAST_BITS, ids=ids(LAST_BITS))
def test_maxima_last_bits(c):
    res = me.ref(c)
    last = [int(x) for x in res.steps[0].infected[:, c.R - 1]]
    if c.R == 64:          # bit 63 of the one word
        assert last[-1] > 1000 and res.counts[63].any()
        report(f"MAXIMA last bit {me.case_id(c)}", dict(holders=last[-1]))
        return
    # the 64th word, one bit of it (R = 4033) and all of it.  One round replayed: word 63 of the hot bitset is not
    # zero after round 0, and rumor R - 1 is hot at more nodes than it was injected at (2), at 4 and more in every case
    start = len({n for n, r in me.injects(c) if r == c.R - 1})
    hot = me.hot_after_round_0(c)
    hot_last = int(((hot[63] >> np.uint64((c.R - 1) % 64)) & np.uint64(1)).sum())
    assert hot.shape[0] == 64 and hot[63].any() and start == 2 and hot_last >= 4 and last[0] >= hot_last
    # it spreads to most nodes, but for PULL over the 257-node ring of sizes.tiny_topology (the nodes n % 3 == 2 ask
    # nobody and cut it): there the holders of round 0, twice the injected ones, are the measured floor
    ring_pull = c.engine == "pull" and c.peers == "rows" and c.N == me.NSMALL
    assert last[-1] >= (4 if ring_pull else c.N // 2 + 1), last[-1]
    report(f"MAXIMA last bit {me.case_id(c)}", dict(injected=start, round0=last[0], hot_round0=hot_last, end=last[-1]))


def test_parts_guards():
    totals = {}
    for c in me.PARTS:
        res, P = me.ref(c), dict(c.faults)["partitions"]
        st = res.steps[0]
        assert st.rounds == 12 and me.guard(res, "lost") > 0
        if P < c.N - 1:
            assert st.stats[0]["messages"] > 1 and me.guard(res, "kept") > 0, c
        elif P == c.N - 1:      # the one block of two nodes: node 0 draws node 1 in round 0
            assert st.stats[0]["messages"] >= 1 and me.guard(res, "lost") == 12 * 2 * c.N - 1, c
        else:
            assert all(s["messages"] == 0 for s in st.stats) and me.guard(res, "quiet") == 12, c
            assert me.guard(res, "lost") == 12 * 2 * c.N and res.hot_nodes == len({n for n, _ in me.injects(c)})
        totals[f"{c.engine}.P{P}"] = sum(s["messages"] for s in st.stats)
    report("PARTS messages", totals)


def test_loss_guards():
    totals = {}
    for c in me.LOSS:
        res, loss = me.ref(c), dict(c.faults)["edge_loss"]
        st = res.steps[0]
        assert st.rounds == 12
        if loss == 1:
            assert me.guard(res, "lost") == 0 and me.guard(res, "cooled") > 0
        elif loss >= A - 1:     # every started exchange of the twelve rounds is lost: nothing moves or cools
            assert me.guard(res, "lost") == 12 * 2 * c.N and me.guard(res, "quiet") == 12
            assert me.guard(res, "cooled") == 0 and np.array_equal(res.hot, res.shard)
            assert res.hot_nodes == len({n for n, _ in me.injects(c)})
        else:
            assert 0.45 < me.guard(res, "lost") / (12 * 2 * c.N) < 0.55 and me.guard(res, "cooled") > 0
        totals[f"{c.engine}.loss{loss:#x}"] = me.guard(res, "lost")
    report("LOSS lost", totals)


@pytest.mark.parametrize("c", me.LATE, ids=ids(me.LATE))
def test_late_guards(c):
    res = me.ref(c)
    first, second = res.steps
    assert first.rounds == 300 and me.guard(res, "cooled", 0) == 0 and first.stats[-1]["round"] == 299
    assert second.stats[0]["round"] == 300 and me.guard(res, "cooled", 1) > 0 and me.guard(res, "kept", 1) > 0
    assert 3 <= second.rounds < 200 and res.hot_nodes == 0 and not res.hot.any()
    assert res.round_index == 300 + second.rounds and res.state_hash == second.stats[-1]["state_hash"]
    report(f"LATE {c.engine}", dict(rounds=second.rounds, cooled=me.guard(res, "cooled", 1)))
