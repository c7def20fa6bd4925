"""GPU: push-pull rumor mongering (GOSSIP_FLAG_MONGER_PUSHPULL) against the numpy
restatement tests/monger_pushpull_ref.py, bit for bit: per round full_nodes, messages, converged, the
per-rumor counts and the state hash, and at the end the known and the hot bitsets, the count of every
node and rumor, the number of hot nodes and the round index.  tests/test_monger_pushpull_ref.py ties
that restatement to the C oracle, to topo_ref.TopoSim, to invariants and to closed forms.

The shapes: below a wave, a wave, a block and a bitmap word (sizes.TINY), many blocks with a ragged
last wave (30011 nodes), hub rows beside empty rows, every fanout class (one batch of four, a second
and a third), one and three words per node, and more nodes than one launch has lanes (2^21 + 4099).
Every instantiation of the request kernel (one word / several x uniform / row peers, each with
feedback and blind) must have, in a compared round, cooled bits, bits counted and kept hot, a node
that gained and lost hot bits in one word, lost exchanges, an exchange in which both ends gained from
each other, and feedback that reached a node as initiator only and as target only; with feedback also
counts reset from above 0 and rumors with a needed and a needless exchange in one round.
test_guards_are_not_vacuous shows it from the restatement alone."""
import functools

import numpy as np
import pytest

import monger_counter_ref as mc
import monger_pull_ref as mp
import monger_pushpull_ref as mpp
import oracle_py as op
import sizes as sz
import topologies as tp
from gossip_hip import (FLAG_DIRECT, FLAG_HASH, FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER_PUSHPULL, FLAG_TOPO_PEERS,
                        Engine, loss_threshold)
from gossip_hip.engine import GossipError

pytestmark = pytest.mark.gpu
N = 30011
NMID = 3001
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 nodes: the last 4099 are a second trip
ALWAYS = 2 ** 32 - 1
LOSS = loss_threshold(0.3)
CAP = 40                  # compared rounds: a limit of 15 and three partitions run on past it
RANDOM = "inject_random"


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":      # hub rows of 300, empty rows, self-loops, repeated entries
        return tp.ragged(N, 7)
    if name == "mid_ragged":
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID, every=2)
    if name == "mid_banded":
        return tp.banded(NMID, 7, hub_every=1024, hub_deg=40)
    raise KeyError(name)


def injects(name, R, n=N):
    """Every rumor somewhere and one at the last node; over a topology also one at a hub and one at
    a node with an empty row (it starts no exchange, and takes part in those of whoever lists it)."""
    out = [((431 * i) % n, i) for i in range(R)] + [(n - 1, R - 1)]
    if name != "uniform":
        deg = np.diff(topo(name)[0].astype(np.int64))
        out += [(int(np.argmax(deg)), 0), (int(np.nonzero(deg == 0)[0][3]), R // 2)]
    return tuple(out)


def make(kind, name, n, R, k, seed, faults=(), topology=None, extra=0):
    """The engine or the restatement of one case, its topology set."""
    rows = name != "uniform"
    if kind == "gpu":
        x = Engine(n, R, "pushpull", k, seed,
                   flags=FLAG_HASH | FLAG_MONGER_PUSHPULL | (FLAG_TOPO_PEERS if rows else 0) | extra, **dict(faults))
    else:
        x = mpp.MongerPushPullSim(n, R, k, seed, topo_peers=rows, **dict(faults))
    if rows:
        x.set_topology(topology if topology is not None else topo(name))
    return x


def start(x, inj):
    if inj == RANDOM:
        x.inject_random()
    else:
        for n, r in inj:
            x.inject(n, r)


def end_state(x):
    return x.read_shard(), x.read_hot(), x.read_counts(), x.hot_nodes(), x.round_index


def run(x, inj, cool, blind, limit, rounds):
    x.set_monger(cool, blind)
    if limit is not None:
        x.set_monger_limit(limit)
    start(x, inj)
    return (x.step(rounds),) + end_state(x)


@functools.lru_cache(maxsize=None)
def ref(name, R, k, cool, blind, limit, seed, faults=(), inj=None):
    """The restatement's run of a case, computed once per session."""
    return run(make("ref", name, N, R, k, seed, faults), inj or injects(name, R), cool, blind, limit, CAP)


def gpu(name, R, k, cool, blind, limit, seed, faults=(), inj=None):
    with make("gpu", name, N, R, k, seed, faults) as e:
        return run(e, inj or injects(name, R), cool, blind, limit, CAP)


def same(got, want):
    (a, sa, ha, ca, na, ta), (b, sb, hb, cb, nb, tb) = got, want
    assert a.rounds == b.rounds and ta == tb
    for x, y in zip(a.stats, b.stats):
        assert x == y
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)
    assert np.array_equal(ha, hb)
    assert ca.dtype == np.uint8 and ca.shape == cb.shape and np.array_equal(ca, cb)
    assert na == nb == int((hb != 0).any(axis=0).sum())


# --- the matrix: a covering set of peers x k x R x cool x limit x variant ---------------------------
# (name, R, k, cool, blind, limit, seed); limit None: never set, the engine holds no counters

MATRIX = [
    ("uniform", 3, 1, ALWAYS, False, 3, 301),
    ("uniform", 3, 2, 0.5, False, 2, 302),
    ("uniform", 3, 4, ALWAYS, True, 15, 303),
    ("uniform", 3, 9, 0.25, True, 3, 304),
    ("uniform", 3, 5, 0.5, True, None, 305),
    ("uniform", 130, 2, 0.25, True, 2, 306),
    ("uniform", 130, 5, ALWAYS, False, 3, 307),
    ("uniform", 130, 9, ALWAYS, False, 15, 308),
    ("uniform", 130, 1, 0.5, True, 3, 309),
    ("uniform", 130, 4, 0.5, False, None, 310),
    ("ragged", 3, 2, 0.5, True, 3, 311),
    ("ragged", 3, 5, 0.25, False, 2, 312),
    ("ragged", 3, 9, ALWAYS, False, 15, 313),
    ("ragged", 3, 4, ALWAYS, True, 2, 314),
    ("ragged", 3, 1, 0.5, False, None, 315),
    ("ragged", 130, 1, 0.5, False, 2, 316),
    ("ragged", 130, 4, 0.5, True, 3, 317),
    ("ragged", 130, 9, ALWAYS, True, 15, 318),
    ("ragged", 130, 2, ALWAYS, False, 3, 319),
    ("ragged", 130, 5, 0.25, True, 1, 320),
]
# loss 0.3, 3 partitions, both: one faulty case per instantiation
FAULTY = [
    ("uniform", 3, 2, 0.5, False, 2, 401, (("edge_loss", LOSS),)),
    ("uniform", 3, 5, 0.5, True, 3, 402, (("partitions", 3),)),
    ("uniform", 130, 4, 0.25, False, 2, 403, (("edge_loss", LOSS), ("partitions", 3))),
    ("uniform", 130, 2, 0.5, True, 15, 404, (("edge_loss", LOSS),)),
    ("ragged", 3, 4, 0.25, False, 3, 405, (("edge_loss", LOSS), ("partitions", 3))),
    ("ragged", 3, 2, 0.5, True, 2, 406, (("edge_loss", LOSS),)),
    ("ragged", 130, 5, 0.5, False, 2, 407, (("partitions", 3),)),
    ("ragged", 130, 5, 0.25, True, 3, 408, (("edge_loss", LOSS), ("partitions", 3))),
]


def case_id(c):
    cool = "always" if c[3] == ALWAYS else str(c[3])
    return f"{c[0]}-R{c[1]}-k{c[2]}-cool{cool}-{'blind' if c[4] else 'feedback'}-limit{c[5]}" + \
        ("-" + "+".join(f[0] for f in c[7]) if len(c) > 7 and c[7] else "")


def test_guards_are_not_vacuous():
    """From the restatement alone (no GPU involved): over the cases compared below, every kernel
    instantiation cools bits, counts bits that stay hot, clears and gains hot bits in one word of one
    node in one round, loses exchanges, has an exchange in which both ends gain, and gives feedback
    to nodes in one role alone; with feedback it also resets counts and sees rumors that one partner
    needed and another held in the same round."""
    seen = {}
    for c in MATRIX + FAULTY:
        res = ref(*c)[0]
        key = (c[1] <= 64, c[0] != "uniform", c[4])
        tot = seen.setdefault(key, dict.fromkeys(mpp.GUARDS, 0))
        for g in res.guards:
            for name in mpp.GUARDS:
                tot[name] += g[name]
    assert len(seen) == 8
    for key, tot in seen.items():
        for name in ("cooled", "kept", "gain_lose", "lost", "mutual", "init_only", "target_only") + \
                (() if key[2] else ("reset", "both")):
            assert tot[name] > 0, (key, name)
    # some runs end inside the compared rounds, with no node hot; the others go to the cap with hot nodes
    ended = [c for c in MATRIX if ref(*c)[0].rounds < CAP]
    assert len(ended) >= 4 and all(ref(*c)[4] == 0 for c in ended)
    assert all(ref(*c)[4] > 0 for c in MATRIX if c not in ended)
    assert {c[2] for c in MATRIX} == {1, 2, 4, 5, 9} and {c[3] for c in MATRIX} == {0.25, 0.5, ALWAYS}
    assert {c[5] for c in MATRIX} == {None, 1, 2, 3, 15} and {c[1] for c in MATRIX} == {3, 130}
    assert {c[4] for c in MATRIX} == {False, True}
    assert {c[7] for c in FAULTY} == {(("edge_loss", LOSS),), (("partitions", 3),), (("edge_loss", LOSS), ("partitions", 3))}


@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_matrix(case):
    want = ref(*case)
    assert want[0].stats[0]["messages"] > 0 and int(want[0].infected[-1].max()) > 1000
    assert sum(g["cooled"] for g in want[0].guards) > 0
    assert case[5] in (None, 1) or want[3].any()
    same(gpu(*case), want)


@pytest.mark.parametrize("case", FAULTY, ids=case_id)
def test_faults(case):
    want = ref(*case)
    assert sum(g["lost"] for g in want[0].guards) > 1000   # the faults change the run
    assert sum(g["cooled"] for g in want[0].guards) > 0
    same(gpu(*case), want)


# --- a wave, a block, a bitmap word --------------------------------------------------------------------

TINY_ITEMS = [(n, peers, R) for n in sz.TINY for peers in ("uniform", "rows") for R in (3, 130)]


@pytest.mark.parametrize("n,peers,R", TINY_ITEMS, ids=[f"{n}-{p}-R{R}" for n, p, R in TINY_ITEMS])
def test_tiny(n, peers, R):
    """sizes.TINY with sizes.tiny_topology: every third row empty, the hub row of node 0.  Five of the
    nine cases of the size: every rule, every k, and both variants (blind alternates along the picks)."""
    name = "uniform" if peers == "uniform" else "tiny"
    cases = [sz.monger_cases(n)[i] for i in (0, 1, 4, 5, 8)]
    assert {c[0] for c in cases} == set(sz.MONGER_RULES) and {c[1] for c in cases} == set(sz.MONGER_K)
    assert {c[3] for c in cases} == {False, True}
    for limit, k, cool, blind in cases:
        runs = []
        for kind in ("gpu", "ref"):
            x = make(kind, name, n, R, k, sz.SEED, topology=sz.tiny_topology(n))
            runs.append(run(x, sz.tiny_injects(n, R), cool, blind, limit, sz.CAP))
            if kind == "gpu":
                x.close()
        same(*runs)
        assert runs[1][0].rounds > 1


# --- more nodes than one launch has lanes ---------------------------------------------------------------

@pytest.mark.parametrize("R,rounds", [(3, 3), (70, 2)])
def test_past_one_grid(R, rounds):
    """2^21 + 4099 nodes at 8192 blocks of 256: the last 4099 are the second trip of the stride loops of
    both passes; they start exchanges, are drawn, gain, are counted and cool."""
    inj = tuple([((1021 * i) % NBIG, i % R) for i in range(4096)] + [(NBIG - 1, 1), (NBIG - 4099, 2)] +
                [(NBIG - 1 - 3 * i, i % R) for i in range(1, 600)])
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, "uniform", NBIG, R, 2, 11)
        runs.append(run(x, inj, ALWAYS, True, 2, rounds))
        if kind == "gpu":
            x.close()
    same(*runs)
    res, S, H, Cn, hot, _ = runs[1]
    assert res.rounds == rounds and hot > 0
    tail = Cn[:, 1 << 21:]    # the second trip holds counted, cooled and hot rumors (any number shows it ran)
    assert np.count_nonzero(tail == 1) > 0 and np.count_nonzero(tail >= 2) > 0
    assert np.count_nonzero(S[0, 1 << 21:] & ~H[0, 1 << 21:]) > 0 and np.count_nonzero(H[:, 1 << 21:]) > 0


# --- identity (item 9): cool = 0 is the unflagged PUSHPULL engine, here the C oracle itself ------------

@pytest.mark.parametrize("k,R,faults", [(2, 3, {}), (5, 70, dict(edge_loss=LOSS, partitions=3))])
def test_cool_zero_equals_the_oracle(k, R, faults):
    n = 1025
    inj = [((431 * i) % n, i) for i in range(R)]
    o = op.OracleEngine(n, R, "pushpull", k, 77, flags=1, **faults)
    for node, r in inj:
        o.inject(node, r)
    want = [o.step(1) for _ in range(14)]   # (its step stops at converged: one round at a time)
    full = o.read_shard()
    o.close()
    assert any(w.stats[0]["converged"] for w in want) or faults
    with Engine(n, R, "pushpull", k, 77, flags=FLAG_HASH | FLAG_MONGER_PUSHPULL, **faults) as e:
        for node, r in inj:
            e.inject(node, r)
        got = e.step(14)                    # H == S for ever: to max_rounds, past converged
        assert got.rounds == 14 and e.round_index == 14
        for i, w in enumerate(want):
            assert dict(got.stats[i], messages=0) == w.stats[0]
            assert np.array_equal(got.infected[i], w.infected[0])
        assert got.stats[0]["messages"] > 0
        assert np.array_equal(e.read_shard(), full) and np.array_equal(e.read_hot(), full)
        assert e.hot_nodes() == int((full != 0).any(axis=0).sum()) and not e.read_counts().any()


# --- the ring closed form -------------------------------------------------------------

@pytest.mark.parametrize("blind", [False, True], ids=["feedback", "blind"])
def test_ring_closed_form(blind):
    n, m = 257, 2
    ring = (np.arange(n + 1, dtype=np.uint32), ((np.arange(n, dtype=np.int64) + 1) % n).astype(np.uint32))
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, "ring", n, 1, 1, 3, topology=ring)
        runs.append(run(x, [(0, 0)], ALWAYS, blind, m, 10 * n))
        if kind == "gpu":
            x.close()
    same(*runs)
    res = runs[0][0]
    assert res.rounds == (n - 1) // 2 + m and res.stats[-1]["full_nodes"] == n
    assert sum(s["messages"] for s in res.stats) == ((n - 1) * (m + 1) + m if blind else (n - 1) * (m + 2) + m - 2)


# --- state changes between steps ------------------------------------------------------------------------

def both(script, name, R, k, seed=0, **faults):
    """Runs script(x) -> list of step results on the GPU and on the restatement; everything equal."""
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, name, NMID, R, k, seed, tuple(faults.items()))
        steps = script(x)
        runs.append((steps,) + end_state(x))
        if kind == "gpu":
            x.close()
    assert len(runs[0][0]) == len(runs[1][0])
    for ra, rb in zip(runs[0][0], runs[1][0]):
        same((ra,) + runs[0][1:], (rb,) + runs[1][1:])
    return runs[1]


@pytest.mark.parametrize("R", [1, 130])
def test_a_zero_message_round_does_not_end_the_run(R):
    """Total loss: every exchange is lost, nothing moves, nothing cools and nothing is counted as a
    message; the hot node stays hot and the run goes to max_rounds."""
    def script(x):
        x.set_monger(ALWAYS, False)
        start(x, [(0, r) for r in range(R)])
        out = [x.step(6)]
        x.set_faults(0, 0)
        out.append(x.step(200))
        return out
    steps = both(script, "uniform", R, 1, seed=3, edge_loss=ALWAYS)[0]
    assert steps[0].rounds == 6 and all(s["messages"] == 0 for s in steps[0].stats)
    assert all(g["quiet"] == 1 for g in steps[0].guards)
    assert 5 < steps[1].rounds < 200 and int(steps[1].infected[-1].min()) > NMID // 2


def test_set_monger_between_steps():
    """cool 0 (plain PUSHPULL) -> feedback 1/2 -> blind 1/2: each takes effect in the next round."""
    def script(x):
        start(x, injects("mid_ragged", 70, NMID))
        out = [x.step(3)]
        x.set_monger(0.5, False)
        out.append(x.step(3))
        x.set_monger(0.5, True)
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 70, 2, seed=9)[0]
    assert sum(g["cooled"] for g in steps[0].guards) == 0 < sum(g["cooled"] for g in steps[1].guards)
    assert steps[2].stats[0]["round"] == 6


def test_limit_raised_and_lowered_between_steps():
    """limit 1 with no planes -> 3 (the planes appear mid-run: what cooled before reads 0) -> 15 -> 2 (hot
    rumors at or past 2 cool at their next counted round) -> 1 (still the counter kernel)."""
    seen = {"early": [], "high": []}

    def script(x):
        x.set_monger(0.5, True)
        start(x, injects("mid_ragged", 70, NMID))
        out = [x.step(3)]
        seen["early"].append((x.read_shard() & ~x.read_hot(), x.read_counts()))
        x.set_monger_limit(3)
        out.append(x.step(3))
        x.set_monger_limit(15)
        out.append(x.step(6))
        seen["high"].append(x.read_counts())
        x.set_monger_limit(2)
        out.append(x.step(2))
        x.set_monger_limit(1)
        out.append(x.step(CAP))
        return out
    steps, S, H, Cn, hot, _ = both(script, "mid_ragged", 70, 2, seed=9)
    (early_cooled, early_counts), high = seen["early"][1], seen["high"][1]
    assert np.array_equal(seen["early"][0][0], early_cooled) and np.array_equal(seen["high"][0], high)
    assert early_cooled.any() and not early_counts.any()
    assert (Cn[mpp.unpack(early_cooled, 70)] == 0).all()         # cooled before the planes: 0 for ever
    assert int(high.max()) > 3                                    # counted on past the old limit while hot
    assert sum(g["kept"] for g in steps[2].guards) > 0 and sum(g["cooled"] for g in steps[3].guards) > 0


def test_inject_into_a_quiescent_run():
    def script(x):
        x.set_monger(ALWAYS, False)
        x.set_monger_limit(3)
        start(x, [(0, 0), (NMID - 1, 1)])
        out = [x.step(200)]
        assert x.hot_nodes() == 0
        out.append(x.step(3))    # quiescent: one round, nobody hot before or after
        x.inject(0, 0)           # held and cooled: neither re-heated nor recounted
        out.append(x.step(3))
        x.inject(1500, 2)        # new: the run starts again, the counts of rumors 0 and 1 stay
        assert x.hot_nodes() == 1
        out.append(x.step(200))
        return out
    steps, S, H, Cn, hot, _ = both(script, "uniform", 3, 2, seed=9)
    assert steps[0].rounds < 200 and steps[1].rounds == 1 and steps[2].rounds == 1
    assert 3 < steps[3].rounds < 200 and int(steps[3].infected[-1][2]) > 1000 and hot == 0
    held = mpp.unpack(S, 3)
    assert (Cn[held] == 3).all() and not Cn[~held].any()


def test_inject_into_a_quiescent_run_several_words():
    """The bitmap of the hot nodes is rebuilt after an inject: rumor 129 alone restarts the run."""
    def script(x):
        x.set_monger(ALWAYS, False)
        start(x, [(0, 0), (NMID - 1, 70)])
        out = [x.step(200)]
        assert x.hot_nodes() == 0
        x.inject(1500, 129)
        out.append(x.step(200))
        return out
    steps, S, H, Cn, hot, _ = both(script, "uniform", 130, 2, seed=9)
    assert steps[0].rounds < 200 and 3 < steps[1].rounds < 200 and int(steps[1].infected[-1][129]) > 1000 and hot == 0


def test_reset_and_rerun():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]
    mid = []

    def script(x):
        x.set_monger(0.5, False)
        x.set_monger_limit(3)
        start(x, inj)
        out = [x.step(8)]
        assert x.read_counts().any() and x.hot_nodes() > 0
        x.reset()                # bitsets, counts and the round index; cool, blind, the limit and the rows stay
        mid.append((x.read_counts(), x.read_hot(), x.hot_nodes()))
        start(x, inj)
        out.append(x.step(200))
        return out
    steps = both(script, "mid_ragged", 70, 4, seed=9, edge_loss=LOSS)[0]
    assert len(mid) == 2 and all(not c.any() and not h.any() and n == 0 for c, h, n in mid)
    assert steps[1].stats[:8] == steps[0].stats
    assert sum(g["kept"] for g in steps[1].guards) > 0    # the limit is still 3


def test_new_topology_between_steps():
    def script(x):
        x.set_monger(0.5, False)
        x.set_monger_limit(2)
        start(x, [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(4)]
        x.set_topology(topo("mid_banded"))
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 3, 5, seed=9)[0]
    assert steps[1].stats[0]["round"] == 4 and steps[1].rounds > 1


def test_heal_partition_between_steps():
    def script(x):
        x.set_monger(0.0, False)
        start(x, [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(8)]
        x.set_faults(LOSS, 0)
        x.set_monger(0.5, False)
        out.append(x.step(200))
        return out
    steps = both(script, "uniform", 3, 2, seed=9, edge_loss=LOSS, partitions=3)[0]
    # behind the cuts a rumor reaches a third of the nodes; after the heal most of them
    assert int(steps[0].infected[-1].max()) <= NMID // 3 + 1 < int(steps[1].infected[-1].min())


# --- the stop rule -------------------------------------------------------------------------------------------

def test_step_stops_when_no_node_is_hot_not_at_converged():
    """k = 4, limit 3: everyone is full rounds before the last node loses interest.  The step returns
    with the first round that leaves no node hot, and the round index and the state are that round's."""
    want = run(make("ref", "uniform", NMID, 3, 4, 5), injects("uniform", 3, NMID), ALWAYS, False, 3, 200)
    conv = [s["converged"] for s in want[0].stats]
    assert 1 in conv and conv.index(1) < want[0].rounds - 2 and want[4] == 0 and want[0].rounds < 200
    with make("gpu", "uniform", NMID, 3, 4, 5) as e:
        got = run(e, injects("uniform", 3, NMID), ALWAYS, False, 3, 200)
        same(got, want)
        assert e.round_index == want[0].rounds and not e.read_hot().any()
        assert e.state_hash() == want[0].stats[-1]["state_hash"]
        again = e.step(200)      # nothing was enqueued ahead: one more round, the same state
        assert again.rounds == 1 and again.stats[0]["round"] == want[0].rounds
        assert again.stats[0]["messages"] == 0 and np.array_equal(e.read_shard(), want[1])


def test_quiescence_with_a_residue():
    """k = 1, blind, every coin holds, no counter: a node cools in the first round it takes part in an
    exchange, which is the round after it learnt the rumor; some nodes never hear it."""
    want = run(make("ref", "uniform", N, 1, 1, 6), [(0, 0)], ALWAYS, True, None, 200)
    assert want[0].rounds < 200 and want[4] == 0 and not want[0].stats[-1]["converged"]
    assert int(want[0].infected[-1][0]) < N
    with make("gpu", "uniform", N, 1, 1, 6) as e:
        same(run(e, [(0, 0)], ALWAYS, True, None, 200), want)


def test_max_rounds_ends_a_run_with_hot_nodes():
    want = run(make("ref", "uniform", N, 3, 2, 6), injects("uniform", 3), 0.25, False, 2, 5)
    assert want[0].rounds == 5 and want[4] > 1000 and want[5] == 5
    with make("gpu", "uniform", N, 3, 2, 6) as e:
        same(run(e, injects("uniform", 3), 0.25, False, 2, 5), want)


# --- engines without the flag --------------------------------------------------------------------------------

def test_unflagged_pushpull_engine_is_untouched():
    inj = [(0, 0), (N - 1, 1), (12345, 2)]
    o = op.OracleEngine(N, 3, "pushpull", 2, 4, flags=1)
    for n, r in inj:
        o.inject(n, r)
    want, full = o.step(12), o.read_shard()
    o.close()
    for flags in (FLAG_HASH, FLAG_HASH | FLAG_DIRECT):   # binned and direct
        with Engine(N, 3, "pushpull", 2, 4, flags=flags) as e:
            for n, r in inj:
                e.inject(n, r)
            for call in (lambda: e.set_monger(0.5), lambda: e.set_monger_limit(2), e.read_hot, e.read_counts,
                         e.hot_nodes):
                with pytest.raises(GossipError) as ei:
                    call()
                assert ei.value.code == -4   # GOSSIP_ESTATE
            got = e.step(12)
            assert got.stats == want.stats and np.array_equal(got.infected, want.infected)
            assert np.array_equal(e.read_shard(), full)


@pytest.mark.parametrize("flag,mode,sim", [(FLAG_MONGER, "push", mc.MongerCounterSim), (FLAG_MONGER_PULL, "pull", mp.MongerPullSim)],
                         ids=["bit8", "bit9"])
def test_the_other_mongering_engines_are_unchanged(flag, mode, sim):
    """GOSSIP_FLAG_MONGER and GOSSIP_FLAG_MONGER_PULL against their own restatements."""
    inj = injects("uniform", 3, NMID)
    m = sim(NMID, 3, 2, 4)
    m.set_monger(0.5, False)
    m.set_monger_limit(2)
    start(m, inj)
    want = m.step(6)
    with Engine(NMID, 3, mode, 2, 4, flags=FLAG_HASH | flag) as e:
        e.set_monger(0.5, False)
        e.set_monger_limit(2)
        start(e, inj)
        got = e.step(6)
        assert got.stats == want.stats and np.array_equal(got.infected, want.infected)
        assert np.array_equal(e.read_shard(), m.S) and np.array_equal(e.read_hot(), m.H)
        assert np.array_equal(e.read_counts(), m.C)
        assert e.hot_nodes() == int((m.H != 0).any(axis=0).sum()) > 0


def test_direct_dense_and_timing_change_nothing():
    want = run(make("ref", "uniform", NMID, 3, 2, 8), injects("uniform", 3, NMID), 0.5, False, 2, 200)
    with make("gpu", "uniform", NMID, 3, 2, 8, extra=FLAG_DIRECT | 1 << 3 | 1 << 1) as e:
        same(run(e, injects("uniform", 3, NMID), 0.5, False, 2, 200), want)
        ms, launches = e.kernel_time(0)
        assert launches == want[0].rounds and ms > 0
