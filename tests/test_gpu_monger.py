"""GPU: rumor mongering (GOSSIP_FLAG_MONGER) against the numpy restatement
tests/monger_ref.py, bit for bit: per round full_nodes, messages, converged, the per-rumor counts
and the state hash, and at the end the known and the hot bitsets and the round index.
tests/test_monger_ref.py ties that restatement to the C oracle, to topo_ref and to closed forms.

The sizes are those at which the kernel can go wrong: many blocks and a ragged last wave (30011
nodes), hub rows of 300 entries beside empty rows, self-loops and repeated entries, every fanout
class (the unrolled block of four, a second and a third Philox block), one and three words per
node with a ragged last word, and more senders than one launch has lanes (2^21 + 4099).  Every
kernel instantiation (one word / several x uniform / row peers x feedback / blind) must have
cooled bits, pushed what the peer held, cleared and gained hot bits in one word of one node in one
round, and lost attempts: test_guards_are_not_vacuous shows it from the restatement alone."""
import functools

import numpy as np
import pytest

import monger_ref as mr
import oracle_py as op
import topologies as tp
from gossip_hip import FLAG_HASH, FLAG_MONGER, FLAG_TOPO_PEERS, Engine, loss_threshold
from gossip_hip.engine import GossipError

pytestmark = pytest.mark.gpu
N = 30011
NMID = 3001
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 senders: the last 4099 are a second trip
NFULL = 1025
ALWAYS = 2 ** 32 - 1
LOSS = loss_threshold(0.3)
CAP = 80                  # rounds: every case without faults is quiescent sooner


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":
        return tp.ragged(N, 7)
    if name == "ragged_half":   # hub rows of 300 and more, empty rows, self-loops, repeated entries
        return tp.symmetrize(*tp.ragged(N, 7), N, every=2)
    if name == "mid_ragged":
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID, every=2)
    if name == "mid_banded":
        return tp.banded(NMID, 7, hub_every=1024, hub_deg=40)
    raise KeyError(name)


def injects(name, R, n=N):
    """Every rumor somewhere and one at the last node; over a topology also one at a hub and one at
    a node with an empty row (it stays hot there and is never pushed)."""
    out = [((431 * i) % n, i) for i in range(R)] + [(n - 1, R - 1)]
    if name != "uniform":
        deg = np.diff(topo(name)[0].astype(np.int64))
        out += [(int(np.argmax(deg)), 0), (int(np.nonzero(deg == 0)[0][3]), R // 2)]
    return tuple(out)


def flags_of(name):
    return FLAG_HASH | FLAG_MONGER | (0 if name == "uniform" else FLAG_TOPO_PEERS)


def make(kind, name, n, R, k, seed, faults=()):
    """The engine or the restatement of one case, its topology set."""
    if kind == "gpu":
        x = Engine(n, R, "push", k, seed, flags=flags_of(name), **dict(faults))
    else:
        x = mr.MongerSim(n, R, k, seed, topo_peers=name != "uniform", **dict(faults))
    if name != "uniform":
        x.set_topology(topo(name))
    return x


def run(x, inj, cool, blind, rounds):
    x.set_monger(cool, blind)
    for n, r in inj:
        x.inject(n, r)
    res = x.step(rounds)
    return res, x.read_shard(), x.read_hot(), x.round_index


@functools.lru_cache(maxsize=None)
def ref(name, R, k, cool, blind, seed, faults=(), rounds=CAP):
    """The restatement's run of a case, computed once per session."""
    return run(make("ref", name, N, R, k, seed, faults), injects(name, R), cool, blind, rounds)


def gpu(name, R, k, cool, blind, seed, faults=(), rounds=CAP):
    with make("gpu", name, N, R, k, seed, faults) as e:
        return run(e, injects(name, R), cool, blind, rounds)


def same(got, want):
    (a, sa, ha, ta), (b, sb, hb, tb) = got, want
    assert a.rounds == b.rounds and ta == tb
    for x, y in zip(a.stats, b.stats):
        assert x == y
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)
    assert np.array_equal(ha, hb)


# --- the matrix: a covering set of peers x k x R x cool x variant ------------------------------------
# (name, R, k, cool, blind, seed): every k with both peer sources, every cool with both variants and
# both widths, every instantiation at least twice

MATRIX = [
    ("uniform", 3, 1, 0.5, False, 101),
    ("uniform", 3, 2, ALWAYS, False, 102),
    ("uniform", 3, 4, ALWAYS, True, 103),
    ("uniform", 3, 9, 0.25, True, 104),
    ("uniform", 130, 2, 0.25, True, 105),
    ("uniform", 130, 5, 0.5, False, 106),
    ("uniform", 130, 9, ALWAYS, True, 107),
    ("uniform", 130, 4, 0.25, False, 108),
    ("ragged", 3, 2, 0.5, True, 109),
    ("ragged", 130, 1, 0.5, False, 110),
    ("ragged", 130, 9, ALWAYS, False, 111),
    ("ragged", 3, 5, 0.25, False, 112),
    ("ragged_half", 3, 9, ALWAYS, True, 113),
    ("ragged_half", 3, 4, 0.5, False, 114),
    ("ragged_half", 130, 4, 0.5, True, 115),
    ("ragged_half", 130, 2, ALWAYS, False, 116),
    ("ragged_half", 130, 5, 0.25, True, 117),
]
# loss 0.3, 3 partitions, both: one faulty case per instantiation
FAULTY = [
    ("uniform", 3, 2, 0.5, False, 201, (("edge_loss", LOSS),)),
    ("uniform", 3, 5, 0.5, True, 202, (("partitions", 3),)),
    ("uniform", 130, 4, 0.25, False, 203, (("edge_loss", LOSS), ("partitions", 3))),
    ("uniform", 130, 2, 0.5, True, 204, (("edge_loss", LOSS),)),
    ("ragged_half", 3, 4, 0.25, False, 205, (("edge_loss", LOSS), ("partitions", 3))),
    ("ragged", 3, 2, 0.5, True, 206, (("edge_loss", LOSS),)),
    ("ragged_half", 130, 5, 0.5, False, 207, (("partitions", 3),)),
    ("ragged", 130, 5, 0.25, True, 208, (("edge_loss", LOSS), ("partitions", 3))),
]


def case_id(c):
    cool = "always" if c[3] == ALWAYS else str(c[3])
    return f"{c[0]}-R{c[1]}-k{c[2]}-cool{cool}-{'blind' if c[4] else 'feedback'}" + \
        ("-" + "+".join(f[0] for f in c[6]) if len(c) > 6 else "")


def test_guards_are_not_vacuous():
    """From the restatement alone (no GPU involved): over the cases compared below, every kernel
    instantiation cools bits, pushes rumors the peer held, clears and gains hot bits in one word of
    one node in one round, and loses attempts."""
    seen = {}
    for c in MATRIX + FAULTY:
        res = ref(*c)[0]
        # (under feedback a node whose row lies behind a cut is never answered and never cools: such
        # runs end at CAP)
        assert c in FAULTY or (res.rounds < CAP and res.stats[-1]["messages"] == 0), case_id(c)
        key = (c[1] <= 64, c[0] != "uniform", c[4])
        tot = seen.setdefault(key, dict.fromkeys(mr.GUARDS, 0))
        for g in res.guards:
            for name in mr.GUARDS:
                tot[name] += g[name]
    assert len(seen) == 8
    for key, tot in seen.items():
        for name in mr.GUARDS:
            assert tot[name] > 0, (key, name)
    assert {c[2] for c in MATRIX} == {1, 2, 4, 5, 9} and {c[3] for c in MATRIX} == {0.25, 0.5, ALWAYS}


@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_matrix(case):
    want = ref(*case)
    assert want[0].stats[0]["messages"] > 0 and int(want[0].infected[-1].max()) > 1000
    same(gpu(*case), want)


@pytest.mark.parametrize("case", FAULTY, ids=case_id)
def test_faults(case):
    want = ref(*case)
    clean = ref(*case[:6])   # the faults change the run
    assert [int(x) for x in want[0].infected[-1]] != [int(x) for x in clean[0].infected[-1]]
    same(gpu(*case), want)


# --- more senders than one launch has lanes -----------------------------------------------------------

def test_past_one_grid():
    """2^21 + 4099 senders at 8192 blocks of 256: the last 4099 are the stride loop's second trip; they
    push, are pushed to and cool."""
    inj = tuple([((1021 * i) % NBIG, i % 3) for i in range(4096)] + [(NBIG - 1, 1), (NBIG - 4099, 2)] +
                [(NBIG - 1 - 3 * i, i % 3) for i in range(1, 600)])
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, "uniform", NBIG, 3, 2, 11)
        runs.append(run(x, inj, 0.25, True, 5))
        if kind == "gpu":
            x.close()
    same(*runs)
    res, S, H, _ = runs[1]
    assert res.rounds == 5 and res.stats[0]["messages"] == 2 * len({n for n, _ in inj})
    tail_s, tail_h = S[0, 1 << 21:], H[0, 1 << 21:]
    assert np.count_nonzero(tail_s) > 1000 > len({n for n, _ in inj if n >= 1 << 21})
    assert np.count_nonzero(tail_s & ~tail_h) > 500 and sum(g["and_or"] for g in res.guards) > 1000


# --- identity: cool = 0 is the unflagged PUSH engine, here the C oracle itself ----------------------

@pytest.mark.parametrize("k,R,faults", [(2, 3, {}), (5, 70, dict(edge_loss=LOSS, partitions=3))])
def test_cool_zero_equals_the_oracle(k, R, faults):
    inj = [((431 * i) % NFULL, i) for i in range(R)]
    o = op.OracleEngine(NFULL, R, "push", k, 77, flags=1, **faults)
    for n, r in inj:
        o.inject(n, r)
    want = [o.step(1) for _ in range(20)]   # (its step stops at converged: one round at a time)
    full = o.read_shard()
    o.close()
    assert any(w.stats[0]["converged"] for w in want) or faults
    with Engine(NFULL, R, "push", k, 77, flags=FLAG_HASH | FLAG_MONGER, **faults) as e:
        for n, r in inj:
            e.inject(n, r)
        got = e.step(20)
        assert got.rounds == 20 and e.round_index == 20
        for i, w in enumerate(want):
            assert got.stats[i]["messages"] > 0 and w.stats[0]["messages"] == 0
            assert dict(got.stats[i], messages=0) == w.stats[0]
            assert np.array_equal(got.infected[i], w.infected[0])
        assert np.array_equal(e.read_shard(), full) and np.array_equal(e.read_hot(), full)


# --- state changes between steps ------------------------------------------------------------------------

def both(script, name, R, k, seed=0, **faults):
    """Runs script(x) -> list of step results on the GPU and on the restatement; everything equal."""
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, name, NMID, R, k, seed, tuple(faults.items()))
        steps = script(x)
        runs.append((steps, x.read_shard(), x.read_hot(), x.round_index))
        if kind == "gpu":
            x.close()
    (a, sa, ha, ta), (b, sb, hb, tb) = runs
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        same((ra, sa, ha, ta), (rb, sb, hb, tb))
    return b


def start(x, inj):
    for n, r in inj:
        x.inject(n, r)


def test_set_monger_between_steps():
    """cool 0 (plain PUSH) -> feedback 1/2 -> blind 1/2: each takes effect in the next round."""
    def script(x):
        start(x, injects("mid_ragged", 70, NMID))
        out = [x.step(4)]
        x.set_monger(0.5, False)
        out.append(x.step(3))
        x.set_monger(0.5, True)
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 70, 2, seed=9)
    assert sum(g["cooled"] for g in steps[0].guards) == 0 < sum(g["cooled"] for g in steps[1].guards)
    assert steps[2].stats[-1]["messages"] == 0 and steps[2].stats[0]["round"] == 7


def test_inject_into_a_quiescent_run():
    def script(x):
        x.set_monger(0.5, True)
        start(x, [(0, 0), (NMID - 1, 1)])
        out = [x.step(CAP)]
        out.append(x.step(3))    # quiescent: one round that sends nothing
        x.inject(0, 0)           # held and cooled: not re-heated
        out.append(x.step(3))
        x.inject(1500, 2)        # new: the run starts again
        out.append(x.step(CAP))
        return out
    steps = both(script, "uniform", 3, 2, seed=9)
    assert steps[0].stats[-1]["messages"] == 0 and steps[1].rounds == 1 and steps[2].rounds == 1
    assert steps[3].rounds > 3 and int(steps[3].infected[-1][2]) > 1000


def test_reset_and_rerun():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]

    def script(x):
        x.set_monger(0.25, False)
        start(x, inj)
        out = [x.step(5)]
        x.reset()                # both bitsets and the round index; cool, blind and the rows stay
        start(x, inj)
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 3, 4, seed=9, edge_loss=LOSS)
    assert steps[1].stats[:5] == steps[0].stats and steps[1].stats[-1]["messages"] == 0


def test_new_topology_between_steps():
    def script(x):
        x.set_monger(0.25, False)
        start(x, [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(4)]
        x.set_topology(topo("mid_banded"))
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 3, 5, seed=9)
    assert steps[1].stats[0]["round"] == 4 and steps[1].stats[-1]["messages"] == 0


def test_heal_partition_between_steps():
    def script(x):
        x.set_monger(0.0, False)
        start(x, [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(8)]
        x.set_faults(LOSS, 0)
        x.set_monger(0.5, False)
        out.append(x.step(CAP))
        return out
    steps = both(script, "uniform", 3, 2, seed=9, edge_loss=LOSS, partitions=3)
    # behind the cuts a rumor reaches a third of the nodes; after the heal nearly all
    assert int(steps[0].infected[-1].max()) <= NMID // 3 + 1 < int(steps[1].infected[-1].min())


# --- the stop rule -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ahead", [None, 1])
def test_step_stops_at_quiescence_not_at_converged(ahead):
    """k = 4, cool 1/8, feedback: everyone is full rounds before the last node loses interest.  The
    step returns with the first round that sends nothing, and the round index and the state are that
    round's, whatever `ahead` says."""
    want = run(mr.MongerSim(NFULL, 3, 4, 5), injects("uniform", 3, NFULL), 0.125, False, CAP)
    conv = [s["converged"] for s in want[0].stats]
    assert 1 in conv and conv.index(1) < want[0].rounds - 2
    assert [s["messages"] == 0 for s in want[0].stats] == [False] * (want[0].rounds - 1) + [True]
    with Engine(NFULL, 3, "push", 4, 5, flags=FLAG_HASH | FLAG_MONGER) as e:
        if ahead:
            e.set_param("ahead", ahead)
        got = run(e, injects("uniform", 3, NFULL), 0.125, False, CAP)
        same(got, want)
        assert e.round_index == want[0].rounds and not e.read_hot().any()
        assert e.state_hash() == want[0].stats[-1]["state_hash"]
        again = e.step(CAP)      # nothing was enqueued ahead: one more quiescent round, the same state
        assert again.rounds == 1 and again.stats[0]["round"] == want[0].rounds
        assert again.stats[0]["messages"] == 0 and np.array_equal(e.read_shard(), want[1])


def test_quiescence_with_a_residue():
    """k = 2, blind, every coin holds: each node pushes twice in the round after it hears a rumor and
    never again; about a fifth of the nodes (s = exp(-2 (1 - s))) never hear it."""
    want = run(mr.MongerSim(N, 3, 2, 6), injects("uniform", 3), ALWAYS, True, CAP)
    assert want[0].rounds < CAP and want[0].stats[-1]["messages"] == 0 and not want[0].stats[-1]["converged"]
    assert N // 2 < int(want[0].infected[-1].min()) and int(want[0].infected[-1].max()) < N - N // 10
    with Engine(N, 3, "push", 2, 6, flags=FLAG_HASH | FLAG_MONGER) as e:
        same(run(e, injects("uniform", 3), ALWAYS, True, CAP), want)


def test_max_rounds_ends_a_run_that_is_not_quiescent():
    with Engine(N, 3, "push", 2, 6, flags=FLAG_HASH | FLAG_MONGER) as e:
        got = run(e, injects("uniform", 3), 0.25, False, 5)
    want = run(mr.MongerSim(N, 3, 2, 6), injects("uniform", 3), 0.25, False, 5)
    assert want[0].rounds == 5 and want[0].stats[-1]["messages"] > 0 and want[3] == 5
    same(got, want)


# --- engines without the flag --------------------------------------------------------------------------------

def test_unflagged_engine_is_untouched():
    inj = [(0, 0), (N - 1, 1), (12345, 2)]
    o = op.OracleEngine(N, 3, "push", 2, 4, flags=1)
    for n, r in inj:
        o.inject(n, r)
    want, full = o.step(12), o.read_shard()
    o.close()
    for flags in (FLAG_HASH, FLAG_HASH | 1 << 2):   # binned and direct
        with Engine(N, 3, "push", 2, 4, flags=flags) as e:
            for n, r in inj:
                e.inject(n, r)
            for call in (lambda: e.set_monger(0.5), e.read_hot):
                with pytest.raises(GossipError) as ei:
                    call()
                assert ei.value.code == -4   # GOSSIP_ESTATE
            got = e.step(12)
            assert got.stats == want.stats and all(s["messages"] == 0 for s in got.stats)
            assert np.array_equal(got.infected, want.infected) and np.array_equal(e.read_shard(), full)


def test_set_monger_rejects_a_bad_variant():
    with Engine(NFULL, 3, "push", 2, 4, flags=FLAG_MONGER) as e:
        with pytest.raises(GossipError) as ei:
            e._check(e._fn("set_monger")(e._h, 1, 2))
        assert ei.value.code == -1   # GOSSIP_EINVAL
