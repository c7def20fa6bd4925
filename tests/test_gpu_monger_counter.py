"""GPU: rumor mongering with counters (gossip_set_monger_limit) against the numpy
restatement tests/monger_counter_ref.py, bit for bit: per round full_nodes, messages, converged, the
per-rumor counts and the state hash, and at the end the known and the hot bitsets, the count of every
node and rumor and the round index.  tests/test_monger_counter_ref.py ties that restatement to
monger_ref.MongerSim, to invariants and to closed forms.

The shapes are those of test_gpu_monger.py: many blocks and a ragged last wave (30011 nodes), hub
rows beside empty rows, every fanout class (one batch of four, a second and a third), one and three
words per node, and more senders than one launch has lanes (2^21 + 4099).  Every instantiation of
the counter kernel (one word / several x uniform / row peers x feedback / blind) must have cooled
bits, incremented bits it kept hot, increments that reached a plane above the lowest, and a node that
lost and gained hot bits in one word in one round; one case must carry out of the highest plane.
test_guards_are_not_vacuous shows it from the restatement alone."""
import functools

import numpy as np
import pytest

import monger_counter_ref as mc
import topologies as tp
from gossip_hip import FLAG_HASH, FLAG_MONGER, FLAG_TOPO_PEERS, Engine, _abi, loss_threshold
from gossip_hip.engine import GossipError

pytestmark = pytest.mark.gpu
N = 30011
NMID = 3001
NBIG = (1 << 21) + 4099   # 8192 blocks of 256 lanes cover 2^21 senders: the last 4099 are a second trip
ALWAYS = 2 ** 32 - 1
LOSS = loss_threshold(0.3)
CAP = 120                 # rounds: every case without faults is quiescent sooner
CAP_FAULTY = 40           # behind a cut a feedback sender is never answered: such runs end here
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
    a node with an empty row (it stays hot there and is never pushed)."""
    out = [((431 * i) % n, i) for i in range(R)] + [(n - 1, R - 1)]
    if name != "uniform":
        deg = np.diff(topo(name)[0].astype(np.int64))
        out += [(int(np.argmax(deg)), 0), (int(np.nonzero(deg == 0)[0][3]), R // 2)]
    return tuple(out)


def make(kind, name, n, R, k, seed, faults=()):
    """The engine or the restatement of one case, its topology set."""
    if kind == "gpu":
        x = Engine(n, R, "push", k, seed, flags=FLAG_HASH | FLAG_MONGER | (0 if name == "uniform" else FLAG_TOPO_PEERS),
                   **dict(faults))
    else:
        x = mc.MongerCounterSim(n, R, k, seed, topo_peers=name != "uniform", **dict(faults))
    if name != "uniform":
        x.set_topology(topo(name))
    return x


def start(x, inj):
    if inj == RANDOM:
        x.inject_random()
    else:
        for n, r in inj:
            x.inject(n, r)


def end_state(x):
    return x.read_shard(), x.read_hot(), x.read_counts(), x.round_index


def run(x, inj, cool, blind, limit, rounds):
    x.set_monger(cool, blind)
    if limit is not None:
        x.set_monger_limit(limit)
    start(x, inj)
    return (x.step(rounds),) + end_state(x)


@functools.lru_cache(maxsize=None)
def ref(name, R, k, cool, blind, limit, seed, faults=(), inj=None):
    """The restatement's run of a case, computed once per session."""
    return run(make("ref", name, N, R, k, seed, faults), inj or injects(name, R), cool, blind, limit,
               CAP_FAULTY if faults else CAP)


def gpu(name, R, k, cool, blind, limit, seed, faults=(), inj=None):
    with make("gpu", name, N, R, k, seed, faults) as e:
        return run(e, inj or injects(name, R), cool, blind, limit, CAP_FAULTY if faults else CAP)


def same(got, want):
    (a, sa, ha, ca, ta), (b, sb, hb, cb, tb) = got, want
    assert a.rounds == b.rounds and ta == tb
    for x, y in zip(a.stats, b.stats):
        assert x == y
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)
    assert np.array_equal(ha, hb)
    assert ca.dtype == np.uint8 and ca.shape == cb.shape and np.array_equal(ca, cb)


# --- the matrix: a covering set of peers x k x R x cool x limit x variant ---------------------------
# (name, R, k, cool, blind, limit, seed): every k with both peer sources and both widths' classes,
# every cool and every limit with both variants, every instantiation at least twice

MATRIX = [
    ("uniform", 3, 1, ALWAYS, False, 3, 301),
    ("uniform", 3, 2, 0.5, False, 2, 302),
    ("uniform", 3, 4, ALWAYS, True, 15, 303),
    ("uniform", 3, 9, 0.25, True, 3, 304),
    ("uniform", 3, 5, 0.5, True, 2, 305),
    ("uniform", 130, 2, 0.25, True, 2, 306),
    ("uniform", 130, 5, 0.5, False, 3, 307),
    ("uniform", 130, 9, ALWAYS, False, 15, 308),
    ("uniform", 130, 1, 0.5, True, 3, 309),
    ("ragged", 3, 2, 0.5, True, 3, 310),
    ("ragged", 3, 5, 0.25, False, 2, 311),
    ("ragged", 3, 9, ALWAYS, False, 15, 312),
    ("ragged", 3, 4, ALWAYS, True, 2, 313),
    ("ragged", 130, 1, 0.5, False, 2, 314),
    ("ragged", 130, 4, 0.5, True, 3, 315),
    ("ragged", 130, 9, ALWAYS, True, 15, 316),
    ("ragged", 130, 2, ALWAYS, False, 3, 317),
]
# the carry out of the highest plane: four counts per round on a hot rumor, 4 -> 8 -> 12 -> 16
SATURATING = ("uniform", 130, 4, ALWAYS, True, 15, 0x5EED0003, (), RANDOM)
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
    instantiation cools bits, increments bits that stay hot, changes a plane above the lowest, clears
    and gains hot bits in one word of one node in one round, and loses attempts; the saturating case
    passes 15."""
    seen = {}
    for c in MATRIX + [SATURATING] + FAULTY:
        res = ref(*c)[0]
        assert c in FAULTY or (res.rounds < CAP and res.stats[-1]["messages"] == 0), case_id(c)
        key = (c[1] <= 64, c[0] != "uniform", c[4])
        tot = seen.setdefault(key, dict.fromkeys(mc.GUARDS, 0))
        for g in res.guards:
            for name in mc.GUARDS:
                tot[name] += g[name]
    assert len(seen) == 8
    for key, tot in seen.items():
        for name in ("cooled", "kept", "carry", "and_or", "lost"):
            assert tot[name] > 0, (key, name)
    sat = ref(*SATURATING)
    assert sum(g["sat"] for g in sat[0].guards) > 1000000 and int(sat[3].max()) == 15
    assert {c[2] for c in MATRIX} == {1, 2, 4, 5, 9} and {c[3] for c in MATRIX} == {0.25, 0.5, ALWAYS}
    assert {c[5] for c in MATRIX} == {2, 3, 15} and {c[1] for c in MATRIX} == {3, 130}


@pytest.mark.parametrize("case", MATRIX + [SATURATING], ids=case_id)
def test_matrix(case):
    want = ref(*case)
    assert want[0].stats[0]["messages"] > 0 and int(want[0].infected[-1].max()) > 1000 and want[3].any()
    same(gpu(*case), want)


@pytest.mark.parametrize("case", FAULTY, ids=case_id)
def test_faults(case):
    want = ref(*case)
    assert sum(g["lost"] for g in want[0].guards) > 1000   # the faults change the run
    same(gpu(*case), want)


# --- more senders than one launch has lanes -----------------------------------------------------------

def test_past_one_grid():
    """2^21 + 4099 senders at 8192 blocks of 256: the last 4099 are the stride loop's second trip; they
    push, are counted, keep some rumors and cool others."""
    inj = tuple([((1021 * i) % NBIG, i % 3) for i in range(4096)] + [(NBIG - 1, 1), (NBIG - 4099, 2)] +
                [(NBIG - 1 - 3 * i, i % 3) for i in range(1, 600)])
    runs = []
    for kind in ("gpu", "ref"):
        x = make(kind, "uniform", NBIG, 3, 2, 11)
        runs.append(run(x, inj, 0.5, True, 2, 5))
        if kind == "gpu":
            x.close()
    same(*runs)
    res, S, H, Cn, _ = runs[1]
    assert res.rounds == 5 and res.stats[0]["messages"] == 2 * len({n for n, _ in inj})
    tail = Cn[:, 1 << 21:]
    assert np.count_nonzero(tail == 1) > 100 and np.count_nonzero(tail >= 2) > 100
    assert np.count_nonzero(S[0, 1 << 21:] & ~H[0, 1 << 21:]) > 100


# --- identity: limit 1 through the counter kernel is the kernel of §2.13 --------------------------------

@pytest.mark.parametrize("name,R,k,cool,blind,faults", [
    ("uniform", 3, 2, 0.5, False, ()),
    ("uniform", 130, 9, 0.25, True, ()),
    ("ragged", 130, 5, 0.5, True, (("edge_loss", LOSS), ("partitions", 3))),
    ("ragged", 3, 4, ALWAYS, False, ()),
])
def test_limit_one_through_the_counter_kernel(name, R, k, cool, blind, faults):
    """set_monger_limit(2) then (1) before the first round: the planes exist, so every round runs the
    counter kernel, and it must equal, per round and in S and H, an engine that never set a limit (held
    to monger_ref by test_gpu_monger.py).  Every cooled bit reads a count of at least 1, every other 0."""
    rounds = CAP_FAULTY if faults else CAP
    with make("gpu", name, N, R, k, 21, faults) as e:
        want = run(e, injects(name, R), cool, blind, None, rounds)
        assert not want[3].any()
    with make("gpu", name, N, R, k, 21, faults) as e:
        e.set_monger_limit(2)
        e.set_monger_limit(1)
        got = run(e, injects(name, R), cool, blind, None, rounds)
    assert want[0].rounds > 5 and (faults or want[0].stats[-1]["messages"] == 0)
    same(got[:3] + (want[3],) + got[4:], want)
    cooled = mc.unpack(got[1] & ~got[2], R)
    assert cooled.any() and np.array_equal(got[3] >= 1, cooled)


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


def test_limit_raised_and_lowered_between_steps():
    """limit 1 with no planes -> 3 (the planes appear mid-run: what cooled before reads 0) -> 15 -> 2 (hot
    rumors at or past 2 cool at their next counted contact) -> 1 (still the counter kernel)."""
    seen = {"early": [], "high": []}

    def script(x):
        x.set_monger(0.5, True)
        start(x, injects("mid_ragged", 70, NMID))
        out = [x.step(3)]
        seen["early"].append((x.read_shard() & ~x.read_hot(), x.read_counts()))
        x.set_monger_limit(3)
        out.append(x.step(3))
        x.set_monger_limit(15)
        out.append(x.step(4))
        seen["high"].append(x.read_counts())
        x.set_monger_limit(2)
        out.append(x.step(2))
        x.set_monger_limit(1)
        out.append(x.step(CAP))
        return out
    steps, S, H, Cn, _ = both(script, "mid_ragged", 70, 2, seed=9)
    (early_cooled, early_counts), high = seen["early"][1], seen["high"][1]
    assert np.array_equal(seen["early"][0][0], early_cooled) and np.array_equal(seen["high"][0], high)
    assert early_cooled.any() and not early_counts.any()
    assert (Cn[mc.unpack(early_cooled, 70)] == 0).all()          # cooled before the planes: 0 for ever
    assert int(high.max()) > 3                                    # counted on past the old limit while hot
    assert steps[-1].stats[-1]["messages"] == 0 and int(Cn.max()) > 3
    assert sum(g["kept"] for g in steps[2].guards) > 0 and sum(g["cooled"] for g in steps[3].guards) > 0


def test_inject_into_a_quiescent_run():
    def script(x):
        x.set_monger(ALWAYS, True)
        x.set_monger_limit(3)
        start(x, [(0, 0), (NMID - 1, 1)])
        out = [x.step(CAP)]
        out.append(x.step(3))    # quiescent: one round that sends nothing
        x.inject(0, 0)           # held and cooled: neither re-heated nor recounted
        out.append(x.step(3))
        x.inject(1500, 2)        # new: the run starts again, the counts of rumors 0 and 1 stay
        out.append(x.step(CAP))
        return out
    steps, S, H, Cn, _ = both(script, "uniform", 3, 2, seed=9)
    assert steps[0].stats[-1]["messages"] == 0 and steps[1].rounds == 1 and steps[2].rounds == 1
    assert steps[3].rounds > 3 and int(steps[3].infected[-1][2]) > 1000
    held = mc.unpack(S, 3)
    assert (Cn[held] >= 3).all() and (Cn[held] <= 4).all() and not Cn[~held].any()


def test_reset_and_rerun():
    inj = [(0, 0), (NMID - 1, 1), (1234, 2)]
    mid = []

    def script(x):
        x.set_monger(0.5, False)
        x.set_monger_limit(3)
        start(x, inj)
        out = [x.step(12)]
        assert x.read_counts().any()
        x.reset()                # bitsets, counts and the round index; cool, blind, the limit and the rows stay
        mid.append(x.read_counts())
        start(x, inj)
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 3, 4, seed=9, edge_loss=LOSS)[0]
    assert len(mid) == 2 and not mid[0].any() and not mid[1].any()
    assert steps[1].stats[:12] == steps[0].stats and steps[1].stats[-1]["messages"] == 0
    assert sum(g["kept"] for g in steps[1].guards) > 0    # the limit is still 3


def test_new_topology_between_steps():
    def script(x):
        x.set_monger(0.5, False)
        x.set_monger_limit(2)
        start(x, [(0, 0), (NMID - 1, 1), (1234, 2)])
        out = [x.step(6)]
        x.set_topology(topo("mid_banded"))
        out.append(x.step(CAP))
        return out
    steps = both(script, "mid_ragged", 3, 5, seed=9)[0]
    assert steps[1].stats[0]["round"] == 6 and steps[1].stats[-1]["messages"] == 0


# --- errors ----------------------------------------------------------------------------------------------------

def test_limit_out_of_range_is_refused_and_changes_nothing():
    want = run(mc.MongerCounterSim(NMID, 3, 2, 4), injects("uniform", 3, NMID), 0.5, True, 2, CAP)
    with Engine(NMID, 3, "push", 2, 4, flags=FLAG_HASH | FLAG_MONGER) as e:
        assert e.read_counts().shape == (3, NMID) and not e.read_counts().any()   # before any limit: zeros
        e.set_monger_limit(2)
        for bad in (0, 16, 2 ** 32 - 1):
            with pytest.raises(GossipError) as ei:
                e.set_monger_limit(bad)
            assert ei.value.code == -1   # GOSSIP_EINVAL
        with pytest.raises(GossipError) as ei:   # n_words must be 4 * W * Nl_owned
            e._check(e._fn("read_monger_counts")(e._h, np.zeros(4 * NMID, dtype=np.uint64).ctypes.data_as(_abi.U64P),
                                                 3 * NMID))
        assert ei.value.code == -1
        same(run(e, injects("uniform", 3, NMID), 0.5, True, None, CAP), want)   # the limit is still 2


def test_unflagged_engine_is_untouched():
    inj = [(0, 0), (N - 1, 1), (12345, 2)]
    runs = []
    for touch in (False, True):
        with Engine(N, 3, "push", 2, 4, flags=FLAG_HASH | 1 << 2) as e:
            for n, r in inj:
                e.inject(n, r)
            if touch:
                for call in (lambda: e.set_monger_limit(2), e.read_counts):
                    with pytest.raises(GossipError) as ei:
                        call()
                    assert ei.value.code == -4   # GOSSIP_ESTATE
            res = e.step(12)
            runs.append((res.stats, res.infected, e.read_shard()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert runs[0][0][-1]["full_nodes"] > 1000
