"""GPU: the full-majority pull shortcut (csrc/frontier.hip `frontier_fp_*`) against
the C oracle, round by round: per-round stats (with FLAG_HASH: the hash of every state), per-rumor
counts and the whole state.

`sparse_frac` = 1 sends every full-majority round of a pulling mode down the shortcut
(plan_choose_fullpull).  Which nodes a round leaves unresolved (not full, no full pulled peer on a
live edge) is computed here from the oracle's states with the peer draws of oracle/numpy_ref.py, so
that no case can pass without its scan pass having had edges to resolve.  Stall mode only adds lost
edges, so the set computed without it is a subset of the real one.
"""
import functools

import numpy as np
import pytest

import numpy_ref as nr
import oracle_py as op
import states as st
import topo_ref as tr
import topologies as tp
from gossip_hip import FLAG_HASH, FLAG_TIMING, FLAG_TOPO_PEERS, Engine, loss_threshold

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F12
N_SMALL = 4099                 # ragged last 64-node group, a fraction of a 32 K staging chunk
N_MID = 65536 + 67             # crosses the 64 K-node mark: several blocks, ragged everywhere
N_BIG = (1 << 21) + 4099       # 512 resolve blocks of 1024 lanes x 2 nodes cover 2^20: several trips and chunks per block
LOSS = loss_threshold(0.25)
MAX_ROUNDS = 40
FP = {"sparse_frac": 1.0}
# non-full nodes packed around the group (64), resolve-step (1024, 2048) and last-group boundaries
PACKED = [(0, 130), (960, 1090), (2040, 2056), (4030, N_SMALL)]


def full_mask(R):
    return np.uint64((1 << R) - 1) if R < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)


def lost_edges(N, loss, parts, n, p, t, j):
    return nr.edge_lost(SEED, N, loss, parts, n, p, t, j)


@functools.lru_cache(maxsize=None)
def built_words(kind, R, loss=0):
    """One u64 word per node of a hand-built N_SMALL state (read only)."""
    N = N_SMALL
    rng = np.random.default_rng(0xF012 + R)
    fm = full_mask(R)
    n = np.arange(N)
    one = np.uint64(1) << (n % R).astype(np.uint64)
    two = one | np.uint64(1) << ((n // 3) % R).astype(np.uint64)
    if kind == "none_full":        # 0 % full: nothing can be resolved
        return one
    if kind == "half":             # 50 % full
        return np.where(rng.random(N) < 0.5, fm, two)
    if kind == "bench81":          # the share the bench's last dense round starts from
        return np.where(rng.random(N) < 0.81, fm, two)
    if kind == "all_full":
        return np.full(N, fm)
    if kind == "packed":
        S = np.full(N, fm)
        for a, b in PACKED:
            S[a:b] = one[a:b]
        S[64] = 0  # and an empty node
        return S
    if kind == "all_but_one":      # the one node that is not full loses its only edge of round 0
        nodes = np.arange(N, dtype=np.int64)
        p = nr.peers(SEED, N, 0, 1).astype(np.int64)[:, 0]
        cand = np.flatnonzero(lost_edges(N, loss, 0, nodes, p, 0, 0))
        assert loss and cand.size
        S = np.full(N, fm)
        S[cand[cand.size // 2]] = fm & ~np.uint64(1 << (R - 1))
        return S
    raise KeyError(kind)


def inject_words(engine, S, R):
    for node in np.flatnonzero(S):
        w = int(S[node])
        for r in range(R):
            if (w >> r) & 1:
                engine.inject(int(node), r)


def unresolved(S, N, R, k, t, loss, parts):
    """nodes of S_t that are not full and have no full pulled peer on a live edge (without stalls);
    past 2^17 nodes that are not full, among the first 2^17 of them"""
    fm = full_mask(R)
    nonfull = np.flatnonzero(S != fm).astype(np.int64)[:1 << 17]
    if nonfull.size == 0:
        return 0
    p = nr.peers(SEED, N, t, k, nodes=nonfull).astype(np.int64)
    hit = np.zeros(nonfull.size, dtype=bool)
    for j in range(k):
        hit |= ~lost_edges(N, loss, parts, nonfull, p[:, j], t, j) & (S[p[:, j]] == fm)
    return int((~hit).sum())


class Ref:
    """One oracle run a round at a time: stats, counts, the state after every round (small sizes),
    and per round whether it starts full-majority and how many nodes it leaves unresolved."""

    def __init__(self, work, N, mode, k, R, loss, parts, stall, keep_states, script=()):
        o = op.OracleEngine(N, R, mode, k, SEED, flags=FLAG_HASH, edge_loss=loss, partitions=parts, stall_rounds=stall,
                            threads=4 if N > (1 << 20) else 1)
        if work == "philox":
            o.inject_random()
        else:
            inject_words(o, built_words(work, R, loss), R)
        self.hash0 = o.state_hash()
        self.stats, inf, self.states, self.fullmaj, self.unres = [], [], [], [], []
        script = dict(script)
        for t in range(MAX_ROUNDS):
            if t in script:
                o.inject(*script[t])
            S = o.read_shard()[0]
            empty, full = st.shares(o.read_shard(), R)
            self.fullmaj.append(1.0 - full < 1.0 - empty)  # fewer non-full nodes than nonzero ones (plan.h)
            self.unres.append(unresolved(S, N, R, k, t, loss, parts) if self.fullmaj[-1] else 0)
            r = o.step(1)
            self.stats += r.stats
            inf.append(r.infected[0])
            if keep_states:
                self.states.append(o.read_shard().copy())
            if r.converged:
                break
        self.infected = np.array(inf, dtype=np.uint64)
        self.rounds = len(self.stats)
        self.converged = bool(self.stats[-1]["converged"])
        self.final = o.read_shard().copy()
        self.hash = o.state_hash()
        o.close()

    @property
    def scanned(self):
        """rounds that start full-majority and leave unresolved nodes: the scan pass has edges"""
        return [t for t in range(self.rounds) if self.fullmaj[t] and self.unres[t] > 0]


@functools.lru_cache(maxsize=None)
def ref(work, N, mode, k, R, loss=0, parts=0, stall=0, keep_states=True, script=()):
    return Ref(work, N, mode, k, R, loss, parts, stall, keep_states, script)


def engine(work, N, mode, k, R, loss=0, parts=0, stall=0, params=FP, flags=0):
    e = Engine(N, R, mode, k, SEED, flags=FLAG_HASH | flags, edge_loss=loss, partitions=parts, stall_rounds=stall,
               params=dict(params))
    if work == "philox":
        e.inject_random()
    else:
        inject_words(e, built_words(work, R, loss), R)
    return e


def run_equals(e, want, chunk=1, script=()):
    """e against want in steps of `chunk` rounds; the whole state after every step where want kept it"""
    fm = full_mask(e.n_rumors)
    script = dict(script)
    assert e.state_hash() == want.hash0
    done = 0
    while done < want.rounds:
        if done in script:
            e.inject(*script[done])
        r = e.step(min(chunk, MAX_ROUNDS - done))
        assert r.rounds == min(chunk, want.rounds - done), done
        assert r.stats == want.stats[done:done + r.rounds], done
        assert np.array_equal(r.infected, want.infected[done:done + r.rounds]), done
        done += r.rounds
        if want.states:
            shard = e.read_shard()
            assert np.array_equal(shard, want.states[done - 1]), done
            assert not (shard[0] & ~fm).any()  # no bit past R: a resolved node gets the mask of R rumors
    assert r.converged == want.converged
    assert np.array_equal(e.read_shard(), want.final)
    assert e.state_hash() == want.hash


# (state, mode, k, R): every state of the issue's table; R = 37 keeps the mask honest
BUILT = [("none_full", "pushpull", 2, 64), ("none_full", "pull", 1, 37),
         ("half", "pushpull", 2, 37), ("half", "pull", 2, 64), ("half", "pushpull", 3, 37), ("half", "pull", 3, 37),
         ("bench81", "pushpull", 2, 64), ("bench81", "pull", 3, 37), ("bench81", "pushpull", 1, 37),
         ("packed", "pull", 1, 37), ("packed", "pushpull", 1, 64), ("packed", "pushpull", 2, 37)]


@pytest.mark.parametrize("work,mode,k,R", BUILT, ids=lambda x: str(x))
def test_built_states(work, mode, k, R):
    want = ref(work, N_SMALL, mode, k, R)
    assert want.converged and want.scanned, (want.fullmaj, want.unres)
    if work == "none_full":
        assert not want.fullmaj[0]  # round 0 stays on the ordinary paths; later rounds take the shortcut
    e = engine(work, N_SMALL, mode, k, R)
    run_equals(e, want)
    e.close()


def test_all_full_has_nothing_to_do():
    want = ref("all_full", N_SMALL, "pushpull", 2, 37)
    assert want.rounds == 1 and want.converged and want.unres == [0]
    e = engine("all_full", N_SMALL, "pushpull", 2, 37)
    run_equals(e, want)
    e.close()


@pytest.mark.parametrize("mode,R", [("pull", 37), ("pushpull", 64)])
def test_all_full_but_one_node(mode, R):
    """k = 1 with 25 % loss: the node's only edge of round 0 is lost, so round 0 leaves it unresolved."""
    want = ref("all_but_one", N_SMALL, mode, 1, R, loss=LOSS)
    assert want.converged and want.unres[0] == 1
    e = engine("all_but_one", N_SMALL, mode, 1, R, loss=LOSS)
    run_equals(e, want)
    e.close()


# (state, mode, k, loss, partitions, stall rounds), R = 37
FAULTY = [("half", "pushpull", 2, LOSS, 0, 0), ("half", "pull", 2, 0, 3, 0), ("bench81", "pushpull", 2, LOSS, 3, 0),
          ("bench81", "pushpull", 2, LOSS, 0, 2), ("half", "pull", 1, LOSS, 0, 1), ("packed", "pushpull", 3, LOSS, 3, 1)]


@pytest.mark.parametrize("work,mode,k,loss,parts,stall", FAULTY, ids=lambda x: str(x))
def test_built_states_with_faults(work, mode, k, loss, parts, stall):
    """Edge loss, three partitions (4099 / 3 is no integer: the blocks cut through groups) and stalled
    initiators (a stalled node that is not full stays so: those runs are compared for MAX_ROUNDS rounds)."""
    want = ref(work, N_SMALL, mode, k, 37, loss, parts, stall)
    assert want.scanned and (want.converged or stall)
    e = engine(work, N_SMALL, mode, k, 37, loss, parts, stall)
    run_equals(e, want)
    e.close()


@pytest.mark.parametrize("ahead", [1, 7])
@pytest.mark.parametrize("work,mode,k", [("half", "pushpull", 2), ("none_full", "pull", 2)])
def test_wrong_prediction_only_costs_time(work, mode, k, ahead):
    """`ahead` rounds are planned from predicted totals: the shortcut is chosen (or not) for a state that
    is not there.  One step of MAX_ROUNDS rounds, then steps of 3."""
    want = ref(work, N_SMALL, mode, k, 37)
    assert want.scanned
    for chunk in (MAX_ROUNDS, 3):
        e = engine(work, N_SMALL, mode, k, 37, params=dict(FP, ahead=ahead))
        run_equals(e, want, chunk=chunk)
        e.close()


# Philox origins, then gossip itself: every round sparse or on the shortcut
SIZES = [(N_MID, "pushpull", 2, 64, 0), (N_MID, "pull", 1, 37, 0), (N_MID, "pushpull", 3, 37, LOSS),
         (N_BIG, "pushpull", 2, 64, 0), (N_BIG, "pull", 2, 37, 0)]


@pytest.mark.parametrize("N,mode,k,R,loss", SIZES, ids=lambda x: str(x))
def test_sizes(N, mode, k, R, loss):
    want = ref("philox", N, mode, k, R, loss, keep_states=N == N_MID)
    assert want.converged and want.scanned
    e = engine("philox", N, mode, k, R, loss)
    run_equals(e, want, chunk=1 if N == N_MID else MAX_ROUNDS)
    e.close()


def test_from_dense_rounds_into_sparse_rounds():
    """One engine, 25 % loss and k = 1 (eight full-majority rounds): dense rounds (sparse_frac -1) up to
    round 15, then the shortcut for the six rounds left, with an inject between two of its steps; after
    a reset ordinary sparse rounds (empty majority) read what it left; then the whole run once more
    with no knob set, where the planner picks every path itself."""
    N, mode, k, R, enter = N_MID, "pushpull", 1, 37, 15
    plain = ref("philox", N, mode, k, R, LOSS)
    assert plain.fullmaj[enter - 2:plain.rounds] == [True] * (plain.rounds - enter + 2)
    # the rumor goes to a node that is still missing it two rounds into the shortcut
    node = int(np.flatnonzero((plain.states[enter + 1][0] & np.uint64(1 << 5)) == 0)[0])
    script = ((enter + 2, (node, 5)),)
    want = ref("philox", N, mode, k, R, LOSS, script=script)
    assert want.converged and want.rounds - enter >= 4 and [t for t in want.scanned if t >= enter][:3] == [15, 16, 17]
    e = engine("philox", N, mode, k, R, LOSS, params={"sparse_frac": -1}, flags=FLAG_TIMING)
    r = e.step(enter)
    assert r.stats == want.stats[:enter] and (e.kernel_time(3)[1], e.kernel_time(4)[1]) == (enter, 0)
    e.set_param("sparse_frac", 1.0)
    for t in range(enter, want.rounds):
        if t == enter + 2:
            e.inject(node, 5)
        r = e.step(1)
        assert r.stats == want.stats[t:t + 1], t
        assert np.array_equal(r.infected, want.infected[t:t + 1]), t
        assert np.array_equal(e.read_shard(), want.states[t]), t
    assert r.converged and (e.kernel_time(3)[1], e.kernel_time(4)[1]) == (enter, want.rounds - enter)
    e.reset()
    e.inject_random()
    r = e.step(3)
    assert r.stats == plain.stats[:3] and e.kernel_time(4)[1] == want.rounds - enter + 3
    e.close()
    e = engine("philox", N, mode, k, R, LOSS, params={})
    run_equals(e, plain, chunk=MAX_ROUNDS)
    e.close()


def test_push_mode_keeps_its_paths():
    """PUSH has no pull to resolve from: full-majority rounds stay on the frontier scan."""
    want = ref("bench81", N_SMALL, "push", 2, 37)
    assert want.converged and any(want.fullmaj)
    e = engine("bench81", N_SMALL, "push", 2, 37)
    run_equals(e, want)
    e.close()


def test_topo_peers_engine_keeps_its_path():
    """GOSSIP_FLAG_TOPO_PEERS draws peers from the rows: no shortcut buffers, the same knob, the old result."""
    N, R = N_SMALL, 37
    topo = tp.ragged(N, 7)
    inj = [((431 * i) % N, i) for i in range(R)]

    def run(x):
        x.set_topology(topo)
        for n, r in inj:
            x.inject(n, r)
        return x.step(MAX_ROUNDS), x.read_shard()

    (a, sa) = run(tr.TopoSim(N, R, "pushpull", 2, SEED))
    with Engine(N, R, "pushpull", 2, SEED, flags=FLAG_HASH | FLAG_TOPO_PEERS, params=dict(FP)) as e:
        (b, sb) = run(e)
    assert a.rounds == b.rounds and a.stats == b.stats
    assert np.array_equal(a.infected, b.infected) and np.array_equal(sa, sb)
