"""GPU: states that gossip never produces, plans made from a wrong prediction, and switches
between rounds — every run equal to the C oracle bit for bit (per-round stats, per-rumor counts,
final state).  The states come from tests/states.py; tests/test_state_builders.py pins, on the
oracle alone, the preconditions used here (class shares, rounds to convergence)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as op
import states as st
from gossip_hip import FLAG_DIRECT, FLAG_TIMING, Engine, GossipError, loss_threshold
from gossip_hip._abi import U64P, RoundStats
from states import N0, SEED

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 64
# workloads: a builder of states.py at N0 nodes, or Philox origins (inject_random)
WORK = dict({name: (N0, R, b) for name, (b, R) in st.BUILDERS.items()},
            philox100k=(100003, 64, None), philox41k=(41037, 64, None), philox_r3=(N0, 3, None))


def _fill(x, work):
    b = WORK[work][2]
    if b is None:
        x.inject_random()
    else:
        b(x, WORK[work][1])


class _Ref:
    """One oracle run, stepped a round at a time: state before round 0, every round's stats and
    per-rumor counts, the class shares at the start of every round, and the final state."""

    def __init__(self, work, mode, k, loss, parts, flags):
        N, R, _ = WORK[work]
        o = op.OracleEngine(N, R, mode, k, SEED, flags=flags, edge_loss=loss, partitions=parts)
        _fill(o, work)
        self.hash0, self.shard0 = o.state_hash(), o.read_shard()
        self.stats, inf, self.shares = [], [], []
        for _ in range(MAX_ROUNDS):
            self.shares.append(st.shares(o.read_shard(), R))
            r = o.step(1)
            self.stats += r.stats
            inf.append(r.infected[0])
            if r.converged:
                break
        self.infected = np.array(inf, dtype=np.uint64)
        self.rounds = len(self.stats)
        self.converged = bool(self.stats[-1]["converged"])
        self.shard, self.hash = o.read_shard(), o.state_hash()
        o.close()


@functools.lru_cache(maxsize=None)
def _ref(work, mode, k, loss=0, parts=0, flags=1):
    """Oracle run of one case, computed once per session and shared by every path (read only)."""
    return _Ref(work, mode, k, loss, parts, flags)


def _engine(work, mode, k, path=(0, {}), loss=0, parts=0, flags=1, stall=0, params=None):
    N, R, _ = WORK[work]
    p = dict(path[1], **(params or {}))
    return Engine(N, R, mode, k, SEED, flags=flags | path[0], edge_loss=loss, partitions=parts, stall_rounds=stall,
                  params=p)


def _run_equals(e, ref, chunk=MAX_ROUNDS, first=0):
    """Steps e to convergence in chunks of `chunk` rounds from round `first`; every round equals ref's."""
    done = first
    while done < ref.rounds:
        r = e.step(min(chunk, MAX_ROUNDS - done))
        assert r.rounds == min(chunk, ref.rounds - done)
        assert r.stats == ref.stats[done:done + r.rounds]
        assert np.array_equal(r.infected, ref.infected[done:done + r.rounds])
        done += r.rounds
    assert ref.converged and r.converged
    assert np.array_equal(e.read_shard(), ref.shard)
    assert e.state_hash() == ref.hash


def test_path_tables_equal_the_parity_tests():
    """states.py restates the path tables of test_gpu_parity.py and test_gpu_faults.py."""
    import test_gpu_faults
    import test_gpu_parity
    assert st.PATHS == test_gpu_parity.PATHS
    assert st.PATH_FLAGS == test_gpu_parity._PATH_FLAGS and st.PATH_PARAMS == test_gpu_parity._PATH_PARAMS
    assert st.FAULT_PATHS == test_gpu_faults.PATHS


# --- 1. a built state before any round ------------------------------------------------------------

BUILT = {"thirds": ("pushpull", 2), "holes": ("push", 1), "noisy_thirds": ("push", 1),
         "noisy_clustered": ("pushpull", 2), "noisy_holes": ("push", 1)}
# engine of each variant: (flags, params), and whether it runs two rounds and is reset before the build
VARIANTS = {"fresh": ((0, {}), False), "direct": ((FLAG_DIRECT, {}), False), "reset": ((0, {}), True),
            "reset_sparse": (st.path_of("sparse"), True), "reset_alld": (st.path_of("sparse_alld"), True)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("work", list(BUILT))
def test_built_state_before_any_round(work, variant):
    """The state as injected, then one round, then the rest of the run.  Which inject kernel
    builds it (engine.hip gossip_inject, prepare_planned):
      fresh  — a new default engine has fr_valid false: every inject is the plain `inject` kernel,
               and the first step's prepare_planned recomputes totals and bitmaps
               (`frontier_rebuild`) from the 12-54 K bits;
      direct — FLAG_DIRECT has no frontier buffers: the plain kernel, totals recomputed per round;
      reset* — gossip_reset zeroes totals and bitmaps and sets fr_valid, so every inject after it
               is `frontier_inject`, which keeps the per-rumor / nonzero / full totals, both
               bitmaps and the telescoped hash incrementally: here through thousands of bits,
               injects that complete a node, and (noisy) duplicates.
    step(1) is what catches a wrong running total, but only where the round's commit adds deltas
    to the totals: dense rounds and direct sparse rounds (the default engine's first round on
    `thirds` and `clustered`) recompute them.  reset_sparse (flag commits) and reset_alld (all-D
    commits into D) force the delta commits on every state; `holes` (full majority) takes the
    all-D delta commit on the default engine too."""
    mode, k = BUILT[work]
    ref = _ref(work, mode, k)
    path, reset = VARIANTS[variant]
    e = _engine(work, mode, k, path=path)
    if reset:
        e.inject(0, 0)
        assert e.step(2).rounds == 2
        e.reset()
    _fill(e, work)
    assert e.state_hash() == ref.hash0
    assert np.array_equal(e.read_shard(), ref.shard0)
    r = e.step(1)
    assert r.stats == ref.stats[:1] and np.array_equal(r.infected, ref.infected[:1])
    _run_equals(e, ref, first=1)
    e.close()


# --- 2. built states on every path -----------------------------------------------------------------

# (workload, mode, k); the last one is not in the issue's list: the only push-pull run of
# `clustered` with a round (4) whose empty and full shares both exceed 0.3
CASES = [("thirds", "pushpull", 2), ("thirds", "push", 1), ("thirds", "pull", 1),
         ("clustered", "push", 1), ("clustered", "pull", 1), ("clustered", "pushpull", 2),
         ("holes", "push", 1), ("clustered", "pushpull", 1)]
# rounds that start with empty share > 0.3 and full share > 0.3 (test_state_builders.BOTH_CLASSES)
BOTH = {("thirds", "pushpull", 2): [0], ("thirds", "push", 1): [0], ("thirds", "pull", 1): [0],
        ("clustered", "push", 1): [6, 7], ("clustered", "pull", 1): [6], ("clustered", "pushpull", 1): [4]}
# the nine paths, `dense_frac` (the dense pipeline of a default engine: sparse_frac -1, default
# filter_frac 0.3 — a FLAG_DENSE engine has no occupancy bitmaps and never filters), and the
# filtering dense paths once more planning from exact totals (ahead 1: nothing predicted)
STATE_PATHS = {name: st.path_of(name) for name in st.PATHS}
STATE_PATHS["dense_frac"] = (0, {"sparse_frac": -1})
STATE_PATHS["dense_frac_ahead1"] = (0, {"sparse_frac": -1, "ahead": 1})
STATE_PATHS["dense_filter_ahead1"] = (0, {"sparse_frac": -1, "filter_frac": 0, "ahead": 1})


def _timed_run(work, mode, k, name, path, loss=0, parts=0):
    """One run on one path; on the forced paths the round timers prove which pipeline ran."""
    ref = _ref(work, mode, k, loss, parts)
    forced = name.startswith("dense") or name.startswith("sparse")
    e = _engine(work, mode, k, path=path, loss=loss, parts=parts, flags=1 | (FLAG_TIMING if forced else 0))
    _fill(e, work)
    _run_equals(e, ref)
    if forced:
        dense, sparse = e.kernel_time(3)[1], e.kernel_time(4)[1]
        assert (dense, sparse) == ((ref.rounds, 0) if name.startswith("dense") else (0, ref.rounds))
    e.close()
    return ref


@pytest.mark.parametrize("path", list(STATE_PATHS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_built_states_every_path(case, path):
    """Empty and full nodes side by side, full-majority rounds with the rare nodes on group and
    tile boundaries (`holes`), perfectly correlated rumors (`clustered`).  By plan_dense_filter() a
    round that starts with both shares above 0.3 sets the push-into-full bit in push and push-pull
    mode and the pull-from-empty bit in pull and push-pull mode, so emit runs with both bits
    (filter 3) in `thirds` push-pull round 0 and `clustered` push-pull k=1 round 4 — on
    `dense_frac` where the plan sees exact totals (round 0, or ahead 1), on `dense_filter` in any
    round with both classes present.  The shares are asserted from the oracle's states."""
    work, mode, k = case
    ref = _timed_run(work, mode, k, path, STATE_PATHS[path])
    for t in BOTH.get(case, []):
        empty, full = ref.shares[t]
        assert empty > 0.3 and full > 0.3
    if work == "holes":  # full majority from round 0, the eight empty nodes on the boundaries
        assert ref.shares[0][1] > 0.98 and not ref.shard0[0][list(st.HOLES)].any()


@pytest.mark.parametrize("path", list(st.FAULT_PATHS))
def test_thirds_with_faults_every_path(path):
    """`thirds` push-pull k=2 with half the edges lost and two partitions (11 rounds)."""
    ref = _timed_run("thirds", "pushpull", 2, path, st.FAULT_PATHS[path], loss=1 << 31, parts=2)
    assert ref.rounds == 11 and ref.shares[0][0] > 0.3 and ref.shares[0][1] > 0.3


# --- 3. prediction errors and `ahead` -------------------------------------------------------------

PREDICT = {"clustered": ("push", 1), "disjoint": ("pushpull", 2), "philox100k": ("pushpull", 2)}


@pytest.mark.parametrize("ahead", [1, 7])
@pytest.mark.parametrize("path", ["auto", "sparse", "sparse_direct", "sparse_bscan", "dense_filter"])
@pytest.mark.parametrize("work", list(PREDICT))
def test_wrong_prediction_only_costs_time(work, path, ahead):
    """plan_predict() multiplies per-rumor miss probabilities as if rumors were independent: with
    perfectly correlated rumors (`clustered`) it sees far too many nonzero nodes a round ahead,
    with disjoint ones too few, so with 7 rounds in flight maj, all_d, the filter bits and the
    binned-scan choice are picked for a state that is not there.  One step(64), then the same run
    in step(3) chunks (a chunk ends with the pipeline full): all equal the oracle round for round,
    hence each other."""
    mode, k = PREDICT[work]
    ref = _ref(work, mode, k)
    for chunk in (MAX_ROUNDS, 3):
        e = _engine(work, mode, k, path=st.path_of(path), params={"ahead": ahead})
        _fill(e, work)
        _run_equals(e, ref, chunk=chunk)
        e.close()


def test_ahead_range():
    e = Engine(1000, 1, "push", 1, SEED)
    for bad in (0, 8):
        with pytest.raises(GossipError):
            e.set_param("ahead", bad)
    e.set_param("ahead", 7)
    e.set_param("ahead", 1)
    e.close()


# --- 4. NULL outputs and an engine without the hash flag ------------------------------------------

def _raw_step(e, want_stats, want_infected):
    stats = (RoundStats * MAX_ROUNDS)()
    inf = np.zeros((MAX_ROUNDS, e.n_rumors), dtype=np.uint64)
    done = C.c_uint32()
    e._check(e._fn("step")(e._h, C.c_uint32(MAX_ROUNDS), stats if want_stats else None,
                           inf.ctypes.data_as(U64P) if want_infected else None, C.byref(done)))
    return done.value, [stats[i].as_dict() for i in range(done.value)], inf[:done.value]


@pytest.mark.parametrize("outputs", ["no_stats", "no_infected", "neither"])
@pytest.mark.parametrize("path", ["auto", "dense"])
def test_step_with_null_outputs(path, outputs):
    ref = _ref("clustered", "pushpull", 2)
    e = _engine("clustered", "pushpull", 2, path=st.path_of(path))
    _fill(e, "clustered")
    rounds, stats, inf = _raw_step(e, outputs == "no_infected", outputs == "no_stats")
    assert rounds == ref.rounds
    if outputs == "no_infected":
        assert stats == ref.stats
    if outputs == "no_stats":
        assert np.array_equal(inf, ref.infected)
    assert e.round_index == ref.rounds
    assert np.array_equal(e.read_shard(), ref.shard) and e.state_hash() == ref.hash
    e.close()


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_engine_without_hash_flag(path):
    """flags = 0: no round carries a hash (the kernels skip it), everything else is unchanged and
    the hash on demand still equals the oracle's."""
    ref, hashed = _ref("clustered", "pushpull", 2, flags=0), _ref("clustered", "pushpull", 2)
    assert [dict(s, state_hash=0) for s in hashed.stats] == [dict(s, state_hash=0) for s in ref.stats]
    e = _engine("clustered", "pushpull", 2, path=st.path_of(path), flags=0)
    _fill(e, "clustered")
    assert e.state_hash() == hashed.hash0 != 0
    r = e.step(MAX_ROUNDS)
    assert all(s["state_hash"] == 0 for s in r.stats)
    assert r.stats == [dict(s, state_hash=0) for s in ref.stats]
    assert np.array_equal(r.infected, ref.infected)
    assert np.array_equal(e.read_shard(), ref.shard)
    assert e.state_hash() == hashed.hash == ref.hash != 0
    e.close()


# --- 5. path carousel ------------------------------------------------------------------------------

CAROUSEL = [("dense", {"sparse_frac": -1})] + [(n, st.PATH_PARAMS[n]) for n in (
    "sparse", "sparse_alld", "sparse_direct", "sparse_bscan", "dense_filter", "sparse_noq")]


@pytest.mark.parametrize("offset", range(7))
@pytest.mark.parametrize("work,mode,k", [("philox100k", "pushpull", 2), ("clustered", "push", 1)])
def test_path_carousel(work, mode, k, offset):
    """gossip_set_param between rounds: every round of one engine runs on another path (each knob
    of the last path first put back to its documented default; `dense` is sparse_frac -1, the
    flag cannot change after creation).  Each path reads the bitmaps, totals and D that the last
    one left, so they must stay exact across any sequence."""
    ref = _ref(work, mode, k)
    e = _engine(work, mode, k, flags=1 | FLAG_TIMING)
    _fill(e, work)
    last, kinds = {}, [0, 0]
    for i in range(ref.rounds):
        name, params = CAROUSEL[(i + offset) % 7]
        for knob in last:
            e.set_param(knob, st.PARAM_DEFAULTS[knob])
        for knob, v in params.items():
            e.set_param(knob, v)
        last = params
        r = e.step(1)
        assert r.stats == ref.stats[i:i + 1], (i, name)
        assert np.array_equal(r.infected, ref.infected[i:i + 1]), (i, name)
        kinds[0 if name.startswith("dense") else 1] += 1
    assert r.converged
    assert (e.kernel_time(3)[1], e.kernel_time(4)[1]) == tuple(kinds)
    assert np.array_equal(e.read_shard(), ref.shard) and e.state_hash() == ref.hash
    e.close()


# --- 6. set_faults mid-run on every path ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _faults_midrun_ref():
    N, R, _ = WORK["philox41k"]
    o = op.OracleEngine(N, R, "pushpull", 2, SEED, flags=1)
    o.inject_random()
    out = [o.step(3)]
    o.set_faults(loss_threshold(0.3), 5)
    out.append(o.step(4))
    o.set_faults(0, 0)
    out.append(o.step(MAX_ROUNDS))
    return out, o.read_shard()


@pytest.mark.parametrize("path", st.PATHS)
def test_set_faults_mid_run_every_path(path):
    """41037 nodes: three tiles, and 41037 / 5 is no integer, so the partition blocks cut through
    64-node groups.  Three rounds without faults, four with 30 % loss and 5 partitions (the
    kernels' FAULTS template flips), then healed until converged."""
    want, shard = _faults_midrun_ref()
    assert [w.rounds for w in want[:2]] == [3, 4] and want[2].converged and not want[1].converged
    e = _engine("philox41k", "pushpull", 2, path=st.path_of(path))
    e.inject_random()
    for phase, (faults, rounds) in enumerate([(None, 3), ((loss_threshold(0.3), 5), 4), ((0, 0), MAX_ROUNDS)]):
        if faults:
            e.set_faults(*faults)
        r = e.step(rounds)
        assert r.stats == want[phase].stats, phase
        assert np.array_equal(r.infected, want[phase].infected), phase
    assert np.array_equal(e.read_shard(), shard)
    e.close()


# --- 7. reset mid-run on every path -----------------------------------------------------------------

@pytest.mark.parametrize("path", st.PATHS)
def test_reset_mid_run_every_path(path):
    mid, fresh = _ref("thirds", "push", 1), _ref("philox_r3", "push", 1)
    assert mid.rounds > 2 and fresh.converged
    e = _engine("thirds", "push", 1, path=st.path_of(path))
    _fill(e, "thirds")
    r = e.step(2)
    assert r.stats == mid.stats[:2] and not r.converged
    e.reset()
    assert e.round_index == 0 and e.state_hash() == 0 and not e.read_shard().any()
    r = e.step(2)
    assert r.rounds == 2 and not r.converged and not r.infected.any()
    assert [s["full_nodes"] for s in r.stats] == [0, 0] and not e.read_shard().any()
    e.reset()
    e.inject_random()
    assert e.state_hash() == fresh.hash0
    _run_equals(e, fresh)
    e.close()


@pytest.mark.parametrize("path", ["auto", "dense"])
def test_reset_clears_stall_streaks(path):
    """stall_rounds 2 with 5 % loss: five rounds build streaks; after reset the rerun equals a
    fresh oracle's, so no streak survived."""
    kw = dict(edge_loss=loss_threshold(0.05), stall_rounds=2)
    o = op.OracleEngine(N0, 3, "push", 1, SEED, flags=1, **kw)
    st.thirds(o, 3)
    want = o.step(MAX_ROUNDS)
    assert want.converged and want.rounds > 5
    flags, params = st.path_of(path)
    e = Engine(N0, 3, "push", 1, SEED, flags=1 | flags, params=params, **kw)
    st.thirds(e, 3)
    r = e.step(5)
    assert r.stats == want.stats[:5]
    e.reset()
    st.thirds(e, 3)
    r = e.step(MAX_ROUNDS)
    assert r.stats == want.stats and np.array_equal(r.infected, want.infected)
    assert np.array_equal(e.read_shard(), o.read_shard())
    e.close()
