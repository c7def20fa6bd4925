"""GPU: ANTIENTROPY state changes between rounds, against the C oracle bit for bit: writes after a
reset with the rows' zeroing still pending, a write to a dead node, churn thresholds at their
extremes, path knobs switched between steps, and one round per step against many.

Every scenario is a function of an engine of the ABI that returns the Runs (ae_cases.snapshot: the
rounds so far, all rows, the sampled alive flags) at its checkpoints; it runs once on the oracle
(cached, read only) and once per path on the HIP engine."""
import functools
import os

import numpy as np
import pytest

import ae_cases as ac
import oracle_py as op
from ae_cases import N
from gossip_hip import Engine
from gossip_hip.engine import StepResult, churn_threshold as ct
from test_gpu_ae_matrix import _oracle as matrix_oracle

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
PATHS = ["auto", "dense", "sparse", "sparse_direct"]
ALL = 0xFFFFFFFF


def _hip(K, k, path, seed, fail=ac.FAIL, rec=ac.RECOVER):
    args, kw = ac.engine_args(K, k, N, seed, fail, rec)
    pf, params = ac.PATHS[path]
    kw["flags"] |= pf
    return Engine(*args, params=params, **kw)


def _cpu(K, k, seed, fail=ac.FAIL, rec=ac.RECOVER):
    args, kw = ac.engine_args(K, k, N, seed, fail, rec)
    return op.OracleEngine(*args, threads=THREADS, **kw)


class Trace:
    """Collects the rounds of an engine and snapshots it at checkpoints."""

    def __init__(self, x):
        self.x, self.stats, self.inf, self.steps, self.marks = x, [], [], [], []

    def step(self, n):
        r = self.x.step(n)
        self.stats += r.stats
        self.inf.append(r.infected)
        self.steps.append(r.rounds)
        return r

    def mark(self):
        self.marks.append(ac.snapshot(self.x, self.stats, self.inf, self.steps))
        return self.marks[-1]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        ac.assert_same(a, b)


def _check(scenario, key, path, *args):
    """scenario(engine, *args) on the HIP engine of `path` equals the oracle's (cached per key)."""
    K, k, seed, fail, rec = key
    want = _oracle_marks(scenario, key, args)
    e = _hip(K, k, path, seed, fail, rec)
    try:
        _same(scenario(e, *args), want)
    finally:
        e.close()
    return want


@functools.lru_cache(maxsize=None)
def _oracle_marks(scenario, key, args):
    o = _cpu(*key)
    marks = scenario(o, *args)
    o.close()
    return marks


# --- 1. reset, then writes only -------------------------------------------------------------------

def reset_then_writes(x):
    """gossip_reset leaves the zeroing of the rows pending; with no inject_random to
    drop it, the first inject must run it before ae_inject_kernel adds to a cell."""
    K = x.n_rumors
    t = Trace(x)
    x.inject_random()
    t.step(3)
    x.reset()
    x.inject(N // 3, K - 1)
    x.inject(N // 3, K - 1)
    x.inject(64, 0)
    assert x.round_index == 0
    t.stats, t.inf, t.steps = [], [], []  # the rounds restart with the reset
    t.mark()
    t.step(400)
    t.mark()
    return t.marks


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("K,k,rounds", [(4, 2, 12), (16, 1, 30), (32, 4, 7)])
def test_reset_then_writes_only(K, k, rounds, path):
    before, after = _check(reset_then_writes, (K, k, 77, ac.FAIL, ac.RECOVER), path)
    want = np.zeros((N, K), np.uint32)
    want[N // 3, K - 1] += 2
    want[64, 0] += 1
    assert np.array_equal(before.rows, want) and all(before.alive)
    assert after.steps == (rounds,) and after.stats[-1]["converged"]
    assert [s["round"] for s in after.stats] == list(range(rounds))
    assert after.stats[0]["full_nodes"] == 0


# --- 2. a write to a dead node --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _first_dead():
    """The first node below 2000 that is dead after three rounds of (16, 1), by the oracle."""
    o = _cpu(16, 1, ac.seed_of(16))
    o.inject_random()
    o.step(3)
    dead = [n for n in range(2000) if not o.read_versions(n)[1]]
    o.close()
    return dead


def write_to_dead(x, node):
    """A client write to a dead node and to its neighbour in the 64-node chunk, after round 2."""
    t = Trace(x)
    x.inject_random()
    t.step(3)
    assert not x.read_versions(node)[1]
    x.inject(node, 0)
    x.inject(node ^ 1, x.n_rumors - 1)
    t.mark()
    t.step(400)
    t.mark()
    return t.marks


@pytest.mark.parametrize("path", PATHS)
def test_write_to_a_dead_node(path):
    dead = _first_dead()
    assert dead[:5] == [12, 14, 23, 59, 64]
    _, after = _check(write_to_dead, (16, 1, ac.seed_of(16), ac.FAIL, ac.RECOVER), path, dead[0])
    assert after.stats[-1]["converged"] and after.steps[1] > 1


# --- 3. churn thresholds at their extremes --------------------------------------------------------

def single_rounds(x, rounds):
    """step(1) calls with a checkpoint after each: gossip_step stops at `converged`, and a round in
    which nobody is alive counts as converged (alive = full = 0)."""
    t = Trace(x)
    x.inject_random()
    t.mark()
    for _ in range(rounds):
        t.step(1)
        t.mark()
    return t.marks


def to_convergence(x, rounds):
    t = Trace(x)
    x.inject_random()
    t.step(rounds)
    t.mark()
    return t.marks


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [2, 4])
def test_churn_everyone_flips_every_round(k, path):
    """fail = recover = 2^32 - 1: every alive node dies and every dead one revives, each round."""
    marks = _check(single_rounds, (4, k, 5, ALL, ALL), path, 6)
    assert [m.stats[-1]["alive_nodes"] for m in marks[1:]] == [0, N, 0, N, 0, N]
    assert [m.stats[-1]["messages"] > 0 for m in marks[1:]] == [False, True] * 3


@pytest.mark.parametrize("path", PATHS)
def test_churn_everyone_dies_for_good(path):
    """fail = 2^32 - 1, recover = 0: one round, nobody alive, the rows as inject_random left them."""
    start, end = _check(single_rounds, (4, 2, 5, ALL, 0), path, 1)
    assert end.stats[0]["alive_nodes"] == 0 and end.stats[0]["messages"] == 0 and not any(end.alive)
    assert np.array_equal(start.rows, end.rows)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fail,rec,rounds,alive", [(0, ALL, 10, N), (ct(0.5), ct(0.5), 34, 20441)])
def test_churn_none_and_half(fail, rec, rounds, alive, path):
    """No churn at all (the recover threshold never applies: nobody dies), and half the nodes
    flipping every round."""
    (end,) = _check(to_convergence, (4, 2, 5, fail, rec), path, 400)
    assert end.steps == (rounds,) and end.stats[-1]["converged"]
    assert end.stats[-1]["alive_nodes"] == alive


@functools.lru_cache(maxsize=None)
def _rare_alive_400():
    o = _cpu(4, 2, 5, ct(0.9), ct(0.02))
    o.inject_random()
    r = o.step(400)
    o.close()
    return r


@pytest.mark.parametrize("path", PATHS)
def test_churn_alive_is_rare(path):
    """fail 0.9, recover 0.02: about 2 % of the nodes are alive in a round; 40 rounds compared.  The
    oracle does not converge in 400."""
    (end,) = _check(to_convergence, (4, 2, 5, ct(0.9), ct(0.02)), path, 40)
    assert end.steps == (40,) and not end.stats[-1]["converged"]
    long = _rare_alive_400()
    assert long.rounds == 400 and not long.converged and long.stats[-1]["alive_nodes"] == 898
    assert long.stats[:40] == end.stats


# --- 4. path knobs switched between steps ---------------------------------------------------------

# each knob walks its own cycle, one place per step of two rounds: the lengths 3, 2, 2, 3, 2 bring
# every pair of settings together within six steps (ae_cap 0 = the default capacity, include/gossip.h)
CYCLES = {"ae_sparse": (0, 1, -1), "ae_dense_bin": (1, 0), "ae_dense_filter": (1, 0), "ae_ahead": (8, 1, 3),
          "ae_cap": (64, 0)}


class Stepped:
    """An engine whose step(n) runs as steps of `chunk` rounds, `before(i)` called ahead of the i-th."""

    def __init__(self, x, chunk, before=None):
        self.x, self.chunk, self.before, self.i = x, chunk, before, 0
        self.n_nodes, self.n_rumors = x.n_nodes, x.n_rumors
        for name in ("inject", "inject_random", "read_rows", "read_versions", "state_hash"):
            setattr(self, name, getattr(x, name))

    def step(self, max_rounds):
        stats, inf = [], []
        while len(stats) < max_rounds:
            if self.before:
                self.before(self.i)
            self.i += 1
            r = self.x.step(min(self.chunk, max_rounds - len(stats)))
            stats += r.stats
            inf.append(r.infected)
            if r.converged:
                break
        return StepResult(len(stats), stats, np.concatenate(inf))


@pytest.mark.parametrize("K,k", [(4, 2), (16, 3), (24, 2), (7, 5)])
def test_knobs_switched_between_steps(K, k):
    """The matrix scenario in steps of two rounds, the path knobs moved before each: a round's path
    never shows in a result bit, whatever ran before it."""
    want, h = matrix_oracle(K, k)
    e = _hip(K, k, "auto", ac.seed_of(K))
    seen = []

    def switch(i):
        for name, cycle in CYCLES.items():
            if name == "ae_dense_bin" and not (K <= 16 and k <= 3):
                continue  # (it does not fit: the engine has the atomic form only)
            e.set_param(name, cycle[i % len(cycle)])
        seen.append(i)

    try:
        got = ac.run(Stepped(e, 2, switch))
        ac.assert_same(got, want)
        assert e.state_hash() == h
    finally:
        e.close()
    assert len(seen) >= 6  # every place of every cycle was taken


# --- 5. one round per step ------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "sparse"])
@pytest.mark.parametrize("K,k", [(2, 1), (16, 2)])
def test_single_steps_equal_one_long_step(K, k, path):
    """step(1) in a loop (no pipelined run of sparse rounds ever forms) gives the stats and rows of
    step(400) on a second engine, and the oracle's."""
    want, _ = matrix_oracle(K, k)
    a, b = _hip(K, k, path, ac.seed_of(K)), _hip(K, k, path, ac.seed_of(K))
    try:
        one, many = ac.run(Stepped(a, 1)), ac.run(b)
    finally:
        a.close()
        b.close()
    ac.assert_same(one, many)
    ac.assert_same(one, want)
