"""GPU: every round path at node counts on, one below and one above the units of its kernels
(tests/sizes.py: waves, blocks, bitmap words, scan steps, regions, tiles, the LDS summary's levels, the
big geometry), bit for bit against the C oracle and the numpy restatements: the state hash before the
first round, per-round stats (with FLAG_HASH: the hash of every node's word after every round), the
per-rumor counts, the final read_shard and the final state_hash.

The states put the interesting nodes on the boundaries: edges_at starts a run with its whole rare set
there, holes_at starts full-majority with every rare node there.  tests/test_size_tables.py shows from
the oracle alone that the cases converge, start rounds of both majorities, lose edges that matter and
finish their steps.  Oracle runs are computed once per case and shared by the paths (read only)."""
import functools
import os

import numpy as np
import pytest

import ae_cases as ac
import monger_counter_ref as mc
import oracle_py as op
import sizes as sz
import states as st
import topo_ref as tr
from gossip_hip import FLAG_HASH, FLAG_MONGER, FLAG_TOPO_PEERS, Engine

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


def run(x, case, rounds):
    """(hash before round 0, step result, final state, final hash) of one case on any engine of the ABI."""
    sz.build(x, case[4], case[1])
    h0 = x.state_hash()
    res = x.step(rounds)
    return h0, res, x.read_shard(), x.state_hash()


def oracle_run(case, faults=(), rounds=sz.CAP, threads=1):
    N, R, mode, k, _ = case
    o = op.OracleEngine(N, R, mode, k, sz.SEED, flags=FLAG_HASH, threads=threads, **dict(faults))
    out = run(o, case, rounds)
    o.close()
    return out


oracle_small = functools.lru_cache(maxsize=None)(oracle_run)
oracle_large = functools.lru_cache(maxsize=2)(oracle_run)   # one size's two state images at a time


def check(case, path, want, faults=(), rounds=sz.CAP, more_params=()):
    N, R, mode, k, _ = case
    flags, params = path
    with Engine(N, R, mode, k, sz.SEED, flags=FLAG_HASH | flags, params=dict(params, **dict(more_params)),
                **dict(faults)) as e:
        h0, got, shard, h = run(e, case, rounds)
    wh0, wres, wshard, wh = want
    assert h0 == wh0, case
    assert got.rounds == wres.rounds, case
    for a, b in zip(got.stats, wres.stats):
        assert a == b, case
    assert np.array_equal(got.infected, wres.infected), case
    assert np.array_equal(shard, wshard), case
    assert h == wh, case
    return got


def ids(items):
    return ["-".join(str(x) for x in it) for it in items]


# --- a. SMALL: every path, push and pull from edges_at, pushpull from Philox origins ---------------------

SMALL_ITEMS = [(N, p) for N in sz.SMALL for p in sz.SMALL_PATHS]


@pytest.mark.parametrize("N,path", SMALL_ITEMS, ids=ids(SMALL_ITEMS))
def test_small(N, path):
    for case in sz.small_cases(N):
        assert check(case, sz.path_of(path), oracle_small(case)).converged


# --- b. LARGE: the sparse paths across the peer tile and the summary's levels ----------------------------

LARGE_ITEMS = [(N, p) for N in sz.LARGE for p in sz.LARGE_PATHS]


@pytest.mark.parametrize("N,path", LARGE_ITEMS, ids=ids(LARGE_ITEMS))
def test_large(N, path):
    for case in sz.large_cases(N):
        assert check(case, sz.path_of(path), oracle_large(case, threads=THREADS)).converged


# --- c. BIG: the smallest big geometry -----------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def oracle_big():
    (case,) = sz.big_cases(sz.BIG[0])
    return oracle_run(case, threads=THREADS)


@pytest.mark.parametrize("path", sz.BIG_PATHS)
def test_big(path):
    (case,) = sz.big_cases(sz.BIG[0])
    oracle_large.cache_clear()
    assert check(case, sz.path_of(path), oracle_big(), more_params=(("place_tries", 1),)).converged


# --- d. TS: the sender tile of every fanout class on the dense paths ---------------------------------------

TS_ITEMS = [(k, N, p) for k, N in sz.TS_SIZES for p in sz.TS_PATHS]


@pytest.mark.parametrize("k,N,path", TS_ITEMS, ids=ids(TS_ITEMS))
def test_sender_tiles(k, N, path):
    (case,) = sz.ts_cases(k, N)
    assert check(case, sz.path_of(path), oracle_small(case)).converged


# --- e. holes_at: full-majority rounds whose rare nodes all sit on boundaries of an aligned N -----------------

HOLES_ITEMS = [(N, p) for N in sz.HOLES_SIZES for p in sz.SMALL_PATHS]


@pytest.mark.parametrize("N,path", HOLES_ITEMS, ids=ids(HOLES_ITEMS))
def test_holes(N, path):
    for case in sz.holes_cases(N):
        assert check(case, sz.path_of(path), oracle_small(case)).converged


# --- f. faults ------------------------------------------------------------------------------------------------

FAULT_ITEMS = [(N, p) for N in sz.FAULT_SIZES for p in st.FAULT_PATHS]
FAULTS = tuple(sorted(sz.FAULTS.items()))


@pytest.mark.parametrize("N,path", FAULT_ITEMS, ids=ids(FAULT_ITEMS))
def test_faults(N, path):
    for case in sz.fault_cases(N):
        want = oracle_small(case, FAULTS, sz.FAULT_ROUNDS)
        clean = oracle_small(case, (), sz.FAULT_ROUNDS)
        assert want[1].rounds == sz.FAULT_ROUNDS and want[1].stats != clean[1].stats[:sz.FAULT_ROUNDS]
        got = check(case, st.FAULT_PATHS[path], want, FAULTS, sz.FAULT_ROUNDS)
        assert not got.converged


# --- g. ANTIENTROPY ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_ae(N, K, k):
    args, kw = ac.engine_args(K, k, n_nodes=N)
    o = op.OracleEngine(*args, threads=THREADS if N > 20000 else 1, **kw)
    r = ac.run(o)
    h = o.state_hash()
    o.close()
    return r, h


@pytest.mark.parametrize("N,K,k,path", sz.AE_ITEMS, ids=ids(sz.AE_ITEMS))
def test_antientropy(N, K, k, path):
    want, h = oracle_ae(N, K, k)
    args, kw = ac.engine_args(K, k, n_nodes=N)
    pf, params = ac.PATHS[path]
    kw["flags"] |= pf
    with Engine(*args, params=params, **kw) as e:
        got = ac.run(e)
        ac.assert_same(got, want)
        assert e.state_hash() == h


# --- h. the one-lane-per-sender kernels at TINY sizes ------------------------------------------------------------

def monger_run(x, N, R, topo_peers, limit, cool, blind):
    if topo_peers:
        x.set_topology(sz.tiny_topology(N))
    x.set_monger(cool, blind)
    if limit is not None:
        x.set_monger_limit(limit)
    for n, r in sz.tiny_injects(N, R):
        x.inject(n, r)
    return x.step(sz.CAP), x.read_shard(), x.read_hot(), x.read_counts(), x.round_index


@functools.lru_cache(maxsize=None)
def monger_ref(N, R, topo_peers, limit, k, cool, blind):
    return monger_run(mc.MongerCounterSim(N, R, k, sz.SEED, topo_peers=topo_peers), N, R, topo_peers, limit, cool, blind)


MONGER_ITEMS = [(N, peers, R) for N in sz.TINY for peers in ("uniform", "rows") for R in (3, 130)]


@pytest.mark.parametrize("N,peers,R", MONGER_ITEMS, ids=ids(MONGER_ITEMS))
def test_mongering(N, peers, R):
    topo_peers = peers == "rows"
    for limit, k, cool, blind in sz.monger_cases(N):
        (b, sb, hb, cb, tb) = monger_ref(N, R, topo_peers, limit, k, cool, blind)
        assert b.rounds < sz.CAP and b.stats[-1]["messages"] == 0
        with Engine(N, R, "push", k, sz.SEED, flags=FLAG_HASH | FLAG_MONGER | (FLAG_TOPO_PEERS if topo_peers else 0)) as e:
            (a, sa, ha, ca, ta) = monger_run(e, N, R, topo_peers, limit, cool, blind)
        what = (limit, k, cool, blind)
        assert a.rounds == b.rounds and ta == tb, what
        for x, y in zip(a.stats, b.stats):
            assert x == y, what
        assert np.array_equal(a.infected, b.infected), what
        assert np.array_equal(sa, sb) and np.array_equal(ha, hb), what
        assert ca.shape == cb.shape and np.array_equal(ca, cb), what


def topo_run(x, N, R, rounds):
    x.set_topology(sz.tiny_topology(N))
    for n, r in sz.tiny_injects(N, R):
        x.inject(n, r)
    return x.step(rounds), x.read_shard()


def same(got, want):
    (a, sa), (b, sb) = got, want
    assert a.rounds == b.rounds
    for x, y in zip(a.stats, b.stats):
        assert x == y
    assert np.array_equal(a.infected, b.infected)
    assert np.array_equal(sa, sb)


TOPO_ITEMS = [(N, mode) for N in sz.TINY for mode in sz.MODES]


@pytest.mark.parametrize("N,mode", TOPO_ITEMS, ids=ids(TOPO_ITEMS))
def test_topo_peers(N, mode):
    """24 rounds: the nodes with an empty row pull nothing, so PULL never converges."""
    i = sz.MODES.index(mode) + sz.TINY.index(N)
    for R, k in (((3, 130)[i % 2], sz.MONGER_K[i % 3]), ((130, 3)[i % 2], sz.MONGER_K[(i + 1) % 3])):
        want = topo_run(tr.TopoSim(N, R, mode, k, sz.SEED), N, R, 24)
        assert want[0].stats[0]["messages"] > 0
        with Engine(N, R, mode, k, sz.SEED, flags=FLAG_HASH | FLAG_TOPO_PEERS) as e:
            same(topo_run(e, N, R, 24), want)


@pytest.mark.parametrize("N", sz.TINY)
def test_flood(N):
    for R in (3, 130):
        runs = []
        for cls in (op.OracleEngine, Engine):
            with cls(N, R, "flood", 0, sz.SEED, flags=FLAG_HASH) as x:
                runs.append(topo_run(x, N, R, 256))
        # (two nodes: the hub's row and the other's are each other, one round fills both)
        assert runs[0][0].stats[0]["messages"] > 0 and runs[0][0].rounds >= (1 if N == 2 else 2)
        same(runs[1], runs[0])
