"""CPU only: the tables and builders of tests/sizes.py, and the preconditions test_gpu_sizes.py relies
on, shown on the C oracle and the numpy restatements alone, so that no GPU case is vacuous.

Every random-mode case that starts from edges_at or from Philox origins converges within sizes.CAP
rounds and, from 7 nodes on, has a round that starts empty-majority and one that starts full-majority
(the criterion of test_gpu_fullpull.py), so a sparse path runs both of its scans.  The holes_at cases
start full-majority by construction (that is their point) and are held to their own figures; the fault
cases never converge (three partitions) and are held to having lost edges that changed the run."""
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

THREADS = min(16, os.cpu_count() or 1)


# --- the tables themselves -------------------------------------------------------------------------

def triples(bs):
    return [b + d for b in bs for d in (-1, 0, 1)]


def test_tables_are_complete_triples():
    assert sz.SMALL == [2, 3, 7, 8, 9] + triples([64, 128, 256, 1024, 2048, 4096, 8192, 16384, 32768])
    assert sz.LARGE == triples([1 << 19, 1 << 20, 1 << 21])
    assert sz.BIG == [(1 << 24) + 1]
    assert sz.AE == [4] + triples([64, 256, 4096, 16384, 131072])
    assert sz.TINY == [2, 3] + triples([64, 256])
    assert sz.FAULT_SIZES == [64, 4096, 16384, 16385, 32768] and sz.HOLES_SIZES == [4096, 16384]


def test_ts_is_the_sender_tile():
    assert [sz.ts(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == \
        [8192, 8192, 4096, 4096, 2048, 2048, 1024, 1024, 512, 512, 256, 256]
    assert list(sz.TS) == [3, 5, 9, 17, 33, 64]
    for k, sizes in sz.TS.items():
        t = sz.ts(k)
        assert sizes == [t - 1, t, t + 1, 2 * t, 16384 + t]
        assert t * k <= 16384 and (t == 8192 or 2 * t * k > 16384)


def test_boundary_nodes():
    assert sz.boundary_nodes(2) == [0, 1] and sz.boundary_nodes(3) == [0, 1, 2]
    assert sz.boundary_nodes(64) == [0, 62, 63] and sz.boundary_nodes(65) == [0, 63, 64]
    assert sz.boundary_nodes(257) == [0, 63, 64, 127, 128, 255, 256]
    for N in sz.SMALL + sz.LARGE + sz.BIG:
        b = sz.boundary_nodes(N)
        assert b == sorted(set(b)) and b[0] == 0 and b[-1] == N - 1 and N - 2 in b and len(b) <= 48
        for u in sz.UNITS:
            for x in (u - 1, u, 2 * u - 1, 2 * u):
                assert (x in b) == (x < N) or x in (0, N - 2, N - 1)
    for u in (64, 256, 1024, 2048, 4096, 8192, 16384, 32768, 1 << 19, 1 << 20, 1 << 21):
        assert u in sz.UNITS


def test_modes_and_fanouts_cover_every_triple():
    """Over the three sizes of a triple: push, pull and pushpull, and in each of them three fanouts of
    K4 (every k class of the binned scan: k <= 2 and k <= 4)."""
    for t in range(5, len(sz.SMALL), 3):
        cases = [c for N in sz.SMALL[t:t + 3] for c in sz.small_cases(N)]
        assert {c[2] for c in cases} == set(sz.MODES)
        assert {c[3] for c in cases} == set(sz.K4)
        for mode in sz.MODES:
            ks = {c[3] for c in cases if c[2] == mode}
            assert len(ks) == 3 and min(ks) <= 2 and max(ks) >= 3
    for t in range(0, len(sz.LARGE), 3):
        cases = [c for N in sz.LARGE[t:t + 3] for c in sz.large_cases(N)]
        assert {(c[2], c[3]) for c in cases} == {("pushpull", 2), ("push", 3), ("pull", 1)}
    for k in sz.TS:
        assert {c[2] for N in sz.TS[k][:3] for c in sz.ts_cases(k, N)} == set(sz.MODES)
    # no path is asked for a fanout it does not take: the binned scan stops at k = 4
    assert all(c[3] <= 4 for N in sz.SMALL for c in sz.small_cases(N))
    assert all(c[3] <= 4 for N in sz.LARGE for c in sz.large_cases(N))
    assert "sparse_bscan" not in sz.TS_PATHS and "sparse_bscan" not in st.FAULT_PATHS
    assert set(sz.LARGE_PATHS) | set(sz.BIG_PATHS) <= set(st.PATHS) and sz.SMALL_PATHS[:-1] == st.PATHS
    assert sz.path_of("dense_frac") == (0, {"sparse_frac": -1}) and sz.path_of("sparse") == st.path_of("sparse")


def test_ae_pairs_cover_every_triple():
    assert sz.ae_cases(4) == [(16, 1)]
    for t in range(1, len(sz.AE), 3):
        lo, mid, hi = (sz.ae_cases(N) for N in sz.AE[t:t + 3])
        assert lo == hi == mid[:1] and mid[1:] == [(17, 1), (2, 4)]
    assert {sz.ae_cases(N)[0] for N in sz.AE} == {(16, 1), (3, 2), (9, 3)}
    for N, K, k, path in sz.AE_ITEMS:
        assert path in ac.PATHS and set(ac.paths_of(K, k)) <= set(sz.ae_paths(K, k))
    assert sz.ae_paths(16, 1) == ac.PATHS_BINNED and sz.ae_paths(17, 1) == sz.ae_paths(2, 4) == ac.PATHS_OTHER


# --- the builders ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", sz.SMALL + sz.LARGE)
def test_edges_at_puts_a_rumor_on_every_boundary_node(N):
    o = op.OracleEngine(N, 3, "push", 1, sz.SEED, flags=1)
    calls = sz.edges_at(o, 3)
    w = o.read_shard()[0]
    b = sz.boundary_nodes(N)
    assert calls == len(b) + 3 <= 51
    assert (w[b] != 0).all() and int(w[N - 1]) == 7
    assert int((w != 0).sum()) == len(b)      # and nowhere else
    o.close()


@pytest.mark.parametrize("N", sz.HOLES_SIZES + [16385, 65, 4097])
def test_holes_at_is_nearly_full_with_empty_boundaries(N):
    o = op.OracleEngine(N, 3, "push", 1, sz.SEED, flags=1)
    calls = sz.holes_at(o, 3)
    w = o.read_shard()[0]
    b = sz.boundary_nodes(N)
    n = np.arange(N, dtype=np.uint64)
    want = np.where(n % 97 == 5, np.uint64(7) & ~(np.uint64(1) << (n % 3)), np.uint64(7))
    want[b] = 0
    assert np.array_equal(w, want) and calls == sum(bin(int(x)).count("1") for x in want) <= 49200
    assert not w[b].any()
    if N in sz.HOLES_SIZES:
        empty, full = st.shares(o.read_shard(), 3)
        assert full > 0.98 and sz.majorities(o.read_shard(), 3) == (True, False)
        assert N % 64 == 0 and {63, 64, N - 1} <= set(b)      # an aligned N, its last node rare
    o.close()


# --- the random-mode cases ---------------------------------------------------------------------------

def oracle_rounds(case, faults=None, rounds=sz.CAP, threads=1):
    """One oracle run a round at a time: (stats, [(full-majority, empty-majority) at the start of each
    round])."""
    N, R, mode, k, builder = case
    o = op.OracleEngine(N, R, mode, k, sz.SEED, flags=1, threads=threads, **(faults or {}))
    sz.build(o, builder, R)
    stats, kinds = [], []
    for _ in range(rounds):
        kinds.append(sz.majorities(o.read_shard(), R))
        r = o.step(1)
        stats += r.stats
        if r.converged:
            break
    o.close()
    return stats, kinds


def check_converges_with_both_kinds(case, threads=1):
    stats, kinds = oracle_rounds(case, threads=threads)
    assert stats[-1]["converged"] and len(stats) <= sz.CAP, case
    if case[0] >= 7:
        assert any(f for f, _ in kinds) and any(e for _, e in kinds), (case, kinds)
    return len(stats)


@pytest.mark.parametrize("N", sz.SMALL)
def test_small_cases(N):
    for case in sz.small_cases(N):
        check_converges_with_both_kinds(case)


@pytest.mark.parametrize("N", sz.LARGE)
def test_large_cases(N):
    for case in sz.large_cases(N):
        assert check_converges_with_both_kinds(case, THREADS) <= 40


def test_big_case():
    (case,) = sz.big_cases(sz.BIG[0])
    check_converges_with_both_kinds(case, THREADS)


# Fanout 33 and 64 from 64 Philox origins: 64 x 64 first contacts cover these sizes at once, the run is
# over in two or three rounds and none of them starts with a full node.  At 255 .. 257 nodes with k = 64
# that holds in every mode, so no rotation of the modes helps; these sizes run on the dense paths only,
# which do not choose their kernels by the majority.
TS_OVER_AT_ONCE = {(33, 255), (64, 255), (64, 256), (64, 257), (64, 16640)}


@pytest.mark.parametrize("k,N", sz.TS_SIZES)
def test_ts_cases(k, N):
    (case,) = sz.ts_cases(k, N)
    assert case[3] == k and case[0] == N
    if (k, N) in TS_OVER_AT_ONCE:
        stats, kinds = oracle_rounds(case)
        assert stats[-1]["converged"] and len(stats) <= 3 and all(e for _, e in kinds)
    else:
        check_converges_with_both_kinds(case)


@pytest.mark.parametrize("N", sz.HOLES_SIZES)
def test_holes_cases(N):
    """Every round starts full-majority; the pulling modes go down the full-pull shortcut on the
    sparse paths, push stays on the frontier scan."""
    for case in sz.holes_cases(N):
        stats, kinds = oracle_rounds(case)
        assert stats[-1]["converged"] and len(stats) <= sz.CAP
        assert all(f for f, _ in kinds)


@pytest.mark.parametrize("N", sz.FAULT_SIZES)
def test_fault_cases_lose_edges_that_matter(N):
    for case in sz.fault_cases(N):
        faulty, _ = oracle_rounds(case, sz.FAULTS, sz.FAULT_ROUNDS)
        clean, _ = oracle_rounds(case, None, sz.FAULT_ROUNDS)
        assert len(faulty) == sz.FAULT_ROUNDS and not faulty[-1]["converged"]
        assert faulty != clean[:sz.FAULT_ROUNDS] and clean[-1]["converged"]


# --- ANTIENTROPY ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", sz.AE)
def test_ae_cases_finish_their_three_steps(N):
    assert N >= 4      # ae_cases.run writes to node 3
    for K, k in sz.ae_cases(N):
        args, kw = ac.engine_args(K, k, n_nodes=N)
        o = op.OracleEngine(*args, threads=THREADS if N > 20000 else 1, **kw)
        r = ac.run(o)
        o.close()
        a, b, c = r.steps
        assert a <= 3 and b < 400 and c < 400 and len(r.stats) == a + b + c
        assert r.stats[a + b - 1]["converged"] and r.stats[-1]["converged"]


# --- the sender kernels at TINY sizes ---------------------------------------------------------------------

def test_tiny_topology():
    for N in sz.TINY:
        rp, col = sz.tiny_topology(N)
        deg = np.diff(rp.astype(np.int64))
        assert rp.size == N + 1 and deg[0] == N and list(col[:N]) == list(range(N))
        assert all(deg[n] == (0 if n % 3 == 2 else 2) for n in range(1, N))
        assert int(col.max()) < N
        inj = sz.tiny_injects(N, 130)
        assert {r for _, r in inj} == set(range(130)) and all(n < N for n, _ in inj)


@functools.lru_cache(maxsize=None)
def monger_ref_run(N, topo_peers, R, limit, k, cool, blind):
    x = mc.MongerCounterSim(N, R, k, sz.SEED, topo_peers=topo_peers)
    if topo_peers:
        x.set_topology(sz.tiny_topology(N))
    x.set_monger(cool, blind)
    if limit is not None:
        x.set_monger_limit(limit)
    for n, r in sz.tiny_injects(N, R):
        x.inject(n, r)
    return x.step(sz.CAP), x.read_counts()


@pytest.mark.parametrize("N", sz.TINY)
def test_monger_cases_go_quiet_and_count(N):
    cases = sz.monger_cases(N)
    assert {(c[0], c[1]) for c in cases} == {(l, k) for l in sz.MONGER_RULES for k in sz.MONGER_K}
    tot = dict.fromkeys(mc.GUARDS, 0)
    for topo_peers in (False, True):
        for R in (3, 130):
            for limit, k, cool, blind in cases:
                res, counts = monger_ref_run(N, topo_peers, R, limit, k, cool, blind)
                assert res.rounds < sz.CAP and res.stats[-1]["messages"] == 0, (N, topo_peers, R, limit, k)
                assert res.stats[0]["messages"] > 0
                for g in res.guards:
                    for name in mc.GUARDS:
                        tot[name] += g[name]
                if limit is not None:
                    assert int(counts.max()) >= limit
    assert tot["cooled"] > 0 and tot["kept"] > 0 and tot["carry"] > 0
    if N == 2:     # k = 9 onto the one peer: a count passes its limit inside one round
        res, counts = monger_ref_run(2, False, 3, 2, 9, *[c[2:] for c in cases if c[:2] == (2, 9)][0])
        assert int(counts.max()) > 2


@pytest.mark.parametrize("N", sz.TINY)
def test_topo_cases_move_rumors(N):
    for i, mode in enumerate(sz.MODES):
        R, k = (3, 130)[(i + sz.TINY.index(N)) % 2], sz.MONGER_K[(i + sz.TINY.index(N)) % 3]
        x = tr.TopoSim(N, R, mode, k, sz.SEED, topology=sz.tiny_topology(N))
        for n, r in sz.tiny_injects(N, R):
            x.inject(n, r)
        before = int(np.count_nonzero(x.read_shard()))
        res = x.step(24)
        assert res.stats[0]["messages"] > 0
        assert int(np.count_nonzero(x.read_shard())) > before or N <= 3
