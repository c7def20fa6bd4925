"""CPU only: the tables of tests/values.py, and the preconditions test_gpu_values.py relies on, shown on
the restatements alone, so that no GPU case is vacuous.

Every case agrees between two independent restatements: the C oracle against oracle/numpy_ref.py
(Sim, AntiEntropySim behind ae_faults_ref.RefEngine), and topo_ref, ae_topo_ref, ae_faults_ref,
monger_ref and monger_counter_ref against the oracle through the identities their own files use (the
complete topology, cool = 0, limit = 1, one component).  The guards: a full-width seed gives another run
than its low word alone; a partition count below N loses edges and keeps edges, one at or above N
freezes the state, 257 blocks cut inside a 64-node group; loss 1 changes nothing and loss 2^32 - 1
everything; the (A, A) churn flips every alive bit every round; the long runs end on draws at
t > 2^8 and t > 2^16."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ae_cases as ac
import ae_faults_ref as fr
import ae_topo_ref as ar
import monger_counter_ref as mc
import monger_ref as mr
import numpy_ref as nr
import oracle_py as op
import shard_cases as sc
import states as st
import topo_ref as tr
import values as va
from gossip_hip.engine import loss_threshold as lt
from gossip_hip.sharded import CLASSCODED, DENSE, EXCHANGE, REP, REP_CLASSCODED, REP_GATHER, SPARSE

A = va.A
LOW = 0xFFFFFFFF


# --- the tables themselves -------------------------------------------------------------------------

def test_tables():
    assert va.SEEDS == [0x9E3779B97F4A7C15, 0xDEADBEEF00000000, 0xFFFFFFFFFFFFFFFF]
    for s in va.SEEDS:
        assert s >> 32 != 0 and s < 2 ** 64
    lo, hi = va.SEEDS[0] & LOW, va.SEEDS[0] >> 32
    assert lo and hi and lo != hi and va.SEEDS[1] & LOW == 0
    assert va.PARTS(1000) == [5, 7, 999, 1000, 1001, 2 ** 31, 2 ** 32 - 1]
    assert va.PARTS(va.N0) == [5, 7, 257, va.N0 - 1, va.N0, va.N0 + 1, 2 ** 31, 2 ** 32 - 1]
    for N in (va.N0, va.NMID, va.AE_N, ac.N):
        assert N % 5 and N % 7
    assert 64 < va.N0 / 257 < 64.01
    assert va.LOSS == [1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1] and va.STALL == [1, 16]
    assert va.CHURN == [(0, 0), (A, 0), (A, A), (0, A), (2 ** 31, 2 ** 31)]
    assert va.LONG == [300, 65600] and va.LONG[0] > 2 ** 8 and va.LONG[1] > 2 ** 16
    assert dict(va.FAULTY) == dict(edge_loss=lt(0.2), partitions=3, stall_rounds=2)


def test_fanouts_cover_one_to_six_in_every_mode():
    for mode in va.MODES:
        ks = {va.fanout(p, mode) for p in st.PATHS if p != "sparse_bscan"}
        assert ks == {1, 2, 3, 4, 5, 6}
        assert va.fanout("sparse_bscan", mode) <= 4
    assert {va.fanout(p, m) for p in st.PATHS for m in va.MODES} == {1, 2, 3, 4, 5, 6}


# --- numpy_ref.Sim behind the calls play() makes ----------------------------------------------------------

class SimEngine:
    def __init__(self, N, R, mode, k, seed, flags=1, **faults):
        self.n_nodes, self.n_rumors, self.make = N, R, lambda **kw: nr.Sim(N, R, mode, k, seed, **kw, **faults)
        self.sim = self.make()

    def set_topology(self, topology):
        """nr.Sim takes its rows when it is made: only before the first inject."""
        assert self.sim.t == 0 and not self.sim.S.any()
        rp, col = topology
        self.sim = self.make(topology=[[int(v) for v in col[rp[u]:rp[u + 1]]] for u in range(self.n_nodes)])

    def inject(self, node, rumor=0):
        self.sim.inject(node, rumor)

    def inject_random(self):
        self.sim.inject_random()

    def set_faults(self, edge_loss=0, partitions=0):
        self.sim.loss, self.sim.parts = edge_loss, partitions

    def reset(self):
        s = self.sim
        s.S, s.Sprev, s.t = np.zeros_like(s.S), np.zeros_like(s.S), 0
        s.streak = np.zeros_like(s.streak)

    def step(self, max_rounds):
        out = self.sim.run(max_rounds)
        stats = [dict(round=s["round"], converged=s["converged"], full_nodes=s["full"], alive_nodes=self.n_nodes,
                      messages=s["messages"], state_hash=s["hash"]) for s in out]
        inf = np.array([s["infected"] for s in out], dtype=np.uint64).reshape(len(out), self.n_rumors)
        return SimpleNamespace(rounds=len(out), stats=stats, infected=inf)

    def read_shard(self):
        return self.sim.S.copy()

    def state_hash(self):
        return nr.state_hash(self.sim.S)


def make(cls, case, seed=None):
    N, R, mode, k, s, faults, _ = case
    return cls(N, R, mode, k, s if seed is None else seed, flags=1, **dict(faults))


@functools.lru_cache(maxsize=None)
def oracle(case, seed=None):
    o = make(op.OracleEngine, case, seed)
    out = va.play(o, case[6])
    o.close()
    return out


def agree(case):
    """The C oracle and numpy_ref.Sim on one case; returns the oracle's play()."""
    want = oracle(case)
    va.same(va.play(make(SimEngine, case), case[6]), want)
    return want


def low_word_differs(case, want):
    """The seed guard: the same case under seed & 0xFFFFFFFF has other per-round stats."""
    other = oracle(case, case[4] & LOW)
    assert va.flat(other) != va.flat(want), case[:6]


# --- seeds: the random modes ---------------------------------------------------------------------------------

SEED_CASES = {seed: sorted({c for p in st.PATHS for c in va.seed_cases(p, seed)}, key=lambda c: c[:4] + (len(c[5]),))
              for seed in va.SEEDS}


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_seed_cases(seed):
    assert len(SEED_CASES[seed]) >= 36
    for case in SEED_CASES[seed]:
        want = agree(case)
        low_word_differs(case, want)
        if case[5]:
            assert want[0]["rounds"] == va.FAULT_ROUNDS and not want[0]["stats"][-1]["converged"]
            clean = oracle(case[:5] + ((),) + case[6:])
            assert va.flat(clean)[:va.FAULT_ROUNDS] != va.flat(want)
        else:
            assert want[0]["stats"][-1]["converged"] and 2 < want[0]["rounds"] < va.CAP


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_fullpull_and_wide_cases(seed):
    for case in va.fullpull_cases(seed):
        want = agree(case)
        low_word_differs(case, want)
        o = make(op.OracleEngine, case)
        va.quarter(o, 3)
        assert va.sz.majorities(o.read_shard(), 3) == (True, False)     # full-majority from the start
        o.close()
        assert want[0]["rounds"] >= 2 and (case[5] or want[0]["stats"][-1]["converged"])
    for case in va.wide_cases(seed):
        want = agree(case)
        low_word_differs(case, want)
        assert want[0]["shard"].shape[0] == 3


# --- seeds: the sender kernels ----------------------------------------------------------------------------------

NFULL = va.NFULL


def topo_sim(case, seed=None):
    N, R, mode, k, s, faults, _ = case
    return tr.TopoSim(N, R, mode, k, s if seed is None else seed, **dict(faults))


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_topo_ref_on_the_complete_graph_is_the_oracle(seed):
    """row_n[i] = i + (i >= n) is the uniform peer map: everything but messages, with the faults and
    the deadline of FAULTY."""
    for mode, k in zip(va.MODES, (2, 5, 3)):
        s = tuple(("inject", (431 * i) % NFULL, i) for i in range(5)) + (("step", 20),)
        case = va.case(NFULL, 5, mode, k, seed, s, **dict(va.FAULTY))
        got = va.play(topo_sim(case), (("topology", "complete"),) + s)
        assert got[0]["stats"][0]["messages"] > 0
        va.same(got, oracle(case), messages=False)


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_topo_seed_cases_depend_on_the_high_word(seed):
    for case in va.topo_seed_cases(seed):
        a, b = va.play(topo_sim(case), case[6]), va.play(topo_sim(case, seed & LOW), case[6])
        # (under the deadline every PUSH sender is stalled within a few rounds: the last rounds send nothing)
        assert va.flat(a) != va.flat(b) and a[0]["rounds"] == 12 and a[0]["stats"][0]["messages"] > 0


def monger_sim(case, topo_peers, seed=None, cls=mc.MongerCounterSim):
    N, R, _, k, s, faults, _ = case
    return cls(N, R, k, s if seed is None else seed, topo_peers=topo_peers, **dict(faults))


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_monger_refs_at_full_width_seeds(seed):
    """cool = 0 is the oracle's PUSH (but for messages); limit 1 is MongerSim; every case of va.MONGER
    goes quiet, cools bits and runs otherwise under the seed's low word."""
    s = tuple(("inject", (431 * i) % NFULL, i) for i in range(5)) + (("step", 14),)
    case = va.case(NFULL, 5, "push", 5, seed, s, edge_loss=lt(0.3), partitions=3)
    va.same(va.play(monger_sim(case, False), s), oracle(case), messages=False)
    for peers, R, k, cool, blind, limit, loss in va.MONGER:
        case, tp_ = va.monger_case(peers, R, k, cool, blind, limit, seed, edge_loss=loss)
        m = monger_sim(case, tp_)
        a = va.play(m, case[6], va.MONGER_READS)
        b = va.play(monger_sim(case, tp_, seed & LOW), case[6], va.MONGER_READS)
        assert va.flat(a) != va.flat(b)
        assert a[0]["rounds"] < va.CAP and a[0]["stats"][-1]["messages"] == 0 and a[0]["stats"][0]["messages"] > 0
        assert (a[0]["shard"] & ~a[0]["extra"]["read_hot"]).any()          # cooled bits
        if limit is None:   # the coin alone: the counter restatement with its limit never set is MongerSim
            va.same(va.play(monger_sim(case, tp_, cls=mr.MongerSim), case[6], ("read_hot", "round_index")),
                    [dict(e, extra={n: v for n, v in e["extra"].items() if n != "read_counts"}) for e in a])
        else:
            assert int(a[0]["extra"]["read_counts"].max()) >= limit


NWALK = va.NWALK


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_flood_walks(seed):
    """The oracle's walks against numpy_ref.Sim's on 301 nodes of ragged rows (loss 0.3, D = 2), and the
    GPU case under the seed's low word: other losses, another run."""
    s = (("topology", "walk"),) + tuple(("inject", (43 * i) % NWALK, i) for i in range(5)) + (("step", 30),)
    case = va.case(NWALK, 5, "flood", 0, seed, s, edge_loss=lt(0.3), stall_rounds=2)
    want = agree(case)
    assert want[0]["rounds"] > 3 and want[0]["stats"][0]["messages"] > 0
    big = va.walk_case(seed)
    low_word_differs(big, oracle(big))


# --- seeds: ANTIENTROPY -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ae_oracle(K, k, seed, n_nodes=ac.N):
    args, kw = ac.engine_args(K, k, n_nodes=n_nodes, seed=seed)
    o = op.OracleEngine(*args, threads=4, **kw)
    r = ac.run(o)
    o.close()
    return r


@pytest.mark.parametrize("K,k", va.AE_PAIRS)
@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_ae_seed_cases(seed, K, k):
    """ae_cases.run at ae_cases.N nodes: the oracle against the numpy restatement, and against its own
    run under the seed's low word (initial versions, churn and peers all move)."""
    want = ae_oracle(K, k, seed)
    args, kw = ac.engine_args(K, k, seed=seed)
    ac.assert_same(ac.run(fr.RefEngine(*args, **kw)), want)
    other = ae_oracle(K, k, seed & LOW)
    assert other.stats != want.stats and not np.array_equal(other.rows, want.rows)
    a, b, c = want.steps
    assert want.stats[a + b - 1]["converged"] and want.stats[-1]["converged"] and b < 400 and c < 400


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_ae_topo_and_faults_refs_at_full_width_seeds(seed):
    """ae_topo_ref on the complete graph is ae_faults_ref with the same faults; ae_faults_ref with one
    component is the oracle's faulty PUSHPULL."""
    kw = dict(flags=1, churn_fail=ac.FAIL, churn_recover=ac.RECOVER, edge_loss=lt(0.25), partitions=2)
    script = va.ae_script(NFULL, 5, 12, (("faults", 0, 0), ("step", 60)))
    r = ar.RefEngine(NFULL, 5, "antientropy", 2, seed, topology=va.topo("complete"), **kw)
    f = fr.RefEngine(NFULL, 5, "antientropy", 2, seed, **kw)
    fr.assert_same(ar.run_script(r, script, (0, NFULL - 1)), fr.run_script(f, script, (0, NFULL - 1)))
    assert r.lost == f.lost and r.lost[0] > 0
    one_component_is_pushpull(va.AE_N, 3, seed, lt(0.25), 3)


@pytest.mark.parametrize("seed", va.SEEDS, ids=hex)
def test_ae_fault_seed_cases_depend_on_the_high_word(seed):
    """The faulted, topology and sharded ANTIENTROPY seed cases up to their heal, in their restatements:
    under the seed's low word the stats, the rows and the lost edges are others."""
    for (args, kw, script, topology, _), (low, *_) in zip(va.ae_fault_seed_cases(seed), va.ae_fault_seed_cases(seed & LOW)):
        runs = []
        for a in (args, low):
            r = ar.RefEngine(*a, topology=va.topo(topology), **kw) if topology else fr.RefEngine(*a, **kw)
            out = fr.run_script(r, script[:5], va.ae_probe(a[0]))
            runs.append((va.flat(out), out[-1]["rows"], r.lost))
        (s0, rows0, lost0), (s1, rows1, lost1) = runs
        assert s0 != s1 and not np.array_equal(rows0, rows1) and len(s0) == len(s1) >= 12
        assert lost0 != lost1 or not (kw.get("edge_loss") or kw.get("partitions"))


def one_component_is_pushpull(N, k, seed, loss, parts, rounds=20):
    f = fr.RefEngine(N, 1, "antientropy", k, seed, edge_loss=loss, partitions=parts)
    o = op.OracleEngine(N, 1, "pushpull", k, seed, edge_loss=loss, partitions=parts)
    for x in (f, o):
        for n in range(0, N, 37):
            x.inject(n, 0)
    for t in range(rounds):
        a, b = f.step(1), o.step(1)
        assert a.stats[0]["full_nodes"] == b.stats[0]["full_nodes"], t
        assert np.array_equal(f.read_rows()[:, 0].astype(np.uint64), o.read_shard()[0]), t
    o.close()
    return f


# --- seeds: sharded -----------------------------------------------------------------------------------------------

SHARD_RUNS = [sc.RUNS[1], sc.RUNS[2]]      # thirds: push k = 1 without faults, pushpull k = 2 with loss and two blocks


def test_sharded_seed_runs_walk_every_kind():
    """The carousel under SEEDS[0] from slot 0, with both tables: D S R r X C and Q between them, and
    other rounds than under the suite's seed."""
    kinds = set()
    for run in SHARD_RUNS:
        _, want = sc.reference(run, seed=va.SEEDS[0])
        assert want[-1]["converged"] and len(want) >= 8
        assert list(want) != list(sc.reference(run, seed=va.SEEDS[0] & LOW)[1])
        for table in (sc.SLOTS, sc.SLOTS_CC):
            kinds |= set(sc.expected_kinds(table, 0, len(want)))
    assert kinds == {DENSE, SPARSE, EXCHANGE, CLASSCODED, REP_GATHER, REP, REP_CLASSCODED}


def test_sharded_carousel_on_oracle_shards():
    """The GPU file's body on host shards: the sharded protocol under a full-width seed equals the
    one-engine oracle."""
    sc.body_carousel(op.OracleEngine, SHARD_RUNS[1], 3, 0, seed=va.SEEDS[0])


# --- partitions -------------------------------------------------------------------------------------------------

def edge_counts(case, rounds):
    """(lost, kept, lost inside one 64-node group) over the first rounds of a partition-only case, from
    numpy_ref's peers and edge test."""
    N, _, _, k, seed, faults, _ = case
    P = dict(faults)["partitions"]
    n = np.arange(N, dtype=np.int64)
    lost = kept = inside = 0
    for t in range(rounds):
        p = nr.peers(seed, N, t, k).astype(np.int64)
        for j in range(k):
            gone = nr.edge_lost(seed, N, 0, P, n, p[:, j], t, j)
            lost += int(gone.sum())
            kept += int((~gone).sum())
            inside += int((gone & (n >> 6 == p[:, j] >> 6)).sum())
    return lost, kept, inside


@pytest.mark.parametrize("N", [va.N0, va.NMID])
def test_partition_cases(N):
    for P in va.PARTS(N):
        case = va.parts_case(N, P)
        want = agree(case)
        lost, kept, inside = edge_counts(case, 3)
        assert want[0]["rounds"] == va.part_rounds(P)
        before = make(op.OracleEngine, case)
        va.play(before, case[6][:-1])
        if P < N:
            assert lost > 0 and kept > 0, P
            assert not np.array_equal(want[0]["shard"], before.read_shard())
            if P == N - 1:      # the one edge that survives: node 1 has rumor 0 from node 0 after round 0, nobody else moves
                assert kept == 1 and before.read_shard()[0, 1] == 0 and want[0]["shard"][0, 1] == 1
                assert np.array_equal(want[0]["shard"][0, 2:], before.read_shard()[0, 2:])
                assert want[0]["stats"][0]["state_hash"] != want[0]["h0"]
        else:
            assert kept == 0
            assert np.array_equal(want[0]["shard"], before.read_shard()) and want[0]["h0"] == want[0]["h"]
        if P == 257:
            assert inside > 0
        before.close()


@pytest.mark.parametrize("N", sorted(va.PAIR_SEED))
def test_partition_one_less_than_n_keeps_one_pair(N):
    """P = N - 1: every block one node but the block of nodes 0 and 1, and under PAIR_SEED[N] node 0 draws
    node 1 in slot 0 of round 0, which no other case's seed does within the rounds it runs."""
    n = np.arange(N, dtype=np.int64)
    blocks = (n * (N - 1)) // N
    assert np.bincount(blocks).max() == 2 and (np.bincount(blocks, minlength=N - 1) == 2).sum() == 1
    assert blocks[0] == blocks[1] == 0
    assert int(nr.peers(va.PAIR_SEED[N], N, 0, 1, nodes=[0])[0, 0]) == 1
    assert not nr.edge_lost(va.PAIR_SEED[N], N, 0, N - 1, [0], [1], 0, 0)[0]


def test_partition_sender_cases():
    """The sender kernels at NMID nodes, in their restatements: a count below N moves the state, one at or
    above N does not; at N - 1 the only nodes that change are 0 and 1, which list each other first."""
    rp, col = va.topo("pair")
    mid = va.topo("mid")
    assert col[rp[0]] == 1 and col[rp[1]] == 0 and col.size == mid[1].size + 2
    assert np.array_equal(col[rp[2]:], mid[1][mid[0][2]:]) and np.array_equal(np.diff(rp.astype(np.int64))[2:],
                                                                             np.diff(mid[0].astype(np.int64))[2:])
    N = va.NMID
    for P in va.PARTS(N):
        for kind, case, topo_peers in va.sender_part_cases(P):
            ref = {"topo": lambda: topo_sim(case), "monger": lambda: monger_sim(case, topo_peers),
                   "walk": lambda: make(op.OracleEngine, case)}[kind]
            x, y = ref(), ref()
            va.play(x, case[6][:[o[0] for o in case[6]].index("step")])
            before, after = x.read_shard(), va.play(y, case[6])[0]["shard"]
            if kind == "walk":
                x.close(), y.close()
            moved = np.nonzero((before != after).any(axis=0))[0].tolist()
            if P >= N:
                assert moved == [], (kind, P)
            elif P == N - 1:
                assert moved and set(moved) <= {0, 1}, (kind, P, moved)
            else:
                assert len(moved) > 2, (kind, P)


def test_partition_midrun_case():
    case = va.parts_midrun_case(va.N0)
    want = agree(case)
    assert want[0]["h0"] == want[0]["h"] and want[0]["rounds"] == 5            # P = N: nothing moves
    assert want[1]["h"] != want[1]["h0"] and not want[1]["stats"][-1]["converged"]
    assert want[2]["stats"][-1]["converged"]


def test_partitions_in_the_other_restatements():
    """ae_faults_ref with one component against the oracle's PUSHPULL at every count of PARTS: the
    block test the topology, mongering and ANTIENTROPY restatements share (numpy_ref.edge_lost)."""
    for P in va.PARTS(va.AE_N):
        f = one_component_is_pushpull(va.AE_N, 2, va.PAIR_SEED[va.AE_N], 0, P, rounds=6)
        assert f.read_rows()[1, 0] == (P < va.AE_N)       # node 1 has it from node 0, at N - 1 too


def test_partition_cases_antientropy():
    """The partitioned rounds of the GPU case in ae_faults_ref: below N alive-alive edges are lost and others
    exchange, at N - 1 exactly one pair a round does, from N on none."""
    N = va.AE_N
    for P in va.PARTS(N):
        args, kw, script = va.ae_parts_case(P)
        f = fr.RefEngine(*args, **kw)
        out = fr.run_script(f, script[:5], va.AE_PROBE)
        msgs = [s["messages"] for s in va.flat(out)]
        assert len(msgs) == 10 and f.lost[0] > 0 and not any(s["converged"] for s in va.flat(out))
        if P < N - 1:
            assert min(msgs) > 0
        elif P == N - 1:
            assert msgs[0] == 1 and out[0]["alive"][0] and set(msgs) <= {0, 1, 2}
        else:
            assert set(msgs) == {0}


@pytest.mark.parametrize("loss", va.LOSS)
def test_loss_values_in_ae_faults_ref(loss):
    """ae_faults_ref with one component against the oracle's PUSHPULL at every threshold of LOSS."""
    f = one_component_is_pushpull(va.AE_N, 2, st.SEED, loss, 0, rounds=12)
    full = int(f.read_rows()[:, 0].sum())
    if loss == A:
        assert full == (va.AE_N + 36) // 37
    elif loss <= 2 ** 31:
        assert full > va.AE_N // 2


# --- loss and stall -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [0, va.LOSS_D])
@pytest.mark.parametrize("loss", va.LOSS)
def test_loss_cases(loss, D):
    case = va.loss_case(va.N0, loss, D)
    want = agree(case)
    first, healed, rebuilt = want
    assert rebuilt["stats"][-1]["converged"]
    if loss == 1:
        # no draw of these runs is 0: the run is the fault-free run, round for round and in its end state
        clean = oracle(va.loss_case(va.N0, 0, D))
        assert [va.flat([e]) for e in want] == [va.flat([e]) for e in clean]
        assert all(np.array_equal(a["shard"], b["shard"]) for a, b in zip(want, clean))
    if loss == A:
        # no draw of these runs is 0xFFFFFFFF: no state bit changes under the loss
        assert first["rounds"] == 2 * va.LOSS_D + 2 and first["h0"] == first["h"]
        assert len({s["state_hash"] for s in first["stats"]}) == 1
        if D:    # every node stalled after D rounds: healed, it still initiates nothing, until reset
            assert healed["h"] == healed["h0"] and healed["rounds"] == 4
        else:    # healed, the run moves again
            assert healed["h"] != healed["h0"]
    if loss == 2 ** 31 and not D:
        assert first["h"] != first["h0"]


def test_everyone_stalled_after_d_rounds():
    """Total loss with a deadline of D: numpy_ref.Sim's streaks are all at D after D rounds and stay."""
    case = va.loss_case(va.N0, A, va.LOSS_D)
    s = make(SimEngine, case)
    va.sprinkle(s, 3)
    s.step(va.LOSS_D)
    assert (s.sim.streak == va.LOSS_D).all()
    s.set_faults(0, 0)
    s.step(3)
    assert (s.sim.streak == va.LOSS_D).all()


@pytest.mark.parametrize("D", va.STALL)
def test_stall_cases(D):
    for mode in va.MODES:
        case = va.stall_case(va.N0, D, mode)
        want = agree(case)
        free = oracle(case[:5] + ((("edge_loss", va.STALL_LOSS[D][0]),),) + case[6:])
        # the first D rounds are those of the run without a deadline; the round after them is not: nodes that lost
        # an edge in each of rounds 0 .. D - 1 initiate nothing in round D
        assert want[0]["rounds"] == va.STALL_ROUNDS > D + 1 and not want[0]["stats"][-1]["converged"]
        assert want[0]["stats"][:D] == free[0]["stats"][:D] and want[0]["stats"][D] != free[0]["stats"][D]
        s = make(SimEngine, case)
        va.play(s, case[6][:1])
        s.step(D)
        first = s.sim.streak.copy()
        # after D rounds some nodes are stalled and some are not, one round short of it among them
        assert first.max() == D and va.N0 // 8 < (first == D).sum() < va.N0 - va.N0 // 8 and (first == D - 1).any()
        s.step(va.STALL_ROUNDS - D)
        last = s.sim.streak >= D
        assert s.sim.streak.max() == D and last.sum() > (first == D).sum()      # more of them in the rounds after
        s.set_faults(0, 0)
        s.step(8)
        assert np.array_equal(s.sim.streak >= D, last)     # healed: nobody stalls any more, nobody comes back
        # D = 1: every node is stalled by then and the healed run stands still; D = 16: the others carry on
        assert last.all() == (D == 1) and (want[1]["h"] == want[1]["h0"]) == (D == 1)
    topo = va.topo_case("mid", 3, "pushpull", 2, st.SEED, va.STALL_ROUNDS, edge_loss=lt(0.3), stall_rounds=D)
    assert va.play(topo_sim(topo), topo[6])[0]["stats"][0]["messages"] > 0


# --- churn ------------------------------------------------------------------------------------------------------------

def ae_pair(K, k, fail, rec, script, seed=st.SEED):
    kw = dict(flags=1, churn_fail=fail, churn_recover=rec)
    o = op.OracleEngine(va.AE_N, K, "antientropy", k, seed, **kw)
    f = fr.RefEngine(va.AE_N, K, "antientropy", k, seed, **kw)
    want = fr.run_script(o, script, va.AE_PROBE)
    fr.assert_same(fr.run_script(f, script, va.AE_PROBE), want)
    o.close()
    return want


@pytest.mark.parametrize("fail,rec", va.CHURN)
@pytest.mark.parametrize("K,k", [(5, 2), (16, 4)])
def test_churn_cases(K, k, fail, rec):
    N = va.AE_N
    want = ae_pair(K, k, fail, rec, va.churn_script(N, K))
    alive = [s["alive_nodes"] for s in va.flat(want)]
    singles = want[:9]
    assert all(len(e["stats"]) == 1 for e in singles)
    if (fail, rec) in ((0, 0), (0, A)):
        assert set(alive) == {N}
    if (fail, rec) == (A, 0):      # no draw is 0xFFFFFFFF: all dead from round 0 on, 0 == 0 converged, no message
        assert set(alive) == {0}
        assert all(s["converged"] == 1 and s["messages"] == 0 and s["full_nodes"] == 0 for s in va.flat(want))
    if (fail, rec) == (A, A):      # every alive bit flips every round (no draw is 0xFFFFFFFF)
        assert alive[:9] == [0, N, 0, N, 0, N, 0, N, 0]
        assert all(not any(e["alive"]) for e in singles[0::2]) and all(all(e["alive"]) for e in singles[1::2])
        assert singles[4]["stats"][0]["alive_nodes"] == 0      # the first write lands while every node is dead
        assert singles[1]["stats"][0]["messages"] > 0
    if (fail, rec) == (2 ** 31, 2 ** 31):
        assert 0 < min(alive) and max(alive) < N


# --- long runs ----------------------------------------------------------------------------------------------------------

def test_300_rounds():
    case = va.long_case(va.N0, va.LONG[0])
    stood, healed = agree(case)
    assert stood["rounds"] == 300 and not stood["stats"][-1]["converged"]
    assert healed["stats"][0]["round"] == 300 and healed["stats"][-1]["converged"] and healed["h"] != healed["h0"]
    topo = va.topo_case("mid", 3, "pushpull", 2, st.SEED, 300, (("faults", 0, 0), ("step", 8)), partitions=2)
    a, b = va.play(topo_sim(topo), topo[6])
    assert a["rounds"] == 300 and b["h"] != b["h0"]


def test_65600_rounds():
    """The C oracle runs them all.  numpy_ref.Sim runs the first 64, by when each block holds its union
    in every node: a fixed point under the standing partition (a round only ORs words of one block
    together), so its round index is set to 65600 for the heal, and the rounds whose draws decide
    the end are compared: t > 2^16 in word 1 of every counter."""
    case = va.long_case(va.NLONG, va.LONG[1], infected=False)
    stood, healed = oracle(case)
    assert stood["rounds"] == 65600 and not stood["stats"][-1]["converged"]
    assert len({s["state_hash"] for s in stood["stats"][64:]}) == 1
    assert healed["stats"][0]["round"] == 65600 and healed["stats"][-1]["converged"] and healed["rounds"] >= 2
    s = make(SimEngine, case)
    for op_ in case[6][:3]:
        s.inject(*op_[1:])
    first = s.step(64)
    assert first.stats == stood["stats"][:64]
    S = s.sim.S[0]
    half = (np.arange(va.NLONG) * 2) // va.NLONG
    assert all(len(set(S[half == b].tolist())) == 1 for b in (0, 1))     # the fixed point
    s.sim.t = 65600
    s.set_faults(0, 0)
    s.inject(1, 0)
    last = s.step(va.CAP)
    assert last.stats == healed["stats"] and np.array_equal(s.read_shard(), healed["shard"])
    # healed at t = 64 instead, the same state takes another way to the end
    early = oracle(case[:6] + (case[6][:3] + (("step", 64, False),) + case[6][4:],))[1]
    assert [x["state_hash"] for x in early["stats"]] != [x["state_hash"] for x in healed["stats"]]
