"""GPU: every round path at the ends of the scalar config values (tests/values.py): full-width seeds
(both Philox key words in use), partition counts from 5 to 2^32 - 1, loss thresholds 1 and 2^32 - 1,
stall deadlines 1 and 16, churn thresholds 0 and 2^32 - 1, and round indices past 2^8 and 2^16; bit for
bit against the C oracle and the numpy restatements: the state hash before the first round, per-round
stats (with FLAG_HASH: the hash of every node's word after every round), the per-rumor or
per-component counts, the full readout (read_shard / read_rows, read_hot / read_counts), sampled alive
flags and the final hash.

tests/test_value_tables.py shows from the restatements alone that the cases mean something: a
full-width seed runs otherwise than its low word, the partition counts lose and keep edges, the loss
and churn ends do what their names say, the long runs end on late draws.  References are computed
once per case and shared by the paths (read only)."""
import functools

import numpy as np
import pytest

import ae_cases as ac
import ae_faults_ref as fr
import ae_topo_ref as ar
import monger_counter_ref as mc
import numpy_ref as nr
import oracle_py as op
import shard_cases as sc
import states as st
import topo_ref as tr
import values as va
from gossip_hip import FLAG_AE_TOPO_PEERS, FLAG_HASH, FLAG_MONGER, FLAG_TIMING, FLAG_TOPO_PEERS, Engine
from gossip_hip.engine import loss_threshold as lt, peer, topo_peer_index
from gossip_hip.sharded import lockstep_run
from shard_cases import GroupDriver

pytestmark = pytest.mark.gpu
A = va.A
FOUR = ["auto", "dense", "sparse", "direct"]
SIX = FOUR + ["dense_filter", "sparse_bscan"]
HEX = [hex(s) for s in va.SEEDS]


# --- references, computed once ------------------------------------------------------------------------

def build(cls, case, **kw):
    N, R, mode, k, seed, faults, _ = case
    return cls(N, R, mode, k, seed, **dict(faults), **kw)


@functools.lru_cache(maxsize=None)
def oracle(case):
    o = build(op.OracleEngine, case, flags=FLAG_HASH)
    out = va.play(o, case[6])
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def topo_ref(case):
    return va.play(build(tr.TopoSim, case), case[6])


@functools.lru_cache(maxsize=None)
def monger_ref(case, topo_peers):
    N, R, _, k, seed, faults, script = case
    return va.play(mc.MongerCounterSim(N, R, k, seed, topo_peers=topo_peers, **dict(faults)), script, va.MONGER_READS)


def check(case, path="auto", want=None, flags=0, reads=()):
    """One HIP engine on one round path through the case's script, against `want` (default: the oracle).
    On a forced path the round timers show that every round ran on that pipeline (timer 3 counts the
    dense rounds, timer 4 the frontier rounds, the pull shortcut's among them)."""
    pf, params = st.path_of(path)
    want = oracle(case) if want is None else want
    forced = path.startswith(("dense", "sparse"))
    with build(Engine, case, flags=FLAG_HASH | pf | flags | (FLAG_TIMING if forced else 0), params=params) as e:
        va.same(va.play(e, case[6], reads), want)
        if forced:
            rounds = sum(w["rounds"] for w in want)
            ran = (e.kernel_time(3)[1], e.kernel_time(4)[1])
            assert ran == ((rounds, 0) if path.startswith("dense") else (0, rounds)), (path, ran)
    return want


def check_topo(case):
    return check(case, want=topo_ref(case), flags=FLAG_TOPO_PEERS)


def check_monger(case, topo_peers):
    return check(case, want=monger_ref(case, topo_peers), flags=FLAG_MONGER | (FLAG_TOPO_PEERS if topo_peers else 0),
                 reads=va.MONGER_READS)


def check_shards(case, G, params=None):
    """G HIP shards on one device in lockstep through the case's script, against the one-engine oracle."""
    want = oracle(case)
    engines = [build(Engine, case, flags=FLAG_HASH, shard_rank=r, shard_count=G, params=params) for r in range(G)]
    try:
        steps = iter(want)
        for op_ in case[6]:
            if op_[0] == "step":
                w = next(steps)
                stats, _ = lockstep_run(engines, op_[1])
                assert stats == w["stats"]
                for e in engines:
                    assert np.array_equal(e.read_shard(), w["shard"][:, e.lo:e.hi]), e.cfg.shard_rank
            else:
                for e in engines:
                    va.play(e, (op_,))
    finally:
        sc.close_all(engines)
    return want


# --- a. seeds: the random modes ---------------------------------------------------------------------------

@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("path", st.PATHS)
def test_seeds_random_modes(path, seed):
    """Per mode a fault-free run from Philox origins and one with loss 0.2, P = 3, D = 2."""
    for case in va.seed_cases(path, seed):
        check(case, path)


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
def test_seeds_pull_shortcut(seed):
    for case in va.fullpull_cases(seed):
        check(case, "sparse")


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("path", ["auto", "direct"])
def test_seeds_three_words(path, seed):
    for case in va.wide_cases(seed):
        check(case, path)


# --- b. seeds: the sender kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
def test_seeds_topo_peers(seed):
    for case in va.topo_seed_cases(seed):
        check_topo(case)


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("i", range(len(va.MONGER)))
def test_seeds_mongering(i, seed):
    peers, R, k, cool, blind, limit, loss = va.MONGER[i]
    case, topo_peers = va.monger_case(peers, R, k, cool, blind, limit, seed, edge_loss=loss)
    want = check_monger(case, topo_peers)
    assert want[0]["stats"][-1]["messages"] == 0 and want[0]["rounds"] < va.CAP


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
def test_seeds_flood_walks(seed):
    want = check(va.walk_case(seed))
    assert want[0]["stats"][0]["messages"] > 0 and want[0]["rounds"] > 3


# --- c. seeds: ANTIENTROPY -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ae_oracle(K, k, seed):
    args, kw = ac.engine_args(K, k, seed=seed)
    o = op.OracleEngine(*args, threads=16, **kw)
    r = ac.run(o)
    h = o.state_hash()
    o.close()
    return r, h


AE_SEED_ITEMS = [(K, k, path) for K, k in va.AE_PAIRS for path in ac.paths_of(K, k)]


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("K,k,path", AE_SEED_ITEMS, ids=[f"K{K}-k{k}-{p}" for K, k, p in AE_SEED_ITEMS])
def test_seeds_antientropy(K, k, path, seed):
    want, h = ae_oracle(K, k, seed)
    args, kw = ac.engine_args(K, k, seed=seed)
    pf, params = ac.PATHS[path]
    kw["flags"] |= pf
    with Engine(*args, params=params, **kw) as e:
        ac.assert_same(ac.run(e), want)
        assert e.state_hash() == h


ae_kw, ae_args = va.ae_kw, va.ae_args


@functools.lru_cache(maxsize=None)
def ae_ref(args, kwitems, script, topology=None):
    """(run_script's result, lost alive-alive edges per round) of ae_faults_ref, or of ae_topo_ref over
    a topology of values.topo."""
    if topology:
        r = ar.RefEngine(*args, topology=va.topo(topology), **dict(kwitems))
    else:
        r = fr.RefEngine(*args, **dict(kwitems))
    return fr.run_script(r, script, va.ae_probe(args[0])), tuple(r.lost)


def check_ae(args, kw, script, path="auto", topology=None, G=0):
    """One engine on a path of ae_cases.PATHS, or G shards in lockstep, against the restatement."""
    want, lost = ae_ref(args, tuple(sorted(kw.items())), script, topology)
    pf, params = ac.PATHS[path]
    params = dict(params)
    if topology and path == "sparse":   # room for every exchange
        params["ae_cap"] = 2 * args[0] * args[3]
    kw = dict(kw, flags=kw["flags"] | pf | (FLAG_AE_TOPO_PEERS if topology else 0))
    if G:
        engines = [Engine(*args, shard_rank=r, shard_count=G, **kw) for r in range(G)]
        try:
            got = fr.run_script(engines, script)
            fr.assert_same(got, want, keys=("stats", "rows"))
        finally:
            sc.close_all(engines)
        return want, lost
    with Engine(*args, params=params, **kw) as e:
        if topology:
            e.set_topology(va.topo(topology))
        fr.assert_same(fr.run_script(e, script, va.ae_probe(args[0])), want)
        assert e.state_hash() == va.flat(want)[-1]["state_hash"]
    return want, lost


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_seeds_antientropy_faults(path, seed):
    """Loss 0.25 and two partitions for 12 rounds with two writes, then the heal."""
    args, kw, script, _, _ = va.ae_fault_seed_cases(seed)[0]
    want, lost = check_ae(args, kw, script, path)
    assert lost[0] > 0 and want[-1]["stats"][-1]["converged"]


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_seeds_antientropy_topo(path, seed):
    """Over the ragged rows (nodes nobody points at: it never converges), with loss."""
    args, kw, script, topology, _ = va.ae_fault_seed_cases(seed)[1]
    want, lost = check_ae(args, kw, script, path, topology=topology)
    assert lost[0] > 0 and va.flat(want)[-1]["messages"] > 0


@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
def test_seeds_antientropy_sharded(seed):
    """G = 3: shards of 1408, 1408 and 1283 nodes; without faults (the C oracle's run, restated) and with."""
    for args, kw, script, _, G in va.ae_fault_seed_cases(seed)[2:]:
        want, _ = check_ae(args, kw, script, G=G)
        assert want[-1]["stats"][-1]["converged"]


# --- d. seeds: sharded --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("table", ["slots", "slots_cc"])
@pytest.mark.parametrize("run", [sc.RUNS[1], sc.RUNS[2]], ids=sc.run_id)
def test_seeds_sharded_carousel(run, table, driver):
    """The plan carousel at G = 3 under SEEDS[0]: the two tables walk D S R r X C and Q between them
    (test_value_tables.py), without faults and with loss 0.5 under two partitions."""
    group = driver == "group"
    sc.body_carousel(None if group else Engine, run, 3, 0, sc.SLOTS if table == "slots" else sc.SLOTS_CC,
                     driver=GroupDriver if group else None, seed=va.SEEDS[0])


# --- e. seeds: the host probes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", va.SEEDS, ids=HEX)
def test_seeds_host_probes(seed):
    """gossip_peer and gossip_topo_peer_index against numpy_ref.peers and topo_ref.row_index."""
    N, nodes = va.N0, [0, 1, 63, 64, 8191, va.N0 - 1]
    for t in (0, 1, 255, 256, 65536, 2 ** 32 - 1):
        want = nr.peers(seed, N, t, 6, nodes=nodes)
        for i, n in enumerate(nodes):
            for j in range(6):
                assert peer(seed, N, n, t, j) == int(want[i, j]), (n, t, j)
                for deg in (1, 7, 300):
                    assert topo_peer_index(seed, deg, n, t, j) == int(tr.row_index(seed, deg, [n], t, j)[0]), (n, t, j, deg)
    assert topo_peer_index(seed, 0, 5, 3, 0) == 0


# --- f. partitions -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", va.PARTS(va.N0))
@pytest.mark.parametrize("path", FOUR)
def test_partitions(path, P):
    check(va.parts_case(va.N0, P), path)


@pytest.mark.parametrize("P", [257, va.N0])
@pytest.mark.parametrize("path", st.PATHS)
def test_partitions_every_path(path, P):
    for mode in va.MODES:
        check(va.parts_case(va.N0, P, mode, va.fanout(path, mode)), path)


@pytest.mark.parametrize("path", FOUR)
def test_partitions_change_midrun(path):
    """P = N for five rounds, seven blocks for five, then healed to convergence."""
    want = check(va.parts_midrun_case(va.N0), path)
    assert want[2]["stats"][-1]["converged"]


@pytest.mark.parametrize("P", va.PARTS(va.N0))
@pytest.mark.parametrize("plan", ["auto", "sparse", "dense"])
def test_partitions_sharded(plan, P):
    """G = 3 over 16449 = 3 x 5483 nodes: no block edge of 5, 7 or 257 blocks falls on a shard edge."""
    params = {} if plan == "auto" else {"sparse_frac": 1.0 if plan == "sparse" else -1}
    check_shards(va.parts_case(va.N0, P), 3, params)


@pytest.mark.parametrize("P", va.PARTS(va.NMID))
def test_partitions_sender_kernels(P):
    """GOSSIP_FLAG_TOPO_PEERS, mongering over the rows and uniform, and the FLOOD walks at NMID nodes: a
    count below N moves the state (at N - 1: nodes 0 and 1 alone, test_value_tables.py), one from N on does not."""
    for kind, case, topo_peers in va.sender_part_cases(P):
        want = {"topo": check_topo, "walk": check}[kind](case) if kind != "monger" else check_monger(case, topo_peers)
        assert (want[0]["h"] != want[0]["h0"]) == (P < va.NMID), kind


@pytest.mark.parametrize("P", va.PARTS(va.AE_N))
@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_partitions_antientropy(path, P):
    """Ten rounds under P blocks with two writes, then the heal and the run to convergence."""
    args, kw, script = va.ae_parts_case(P)
    want, lost = check_ae(args, kw, script, path)
    assert lost[0] > 0 and not any(s["converged"] for s in va.flat(want[:2])) and want[-1]["stats"][-1]["converged"]
    # below N some alive-alive edge gets through in every round but at N - 1, where the one pair meets in round 0
    msgs = [s["messages"] for s in va.flat(want[:2])]
    assert (min(msgs) > 0 if P < va.AE_N - 1 else msgs[0] == 1 if P == va.AE_N - 1 else max(msgs) == 0), msgs


# --- g. loss ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", va.LOSS)
@pytest.mark.parametrize("path", SIX)
def test_loss(path, loss):
    """2 D + 2 rounds, the heal, four rounds, reset and a run to convergence; without a deadline and with
    D = 2 (under 2^32 - 1 every node is stalled after two rounds and the heal moves nothing)."""
    for D in (0, va.LOSS_D):
        want = check(va.loss_case(va.N0, loss, D), path)
        assert want[2]["stats"][-1]["converged"]


@pytest.mark.parametrize("loss", va.LOSS)
def test_loss_sender_kernels(loss):
    heal = (("faults", 0, 0), ("step", va.CAP))
    check_topo(va.topo_case("mid", 3, "pushpull", 2, st.SEED, 6, heal, edge_loss=loss, stall_rounds=2))
    for peers, R, k, cool, blind, limit, _ in va.MONGER:
        case, topo_peers = va.monger_case(peers, R, k, cool, blind, limit, st.SEED, rounds=12, tail=heal, edge_loss=loss)
        check_monger(case, topo_peers)
    check(va.walk_case(st.SEED, heal, edge_loss=loss, stall_rounds=2))


@pytest.mark.parametrize("loss", va.LOSS)
@pytest.mark.parametrize("path", ["auto", "dense", "dense_atomic", "sparse", "sparse_direct"])
def test_loss_antientropy(path, loss):
    script = va.ae_script(va.AE_N, 5, 6, (("step", 6), ("faults", 0, 0), ("step", 400)))
    want, lost = check_ae(ae_args(5, 2), ae_kw(edge_loss=loss), script, path)
    assert want[-1]["stats"][-1]["converged"]
    if loss == A:
        assert all(s["messages"] == 0 for s in va.flat(want[:2]))


# --- h. stall -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", va.STALL)
@pytest.mark.parametrize("path", FOUR)
def test_stall(path, D):
    """STALL_LOSS[D] for 24 rounds: some nodes are stalled after D rounds and more in each round after
    (test_value_tables.py), then the heal, under which none of them comes back."""
    for mode in va.MODES:
        check(va.stall_case(va.N0, D, mode), path)


@pytest.mark.parametrize("D", va.STALL)
def test_stall_topo_peers(D):
    for mode, k, R in (("pushpull", 2, 3), ("push", 5, 130), ("pull", 4, 3)):
        check_topo(va.topo_case("mid", R, mode, k, st.SEED, va.STALL_ROUNDS, edge_loss=lt(0.3), stall_rounds=D))


# --- i. churn -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fail,rec", va.CHURN, ids=[f"{f:#x}-{r:#x}" for f, r in va.CHURN])
@pytest.mark.parametrize("path", ["auto", "dense", "dense_atomic", "sparse", "sparse_direct"])
def test_churn(path, fail, rec):
    """Single-round steps, a write while every node is dead ((A, 0) and the odd rounds of (A, A))."""
    for K, k in ((5, 2), (16, 4)):
        want, _ = check_ae(ae_args(K, k), ae_kw(fail, rec), va.churn_script(va.AE_N, K), path)
        if (fail, rec) == (A, A):
            assert [s["alive_nodes"] for s in va.flat(want)][:4] == [0, va.AE_N, 0, va.AE_N]


@pytest.mark.parametrize("fail,rec", va.CHURN, ids=[f"{f:#x}-{r:#x}" for f, r in va.CHURN])
def test_churn_sharded(fail, rec):
    check_ae(ae_args(5, 2), ae_kw(fail, rec), va.churn_script(va.AE_N, 5), G=2)


# --- j. rounds ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", st.PATHS)
def test_300_rounds(path):
    mode = va.MODES[st.PATHS.index(path) % 3]
    want = check(va.long_case(va.N0, va.LONG[0], mode, min(va.fanout(path, mode), 3)), path)
    assert want[0]["rounds"] == 300 and want[1]["stats"][-1]["converged"]


def test_300_rounds_sender_kernels():
    heal = (("faults", 0, 0), ("step", 8))
    want = check_topo(va.topo_case("mid", 3, "pushpull", 2, st.SEED, 300, heal, partitions=2))
    assert want[0]["rounds"] == 300 and want[1]["h"] != want[1]["h0"]
    # cool = 1 / 2^32: no coin ever holds, every rumor stays hot and the run never goes quiet
    case, topo_peers = va.monger_case("mid", 3, 2, 1, False, None, st.SEED, rounds=300, tail=heal, partitions=2)
    want = check_monger(case, topo_peers)
    assert want[0]["rounds"] == 300 and want[1]["stats"][-1]["messages"] > 0 and want[1]["h"] != want[1]["h0"]


@pytest.mark.parametrize("path", ["auto", "sparse"])
def test_300_rounds_antientropy(path):
    script = (("random",), ("step", 300), ("faults", 0, 0)) + va.ae_writes(va.AE_N, 5) + (("step", 400),)
    want, _ = check_ae(ae_args(5, 2), ae_kw(partitions=2), script, path)
    assert len(want[0]["stats"]) == 300 and want[1]["stats"][-1]["converged"]


@pytest.mark.parametrize("path", ["direct", "auto"])
def test_65600_rounds(path):
    want = check(va.long_case(va.NLONG, va.LONG[1], infected=False), path)
    assert want[0]["rounds"] == 65600 and want[1]["stats"][-1]["converged"]
