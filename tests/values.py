"""Scalar config values at the ends of what gossip_config_t and gossip_set_faults accept, and the
cases run at them; shared by test_value_tables.py (CPU) and test_gpu_values.py.  A plain module, not a
conftest; it holds tables, scripts and helpers, no tests.  tests/sizes.py does the same for the node
count; here N stays small and the seed, the partition count, the loss threshold, the stall deadline,
the churn thresholds and the round index move.

A script is a tuple of ops that `play` applies to any engine of the ABI (HIP, C oracle, or a numpy
restatement behind the same calls), so the same tuple drives both sides of a comparison:
  ("build", name, R)  a builder of BUILDERS        ("inject", node, rumor)
  ("topology", name)  set_topology(topo(name))                 ("monger", cool, blind) / ("limit", m)
  ("faults", l, P)    set_faults                    ("reset",)
  ("step", rounds)    one step call; ("step", rounds, False): without the per-rumor counts
ANTIENTROPY scripts are those of ae_faults_ref.run_script.
"""
import functools

import numpy as np

import ae_cases as ac
import numpy_ref as nr
import sizes as sz
import states as st
import topo_ref as tr
import topologies as tp
from gossip_hip import FLAG_HASH, loss_threshold as lt, total_topology

A = 2 ** 32 - 1          # the largest threshold: every draw but 0xFFFFFFFF is below it
N0 = st.N0               # 16449: two 16384-node tiles, the second a ragged 64-node group and one node
NMID = 3001              # the one-lane-per-sender kernels: twelve blocks of 256, a ragged last wave
NROWS = 30011            # the ragged rows of test_gpu_topo_peers.py
NLONG = 130              # the 65600-round run: three bitmap words, the last of two nodes
NWALK = 301              # the FLOOD walks on the CPU
NFULL = 257              # the complete topology of the CPU identities
AE_N = 4099              # ANTIENTROPY's fault, churn and long cases: a ragged chunk, two sparse-scan tiles
MODES = ("push", "pull", "pushpull")
# P = N - 1 leaves one block of two nodes, 0 and 1, and blocks of one.  Under PAIR_SEED[N] node 0 draws node 1
# in slot 0 of round 0 (any fanout), so the one edge that survives is used in the first round of every
# partition case: node 0 holds rumor 0 in every builder below, and a random row of its own under ANTIENTROPY.
PAIR_SEED = {N0: 0x5EED5F9D, NMID: 0x5EED188E, AE_N: 0x5EED3B10}

# --- the tables --------------------------------------------------------------------------------------
SEEDS = [
    0x9E3779B97F4A7C15,  # key0 != key1, both nonzero: a dropped or a swapped key word changes every draw
    0xDEADBEEF00000000,  # key0 = 0: a kernel that reads key1 where key0 belongs sees the wrong stream
    0xFFFFFFFFFFFFFFFF,  # both words all ones: the key schedule's additions wrap in the first round
]


def PARTS(N):
    """The partition counts run at N nodes."""
    return ([5, 7]                      # divide none of the test sizes: every block edge is a ceiling
            + ([257] if N == N0 else [])  # blocks of 64.004 nodes: edges at every offset in the 64-node groups,
                                          # and one block across the 16384 tile edge
            + [N - 1,                   # blocks of one node, but one of two
               N,                       # blocks of one node: no edge survives
               N + 1,                   # more blocks than nodes: some blocks are empty
               2 ** 31,                 # n * P needs 64 bits, q * N + P - 1 passes 2^32
               A])                      # the largest count the field holds


LOSS = [
    1,          # only a draw of 0 is lost: the smallest loss that is on
    2 ** 31,    # the sign bit of the comparison
    A - 1,      # draws of 0xFFFFFFFE and 0xFFFFFFFF get through
    A,          # total loss but for a draw of 0xFFFFFFFF: no state bit changes
]
STALL = [
    1,          # one lost round stalls a node for good
    16,         # the documented maximum of stall_rounds
]
CHURN = [       # (churn_fail, churn_recover)
    (0, 0),     # churn off: alive_nodes = N throughout
    (A, 0),     # every node dies in round 0 and stays dead: alive_nodes = 0, converged (0 == 0)
    (A, A),     # every alive bit flips every round
    (0, A),     # nobody dies, so nobody is ever there to recover
    (2 ** 31, 2 ** 31),  # the sign bit of both comparisons
]
LONG = [
    300,        # t past 2^8
    65600,      # t past 2^16
]
# the loss and the builder under which each deadline of STALL is run (k = 2; a node's streak grows while any of
# its edges is lost).  Loss 0.3 loses an edge of a node in 51 % of the rounds: half of the nodes are stalled after
# round 0 and all of them long before STALL_ROUNDS.  Loss 0.8 does so in 96 %: 0.96^16 = 52 % of the nodes reach
# a streak of 16 in the first 16 rounds and more in each round after, while others stand at 15 or are back at 0;
# from `ends` (three holders) no mode converges under it within STALL_ROUNDS (PUSHPULL from sprinkle would, under
# loss 0.7 before round 16)
STALL_LOSS = {1: (lt(0.3), "sprinkle"), 16: (lt(0.8), "ends")}

# the faulted run of the seed cases: loss 0.2 + three partitions (never converges) + a deadline of two rounds
FAULTY = (("edge_loss", lt(0.2)), ("partitions", 3), ("stall_rounds", 2))
CAP = 128               # rounds: every random-mode case that can converge does so sooner
FAULT_ROUNDS = 16
LOSS_D = 2              # the deadline of the LOSS cases: 2 D + 2 rounds, then the heal


# --- builders ----------------------------------------------------------------------------------------

def sprinkle(engine, R):
    """Rumor i % R at node 37 i: a holder in nearly every 64-node group, so under any partition count
    below N the first round already has edges inside a block that carry something."""
    N = engine.n_nodes if hasattr(engine, "n_nodes") else engine.N
    for i, n in enumerate(range(0, N, 37)):
        engine.inject(n, i % R)
    return (N + 36) // 37


def ends(engine, R):
    """Rumor r at the node r (N - 1) / (R - 1): the first and the last node hold something, whatever N."""
    N = engine.n_nodes if hasattr(engine, "n_nodes") else engine.N
    for r in range(R):
        engine.inject(r * (N - 1) // max(R - 1, 1), r)
    return R


def quarter(engine, R):
    """Full-majority for several rounds: n % 4 == 3 holds rumor n % R alone, every other node is full but
    the boundary nodes of sizes.py, which are empty."""
    N = engine.n_nodes if hasattr(engine, "n_nodes") else engine.N
    empty = set(sz.boundary_nodes(N))
    calls = 0
    for n in range(N):
        if n in empty:
            continue
        for r in ((n % R,) if n % 4 == 3 else range(R)):
            engine.inject(n, r)
            calls += 1
    return calls


def cut_injects(N, P, R=3):
    """Inject ops that put a rumor on both sides of every cut of P blocks (up to 257: from N - 1 on a
    block is one node): rumor q % R at the last node of block q, rumor (q + 1) % R at the first node of
    block q + 1.  A block edge that is off by one moves exactly these nodes, and they exchange from
    round 0 on."""
    if P > 257:
        return ()
    out = []
    for q in range(P - 1):
        first = -(-(q + 1) * N // P)          # the first node of block q + 1: ceil((q + 1) N / P)
        out += [("inject", first - 1, q % R), ("inject", first, (q + 1) % R)]
    return tuple(out)


def random(engine, R):
    engine.inject_random()
    return 1


BUILDERS = {"random": random, "sprinkle": sprinkle, "ends": ends, "quarter": quarter}


# --- play and same -----------------------------------------------------------------------------------

def hash_of(x):
    return x.state_hash() if hasattr(x, "state_hash") else nr.state_hash(x.read_shard())


def play(x, script, reads=()):
    """Applies `script` to x; one entry per step: the hash before it, the step's rounds, stats and
    per-rumor counts, the whole state and its hash after it, and whatever `reads` names (methods or
    properties of x, read after the step: read_hot, read_counts, round_index)."""
    out = []
    for op in script:
        if op[0] == "step":
            h0 = hash_of(x)
            res = x.step(op[1], with_infected=False) if len(op) > 2 else x.step(op[1])
            extra = {}
            for name in reads:
                v = getattr(x, name)
                extra[name] = v() if callable(v) else v
            out.append(dict(h0=h0, rounds=res.rounds, stats=list(res.stats),
                            infected=None if len(op) > 2 else np.array(res.infected), shard=x.read_shard(),
                            h=hash_of(x), extra=extra))
        elif op[0] == "build":
            BUILDERS[op[1]](x, *op[2:])
        else:
            name = {"inject": "inject", "topology": "set_topology", "monger": "set_monger", "limit": "set_monger_limit",
                    "faults": "set_faults", "reset": "reset"}[op[0]]
            getattr(x, name)(*((topo(op[1]),) if op[0] == "topology" else op[1:]))
    return out


def same(got, want, messages=True):
    """Bit-exact equality of two play() results; messages=False: but for stats.messages (the complete
    topology's identity: the uniform draw counts no messages)."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["h0"] == w["h0"], i
        assert g["rounds"] == w["rounds"], (i, g["rounds"], w["rounds"])
        for t, (a, b) in enumerate(zip(g["stats"], w["stats"])):
            if not messages:
                a, b = dict(a, messages=0), dict(b, messages=0)
            assert a == b, (i, t, a, b)
        assert (g["infected"] is None) == (w["infected"] is None)
        if g["infected"] is not None:
            assert np.array_equal(g["infected"], w["infected"]), i
        assert np.array_equal(g["shard"], w["shard"]), i
        assert g["h"] == w["h"], i
        assert sorted(g["extra"]) == sorted(w["extra"])
        for name, v in g["extra"].items():
            assert np.array_equal(v, w["extra"][name]), (i, name)


def flat(out):
    return [s for o in out for s in o["stats"]]


# --- random modes: a case is (N, R, mode, k, seed, faults as sorted items, script) ---------------------------

def fanout(path, mode):
    """k rotates over 1 .. 6 with the path and the mode (5 and 6: a second Philox block of peer and of
    loss draws); the binned scan takes k <= 4."""
    k = (st.PATHS.index(path) + 2 * MODES.index(mode)) % 6 + 1
    return (k - 1) % 4 + 1 if path == "sparse_bscan" else k


def case(N, R, mode, k, seed, script, **faults):
    return (N, R, mode, k, seed, tuple(sorted(faults.items())), tuple(script))


def seed_cases(path, seed):
    """Per mode one fault-free run to convergence from Philox origins (stream tag 2) and one faulted
    run of FAULT_ROUNDS rounds."""
    out = []
    for mode in MODES:
        k = fanout(path, mode)
        out.append(case(N0, 7, mode, k, seed, (("build", "random", 7), ("step", CAP))))
        out.append(case(N0, 7, mode, k, seed, (("build", "random", 7), ("step", FAULT_ROUNDS)), **dict(FAULTY)))
    return out


NHOLES = 4097


def fullpull_cases(seed):
    """test_gpu_fullpull's workload: a full-majority state (quarter) in the pulling modes, which
    the sparse path (sparse_frac 1) sends down the pull shortcut; clean and with loss."""
    s = (("build", "quarter", 3), ("step", CAP))
    return [case(NHOLES, 3, "pull", 1, seed, s), case(NHOLES, 3, "pushpull", 2, seed, s),
            case(NHOLES, 3, "pull", 2, seed, s, edge_loss=lt(0.2), stall_rounds=2)]


def wide_cases(seed):
    """Three words per node with a ragged last word."""
    return [case(NMID, 130, "pushpull", 5, seed, (("build", "random", 130), ("step", CAP))),
            case(NMID, 130, "push", 2, seed, (("build", "random", 130), ("step", FAULT_ROUNDS)), **dict(FAULTY))]


PART_ROUNDS = 10


def part_rounds(P):
    """Uniform peers at N0 nodes seldom fall into one block of 64: a node at a cut of 257 blocks is on an
    edge inside its block in about one round of forty (k = 3), so that case runs 128 rounds."""
    return 128 if P == 257 else PART_ROUNDS


def parts_case(N, P, mode="pushpull", k=3):
    """PART_ROUNDS rounds under P blocks from sprinkle and cut_injects (a standing partition never
    converges), under PAIR_SEED[N]: at P = N - 1 node 1 learns rumor 0 from node 0 in round 0."""
    return case(N, 3, mode, k, PAIR_SEED[N], (("build", "sprinkle", 3),) + cut_injects(N, P) + (("step", part_rounds(P)),),
                partitions=P)


def parts_midrun_case(N):
    """P = N for 5 rounds (nothing moves), 7 blocks for 5 rounds, then healed to convergence."""
    s = (("build", "sprinkle", 3),) + cut_injects(N, 7) + (("step", 5), ("faults", 0, 7), ("step", 5), ("faults", 0, 0),
                                                         ("step", CAP))
    return case(N, 3, "pushpull", 3, st.SEED, s, partitions=N)


def loss_case(N, loss, D, mode="pushpull", k=3):
    """2 D + 2 rounds under the loss, the heal, four rounds, a reset (the streaks go), the state built
    again and run to convergence."""
    s = (("build", "sprinkle", 3), ("step", 2 * LOSS_D + 2), ("faults", 0, 0), ("step", 4), ("reset",),
         ("build", "sprinkle", 3), ("step", CAP))
    return case(N, 3, mode, k, st.SEED, s, edge_loss=loss, stall_rounds=D)


STALL_ROUNDS = 24


def stall_case(N, D, mode, k=2):
    """STALL_LOSS[D] under the deadline D for STALL_ROUNDS rounds (at D = 16: nodes stall from round 16 on,
    some in each round), then the heal and eight rounds in which the stalled nodes still initiate nothing."""
    loss, builder = STALL_LOSS[D]
    s = (("build", builder, 3), ("step", STALL_ROUNDS), ("faults", 0, 0), ("step", 8))
    return case(N, 3, mode, k, st.SEED, s, edge_loss=loss, stall_rounds=D)


def long_case(N, rounds, mode="pushpull", k=2, infected=True):
    """`rounds` rounds under two partitions, one rumor in each block and one on the cut; then the heal
    and the run to convergence: only draws at t >= rounds decide the end."""
    step = ("step", rounds) if infected else ("step", rounds, False)
    last = ("step", CAP) if infected else ("step", CAP, False)
    s = (("inject", 0, 0), ("inject", N - 1, 1), ("inject", N // 2, 2), step, ("faults", 0, 0), ("inject", 1, 0), last)
    return case(N, 3, mode, k, st.SEED, s, partitions=2)


# --- the sender kernels --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":      # hub rows of 300, empty rows, self-loops, repeated entries
        return tp.ragged(NROWS, 7)
    if name == "mid":         # the same at NMID nodes, half of the listings returned
        return tp.symmetrize(*tp.ragged(NMID, 7, hub_every=1024, hub_deg=40), NMID, every=2)
    if name == "pair":
        # mid with 1 at the head of row 0 and 0 at the head of row 1: the two nodes that share a block under
        # P = NMID - 1 list each other, and first (a FLOOD walk never gets past a neighbour it keeps losing)
        rp, col = topo("mid")
        col = np.concatenate([[1], col[:rp[1]], [0], col[rp[1]:]])
        rp = rp.astype(np.int64) + np.r_[0, 1, np.full(NMID - 1, 2)]
        return rp.astype(np.uint32), col.astype(np.uint32)
    if name == "walk":        # small enough for numpy_ref.Sim's walks, one node and value at a time
        return tp.symmetrize(*tp.ragged(NWALK, 7, hub_every=128, hub_deg=20), NWALK, every=2)
    if name == "complete":    # row_n[i] = i + (i >= n): the uniform peer map
        return tr.csr_of_names(total_topology(NFULL))
    raise KeyError(name)


def row_injects(name, R):
    """Every rumor somewhere, one at a hub, one at a node with an empty row, one at the last node."""
    rp = topo(name)[0].astype(np.int64)
    n, deg = rp.size - 1, np.diff(rp)
    return tuple([("inject", (431 * i) % n, i) for i in range(R)] +
                 [("inject", int(np.argmax(deg)), 0), ("inject", int(np.nonzero(deg == 0)[0][3]), R // 2),
                  ("inject", n - 1, R - 1)])


def topo_case(name, R, mode, k, seed, rounds, tail=(), extra=(), **faults):
    """GOSSIP_FLAG_TOPO_PEERS: the rows set, row_injects and `extra`, `rounds` rounds, then `tail`."""
    n = topo(name)[0].size - 1
    s = (("topology", name),) + row_injects(name, R) + tuple(extra) + (("step", rounds),) + tuple(tail)
    return case(n, R, mode, k, seed, s, **faults)


def topo_seed_cases(seed):
    """The ragged 30011-node rows in three modes with FAULTY."""
    return [topo_case("ragged", R, mode, k, seed, 12, **dict(FAULTY))
            for mode, k, R in (("pushpull", 2, 3), ("push", 5, 130), ("pull", 4, 3))]


# (peers, R, k, cool, blind, limit, loss): the coin with feedback, blind, counters with limit 3
MONGER = [("uniform", 3, 2, 0.5, False, None, lt(0.3)), ("mid", 130, 5, 0.5, True, None, 0),
          ("mid", 3, 4, 0.25, False, 3, lt(0.3)), ("uniform", 130, 9, 0.5, True, 3, 0)]
MONGER_READS = ("read_hot", "read_counts", "round_index")


def monger_case(peers, R, k, cool, blind, limit, seed, rounds=CAP, tail=(), extra=(), **faults):
    """GOSSIP_FLAG_MONGER on a PUSH engine of NMID nodes: returns (case, topo_peers)."""
    s = () if peers == "uniform" else (("topology", peers),)
    s += (("monger", cool, blind),) + ((("limit", limit),) if limit is not None else ())
    s += (row_injects(peers, R) if peers != "uniform" else tuple(("inject", (431 * i) % NMID, i) for i in range(R)))
    s += tuple(extra) + (("step", rounds),) + tuple(tail)
    return case(NMID, R, "push", k, seed, s, **faults), peers != "uniform"


def walk_case(seed, tail=(), extra=(), name="mid", **faults):
    """The FLOOD walks (one draw per message, the value's slot in the tag word) on the mid rows, in the
    message's order, with loss 0.3 and a deadline of two lost attempts unless `faults` says otherwise."""
    faults = faults or dict(edge_loss=lt(0.3), stall_rounds=2)
    s = (("topology", name),) + row_injects(name, 5) + tuple(extra) + (("step", 40),) + tuple(tail)
    return case(NMID, 5, "flood", 0, seed, s, **faults)


def sender_part_cases(P):
    """The sender kernels under P blocks at NMID nodes, over the `pair` rows and under PAIR_SEED[NMID]:
    [(kind, case, topo_peers)], kind "topo" (GOSSIP_FLAG_TOPO_PEERS), "monger" (over the rows and uniform)
    or "walk" (FLOOD).  A rumor on both sides of every cut, and rumor 1 at node 0, which sends to node 1 in
    round 0: row_injects gives rumor 0 to node 0 and to the first hub, which is node 1."""
    seed, extra = PAIR_SEED[NMID], cut_injects(NMID, P) + (("inject", 0, 1),)
    out = [("topo", topo_case("pair", 3, "pushpull", 2, seed, PART_ROUNDS, extra=extra, partitions=P), True),
           ("topo", topo_case("pair", 130, "push", 5, seed, PART_ROUNDS, extra=extra, partitions=P, edge_loss=lt(0.2),
                              stall_rounds=2), True)]
    for peers, R, k, cool, blind, limit, loss in MONGER[:3]:
        peers = "uniform" if peers == "uniform" else "pair"
        out.append(("monger",) + monger_case(peers, R, k, cool, blind, limit, seed, rounds=24, extra=extra, edge_loss=loss,
                                             partitions=P))
    out.append(("walk", walk_case(seed, extra=extra, name="pair", edge_loss=lt(0.3), stall_rounds=2, partitions=P), True))
    out.append(("walk", walk_case(seed, extra=extra, name="pair", partitions=P), True))
    return out


# --- ANTIENTROPY -------------------------------------------------------------------------------------------
# (K, k): the churn word shared with the first peer draw (k <= 3), on its own stream (k >= 4), wide rows
AE_PAIRS = [(2, 3), (16, 4), (33, 1)]


def ae_probe(N):
    """Nodes whose alive flags are read: chunk (64) edges, the middle and the last two."""
    return (0, 63, 64, N // 2, N - 2, N - 1)


AE_PROBE = ae_probe(AE_N)


def ae_writes(N, K):
    return (("inject", N // 2, K - 1), ("inject", 3, 0))


def ae_args(K, k, seed=st.SEED, N=AE_N):
    return (N, K, "antientropy", k, seed)


def ae_kw(fail=ac.FAIL, rec=ac.RECOVER, **faults):
    return dict(flags=FLAG_HASH, churn_fail=fail, churn_recover=rec, **faults)


def ae_script(N, K, rounds=6, tail=()):
    """Random rows, `rounds` rounds, two client writes, then `tail` (default: to convergence)."""
    return (("random",), ("step", rounds)) + ae_writes(N, K) + (tuple(tail) or (("step", 400),))


def churn_script(N, K):
    """Single-round steps past the first "converged" round (step would stop there), a write to a node
    in the middle of them (under (A, 0) and in the odd rounds of (A, A): while every node is dead), more
    single rounds, then a step of its own."""
    one = (("step", 1),)
    return (("random",),) + one * 5 + (("inject", N // 2, K - 1),) + one * 4 + (("inject", 3, 0), ("step", 12))


AE_HEAL = (("step", 6), ("faults", 0, 0), ("step", 400))


def ae_fault_seed_cases(seed):
    """The faulted ANTIENTROPY seed cases, (args, kw, script, topology, G): loss 0.25 and two partitions for
    12 rounds with two writes, then the heal; over the ragged rows (nodes nobody points at: it never
    converges) with loss; and the two sharded runs (G = 3: shards of 1408, 1408 and 1283 nodes)."""
    faulty = ae_kw(edge_loss=lt(0.25), partitions=2)
    return [(ae_args(5, 2, seed), faulty, ae_script(AE_N, 5, 6, AE_HEAL), None, 0),
            (ae_args(5, 2, seed, NMID), ae_kw(edge_loss=lt(0.25)), ae_script(NMID, 5, 6, (("step", 10),)), "mid", 0),
            (ae_args(5, 2, seed), ae_kw(), ae_script(AE_N, 5, 6, AE_HEAL), None, 3),
            (ae_args(16, 4, seed), faulty, ae_script(AE_N, 16, 6, AE_HEAL), None, 3)]


def ae_parts_case(P):
    """Ten rounds under P blocks with two writes, then the heal and the run to convergence; PAIR_SEED: at
    P = N - 1 nodes 0 and 1 exchange their rows in round 0 (both are alive)."""
    return (ae_args(5, 2, PAIR_SEED[AE_N]), ae_kw(partitions=P),
            ae_script(AE_N, 5, 6, (("step", 4), ("faults", 0, 0), ("step", 400))))
