"""Node counts on, one below and one above the units of the per-node kernels, the states built for
them, and the cases run at them; shared by test_size_tables.py (CPU) and test_gpu_sizes.py.  A
plain module, not a conftest; it holds tables and builders, no tests.

A builder is `build(engine, R) -> number of inject calls`, as in states.py: it only calls
`engine.inject`, so the same call builds the CPU oracle and the HIP engine.  The round paths are
those of states.py (PATHS, path_of, FAULT_PATHS) and of ae_cases.py.
"""
import numpy as np

import ae_cases as ac
import states as st
from gossip_hip import loss_threshold

# (with seeds 0x5EED0515, ..18, ..19 the oracle's 64-node pushpull k = 4 run from 64 Philox origins has no
# node full before its last round: test_size_tables.py wants a full-majority round in every case)
SEED = 0x5EED0516
CAP = 128            # rounds: every random-mode case without faults converges sooner

# --- size tables -----------------------------------------------------------------------------------
# SMALL: below one unit (2, 3, 7, 8, 9: one partial wave, one block, fewer nodes than fanout 4 .. 64),
# then b - 1, b, b + 1 for
#   64     one wave (csrc/sender.h, csrc/kernels.hip), one bitmap word ((N + 63) >> 6, csrc/frontier.hip),
#          one 64-node chunk of csrc/antientropy.hip
#   128    two words / waves
#   256    one block of 256 lanes (csrc/kernels.hip, csrc/sender.h); ts(64) of make_bin_geom
#   1024   the scan step's lanes (csrc/frontier.hip); ts(16)
#   2048   the scan step of 1024 lanes x 2 nodes; ts(8)
#   4096   kBsRegLog = 12 (csrc/frontier.hip): the binned scan's sender regions; kCommitChunkLog = 6:
#          64 groups of 64 nodes per commit wave chunk; ts(4); the sparse-scan tiles of antientropy.hip
#   8192   ts(2) of make_bin_geom (csrc/binned.hip)
#   16384  the destination tile of csrc/binned.hip (kTileD); kAeDTileLog = 14
#   32768  kRwWords = 512 words (csrc/frontier.hip): the staging chunk of the scan
SMALL = [2, 3, 7, 8, 9,
         63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049,
         4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769]
# LARGE: b - 1, b, b + 1 for
#   2^19   GOSSIP_BS_TILE_LOG = 19 (csrc/frontier.hip): the binned scan's peer tiles
#   2^20   frontier_glog 0 -> 1 (the LDS summary); the full-pull resolve trip of 2^20 nodes
#   2^21   frontier_glog 1 -> 2; 8192 blocks x 256 lanes of the sender kernels
LARGE = [524287, 524288, 524289, 1048575, 1048576, 1048577, 2097151, 2097152, 2097153]
# BIG: kBigFromTiles = 1024 destination tiles (csrc/binned.h): 2^24 + 1 is the smallest big geometry
BIG = [16777217]
# AE: 4 (ae_cases.run writes to node 3), then b - 1, b, b + 1 for the 64-node chunk, the 256-lane
# block, the 2^12 sparse-scan tile, kAeDTileLog = 14 and kAeBinTileLog = 17 of csrc/antientropy.hip
AE = [4, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 131071, 131072, 131073]
# TINY: the one-lane-per-sender kernels (csrc/sender.h: csrc/monger.hip, csrc/topo_peers.hip; FLOOD
# of csrc/kernels.hip): below a wave, a wave of 64, a block of 256
TINY = [2, 3, 63, 64, 65, 255, 256, 257]


def ts(k):
    """make_bin_geom's sender tile (csrc/binned.hip): the largest power of two at most 8192 with
    ts * k <= 16384."""
    t = 8192
    while t * k > 16384:
        t >>= 1
    return t


# TS: fanout k -> ts - 1, ts, ts + 1, 2 ts and 16384 + ts (one destination tile and one sender tile)
TS = {3: [4095, 4096, 4097, 8192, 20480], 5: [2047, 2048, 2049, 4096, 18432],
      9: [1023, 1024, 1025, 2048, 17408], 17: [511, 512, 513, 1024, 16896],
      33: [255, 256, 257, 512, 16640], 64: [255, 256, 257, 512, 16640]}

# every unit above: boundary_nodes() puts a node on each side of u and of 2 u
UNITS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 131072, 1 << 19, 1 << 20, 1 << 21, 1 << 24)


def boundary_nodes(N):
    """0, N - 2, N - 1, and u * m - 1 and u * m for every unit u and m in (1, 2) where below N; sorted."""
    out = {0, N - 2, N - 1}
    for u in UNITS:
        for m in (1, 2):
            out.update(x for x in (u * m - 1, u * m) if x < N)
    return sorted(out)


# --- builders ----------------------------------------------------------------------------------------

def edges_at(engine, R):
    """Rumor i % R at the i-th boundary node and every rumor at N - 1: a few dozen calls at any N; the
    first sparse rounds have their whole rare set on boundaries."""
    N = engine.n_nodes
    calls = 0
    for i, n in enumerate(boundary_nodes(N)):
        engine.inject(n, i % R)
        calls += 1
    for r in range(R):
        engine.inject(N - 1, r)
    return calls + R


def holes_at(engine, R):
    """states.holes for any N: every node full but the boundary nodes, which are empty; nodes with
    n % 97 == 5 lack rumor n % R.  About 3 N calls: for N <= 16385."""
    N = engine.n_nodes
    empty = set(boundary_nodes(N))
    calls = 0
    for n in range(N):
        if n in empty:
            continue
        for r in range(R):
            if n % 97 == 5 and r == n % R:
                continue
            engine.inject(n, r)
            calls += 1
    return calls


def random(engine, R):
    engine.inject_random()
    return 1


BUILDERS = {"edges": edges_at, "holes": holes_at, "random": random}

# --- cases: (N, R, mode, k, builder) -------------------------------------------------------------------
K4 = (1, 2, 3, 4)       # the fanouts of the binned scan: ts 8192 for k <= 2, 4096 for k <= 4
MODES = ("push", "pull", "pushpull")
DENSE_FRAC = "dense_frac"
SMALL_PATHS = st.PATHS + [DENSE_FRAC]
LARGE_PATHS = ["auto", "sparse", "sparse_alld", "sparse_direct", "sparse_noq", "sparse_bscan"]
BIG_PATHS = ["auto", "dense", "dense_filter"]
TS_PATHS = ["dense", "dense_filter", DENSE_FRAC]


def path_of(name):
    """(flags, params) of a path of states.PATHS, or of dense_frac: every round dense by the planner's
    own knob (sparse_frac -1), the emit filter left to the planner."""
    return (0, {"sparse_frac": -1}) if name == DENSE_FRAC else st.path_of(name)


def small_cases(N):
    """push and pull from edges_at, pushpull from Philox origins; k rotates with the size's index, so
    the three sizes of a triple see three fanouts of K4 in every mode and all four between them.  (The
    pushpull offset gives 8 and 9 nodes k = 1 and 2: at k = 3 they converge in two rounds, none of which
    starts with a full node.)"""
    i = SMALL.index(N)
    return [(N, 3, "push", K4[i % 4], "edges"), (N, 3, "pull", K4[(i + 2) % 4], "edges"),
            (N, 64, "pushpull", K4[(i + 1) % 4], "random")]


def large_cases(N):
    i = LARGE.index(N)
    return [(N, 3, "pushpull", 2, "edges"), (N, 3, "push", 3, "edges") if i % 2 == 0 else (N, 3, "pull", 1, "edges")]


def big_cases(N):
    return [(N, 64, "pushpull", 2, "random")]


TS_SIZES = [(k, N) for k in TS for N in TS[k]]


def ts_cases(k, N):
    return [(N, 64, MODES[TS_SIZES.index((k, N)) % 3], k, "random")]


HOLES_SIZES = [4096, 16384]


def holes_cases(N):
    return [(N, 3, "push", 1, "holes"), (N, 3, "pull", 1, "holes"), (N, 3, "pushpull", 2, "holes")]


FAULT_SIZES = [64, 4096, 16384, 16385, 32768]
FAULTS = dict(edge_loss=loss_threshold(0.25), partitions=3)
FAULT_ROUNDS = 24       # three partitions never converge


def fault_cases(N):
    return [(N, 3, "pushpull", 2, "edges"), (N, 3, "push", 5, "edges")]


# ANTIENTROPY: (K, k) per boundary triple, rotated; at the aligned sizes also a wide row and a fanout
# past the binned dense round
AE_PAIRS = [(16, 1), (3, 2), (9, 3)]
AE_ALIGNED = [(17, 1), (2, 4)]


def ae_cases(N):
    """The (K, k) pairs run at N nodes."""
    i = AE.index(N)
    pairs = [AE_PAIRS[((i - 1) // 3) % 3 if i else 0]]
    if i and (i - 1) % 3 == 1:
        pairs += AE_ALIGNED
    return pairs


def ae_paths(K, k):
    """ae_cases.paths_of(K, k), and the other forms of the binned dense round wherever it fits (K <= 16,
    k <= 3), not only at the pairs of ae_cases.MATRIX_BINNED."""
    return ac.PATHS_BINNED if K <= 16 and k <= 3 else ac.paths_of(K, k)


AE_ITEMS = [(N, K, k, path) for N in AE for K, k in ae_cases(N) for path in ae_paths(K, k)]

# sender kernels at TINY sizes: (rule, k) x peers x R; rule = the limit, None = the coin alone
MONGER_RULES = (None, 2, 3)
MONGER_K = (2, 5, 9)
ALWAYS = 2 ** 32 - 1


def monger_cases(N):
    """(limit, k, cool, blind) of the nine runs of one size: every rule with every k; cool and the
    variant rotate.  (N = 2 with k = 9: every edge of a sender hits the one peer, so a count passes
    its limit inside one round.)"""
    i = TINY.index(N)
    out = []
    for a, limit in enumerate(MONGER_RULES):
        for b, k in enumerate(MONGER_K):
            out.append((limit, k, (0.5, ALWAYS, 0.25)[(a + b + i) % 3], bool((a + b + i) % 2)))
    return out


def tiny_topology(N):
    """(row_ptr, col) uint32 for any N >= 2: a ring in which every third row (n % 3 == 2) is empty, and
    the hub row of node 0, which lists every node (itself too)."""
    rows = []
    for n in range(N):
        if n == 0:
            rows.append(list(range(N)))
        elif n % 3 == 2:
            rows.append([])
        else:
            rows.append([(n + 1) % N, (n - 1) % N])
    rp = np.zeros(N + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, np.array([v for r in rows for v in r], dtype=np.uint32)


def tiny_injects(N, R):
    """Every rumor somewhere, one at the hub, one at the last node."""
    return tuple([((431 * i) % N, i) for i in range(R)] + [(0, R - 1), (N - 1, 0)])


def build(engine, builder, R):
    return BUILDERS[builder](engine, R)


def majorities(shard, R):
    """(starts full-majority, starts empty-majority) of one state: the criterion of
    test_gpu_fullpull.py (plan.h): fewer nodes that are not full than nodes that hold something."""
    empty, full = st.shares(shard, R)
    fullmaj = 1.0 - full < 1.0 - empty
    return fullmaj, not fullmaj
