"""Hand-built states and round-path tables shared by test_state_builders.py (CPU),
test_gpu_states.py and test_gpu_geometry.py, and the wide sparse workload of test_wide_state.py
and test_gpu_wide_state.py.  A plain module, not a conftest.

A builder is `build(engine, R) -> number of inject calls`; it only calls
`engine.inject`, so the same call builds the CPU oracle and the HIP engine.
Every builder of BUILDERS is written for N0 nodes: one full 16384-node tile, one
64-node group and one node of a ragged last group; sparse_words takes any size.
"""
import numpy as np

from gossip_hip import FLAG_DENSE, FLAG_DIRECT

N0 = 16449
SEED = 0x5EED0021
HOLES = (0, 63, 64, 8191, 8192, 16383, 16384, N0 - 1)

# the round paths of test_gpu_parity.py (PATHS / _PATH_FLAGS / _PATH_PARAMS), restated so the CPU
# tests need not import a GPU test module; test_gpu_states.py asserts the two tables are equal
PATHS = ["auto", "dense", "dense_filter", "sparse", "sparse_alld", "sparse_direct", "sparse_noq", "sparse_bscan",
         "direct"]
PATH_FLAGS = {"auto": 0, "dense": FLAG_DENSE, "dense_filter": 0, "sparse": 0, "sparse_alld": 0, "sparse_direct": 0,
              "sparse_noq": 0, "sparse_bscan": 0, "direct": FLAG_DIRECT}
PATH_PARAMS = {"dense_filter": {"sparse_frac": -1, "filter_frac": 0},
               "sparse": {"sparse_frac": 1.0, "alld_frac": 1e30},
               "sparse_alld": {"sparse_frac": 1.0, "alld_frac": 0, "sparse_direct": 0},
               "sparse_direct": {"sparse_frac": 1.0, "alld_frac": 0, "sparse_direct": 1},
               "sparse_noq": {"sparse_frac": 1.0, "scan_queue": 0},
               "sparse_bscan": {"sparse_frac": 1.0, "bin_scan_frac": 0}}
# the seven paths of test_gpu_faults.PATHS, name -> (flags, params)
FAULT_PATHS = {"auto": (0, {}), "dense": (FLAG_DENSE, {}), "dense_filter": (0, {"sparse_frac": -1, "filter_frac": 0}),
               "sparse": (0, {"sparse_frac": 1.0, "alld_frac": 1e30}),
               "sparse_alld": (0, {"sparse_frac": 1.0, "alld_frac": 0, "sparse_direct": 0}),
               "sparse_direct": (0, {"sparse_frac": 1.0, "alld_frac": 0}), "direct": (FLAG_DIRECT, {})}
# the documented defaults (include/gossip.h) of every knob a path sets, as a one-shard engine of at
# most 2^25 nodes reads them
PARAM_DEFAULTS = {"sparse_frac": 1.0 / 16, "alld_frac": 1.0 / 128, "sparse_direct": 1, "scan_queue": 1,
                  "bin_scan_frac": 0.6, "filter_frac": 0.3}


def path_of(name):
    """(flags, params) of one entry of PATHS"""
    return PATH_FLAGS[name], PATH_PARAMS.get(name, {})


def thirds(engine, R=3):
    """n % 3 == 0 empty, == 1 full, == 2 holds rumor n % R only."""
    calls = 0
    for n in range(N0):
        if n % 3 == 1:
            for r in range(R):
                engine.inject(n, r)
            calls += R
        elif n % 3 == 2:
            engine.inject(n, n % R)
            calls += 1
    return calls


def clustered(engine, R=64):
    """Nodes [0, 64) and [16320, N0) full, every other node empty: the second cluster crosses the
    16384 tile boundary and takes in the ragged last group; the rumors are perfectly correlated."""
    calls = 0
    for n in list(range(64)) + list(range(16320, N0)):
        for r in range(R):
            engine.inject(n, r)
        calls += R
    return calls


def holes(engine, R=3):
    """Every node full but the eight empty ones on group and tile boundaries (HOLES); nodes with
    n % 97 == 5 lack rumor n % R."""
    calls = 0
    for n in range(N0):
        if n in HOLES:
            continue
        for r in range(R):
            if n % 97 == 5 and r == n % R:
                continue
            engine.inject(n, r)
            calls += 1
    return calls


def disjoint(engine, R=64):
    """Node n holds rumor n % 64 only: no empty node, no full node, anti-correlated rumors."""
    for n in range(N0):
        engine.inject(n, n % R)
    return N0


def sparse_word_ids(R):
    """The state words the `sparse_words` workload touches: the first, word 17 (the middle word of
    a state with fewer) and the last."""
    W = (R + 63) // 64
    return sorted({0, 17 if W > 18 else W // 2, W - 1})


def sparse_words(engine, R, N=None):
    """Wide states (R > 64), any N: rumors in the words of sparse_word_ids only, every other word of
    every node stays empty for good.  Per touched word its bits 0, 31 and 63 (those below R) and
    rumor R - 1, each at three nodes; no node can ever be full, so runs take a fixed number of rounds."""
    N = N or engine.n_nodes
    rumors = sorted({64 * w + b for w in sparse_word_ids(R) for b in (0, 31, 63) if 64 * w + b < R} | {R - 1})
    for r in rumors:
        for i in range(3):
            engine.inject((r * 2654435761 + i * 40503 + 7) % N, r)
    return 3 * len(rumors)


class _Recorder:
    def __init__(self):
        self.calls = []

    def inject(self, node, rumor=0):
        self.calls.append((node, rumor))


def noisy(builder, seed=0x5EED):
    """The same bits as `builder`, injected in an order shuffled by a fixed numpy seed, every 10th
    call repeated at once (a duplicate)."""
    def build(engine, R):
        rec = _Recorder()
        builder(rec, R)
        order = np.random.default_rng(seed).permutation(len(rec.calls))
        calls = 0
        for i, j in enumerate(order):
            n, r = rec.calls[j]
            engine.inject(n, r)
            calls += 1
            if i % 10 == 9:
                engine.inject(n, r)
                calls += 1
        return calls
    build.__name__ = "noisy_" + builder.__name__
    return build


BUILDERS = {"thirds": (thirds, 3), "clustered": (clustered, 64), "holes": (holes, 3), "disjoint": (disjoint, 64)}
BUILDERS.update({"noisy_" + k: (noisy(b), R) for k, (b, R) in list(BUILDERS.items())})


def shares(shard, R):
    """(empty share, full share) of a read_shard() image of a one-word state"""
    full = np.uint64((1 << R) - 1) if R < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    w = shard[0]
    return float((w == 0).mean()), float((w == full).mean())
