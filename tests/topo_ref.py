"""Random gossip over the topology, restated in vectorised numpy.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest) that the CPU and GPU tests of
GOSSIP_FLAG_TOPO_PEERS share.  It is built on oracle/numpy_ref.py's Philox, loss draw, edge
test, stats and hash, and shares no code with the engine.

The reference's (*NodeState).Gossip ranges over Topology[node.ID()] (main.go:72) and sends to
every neighbour; here node n draws k of them per round, with replacement:

    x   = Philox4x32-10({n, t, 0, j >> 2}, key)[j & 3]          (the draw of §2.2)
    i_j = floor(x * deg(n) / 2^32),   p_j(n, t) = row_n[i_j]     (rows as sorted sets)

and PUSH / PULL / PUSHPULL, faults (§2.8) and stall streaks (§2.9) read as for uniform peers.
A node with an empty row initiates nothing.  messages = exchanges initiated in the round, lost
attempts included: k per node that has a row, is not stalled and (PUSH) holds something.
"""
from types import SimpleNamespace

import numpy as np

import numpy_ref as nr

_U = np.uint64


def rows_as_sets(row_ptr, col, N):
    """(row_ptr, col) with every row a sorted set (duplicates dropped, self-loops kept)."""
    rp = np.asarray(row_ptr, dtype=np.int64)
    src = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
    key = np.unique(src * N + np.asarray(col, dtype=np.int64))
    out = np.zeros(N + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(key // N, minlength=N))
    return out, key % N


def csr_of_names(topo):
    """A Maelstrom topology message ({"n3": ["n1", ...]}, gossip_hip.total_topology and its
    kin) as (row_ptr, col) uint32 arrays."""
    N = len(topo)
    rows = [[int(v[1:]) for v in topo[f"n{u}"]] for u in range(N)]
    rp = np.zeros(N + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, np.array([v for r in rows for v in r], dtype=np.uint32)


def row_index(seed, degree, nodes, t, j):
    """i_j of §2.10 for an array of nodes: floor(x * degree / 2^32); 0 where degree is 0."""
    n = np.asarray(nodes, dtype=np.uint32)
    x = nr.philox4x32_10(n, np.uint32(t), np.uint32(0), np.uint32(j >> 2), seed & 0xFFFFFFFF,
                         (seed >> 32) & 0xFFFFFFFF)[j & 3]
    return ((x.astype(_U) * np.asarray(degree, dtype=_U)) >> _U(32)).astype(np.int64)


class TopoSim:
    """Unsharded reference loop; mode 'push' | 'pull' | 'pushpull'; topology (row_ptr, col)."""

    def __init__(self, n_nodes, n_rumors, mode, fanout, seed=0, topology=None, edge_loss=0, partitions=0,
                 stall_rounds=0):
        assert mode in ("push", "pull", "pushpull")
        self.N, self.R, self.mode, self.k, self.seed = n_nodes, n_rumors, mode, fanout, seed
        self.loss, self.parts, self.D = edge_loss, partitions, stall_rounds
        self.W = (n_rumors + 63) // 64
        self.rp = self.col = None
        self.reset()
        if topology is not None:
            self.set_topology(topology)

    def set_topology(self, topology):
        """Takes effect in the next round; state, round index and streaks stay."""
        self.rp, self.col = rows_as_sets(topology[0], topology[1], self.N)
        self.deg = np.diff(self.rp)

    def set_faults(self, edge_loss=0, partitions=0):
        self.loss, self.parts = edge_loss, partitions

    def reset(self):
        self.S = np.zeros((self.W, self.N), dtype=np.uint64)
        self.streak = np.zeros(self.N, dtype=np.int64)
        self.t = 0

    def inject(self, node, rumor):
        self.S[rumor // 64, node] |= _U(1 << (rumor % 64))

    def peers(self, j):
        """p_j(n, t) for every n (n itself where the row is empty: never used)."""
        n = np.arange(self.N, dtype=np.int64)
        at = self.rp[:-1] + row_index(self.seed, self.deg, n, self.t, j)
        if self.col.size == 0:
            return n
        return np.where(self.deg > 0, self.col[np.minimum(at, self.col.size - 1)], n)

    def round(self):
        assert self.rp is not None, "needs a topology"
        S, N = self.S, self.N
        Sn = S.copy()
        n = np.arange(N, dtype=np.int64)
        has = self.deg > 0
        stalled = self.streak >= self.D if self.D else np.zeros(N, dtype=bool)
        pull, push = self.mode in ("pull", "pushpull"), self.mode in ("push", "pushpull")
        lost_any = np.zeros(N, dtype=bool)
        for j in range(self.k):
            p = self.peers(j)
            lost = nr.edge_lost(self.seed, N, self.loss, self.parts, n, p, self.t, j)
            lost_any |= lost & has
            live = has & ~stalled & ~lost
            src, dst = n[live], p[live]
            for w in range(self.W):
                if pull:
                    np.bitwise_or.at(Sn[w], src, S[w][dst])
                if push:
                    np.bitwise_or.at(Sn[w], dst, S[w][src])
        initiates = has & ~stalled
        if not pull:  # PUSH sends only what it holds
            initiates &= (S != 0).any(axis=0)
        msgs = self.k * int(initiates.sum())
        if self.D:  # an empty row has no exchange to lose: its streak starts over
            self.streak = np.where(stalled, self.streak, np.where(lost_any, self.streak + 1, 0))
        self.S = Sn
        full, inf = nr.stats_of(Sn, self.R)
        st = dict(round=self.t, converged=int(full == N), full_nodes=full, alive_nodes=N, messages=msgs,
                  state_hash=nr.state_hash(Sn))
        self.t += 1
        return st, inf

    def step(self, max_rounds):
        """Rounds until converged or max_rounds, shaped like Engine.step's result (rounds, stats as
        gossip_round_stats_t dicts with the hash filled, infected [rounds, R])."""
        stats, infected = [], []
        for _ in range(max_rounds):
            st, inf = self.round()
            stats.append(st)
            infected.append(inf)
            if st["converged"]:
                break
        return SimpleNamespace(rounds=len(stats), stats=stats,
                               infected=np.array(infected, dtype=np.uint64).reshape(len(stats), self.R))

    def read_shard(self):
        return self.S.copy()
