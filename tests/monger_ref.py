"""Rumor mongering (GOSSIP_FLAG_MONGER), restated in vectorised numpy.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest) that the CPU and GPU tests of the flag
share.  It is built on oracle/numpy_ref.py's Philox, peers, edge test, stats and hash and on
tests/topo_ref.py's rows and row index, and shares no code with the engine.

Per node two bitsets: S (known) and H ⊆ S (hot).  Round t reads S_t and H_t only:

    n initiates        iff H_t[n] != 0 (and, over the topology, its row is not empty)
    p_j(n, t)          the uniform draw of §2.2, or row_n[i_j] of §2.10; lost as in §2.8
    delivered push     S_{t+1}[p] |= H_t[n];   H_{t+1}[p] |= H_t[n] & ~S_t[p]
    coin of edge j     Philox4x32-10({n, t, 5, j >> 2}, key)[j & 3] < cool
    counted set        feedback: H_t[n] & S_t[p] when delivered, nothing when lost
                       blind:    H_t[n] for every attempt
    coin holds         H_{t+1}[n] &= ~counted

messages = k per initiating node, lost attempts included.  A run ends with the first round that
sends nothing (that round is reported) or after max_rounds, never at `converged`.

Beside the stats every round reports the guards the GPU tests need to know that a pass is not
vacuous: bits cooled, delivered pushes that carried nothing new, nodes that in one round lost a bit
and gained a hot bit in the same word, and lost attempts.
"""
from types import SimpleNamespace

import numpy as np

import numpy_ref as nr
import topo_ref as tr

_U = np.uint64
GUARDS = ("cooled", "stale", "and_or", "lost")


def threshold(p):
    """A probability (float) as x / 2^32, or the u32 threshold itself (int)."""
    return min(int(round(p * 2 ** 32)), 2 ** 32 - 1) if isinstance(p, float) else int(p)


def popcount(a):
    """Set bits of a uint64 array."""
    nz = np.ascontiguousarray(a[a != 0])
    return int(np.unpackbits(nz.view(np.uint8)).sum())


def coin_word(seed, nodes, t, j):
    """The word of edge j's coin: Philox({n, t, 5, j >> 2})[j & 3]."""
    n = np.asarray(nodes, dtype=np.uint32)
    return nr.philox4x32_10(n, np.uint32(t), np.uint32(5), np.uint32(j >> 2), seed & 0xFFFFFFFF,
                            (seed >> 32) & 0xFFFFFFFF)[j & 3]


class MongerSim:
    """Unsharded reference loop of a PUSH engine with GOSSIP_FLAG_MONGER; topo_peers: the peers come
    from the rows (GOSSIP_FLAG_TOPO_PEERS), else from all N nodes whatever topology was set."""

    def __init__(self, n_nodes, n_rumors, fanout, seed=0, topo_peers=False, topology=None, edge_loss=0, partitions=0):
        self.N, self.R, self.k, self.seed, self.topo = n_nodes, n_rumors, fanout, seed, topo_peers
        self.loss, self.parts = edge_loss, partitions
        self.W = (n_rumors + 63) // 64
        self.cool, self.blind = 0, False
        self.rp = self.col = None
        self.reset()
        if topology is not None:
            self.set_topology(topology)

    # -- the calls of the engine ----------------------------------------------------------------
    def set_topology(self, topology):
        self.rp, self.col = tr.rows_as_sets(topology[0], topology[1], self.N)
        self.deg = np.diff(self.rp)

    def set_faults(self, edge_loss=0, partitions=0):
        self.loss, self.parts = edge_loss, partitions

    def set_monger(self, cool, blind=False):
        self.cool, self.blind = threshold(cool), bool(blind)

    def reset(self):
        """Clears both bitsets and the round index; cool and blind stay."""
        self.S = np.zeros((self.W, self.N), dtype=np.uint64)
        self.H = np.zeros((self.W, self.N), dtype=np.uint64)
        self.t = 0

    def inject(self, node, rumor):
        w, bit = rumor // 64, _U(1 << (rumor % 64))
        if not self.S[w, node] & bit:   # a held rumor, cooled or not, stays as it is
            self.S[w, node] |= bit
            self.H[w, node] |= bit

    def inject_random(self):
        for r, o in enumerate(nr.origins(self.seed, self.N, self.R)):
            self.inject(int(o), r)

    def read_shard(self):
        return self.S.copy()

    def read_hot(self):
        return self.H.copy()

    @property
    def round_index(self):
        return self.t

    # -- one round --------------------------------------------------------------------------------
    def peers(self, j):
        """p_j(n, t) over the rows, for every n (n itself where the row is empty: never used)."""
        n = np.arange(self.N, dtype=np.int64)
        if self.col.size == 0:
            return n
        at = self.rp[:-1] + tr.row_index(self.seed, self.deg, n, self.t, j)
        return np.where(self.deg > 0, self.col[np.minimum(at, self.col.size - 1)], n)

    def round(self):
        assert not self.topo or self.rp is not None, "needs a topology"
        S, H, N = self.S, self.H, self.N
        n = np.arange(N, dtype=np.int64)
        init = (H != 0).any(axis=0)
        if self.topo:
            init &= self.deg > 0
        gain_s = np.zeros_like(S)
        gain_h = np.zeros_like(S)
        cleared = np.zeros_like(S)
        g = dict.fromkeys(GUARDS, 0)
        uniform = None if self.topo else nr.peers(self.seed, N, self.t, self.k).astype(np.int64)
        for j in range(self.k):
            p = self.peers(j) if self.topo else uniform[:, j]
            lost = nr.edge_lost(self.seed, N, self.loss, self.parts, n, p, self.t, j)
            live = init & ~lost
            coin = init & (coin_word(self.seed, n, self.t, j).astype(np.int64) < self.cool)
            src, dst = n[live], p[live]
            fresh = np.zeros(src.size, dtype=bool)
            for w in range(self.W):
                np.bitwise_or.at(gain_s[w], dst, H[w][src])
                new = H[w][src] & ~S[w][dst]
                np.bitwise_or.at(gain_h[w], dst, new)
                fresh |= new != 0
                counted = H[w] if self.blind else np.where(live, H[w] & S[w][p], _U(0))
                cleared[w] |= np.where(coin, counted, _U(0))
            g["stale"] += int((~fresh).sum())
            g["lost"] += int((init & lost).sum())
        # gains lie outside S_t[n], losses inside H_t[n] ⊆ S_t[n]: they cannot collide
        assert not (gain_h & S).any() and not (cleared & ~H).any()
        g["cooled"] = popcount(cleared)
        g["and_or"] = int(((cleared != 0) & (gain_h != 0)).any(axis=0).sum())
        self.S = S | gain_s
        self.H = (H | gain_h) & ~cleared
        full, inf = nr.stats_of(self.S, self.R)
        st = dict(round=self.t, converged=int(full == N), full_nodes=full, alive_nodes=N,
                  messages=self.k * int(init.sum()), state_hash=nr.state_hash(self.S))
        self.t += 1
        return st, inf, g

    def step(self, max_rounds):
        """Rounds until one sends nothing (reported) or max_rounds, shaped like Engine.step's result,
        with the guards of every round beside it."""
        stats, infected, guards = [], [], []
        for _ in range(max_rounds):
            st, inf, g = self.round()
            stats.append(st)
            infected.append(inf)
            guards.append(g)
            if st["messages"] == 0:
                break
        return SimpleNamespace(rounds=len(stats), stats=stats, guards=guards,
                               infected=np.array(infected, dtype=np.uint64).reshape(len(stats), self.R))
