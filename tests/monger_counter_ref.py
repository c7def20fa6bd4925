"""Rumor mongering with counters (gossip_set_monger_limit), restated in numpy.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest) that the CPU and GPU tests of the counter
rule share.  It is built on tests/monger_ref.py's MongerSim (peers, edge_lost, coin_word, stats,
hash) with an integer count per node and rumor, and shares no code with the engine.

Round t is §2.13's round with the cooling replaced:

    inc[n][r]          the edges j < k whose coin holds and whose counted set contains r
    C_{t+1}[n][r]      min(C_t[n][r] + inc, 15)
    r cools at n       iff inc > 0 and C_{t+1}[n][r] >= limit

With limit = 1 that is §2.13 itself.  Beside the stats every round reports the guards the GPU tests
need to know that a pass is not vacuous: bits cooled, bits incremented and kept hot, increments that
changed a bit above the lowest of a count, bits whose raw sum passed 15, nodes that in one round
lost a bit and gained a hot bit in the same word, and lost attempts.
"""
import numpy as np

import monger_ref as mr
import numpy_ref as nr

_U = np.uint64
GUARDS = ("cooled", "kept", "carry", "sat", "and_or", "lost")
CMAX = 15


def unpack(words, R):
    """[W][N] uint64 -> bool [R][N]."""
    return np.array([((words[r // 64] >> _U(r % 64)) & _U(1)).astype(bool) for r in range(R)])


def pack(bits, W):
    """bool [R][N] -> [W][N] uint64."""
    out = np.zeros((W, bits.shape[1]), dtype=np.uint64)
    for r in range(bits.shape[0]):
        out[r // 64] |= bits[r].astype(np.uint64) << _U(r % 64)
    return out


class MongerCounterSim(mr.MongerSim):
    """MongerSim with gossip_set_monger_limit: C is an integer array [R][N], kept from the first limit
    above 1 on (item 9: until then every count reads 0, and a reset does not end the keeping)."""

    def __init__(self, *a, **kw):
        self.limit = 1
        self.tracking = False
        super().__init__(*a, **kw)

    def set_monger_limit(self, limit):
        assert 1 <= limit <= CMAX
        self.limit = int(limit)
        if limit > 1:
            self.tracking = True

    def reset(self):
        """Clears the bitsets, the counts and the round index; cool, blind and the limit stay."""
        super().reset()
        self.C = np.zeros((self.R, self.N), dtype=np.uint8)

    def read_counts(self):
        return self.C.copy()

    def edges(self):
        """Per edge j: (peers, live, coin) of round t, for the initiating nodes."""
        n = np.arange(self.N, dtype=np.int64)
        init = (self.H != 0).any(axis=0)
        if self.topo:
            init &= self.deg > 0
        uniform = None if self.topo else nr.peers(self.seed, self.N, self.t, self.k).astype(np.int64)
        out = []
        for j in range(self.k):
            p = self.peers(j) if self.topo else uniform[:, j]
            lost = nr.edge_lost(self.seed, self.N, self.loss, self.parts, n, p, self.t, j)
            coin = init & (mr.coin_word(self.seed, n, self.t, j).astype(np.int64) < self.cool)
            out.append((p, init & ~lost, coin, int((init & lost).sum())))
        return init, out

    def round(self, batch=None):
        """One round.  batch: evaluate the cooling rule per `batch` edges (the kernel's schedule for
        k > 4, item 7) instead of once for the whole round; the result must not differ."""
        assert not self.topo or self.rp is not None, "needs a topology"
        S, H, N, R = self.S, self.H, self.N, self.R
        n = np.arange(N, dtype=np.int64)
        init, edges = self.edges()
        gain_s = np.zeros_like(S)
        gain_h = np.zeros_like(S)
        hot = unpack(H, R)
        g = dict.fromkeys(GUARDS, 0)
        C0 = self.C
        C = C0.copy()
        raw = np.zeros_like(C0)
        cooled = np.zeros((R, N), dtype=bool)
        step = batch or self.k
        for j0 in range(0, self.k, step):
            inc = np.zeros_like(C0)
            for p, live, coin, lost in edges[j0:j0 + step]:
                src, dst = n[live], p[live]
                for w in range(self.W):
                    np.bitwise_or.at(gain_s[w], dst, H[w][src])
                    np.bitwise_or.at(gain_h[w], dst, H[w][src] & ~S[w][dst])
                # feedback: what the peer held, when delivered; blind: every attempt
                counted = hot if self.blind else hot & unpack(S[:, p], R) & live
                inc += (counted & coin).astype(np.uint8)
                g["lost"] += lost
            raw += inc
            C = np.minimum(C + inc, CMAX).astype(np.uint8)   # (k <= 64: no uint8 sum wraps)
            cooled |= (inc > 0) & (C >= self.limit)
        g["sat"] = int((C0.astype(np.int64) + raw > CMAX).sum())
        g["carry"] = int(((raw > 0) & ((C0 >> 1) != (C >> 1))).sum())
        g["cooled"] = int(cooled.sum())
        g["kept"] = int(((raw > 0) & ~cooled).sum())
        cleared = pack(cooled, self.W)
        # gains lie outside S_t[n], losses inside H_t[n] ⊆ S_t[n]: they cannot collide
        assert not (gain_h & S).any() and not (cleared & ~H).any()
        g["and_or"] = int(((cleared != 0) & (gain_h != 0)).any(axis=0).sum())
        self.S = S | gain_s
        self.H = (H | gain_h) & ~cleared
        if self.tracking:
            self.C = C
        full, inf = nr.stats_of(self.S, R)
        st = dict(round=self.t, converged=int(full == N), full_nodes=full, alive_nodes=N,
                  messages=self.k * int(init.sum()), state_hash=nr.state_hash(self.S))
        self.t += 1
        return st, inf, g
