"""Push-pull rumor mongering (GOSSIP_FLAG_MONGER_PUSHPULL), restated in vectorised numpy.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest) that the CPU and GPU tests of the flag
share.  It is built on oracle/numpy_ref.py's Philox, peers, edge test, stats and hash, on
tests/topo_ref.py's rows and row index and on tests/monger_ref.py's coin word, and shares no code
with the engine.  Its call surface is tests/monger_pull_ref.py's MongerPullSim's.

Per node two bitsets, S (known) and H ⊆ S (hot), and a count C[n][r].  Round t reads S_t, H_t, C_t:

    n initiates         always (over the topology: iff its row is not empty), k exchanges, full, cold or not
    p_j(n, t)           the uniform draw of §2.2, or row_n[i_j] of §2.10; lost as in §2.8 (by n's draw)
    delivered (n, p)    S_{t+1}[n] |= H_t[p];   H_{t+1}[n] |= H_t[p] & ~S_t[n]
                        S_{t+1}[p] |= H_t[n];   H_{t+1}[p] |= H_t[n] & ~S_t[p]
    need[x]             OR over the delivered exchanges of x with y, in either role, of H_t[x] & ~S_t[y]
    less[x]             the same of H_t[x] & S_t[y]           (blind: need nothing, less H_t[x] if touched)
    coin of x           Philox4x32-10({x, t, 5, 0}, key)[0] < cool, one per node and round
    r in need[x]        C_{t+1}[x][r] = 0, and nothing else
    else r in less[x]   and the coin holds: C_{t+1} = C_t + 1; r cools at x iff C_{t+1} >= limit

messages = the delivered exchanges in which at least one end had something hot.  A run ends with the
first round that leaves no node hot (that round is reported) or after max_rounds; neither
`converged` nor a round without messages ends it.

Beside the stats every round reports the guards the GPU tests need to know that a pass is not
vacuous: bits cooled, counts reset from above 0, bits counted and kept hot, rumors with both a needed
and a needless exchange at one node in the round, nodes that gained and lost hot bits in one word,
lost exchanges, exchanges in which both ends gained from each other (what tells the round from a
pull round followed by a push round), nodes whose feedback came in the initiator role only and in
the target role only, and whether the round sent nothing while leaving nodes hot.
"""
from types import SimpleNamespace

import numpy as np

import monger_ref as mr
import numpy_ref as nr
import topo_ref as tr

_U = np.uint64
GUARDS = ("cooled", "reset", "kept", "both", "gain_lose", "lost", "mutual", "init_only", "target_only", "quiet")
CMAX = 15


def unpack(words, R):
    """[W][n] uint64 -> bool [R][n]."""
    return np.array([((words[r // 64] >> _U(r % 64)) & _U(1)).astype(bool) for r in range(R)])


def pack(bits, W):
    """bool [R][n] -> [W][n] uint64."""
    out = np.zeros((W, bits.shape[1]), dtype=np.uint64)
    for r in range(bits.shape[0]):
        out[r // 64] |= bits[r].astype(np.uint64) << _U(r % 64)
    return out


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def _or_at(words, idx, values):
    """words[idx] |= values where idx may repeat (the zero values skipped: late in a run most are)."""
    nz = values != 0
    if nz.any():
        np.bitwise_or.at(words, idx[nz], values[nz])


class MongerPushPullSim:
    """Unsharded reference loop of a PUSHPULL engine with GOSSIP_FLAG_MONGER_PUSHPULL; topo_peers: the
    peers come from the rows (GOSSIP_FLAG_TOPO_PEERS), else from all N nodes whatever topology was set."""

    def __init__(self, n_nodes, n_rumors, fanout, seed=0, topo_peers=False, topology=None, edge_loss=0, partitions=0):
        self.N, self.R, self.k, self.seed, self.topo = n_nodes, n_rumors, fanout, seed, topo_peers
        self.loss, self.parts = edge_loss, partitions
        self.W = (n_rumors + 63) // 64
        self.cool, self.blind, self.limit, self.tracking = 0, False, 1, False
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
        self.cool, self.blind = mr.threshold(cool), bool(blind)

    def set_monger_limit(self, limit):
        """Counts are kept from the first limit above 1 on (until then every count reads 0)."""
        assert 1 <= limit <= CMAX
        self.limit = int(limit)
        if limit > 1:
            self.tracking = True

    def reset(self):
        """Clears both bitsets, the counts and the round index; cool, blind and the limit stay."""
        self.S = np.zeros((self.W, self.N), dtype=np.uint64)
        self.H = np.zeros((self.W, self.N), dtype=np.uint64)
        self.C = np.zeros((self.R, self.N), dtype=np.uint8)
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

    def read_counts(self):
        return self.C.copy()

    def hot_nodes(self):
        return int((self.H != 0).any(axis=0).sum())

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
        S, H, N, R = self.S, self.H, self.N, self.R
        n = np.arange(N, dtype=np.int64)
        starts = self.deg > 0 if self.topo else np.ones(N, dtype=bool)
        gain = np.zeros_like(S)
        need = np.zeros_like(S)        # the feedback sets whatever the variant
        less = np.zeros_like(S)
        touched = np.zeros(N, dtype=bool)
        as_init = np.zeros(N, dtype=bool)     # feedback about something hot reached the node in this role
        as_target = np.zeros(N, dtype=bool)
        g = dict.fromkeys(GUARDS, 0)
        msgs = 0
        uniform = None if self.topo else nr.peers(self.seed, N, self.t, self.k).astype(np.int64)
        for j in range(self.k):
            p = self.peers(j) if self.topo else uniform[:, j]
            lost = nr.edge_lost(self.seed, N, self.loss, self.parts, n, p, self.t, j)
            g["lost"] += int((starts & lost).sum())
            live = starts & ~lost
            src, dst = n[live], p[live]          # a lost exchange moves nothing and tells nobody anything
            touched[src] = True
            touched[dst] = True
            carried = np.zeros(src.size, dtype=bool)
            src_gained = np.zeros(src.size, dtype=bool)
            dst_gained = np.zeros(src.size, dtype=bool)
            for w in range(self.W):
                hs, hd, ss, sd = H[w][src], H[w][dst], S[w][src], S[w][dst]
                carried |= (hs | hd) != 0
                src_gained |= (hd & ~ss) != 0
                dst_gained |= (hs & ~sd) != 0
                gain[w][src] |= hd               # (src holds every node at most once)
                need[w][src] |= hs & ~sd
                less[w][src] |= hs & sd
                _or_at(gain[w], dst, hs)
                _or_at(need[w], dst, hd & ~ss)
                _or_at(less[w], dst, hd & ss)
                as_init[src[hs != 0]] = True
                as_target[dst[hd != 0]] = True
            msgs += int(carried.sum())
            g["mutual"] += int((src_gained & dst_gained).sum())
        g["init_only"] = int((as_init & ~as_target).sum())
        g["target_only"] = int((as_target & ~as_init).sum())
        assert not (need & ~H).any() and not (less & ~H).any()
        if self.blind:                           # a node learns only that an exchange took place
            need, less = np.zeros_like(S), np.where(touched, H, _U(0))
        else:
            g["both"] = popcount(need & less)
        # one coin per node and round; one counter step per round, and none where the rumor was needed
        coin = mr.coin_word(self.seed, n, self.t, 0).astype(np.int64) < self.cool
        inc = np.where(coin, less & ~need, _U(0))
        cleared = np.zeros_like(S)
        cols = np.nonzero(((need | inc) != 0).any(axis=0))[0]
        if cols.size:
            C = self.C[:, cols].copy()
            nd, up = unpack(need[:, cols], R), unpack(inc[:, cols], R)
            g["reset"] = int((nd & (C > 0)).sum())
            C[nd] = 0
            C[up] += 1
            assert int(C.max()) <= CMAX           # hot means below the limit: 15 is never passed
            cool = up & (C >= self.limit)
            g["cooled"], g["kept"] = int(cool.sum()), int((up & ~cool).sum())
            cleared[:, cols] = pack(cool, self.W)
            if self.tracking:
                self.C[:, cols] = C
        gain_h = gain & ~S
        # gains lie outside S_t[x] ⊇ H_t[x], losses inside H_t[x]: they cannot collide
        assert not (cleared & ~H).any() and not (gain_h & H).any()
        g["gain_lose"] = int(((cleared != 0) & (gain_h != 0)).any(axis=0).sum())
        self.S = S | gain
        self.H = (H | gain_h) & ~cleared
        g["quiet"] = int(msgs == 0 and self.H.any())
        full, inf = nr.stats_of(self.S, R)
        st = dict(round=self.t, converged=int(full == N), full_nodes=full, alive_nodes=N, messages=msgs,
                  state_hash=nr.state_hash(self.S))
        self.t += 1
        return st, inf, g

    def step(self, max_rounds):
        """Rounds until one leaves no node hot (reported) or max_rounds, shaped like Engine.step's
        result, with the guards of every round beside it."""
        stats, infected, guards = [], [], []
        for _ in range(max_rounds):
            st, inf, g = self.round()
            stats.append(st)
            infected.append(inf)
            guards.append(g)
            if not self.H.any():
                break
        return SimpleNamespace(rounds=len(stats), stats=stats, guards=guards,
                               infected=np.array(infected, dtype=np.uint64).reshape(len(stats), self.R))
