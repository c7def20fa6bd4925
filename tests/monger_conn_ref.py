"""Mongering with connection limits and hunting (gossip_set_monger_connections),
restated in vectorised numpy for the three mongering modes.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest) that the CPU and GPU tests of the limit
share.  It is built on oracle/numpy_ref.py's Philox, peers, edge test, stats and hash, on
tests/topo_ref.py's rows and row index and on tests/monger_ref.py's coin word, and shares no code
with the engine or with the three unlimited restatements it is held to (tests/test_monger_conn_ref.py).

Round t with a limit c >= 1 and h hunts: who initiates, k, the stage-0 peer, the loss draw, the
coins and a delivered exchange are §2.13-§2.16; the limit decides which edges are delivered and where:

    stage s = 0 .. h   every open edge (n, j) attempts q_s; q_0 = p_j(n, t), and for s >= 1
                       hw = Philox4x32-10({n, t, 6 | s << 16, 16 + (j >> 2)}, key)[j & 3] mapped as the
                       stage-0 word (over all nodes, or over n's row), with replacement
    lost               the tag-4 draw of the edge (once, at stage 0), or a target outside n's partition
                       block (any stage): the edge closes, takes no place and is not hunted for
    contend            prio = top 22 bits of Philox4x32-10({n, t, 6 | s << 16, j >> 2}, key)[j & 3]; the
                       free places of a target go to the lowest (prio, n, j) of the stage's contenders;
                       a place taken in an earlier stage stays taken
    accepted at s      a delivered edge of the round with peer q_s
    refused at s < h   open in stage s + 1;  refused at h: treated exactly as a lost edge

Arbitration here is a lexsort per stage.  messages: push = attempts made (hunts and lost ones
included); pull and push-pull: their definitions with "delivered" read as "accepted".
connections() = {attempts, accepted, refused, hunts} of the last round; edges = accepted + lost +
refused and attempts = edges + hunts.

Beside the stats every round reports the guards the tests need to know that a pass is not vacuous:
refusals; edges accepted at a stage >= 1; edges refused at the last stage; targets whose places
filled over two stages; edges closed by a partition at a hunt stage; groups of edges of one initiator
at one target in one stage of which some were accepted and some refused.
"""
from types import SimpleNamespace

import numpy as np

import monger_ref as mr
import numpy_ref as nr
import topo_ref as tr

_U = np.uint64
GUARDS = ("refusals", "hunt_accepted", "refused_last", "two_stage", "hunt_partition", "split", "lost", "cooled")
CMAX = 15
MODES = ("push", "pull", "pushpull")
CONN_KEYS = ("attempts", "accepted", "refused", "hunts")


def conn_words(seed, nodes, t, s, j):
    """(priority word, hunt word) of edge j at stage s: stream tag 6, the stage in the tag word's
    upper half; counter word 3 = j >> 2 for the priority, 16 + (j >> 2) for the hunt."""
    n = np.asarray(nodes, dtype=np.uint32)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    tag = np.uint32(6 | (s << 16))
    pw = nr.philox4x32_10(n, np.uint32(t), tag, np.uint32(j >> 2), k0, k1)[j & 3]
    hw = nr.philox4x32_10(n, np.uint32(t), tag, np.uint32(16 + (j >> 2)), k0, k1)[j & 3]
    return pw, hw


def unpack(words, R):
    """[W][n] uint64 -> bool [R][n]."""
    return np.array([((words[r // 64] >> _U(r % 64)) & _U(1)).astype(bool) for r in range(R)])


def pack(bits, W):
    """bool [R][n] -> [W][n] uint64."""
    out = np.zeros((W, bits.shape[1]), dtype=np.uint64)
    for r in range(bits.shape[0]):
        out[r // 64] |= bits[r].astype(np.uint64) << _U(r % 64)
    return out


def _or_at(words, idx, values):
    nz = values != 0
    if nz.any():
        np.bitwise_or.at(words, idx[nz], values[nz])


class MongerConnSim:
    """Unsharded reference loop of a mongering engine of one of the three modes with
    gossip_set_monger_connections; topo_peers: the peers, hunted ones included, come from the rows."""

    def __init__(self, mode, n_nodes, n_rumors, fanout, seed=0, topo_peers=False, topology=None, edge_loss=0,
                 partitions=0):
        assert mode in MODES
        self.mode, self.N, self.R, self.k, self.seed, self.topo = mode, n_nodes, n_rumors, fanout, seed, topo_peers
        self.loss, self.parts = edge_loss, partitions
        self.W = (n_rumors + 63) // 64
        self.cool, self.blind, self.limit, self.tracking = 0, False, 1, False
        self.c, self.h = 0, 0
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
        assert 1 <= limit <= CMAX
        self.limit = int(limit)
        if limit > 1:
            self.tracking = True

    def set_monger_connections(self, conn_limit, hunt_limit=0):
        assert 0 <= conn_limit <= 8 and 0 <= hunt_limit <= 15 and (conn_limit or not hunt_limit)
        self.c, self.h = int(conn_limit), int(hunt_limit)

    def reset(self):
        """Clears the bitsets, the counts, the round index and the readout; every parameter stays."""
        self.S = np.zeros((self.W, self.N), dtype=np.uint64)
        self.H = np.zeros((self.W, self.N), dtype=np.uint64)
        self.C = np.zeros((self.R, self.N), dtype=np.uint8)
        self.t = 0
        self.last = None

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

    def connections(self):
        """Of the last round; zeros before the first, after reset, after an unlimited round and while c = 0."""
        if self.last is None or self.c == 0:
            return dict.fromkeys(CONN_KEYS, 0)
        return dict(self.last)

    @property
    def round_index(self):
        return self.t

    # -- which edges are delivered, and where ---------------------------------------------------------
    def _target(self, word, n):
        """A Philox word of node n as a peer: over all other nodes, or over n's row."""
        if self.topo:
            idx = (word.astype(_U) * self.deg[n].astype(_U)) >> _U(32)
            return self.col[self.rp[n] + idx.astype(np.int64)]
        p = ((word.astype(_U) * _U(self.N - 1)) >> _U(32)).astype(np.int64)
        return p + (p >= n)

    def _same_block(self, n, p):
        if self.parts <= 1:
            return np.ones(n.shape, dtype=bool)
        return (n * self.parts) // self.N == (p * self.parts) // self.N

    def initiators(self):
        init = (self.H != 0).any(axis=0) if self.mode == "push" else np.ones(self.N, dtype=bool)
        if self.topo:
            init = init & (self.deg > 0)
        return init

    def edges(self):
        """(init, peer [k][N], delivered [k][N], lost at stage 0 [k][N], conn, guards): the round's edges
        after arbitration.  peer is the accepting target where delivered; conn is None without a limit."""
        N, k, t = self.N, self.k, self.t
        init = self.initiators()
        g = dict.fromkeys(GUARDS, 0)
        node = np.arange(N, dtype=np.int64)
        peer = np.empty((k, N), dtype=np.int64)
        lost0 = np.zeros((k, N), dtype=bool)
        if self.topo:
            for j in range(k):   # (n itself where the row is empty: never used)
                peer[j] = node
                if self.col.size:
                    at = self.rp[:-1] + tr.row_index(self.seed, self.deg, node, t, j)
                    peer[j] = np.where(self.deg > 0, self.col[np.minimum(at, self.col.size - 1)], node)
        else:
            peer[:] = nr.peers(self.seed, N, t, k).astype(np.int64).T
        for j in range(k):
            lost0[j] = init & nr.edge_lost(self.seed, N, self.loss, self.parts, node, peer[j], t, j)
        g["lost"] = int(lost0.sum())
        open_ = init[None, :] & ~lost0
        if self.c == 0:
            return init, peer, open_, lost0, None, g
        n_edges = k * int(init.sum())
        conn = dict(attempts=n_edges, accepted=0, refused=0, hunts=0)
        delivered = np.zeros((k, N), dtype=bool)
        free = np.full(N, self.c, dtype=np.int64)
        filled_in = np.zeros(N, dtype=np.int64)   # stages in which the target accepted something
        lost_total = int(lost0.sum())
        for s in range(self.h + 1):
            jj, nn = np.nonzero(open_)
            if nn.size == 0:
                break
            q = peer[jj, nn]
            prio = np.empty(nn.size, dtype=np.int64)
            for j in np.unique(jj):
                m = jj == j
                prio[m] = conn_words(self.seed, nn[m], t, s, int(j))[0].astype(np.int64) >> 10
            order = np.lexsort((jj, nn, prio, q))
            qs = q[order]
            first = np.r_[0, np.nonzero(np.diff(qs))[0] + 1]
            rank = np.arange(qs.size) - np.repeat(first, np.diff(np.r_[first, qs.size]))
            ok_sorted = rank < free[qs]
            ok = np.empty(nn.size, dtype=bool)
            ok[order] = ok_sorted
            # the invariants: a target takes no more than it has free, and refuses only when it is full
            took = np.bincount(q[ok], minlength=N)
            assert (took <= free).all()
            full_after = (free - took) == 0
            assert full_after[q[~ok]].all()
            free = free - took
            filled_in += took > 0
            delivered[jj[ok], nn[ok]] = True
            conn["accepted"] += int(ok.sum())
            if s >= 1:
                g["hunt_accepted"] += int(ok.sum())
            g["refusals"] += int((~ok).sum())
            # edges of one initiator at one target: some in, some out
            grp = (nn * N + q)
            both = np.intersect1d(grp[ok], grp[~ok])
            g["split"] += int(both.size)
            open_ = np.zeros((k, N), dtype=bool)
            rj, rn = jj[~ok], nn[~ok]
            if s == self.h:
                conn["refused"] += int(rj.size)
                g["refused_last"] += int(rj.size)
                break
            conn["hunts"] += int(rj.size)
            for j in np.unique(rj):
                m = rj == j
                tgt = self._target(conn_words(self.seed, rn[m], t, s + 1, int(j))[1], rn[m])
                peer[j, rn[m]] = tgt
                inside = self._same_block(rn[m], tgt)
                g["hunt_partition"] += int((~inside).sum())
                lost_total += int((~inside).sum())
                open_[j, rn[m][inside]] = True
        conn["attempts"] += conn["hunts"]
        g["two_stage"] = int((filled_in >= 2).sum())
        assert n_edges == conn["accepted"] + lost_total + conn["refused"]
        assert conn["attempts"] == n_edges + conn["hunts"]
        assert (np.bincount(peer[delivered], minlength=N) <= self.c).all()
        return init, peer, delivered, lost0, conn, g

    # -- one round --------------------------------------------------------------------------------
    def round(self):
        assert not self.topo or self.rp is not None, "needs a topology"
        init, peer, live, _, conn, g = self.edges()
        if self.mode == "push":
            msgs = self._push(init, peer, live, g)
            if conn is not None:
                msgs = conn["attempts"]
        elif self.mode == "pull":
            msgs = self._pull(peer, live, g)
        else:
            msgs = self._pushpull(peer, live, g)
        self.last = conn
        full, inf = nr.stats_of(self.S, self.R)
        st = dict(round=self.t, converged=int(full == self.N), full_nodes=full, alive_nodes=self.N, messages=msgs,
                  state_hash=nr.state_hash(self.S))
        self.t += 1
        return st, inf, g

    def _push(self, init, peer, live, g):
        """§2.13 / §2.14: a coin per edge; the counted set of an edge that is not delivered is H_t[n]
        under blind and nothing under feedback."""
        S, H, N, R = self.S, self.H, self.N, self.R
        node = np.arange(N, dtype=np.int64)
        gain_s, gain_h = np.zeros_like(S), np.zeros_like(S)
        hot = unpack(H, R)
        inc = np.zeros((R, N), dtype=np.uint8)
        for j in range(self.k):
            coin = init & (mr.coin_word(self.seed, node, self.t, j).astype(np.int64) < self.cool)
            src, dst = node[live[j]], peer[j][live[j]]
            for w in range(self.W):
                np.bitwise_or.at(gain_s[w], dst, H[w][src])
                np.bitwise_or.at(gain_h[w], dst, H[w][src] & ~S[w][dst])
            counted = hot if self.blind else hot & unpack(S[:, peer[j]], R) & live[j]
            inc += (counted & coin).astype(np.uint8)
        C = np.minimum(self.C + inc, CMAX).astype(np.uint8)   # (k <= 64: no uint8 sum wraps)
        cooled = (inc > 0) & (C >= self.limit)
        g["cooled"] = int(cooled.sum())
        cleared = pack(cooled, self.W)
        assert not (gain_h & S).any() and not (cleared & ~H).any()
        self.S = S | gain_s
        self.H = (H | gain_h) & ~cleared
        if self.tracking:
            self.C = C
        return self.k * int(init.sum())

    def _close(self, need, less, gain, g):
        """§2.15 items 4-5 / §2.16 item 5: one coin per node and round, one counter step per round."""
        S, H, N, R = self.S, self.H, self.N, self.R
        node = np.arange(N, dtype=np.int64)
        coin = mr.coin_word(self.seed, node, self.t, 0).astype(np.int64) < self.cool
        inc = np.where(coin, less & ~need, _U(0))
        cleared = np.zeros_like(S)
        cols = np.nonzero(((need | inc) != 0).any(axis=0))[0]
        if cols.size:
            C = self.C[:, cols].copy()
            nd, up = unpack(need[:, cols], R), unpack(inc[:, cols], R)
            C[nd] = 0
            C[up] += 1
            assert int(C.max()) <= CMAX
            cool = up & (C >= self.limit)
            g["cooled"] = int(cool.sum())
            cleared[:, cols] = pack(cool, self.W)
            if self.tracking:
                self.C[:, cols] = C
        gain_h = gain & ~S
        assert not (cleared & ~H).any() and not (gain_h & H).any()
        self.S = S | gain
        self.H = (H | gain_h) & ~cleared

    def _pull(self, peer, live, g):
        S, H, N = self.S, self.H, self.N
        node = np.arange(N, dtype=np.int64)
        gain, need, less = np.zeros_like(S), np.zeros_like(S), np.zeros_like(S)
        msgs = 0
        for j in range(self.k):
            src, dst = node[live[j]], peer[j][live[j]]
            carried = np.zeros(src.size, dtype=bool)
            for w in range(self.W):
                reply = H[w][dst]
                carried |= reply != 0
                gain[w][src] |= reply
                if self.blind:
                    _or_at(less[w], dst, reply)
                else:
                    _or_at(need[w], dst, reply & ~S[w][src])
                    _or_at(less[w], dst, reply & S[w][src])
            msgs += int(carried.sum())
        self._close(need, less, gain, g)
        return msgs

    def _pushpull(self, peer, live, g):
        S, H, N = self.S, self.H, self.N
        node = np.arange(N, dtype=np.int64)
        gain, need, less = np.zeros_like(S), np.zeros_like(S), np.zeros_like(S)
        touched = np.zeros(N, dtype=bool)
        msgs = 0
        for j in range(self.k):
            src, dst = node[live[j]], peer[j][live[j]]
            touched[src] = True
            touched[dst] = True
            carried = np.zeros(src.size, dtype=bool)
            for w in range(self.W):
                hs, hd, ss, sd = H[w][src], H[w][dst], S[w][src], S[w][dst]
                carried |= (hs | hd) != 0
                gain[w][src] |= hd
                need[w][src] |= hs & ~sd
                less[w][src] |= hs & sd
                _or_at(gain[w], dst, hs)
                _or_at(need[w], dst, hd & ~ss)
                _or_at(less[w], dst, hd & ss)
            msgs += int(carried.sum())
        if self.blind:   # a node learns only that an exchange took place
            need, less = np.zeros_like(S), np.where(touched, H, _U(0))
        self._close(need, less, gain, g)
        return msgs

    def step(self, max_rounds):
        """Rounds until the mode's stop rule (push: a round that sends nothing; else: one that leaves no
        node hot; that round is reported) or max_rounds, shaped like Engine.step's result, with the
        guards and the connections() of every round beside it."""
        stats, infected, guards, conns = [], [], [], []
        for _ in range(max_rounds):
            st, inf, g = self.round()
            stats.append(st)
            infected.append(inf)
            guards.append(g)
            conns.append(self.connections())
            if (st["messages"] == 0) if self.mode == "push" else not self.H.any():
                break
        return SimpleNamespace(rounds=len(stats), stats=stats, guards=guards, conns=conns,
                               infected=np.array(infected, dtype=np.uint64).reshape(len(stats), self.R))
