"""numpy restatement of ANTIENTROPY over the topology (GOSSIP_FLAG_AE_TOPO_PEERS),
and the engine-shaped wrapper the parity tests drive it through.

TEST INFRASTRUCTURE ONLY: a plain module (not a conftest).  It is built on oracle/numpy_ref.py's
Philox, edge test and AntiEntropySim (churn, target, stats, hash) and on topo_ref.py's
rows_as_sets / row_index, and shares no code with the engine.

The round is §2.7's with §2.11's lost edges and one change, the peer draw, which is §2.10's:

    x   = Philox4x32-10({n, t, 0, j >> 2}, key)[j & 3]
    i_j = floor(x * deg(n) / 2^32),   p_j(n, t) = row_n[i_j]     (rows as sorted sets)

A node with an empty row initiates nothing; it still churns, answers and can be picked.  Draws are
with replacement: a node may draw one neighbour twice and, on a self-loop, itself.  messages =
exchanges that took place (both ends alive after the churn, edge not lost), self-exchanges included.

Besides the engine's stats a round reports `lost` (alive-alive edges the fault rule dropped, as
ae_faults_ref), `selfs` (exchanges with oneself), `repeats` (exchanges whose (n, p) pair took place
earlier in the same round) and `empty_alive` (alive nodes with an empty row).  The engine has no such
stats; the tests use them to show that a case is not vacuous."""
import numpy as np

# (ae_faults_ref loads torch through gossip_hip.sharded: before the first HIP engine exists)
import ae_faults_ref as fr
import numpy_ref as nr
import topo_ref as tr
from gossip_hip.engine import StepResult


class AeTopoSim(nr.AntiEntropySim):
    def __init__(self, n_nodes, k_comp, fanout, seed, fail=0, recover=0, edge_loss=0, partitions=0, topology=None):
        super().__init__(n_nodes, k_comp, fanout, seed, fail, recover)
        self.loss, self.parts = edge_loss, partitions
        self.rp = self.col = self.deg = None
        if topology is not None:
            self.set_topology(topology)

    def set_topology(self, topology):
        """Takes effect in the next round; rows, alive bits and the round index stay."""
        self.rp, self.col = tr.rows_as_sets(topology[0], topology[1], self.N)
        self.deg = np.diff(self.rp)

    def set_faults(self, edge_loss=0, partitions=0):
        self.loss, self.parts = edge_loss, partitions

    def peers(self, j):
        """p_j(n, t) for every n (n itself where the row is empty: never used)."""
        n = np.arange(self.N, dtype=np.int64)
        if self.col.size == 0:
            return n
        at = self.rp[:-1] + tr.row_index(self.seed, self.deg, n, self.t, j)
        return np.where(self.deg > 0, self.col[np.minimum(at, self.col.size - 1)], n)

    def round(self):
        assert self.rp is not None, "needs a topology"
        N = self.N
        k0, k1 = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        n32 = np.arange(N, dtype=np.uint32)
        if self.k <= 3:
            x0 = nr.philox4x32_10(n32, np.uint32(self.t), np.uint32(0), np.uint32(0), k0, k1)[3]
        else:
            x0 = nr.philox4x32_10(n32, np.uint32(self.t), np.uint32(1), np.uint32(0), k0, k1)[0]
        alive = np.where(self.alive, ~(x0 < np.uint32(self.fail)), x0 < np.uint32(self.rec))
        n = np.arange(N, dtype=np.int64)
        has = self.deg > 0
        V = self.V
        Vn = V.copy()
        msgs = lost_n = selfs = 0
        pairs = []
        for j in range(self.k):
            p = self.peers(j)
            both = has & alive & alive[p]
            lost = nr.edge_lost(self.seed, N, self.loss, self.parts, n, p, self.t, j)
            e = both & ~lost
            lost_n += int((both & lost).sum())
            src = np.nonzero(e)[0]
            dst = p[e]
            msgs += int(src.size)
            selfs += int((src == dst).sum())
            pairs.append(src * N + dst)
            if not src.size:
                continue
            Vn[src] = np.maximum(Vn[src], V[dst])  # pull (src holds each node once)
            # push: the max over the S_t rows of a node's senders, by sorted runs (ae_faults_ref)
            order = np.argsort(dst, kind="stable")
            d = dst[order]
            starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
            Vn[d[starts]] = np.maximum(Vn[d[starts]], np.maximum.reduceat(V[src[order]], starts, axis=0))
        allp = np.concatenate(pairs) if pairs else np.zeros(0, dtype=np.int64)
        repeats = int(allp.size - np.unique(allp).size)
        self.V, self.alive = Vn, alive
        target = V.max(axis=0)  # over every node, whatever the graph
        eq = Vn == target[None, :]
        full = int((eq.all(axis=1) & alive).sum())
        inf = [int(x) for x in (eq & alive[:, None]).sum(axis=0)]
        idx = (np.arange(self.K, dtype=np.uint64)[None, :] * np.uint64(N) + np.arange(N, dtype=np.uint64)[:, None])
        with np.errstate(over="ignore"):
            h = nr.mix64(Vn.astype(np.uint64) + idx * np.uint64(nr.GOLD))
        h = int(np.sum(np.where(Vn != 0, h, np.uint64(0)), dtype=np.uint64))
        st = dict(round=self.t, full=full, alive=int(alive.sum()), converged=int(full == int(alive.sum())),
                  messages=msgs, hash=h, infected=inf, lost=lost_n, selfs=selfs, repeats=repeats,
                  empty_alive=int((alive & ~has).sum()))
        self.t += 1
        return st


class RefEngine:
    """AeTopoSim behind the AbiEngine calls the tests make (ae_faults_ref.RefEngine with
    set_topology), so ae_faults_ref.run_script / assert_same drive it.  `lost`, `selfs`, `repeats`
    and `empty_alive` collect the per-round figures in step order."""

    def __init__(self, n_nodes, K, mode, k, seed, flags=1, churn_fail=0, churn_recover=0, edge_loss=0, partitions=0,
                 topology=None):
        assert mode == "antientropy"
        self.n_nodes, self.n_rumors = n_nodes, K
        self.sim = AeTopoSim(n_nodes, K, k, seed, churn_fail, churn_recover, edge_loss, partitions, topology)
        self.lost, self.selfs, self.repeats, self.empty_alive = [], [], [], []

    def set_topology(self, topology):
        self.sim.set_topology(topology)

    def inject_random(self):
        self.sim.inject_random()

    def inject(self, node, comp=0):
        self.sim.inject(node, comp)

    def set_faults(self, edge_loss=0, partitions=0):
        self.sim.set_faults(edge_loss, partitions)

    def reset(self):
        """gossip_reset: rows zero, every node alive, round 0; the faults and the topology stay."""
        self.sim.V[:] = 0
        self.sim.alive[:] = True
        self.sim.t = 0

    def step(self, max_rounds):
        out = self.sim.run(max_rounds)
        for key in ("lost", "selfs", "repeats", "empty_alive"):
            getattr(self, key).extend(s[key] for s in out)
        stats = [dict(round=s["round"], converged=s["converged"], full_nodes=s["full"], alive_nodes=s["alive"],
                      messages=s["messages"], state_hash=s["hash"]) for s in out]
        inf = np.array([s["infected"] for s in out], dtype=np.uint64).reshape(len(out), self.n_rumors)
        return StepResult(len(out), stats, inf)

    def read_rows(self):
        return self.sim.V.copy()

    def read_versions(self, node):
        return self.sim.V[node].copy(), bool(self.sim.alive[node])

    def close(self):
        pass


def run_script(e, script, probe=()):
    """ae_faults_ref.run_script with one more op, ("topology", (row_ptr, col)): applied to every
    shard alike, like the other state changes."""
    out, rest = [], []
    for op in tuple(script) + (None,):
        if op is not None and op[0] != "topology":
            rest.append(op)
            continue
        out += fr.run_script(e, rest, probe)
        rest = []
        if op is not None:
            for x in e if isinstance(e, list) else [e]:
                x.set_topology(op[1])
    return out
