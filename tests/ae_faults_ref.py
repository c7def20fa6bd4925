"""numpy restatement of ANTIENTROPY under edge loss and partitions, and the
engine-shaped wrapper the fault tests drive it through.

numpy_ref.AntiEntropySim is the fault-free round of §2.7.  Here an exchange n -> p_j(n, t) takes
place iff both ends are alive after the round's churn and the edge is not lost by the §2.8 rule
(numpy_ref.edge_lost: a partition between the ends, or the loss draw of stream tag 4: the draw a
random-mode engine of the same seed, N and k makes for that edge).  A lost exchange moves neither
row and is no message.  Everything else (churn, target, stats, hash) is the parent's.

Besides the engine's stats a round reports `lost`: the alive-alive edges the fault rule dropped.
The engine has no such stat; the tests use it to show that their faults did drop something."""
import numpy as np

import numpy_ref as nr
from gossip_hip.engine import StepResult
# (imported here, not where it is used: torch has to be loaded before the first HIP engine exists)
from gossip_hip.sharded import lockstep_run


class AeFaultsSim(nr.AntiEntropySim):
    def __init__(self, n_nodes, k_comp, fanout, seed, fail=0, recover=0, edge_loss=0, partitions=0):
        super().__init__(n_nodes, k_comp, fanout, seed, fail, recover)
        self.loss, self.parts = edge_loss, partitions

    def set_faults(self, edge_loss=0, partitions=0):
        """Takes effect in the next round; rows, alive bits and the round index stay."""
        self.loss, self.parts = edge_loss, partitions

    def round(self):
        N = self.N
        k0, k1 = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        n32 = np.arange(N, dtype=np.uint32)
        if self.k <= 3:
            x0 = nr.philox4x32_10(n32, np.uint32(self.t), np.uint32(0), np.uint32(0), k0, k1)[3]
        else:
            x0 = nr.philox4x32_10(n32, np.uint32(self.t), np.uint32(1), np.uint32(0), k0, k1)[0]
        alive = np.where(self.alive, ~(x0 < np.uint32(self.fail)), x0 < np.uint32(self.rec))
        P = nr.peers(self.seed, N, self.t, self.k).astype(np.int64)
        n = np.arange(N, dtype=np.int64)
        V = self.V
        Vn = V.copy()
        msgs = lost_n = 0
        for j in range(self.k):
            p = P[:, j]
            both = alive & alive[p]
            lost = nr.edge_lost(self.seed, N, self.loss, self.parts, n, p, self.t, j)
            e = both & ~lost
            lost_n += int((both & lost).sum())
            src = np.nonzero(e)[0]
            dst = p[e]
            msgs += int(src.size)
            if not src.size:
                continue
            Vn[src] = np.maximum(Vn[src], V[dst])  # pull (src holds each node once)
            # push: a node may be picked by many; the max over its senders' S_t rows, by sorted runs
            # (np.maximum.at(Vn, dst, V[src]), which is slow at the GPU tests' sizes)
            order = np.argsort(dst, kind="stable")
            d = dst[order]
            starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
            Vn[d[starts]] = np.maximum(Vn[d[starts]], np.maximum.reduceat(V[src[order]], starts, axis=0))
        self.V, self.alive = Vn, alive
        target = V.max(axis=0)  # over every node, whatever the partition
        eq = Vn == target[None, :]
        full = int((eq.all(axis=1) & alive).sum())
        inf = [int(x) for x in (eq & alive[:, None]).sum(axis=0)]
        idx = (np.arange(self.K, dtype=np.uint64)[None, :] * np.uint64(N) + np.arange(N, dtype=np.uint64)[:, None])
        with np.errstate(over="ignore"):
            h = nr.mix64(Vn.astype(np.uint64) + idx * np.uint64(nr.GOLD))
        h = int(np.sum(np.where(Vn != 0, h, np.uint64(0)), dtype=np.uint64))
        st = dict(round=self.t, full=full, alive=int(alive.sum()), converged=int(full == int(alive.sum())),
                  messages=msgs, hash=h, infected=inf, lost=lost_n)
        self.t += 1
        return st


class RefEngine:
    """AeFaultsSim behind the AbiEngine calls the tests make (stats in gossip_round_stats_t's names).
    `lost` collects the per-round count of dropped alive-alive edges, in step order."""

    def __init__(self, n_nodes, K, mode, k, seed, flags=1, churn_fail=0, churn_recover=0, edge_loss=0, partitions=0):
        assert mode == "antientropy"
        self.n_nodes, self.n_rumors = n_nodes, K
        self.sim = AeFaultsSim(n_nodes, K, k, seed, churn_fail, churn_recover, edge_loss, partitions)
        self.lost = []

    def inject_random(self):
        self.sim.inject_random()

    def inject(self, node, comp=0):
        self.sim.inject(node, comp)

    def set_faults(self, edge_loss=0, partitions=0):
        self.sim.set_faults(edge_loss, partitions)

    def reset(self):
        """gossip_reset: rows zero, every node alive, round 0; the faults stay."""
        self.sim.V[:] = 0
        self.sim.alive[:] = True
        self.sim.t = 0

    def step(self, max_rounds):
        out = self.sim.run(max_rounds)
        self.lost += [s["lost"] for s in out]
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
    """Drives one engine (HIP, oracle or RefEngine) or a list of shard engines in lockstep through
    `script` and returns what a parity test compares, one entry per ("step", rounds): the per-round
    stats, the per-component counts (one engine), every row, the probed alive flags (one engine),
    the round kinds (shards).  Other ops: ("random",), ("inject", node, comp), ("faults", edge_loss,
    partitions), ("reset",): applied to every shard alike."""
    shards = e if isinstance(e, list) else None
    out = []
    for op in script:
        if op[0] == "step" and shards:
            stats, kinds = lockstep_run(shards, op[1])
            rows = np.concatenate([x.read_rows() for x in shards])
            out.append(dict(stats=stats, rows=rows, kinds=sorted(set(kinds))))
        elif op[0] == "step":
            r = e.step(op[1])
            out.append(dict(stats=r.stats, infected=np.array(r.infected), rows=e.read_rows(),
                            alive=[e.read_versions(n)[1] for n in probe]))
        else:
            name = {"random": "inject_random", "inject": "inject", "faults": "set_faults", "reset": "reset"}[op[0]]
            for x in shards or [e]:
                getattr(x, name)(*op[1:])
    return out


def assert_same(got, want, keys=("stats", "infected", "rows", "alive")):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g["stats"]) == len(w["stats"]), (i, len(g["stats"]), len(w["stats"]))
        for t, (a, b) in enumerate(zip(g["stats"], w["stats"])):
            assert a == b, (i, t, a, b)
        for k in keys[1:]:
            if k in g and k in w:
                assert np.array_equal(g[k], w[k]), (i, k)
