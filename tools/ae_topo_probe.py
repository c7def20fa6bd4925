"""Anti-entropy over a topology (GOSSIP_FLAG_AE_TOPO_PEERS) at scale: the
2048 x 2048 grid (Maelstrom's default topology, 4-neighbourhood), K = 16 components, k = 2 exchanges
per node and round, configs[4]'s churn (1 % fail, 10 % recover), rows from inject_random.  Beside it,
at the same N, K, k and churn, an unflagged engine forced onto the same kernels (ae_dense_bin = 0 and
GOSSIP_FLAG_AE_DIRECT_SCAN: the atomic dense round and the direct sparse scan) that draws its peers
over all N nodes: the difference is the price of the row lookup and the gain of the rows' locality.

Per engine:
  dense   `--dense-rounds` rounds from inject_random with ae_sparse = 0, three times (the first run
          untimed: warm-up); us per round = (timer 0 + timer 1) / rounds: churn, pull and push
          passes, then the stats pass.
  run     the planner's own choice from inject_random to convergence or `--max-rounds`, one
          gossip_step per round, each round classed by the timers it moved: dense (timers 0 and 1),
          sparse (timers 2 and 1: scan, gather, apply, fix-up, then the stats), or overflowed (a
          sparse round whose edge list overflowed and was rerun dense: all three).  Twice: with the
          engine's own edge-list capacity, and with room for every exchange (ae_cap = 2 k N), where
          no round can overflow.
Excluded: set_topology, inject_random, and the host's share of a round (the read-back of the totals
after every round is inside no timer).  The two engines' states differ (a grid's stale nodes are
neighbours in id space and it takes more rounds; the complete graph's are spread evenly), so the
sparse figures compare rounds with different edge lists: the counts are reported with them.
Writes one JSON file into the output directory and prints it.
Usage: ae_topo_probe.py [--out DIR] [--log2 22] [--dense-rounds 16] [--max-rounds 8192]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gossip-protocol_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gossip_hip import FLAG_AE_DIRECT_SCAN, FLAG_AE_TOPO_PEERS, FLAG_TIMING, Engine  # noqa: E402
from gossip_hip.engine import churn_threshold  # noqa: E402
from topo_probe import grid_topology  # noqa: E402

K, FANOUT, SEED, FAIL, RECOVER = 16, 2, 0x5EED0005, 0.01, 0.1


def timers(e):
    return [e.kernel_time(w) for w in (0, 1, 2)]


def classed_run(e, max_rounds):
    """One gossip_step per round from inject_random; per class: rounds and device us per round."""
    e.reset()
    e.inject_random()
    e.reset_timing()
    acc = {c: [0, 0.0] for c in ("dense", "sparse", "overflowed")}
    before, rounds, res = timers(e), 0, None
    while rounds < max_rounds:
        res = e.step(1, with_infected=False)
        rounds += 1
        after = timers(e)
        d = [(a[0] - b[0], a[1] - b[1]) for a, b in zip(after, before)]
        before = after
        cls = "overflowed" if d[0][1] and d[2][1] else "sparse" if d[2][1] else "dense"
        acc[cls][0] += 1
        acc[cls][1] += d[0][0] + d[1][0] + d[2][0]
        if res.converged:
            break
    out = {c: {"rounds": n, "us_per_round": ms * 1e3 / n if n else None} for c, (n, ms) in acc.items()}
    out.update(rounds=rounds, converged=bool(res.converged), full_nodes=res.stats[-1]["full_nodes"],
               alive_nodes=res.stats[-1]["alive_nodes"])
    return out


def measure(n, flags, params, topo, dense_rounds, max_rounds):
    e = Engine(n, K, "antientropy", FANOUT, SEED, flags=flags | FLAG_TIMING, params=params,
               churn_fail=churn_threshold(FAIL), churn_recover=churn_threshold(RECOVER))
    if topo is not None:
        e.set_topology(topo)
    e.set_param("ae_sparse", 0)
    for rep in range(3):
        if rep == 1:
            e.reset_timing()
        e.reset()
        e.inject_random()
        e.step(dense_rounds, with_infected=False)
    t = timers(e)
    assert t[2][1] == 0 and 0 < t[0][1] <= 2 * dense_rounds  # (a run that converges early ends there)
    out = {"dense_us_per_round": (t[0][0] + t[1][0]) * 1e3 / t[0][1], "dense_round_us": t[0][0] * 1e3 / t[0][1],
           "dense_stats_us": t[1][0] * 1e3 / t[1][1], "dense_rounds_timed": t[0][1]}
    e.set_param("ae_sparse", -1)
    out["run_default_cap"] = classed_run(e, max_rounds)
    e.set_param("ae_cap", 2 * FANOUT * n)
    out["run_roomy_cap"] = classed_run(e, max_rounds)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_topo"))
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--dense-rounds", type=int, default=16)
    ap.add_argument("--max-rounds", type=int, default=8192)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n = 1 << a.log2
    t0 = time.perf_counter()
    topo = grid_topology(1 << (a.log2 // 2))
    assert topo[0].size - 1 == n
    out = {"workload": f"grid, N = 2^{a.log2}, antientropy K = {K}, k = {FANOUT}, churn {FAIL} / {RECOVER}",
           "nodes": n, "edges": int(topo[1].size), "dense_rounds": a.dense_rounds, "max_rounds": a.max_rounds,
           "topo": measure(n, FLAG_AE_TOPO_PEERS, {}, topo, a.dense_rounds, a.max_rounds),
           "uniform_same_kernels": measure(n, FLAG_AE_DIRECT_SCAN, {"ae_dense_bin": 0}, None, a.dense_rounds,
                                           a.max_rounds)}
    tp, un = out["topo"], out["uniform_same_kernels"]
    out["dense_topo_over_uniform"] = tp["dense_us_per_round"] / un["dense_us_per_round"]
    a_, b_ = tp["run_roomy_cap"]["sparse"]["us_per_round"], un["run_roomy_cap"]["sparse"]["us_per_round"]
    out["sparse_topo_over_uniform"] = a_ / b_ if a_ and b_ else None
    out["wall_s"] = time.perf_counter() - t0
    with open(os.path.join(a.out, f"grid_2p{a.log2}.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
