"""ANTIENTROPY dense rounds under faults at scale: 2^22 nodes x 16
components, k = 1, churn 1 % / 10 %, every round dense (param ae_sparse 0), for
  none        no faults (the kernels without fault code),
  partitions  partitions = 2 (a range check per exchange), and
  loss        edge_loss = 0.3 (one more Philox block per node and round).
Each engine runs `rounds` rounds (or to convergence) three times, the first untimed; the figure is
device time per dense round from engine timer 0.  Under the standing partition the run does not
converge and every round stays dense whatever the plan: every node outside the block that holds
the maximum stays stale.  Writes one JSON file into the output directory.
Usage: ae_faults_probe.py [--out DIR] [--log2 22] [--rounds 24]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gossip-protocol_amd"))
from gossip_hip import FLAG_TIMING, Engine, loss_threshold  # noqa: E402

K, FANOUT, SEED = 16, 1, 0x5EED0005


def measure(n, rounds, **faults):
    """us per dense round (timer 0) of the last two of three runs, and what the last run did."""
    e = Engine(n, K, "antientropy", FANOUT, SEED, flags=FLAG_TIMING, params={"ae_sparse": 0},
               churn_fail=loss_threshold(0.01), churn_recover=loss_threshold(0.1), **faults)
    for rep in range(3):
        if rep == 1:
            e.reset_timing()
        e.reset()
        e.inject_random()
        res = e.step(rounds, with_infected=False)
    ms, launches = e.kernel_time(0)
    e.close()
    return {"us_per_dense_round": ms * 1e3 / max(launches, 1), "dense_rounds_timed": launches, "rounds": res.rounds,
            "converged": bool(res.converged), "full_nodes": res.stats[-1]["full_nodes"],
            "alive_nodes": res.stats[-1]["alive_nodes"], "messages_round0": res.stats[0]["messages"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_faults"))
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=24)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n = 1 << a.log2
    t0 = time.perf_counter()
    out = {"workload": f"antientropy K = {K}, k = {FANOUT}, churn 1 % / 10 %, N = 2^{a.log2}, dense rounds only",
           "nodes": n, "max_rounds": a.rounds,
           "none": measure(n, a.rounds),
           "partitions": measure(n, a.rounds, partitions=2),
           "loss": measure(n, a.rounds, edge_loss=loss_threshold(0.3))}
    for name in ("partitions", "loss"):
        out[f"{name}_over_none"] = out[name]["us_per_dense_round"] / out["none"]["us_per_dense_round"]
    out["wall_s"] = time.perf_counter() - t0
    with open(os.path.join(a.out, f"dense_2p{a.log2}.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
