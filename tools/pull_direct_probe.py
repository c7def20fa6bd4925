"""The baseline column of DESIGN.md §3.13: a PULL engine with GOSSIP_FLAG_DIRECT and no mongering in
monger_probe.py's setup (2^log2 nodes, R = 64, k = 2, uniform peers, inject_random, GOSSIP_FLAG_TIMING),
one gossip_step per round to converged, timer 0 (seed copy + round kernel) + timer 1 (stats) read after
each.  One untimed run, then three timed ones.  Prints one JSON line: rounds, the range of every
round's device time over the timed runs (round_us), the slowest round and the whole run.
--mode pushpull: the same for a PUSHPULL engine, the baseline column of §3.14; --pkg names another
build's package directory to measure that one instead.
Usage: pull_direct_probe.py [--log2 24] [--mode pull|pushpull] [--pkg DIR [--build NAME]]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24)
ap.add_argument("--mode", default="pull", choices=["pull", "pushpull"])
ap.add_argument("--build", default="this tree", help="a name for the measured build, echoed in the JSON line")
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "gossip-protocol_amd"))
a = ap.parse_args()
sys.path.insert(0, a.pkg)
from gossip_hip import FLAG_DIRECT, FLAG_TIMING, Engine  # noqa: E402

N, R, K = 1 << a.log2, 64, 2
runs = []
with Engine(N, R, a.mode, K, 0x5EED0003, flags=FLAG_DIRECT | FLAG_TIMING) as e:
    for rep in range(4):
        e.reset()
        e.inject_random()
        per = []
        for _ in range(200):
            e.reset_timing()
            res = e.step(1)
            per.append((e.kernel_time(0)[0] * 1e3, e.kernel_time(1)[0] * 1e3, res.stats[0]["full_nodes"]))
            if res.stats[0]["converged"]:
                break
        if rep:
            runs.append(per)
last = runs[-1]
worst = max(range(len(last)), key=lambda i: last[i][0] + last[i][1])
print(json.dumps({
    "build": a.build, "engine": a.mode.upper() + ", GOSSIP_FLAG_DIRECT", "nodes": N, "rumors": R, "fanout": K, "rounds": len(last),
    "round_us": [[round(min(r[i][0] + r[i][1] for r in runs), 1), round(max(r[i][0] + r[i][1] for r in runs), 1)]
                 for i in range(len(last))],
    "slowest_round": worst,
    "whole_run_ms": [round(min(sum(p[0] + p[1] for p in r) for r in runs) / 1e3, 2),
                     round(max(sum(p[0] + p[1] for p in r) for r in runs) / 1e3, 2)]}), flush=True)
