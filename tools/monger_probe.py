"""Rumor mongering at scale: one engine of 2^log2 nodes, R = 64, k = 2,
uniform peers, inject_random, run to quiescence one round per gossip_step with GOSSIP_FLAG_TIMING;
after each round timer 0 (the seed copies and the round kernel) and timer 1 (the stats pass) are
read.  One untimed run, then `runs` timed ones.  Prints one JSON line: rounds, the residue per
rumor, messages per node, and the device time of the peak round (the one with the most messages),
of the early rounds, of the tail and of the whole run, each as the range over the timed runs.
--limit 0 never calls set_monger_limit (the coin engine of §2.13; the only form a library without
the call can run); --planes sets the limit to 2 and back to 1 first, so that the same run goes
through the counter kernel (§2.14 item 9); --pkg names another build's package directory to
measure that one instead.  --pull runs a PULL engine with GOSSIP_FLAG_MONGER_PULL (§2.15, §3.13): timer 0
is then the request and the close pass, a run ends with the first round that leaves no node hot, and
the messages are the replies that carried a rumor.  --pushpull runs a PUSHPULL engine with
GOSSIP_FLAG_MONGER_PUSHPULL (§2.16, §3.14): the same timers and stop rule, and the messages are the exchanges
in which an end was hot.  --conn-limit C [--hunt H] sets gossip_set_monger_connections (§2.17, §3.15): timer 0
then also covers the arbitration, and the line carries the attempts, accepted and refused edges and hunts per node.
Usage: monger_probe.py [--log2 24] [--cool 0.5|always] [--limit 0] [--planes] [--blind] [--pull | --pushpull] [--runs 3]
                       [--conn-limit 0 [--hunt 0]] [--pkg DIR [--build NAME]]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24)
ap.add_argument("--cool", default="0.5")
ap.add_argument("--limit", type=int, default=0)
ap.add_argument("--blind", action="store_true")
ap.add_argument("--planes", action="store_true")
ap.add_argument("--pull", action="store_true")
ap.add_argument("--pushpull", action="store_true")
ap.add_argument("--conn-limit", type=int, default=0)
ap.add_argument("--hunt", type=int, default=0)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
ap.add_argument("--build", default="this tree", help="a name for the measured build, echoed in the JSON line")
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "gossip-protocol_amd"))
a = ap.parse_args()
sys.path.insert(0, a.pkg)
from gossip_hip import FLAG_MONGER, FLAG_TIMING, Engine  # noqa: E402

if a.pull:
    from gossip_hip import FLAG_MONGER_PULL  # noqa: E402  (not in a build from before the flag)
if a.pushpull:
    from gossip_hip import FLAG_MONGER_PUSHPULL  # noqa: E402  (likewise)
assert not (a.pull and a.pushpull)
by_hot = a.pull or a.pushpull   # the run ends when no node is hot

N, R, K, CAP = 1 << a.log2, 64, 2, 1024
cool = 2 ** 32 - 1 if a.cool == "always" else float(a.cool)


def rng(xs):
    return [round(min(xs), 1), round(max(xs), 1)]


runs = []
with Engine(N, R, "pushpull" if a.pushpull else "pull" if a.pull else "push", K, a.seed,
            flags=(FLAG_MONGER_PUSHPULL if a.pushpull else FLAG_MONGER_PULL if a.pull else FLAG_MONGER) | FLAG_TIMING) as e:
    e.set_monger(cool, a.blind)
    if a.planes:
        e.set_monger_limit(2)
        e.set_monger_limit(1)
    if a.limit:
        e.set_monger_limit(a.limit)
    if a.conn_limit:   # (never called without one: a build from before the call runs the rest)
        e.set_monger_connections(a.conn_limit, a.hunt)
    for rep in range(a.runs + 1):
        e.reset()
        e.inject_random()
        per_round = []
        conn = dict(attempts=0, accepted=0, refused=0, hunts=0)
        for _ in range(CAP):
            e.reset_timing()
            res = e.step(1)
            t0, t1 = e.kernel_time(0)[0] * 1e3, e.kernel_time(1)[0] * 1e3
            per_round.append((res.stats[0]["messages"], t0, t1, res.stats[0]["full_nodes"], res.infected[0]))
            if a.conn_limit:
                for key, v in e.connections().items():
                    conn[key] += v
            if (e.hot_nodes() if by_hot else res.stats[0]["messages"]) == 0:
                break
        if rep:
            runs.append(per_round)

last = runs[-1]
assert all([p[0] for p in r] == [p[0] for p in last] for r in runs) and len(last) < CAP
peak = max(range(len(last)), key=lambda i: last[i][0])
early = [i for i, p in enumerate(last[:peak]) if p[0] <= 4096]
tail = [i for i, p in enumerate(last) if i > peak and p[0] <= 4096]
miss = [N - int(x) for x in last[-1][4]]


def us(idx, col):
    """The range, over the timed runs and the rounds idx, of a round's time in the timers col."""
    return rng([sum(r[i][c] for c in col) for r in runs for i in idx] or [0])


print(json.dumps({
    "build": a.build, "conn_limit": a.conn_limit, "hunt": a.hunt, "conn_per_node": {k: v / N for k, v in conn.items()},
    "pull": a.pull, "pushpull": a.pushpull, "nodes": N, "rumors": R, "fanout": K, "cool": a.cool, "blind": a.blind, "limit": a.limit, "planes": a.planes,
    "rounds": len(last), "residue_nodes": [min(miss), max(miss)], "residue_share": [min(miss) / N, max(miss) / N],
    "full_nodes": last[-1][3], "messages_per_node": sum(p[0] for p in last) / N,
    "peak_round": peak, "peak_messages": last[peak][0],
    "peak_us": us([peak], (1, 2)), "peak_timer0_us": us([peak], (1,)), "peak_timer1_us": us([peak], (2,)),
    "early_rounds": len(early), "early_us": us(early, (1, 2)), "tail_rounds": len(tail), "tail_us": us(tail, (1, 2)),
    "whole_run_ms": [round(x / 1e3, 2) for x in rng([sum(p[1] + p[2] for p in r) for r in runs])],
}), flush=True)
