"""Rumor mongering's residue against its traffic, the three
tables of Demers et al., "Epidemic algorithms for replicated database maintenance", a fourth for push-pull
and a fifth under a connection limit, on the GPU engine: one rumor injected at node 0 of N nodes, uniform peers, one run to quiescence per row.

  feedback + counter   cool = 2^32 - 1 (a coin that fails with probability 2^-32), limit = m:
                       a sender loses interest after m pushes to peers that knew the rumor
  blind + coin         cool = 1 / m, the limit left at 1: a sender loses interest with
                       probability 1 / m after every push
  pull, feedback +     GOSSIP_FLAG_MONGER_PULL, cool = 2^32 - 1, limit = m: a node that answers pulls
  counter              loses interest after m rounds in which a pull did not need the rumor and no pull
                       did; the messages are the replies that carried the rumor
  push-pull, feedback  GOSSIP_FLAG_MONGER_PUSHPULL, cool = 2^32 - 1, limit = m: both ends of an exchange
  + counter            send the rumor while hot, and each loses interest after m rounds in which a
                       partner held the rumor and none lacked it; the messages are the exchanges in
                       which an end was hot
  connection limit     the three feedback + counter rows at limit = m = 2 when a node accepts one
                       connection per round (gossip_set_monger_connections, c = 1) and a refused
                       initiator hunts for h = 0, 1 or 15 further peers, beside the unlimited engine;
                       push counts every attempt as a message

Per m it prints the residue (the share of nodes that never heard the rumor), the messages per node
and the rounds to quiescence (the quiescent round included).  The paper's figures (N = 1000, its own
timing model) are for orientation only.  A report, not a test.
Usage: monger_table.py [--log2 20] [--fanout 1] [--seed S] [--max-m 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gossip-protocol_amd"))
from gossip_hip import FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER_PUSHPULL, Engine  # noqa: E402

ALWAYS = 2 ** 32 - 1
CAP = 4096


KINDS = {"push": FLAG_MONGER, "pull": FLAG_MONGER_PULL, "pushpull": FLAG_MONGER_PUSHPULL}


def row(n, k, seed, cool, blind, limit, mode="push", conn=None):
    with Engine(n, 1, mode, k, seed, flags=KINDS[mode]) as e:
        e.set_monger(cool, blind)
        if limit > 1:
            e.set_monger_limit(limit)
        if conn:
            e.set_monger_connections(*conn)
        e.inject(0, 0)
        res = e.step(CAP)
        quiet = e.hot_nodes() == 0 if mode != "push" else res.stats[-1]["messages"] == 0
    assert quiet, "not quiescent after %d rounds" % CAP
    heard = int(res.infected[-1][0])
    return (n - heard) / n, sum(s["messages"] for s in res.stats) / n, res.rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--fanout", type=int, default=1)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
    ap.add_argument("--max-m", type=int, default=5)
    a = ap.parse_args()
    n = 1 << a.log2
    print(f"N = 2^{a.log2}, k = {a.fanout}, one rumor at node 0, seed {a.seed:#x}")
    for title, args in (("feedback, counter (cool = 2^32 - 1, limit = m)", lambda m: (ALWAYS, False, m)),
                        ("blind, coin (cool = 1 / m, limit = 1)", lambda m: (1.0 / m, True, 1)),
                        ("pull, feedback, counter (cool = 2^32 - 1, limit = m)", lambda m: (ALWAYS, False, m, "pull")),
                        ("push-pull, feedback, counter (cool = 2^32 - 1, limit = m)",
                         lambda m: (ALWAYS, False, m, "pushpull"))):
        print(f"\n{title}\n| m | residue | messages per node | rounds |\n|---|---|---|---|")
        for m in range(1, a.max_m + 1):
            s, msgs, rounds = row(n, a.fanout, a.seed, *args(m))
            print(f"| {m} | {s:.5f} | {msgs:.3f} | {rounds} |", flush=True)
    print("\nconnection limit c = 1 (feedback, counter, cool = 2^32 - 1, limit = 2)\n"
          "| mode | hunts | residue | messages per node | rounds |\n|---|---|---|---|---|")
    for mode in KINDS:
        for conn in (None, (1, 0), (1, 1), (1, 15)):
            s, msgs, rounds = row(n, a.fanout, a.seed, ALWAYS, False, 2, mode, conn)
            print(f"| {mode} | {'unlimited' if conn is None else conn[1]} | {s:.5f} | {msgs:.3f} | {rounds} |", flush=True)


if __name__ == "__main__":
    main()
