"""Random gossip over a topology (GOSSIP_FLAG_TOPO_PEERS) at scale:
pushpull k = 2, one word per node (64 rumors at Philox origins), on
  random8  a random directed topology of 2^22 nodes with 8 out-neighbours each, and
  grid     the 2048 x 2048 grid (Maelstrom's default topology, 4-neighbourhood),
and beside each, at the same N and k, the uniform round of a GOSSIP_FLAG_DIRECT engine (the same
kernel shape without the row load) and the FLOOD round over the same rows (the reference's own
rule, main.go:65-89: every neighbour).  Each engine runs to convergence or `rounds` rounds, three
times (the first untimed); the figure is device time per round from engine timer 0.  Writes one
JSON file per topology into the output directory.  --pkg names another build's package directory to
measure that one instead; --build is a name for it, echoed in the JSON.
Usage: topo_probe.py [--out DIR] [--log2 22] [--rounds 256] [--pkg DIR [--build NAME]]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

gh = None  # the measured build's gossip_hip, imported by main() from --pkg

K, R, SEED = 2, 64, 0x5EED0007


def random_topology(n, d):
    rng = np.random.default_rng(7)
    col = rng.integers(0, n - 1, size=n * d, dtype=np.uint64).astype(np.uint32)
    own = np.repeat(np.arange(n, dtype=np.uint32), d)
    col = np.where(col >= own, col + 1, col).astype(np.uint32)  # no self loops
    return (np.arange(n + 1, dtype=np.uint64) * d).astype(np.uint32), col


def grid_topology(w):
    """Row-major w x w grid, 4-neighbourhood (gossip_hip.grid_topology's rows, as arrays)."""
    i = np.arange(w * w, dtype=np.int64)
    r, c = i // w, i % w
    cand = np.stack([i - w, i + w, i - 1, i + 1], axis=1)
    ok = np.stack([r > 0, r < w - 1, c > 0, c < w - 1], axis=1)
    row_ptr = np.zeros(w * w + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(ok.sum(axis=1))
    return row_ptr.astype(np.uint32), cand[ok].astype(np.uint32)


def measure(mode, flags, topo, n, rounds):
    """us per round (timer 0) of the last two of three runs, and what the last run did."""
    e = gh.Engine(n, R, mode, K, SEED, flags=flags | gh.FLAG_TIMING)
    if topo is not None:
        e.set_topology(topo)
    for rep in range(3):
        if rep == 1:
            e.reset_timing()
        e.reset()
        e.inject_random()
        res = e.step(rounds, with_infected=False)
    ms, launches = e.kernel_time(0)
    e.close()
    return {"us_per_round": ms * 1e3 / max(launches, 1), "rounds": res.rounds,
            "converged": bool(res.converged), "full_nodes": res.stats[-1]["full_nodes"],
            "messages": sum(s["messages"] for s in res.stats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo_peers"))
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=256)
    ap.add_argument("--build", default="this tree", help="a name for the measured build, echoed in the JSON")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "gossip-protocol_amd"))
    a = ap.parse_args()
    global gh
    sys.path.insert(0, a.pkg)
    import gossip_hip as gh
    os.makedirs(a.out, exist_ok=True)
    n = 1 << a.log2
    for name, build in (("random8", lambda: random_topology(n, 8)), ("grid", lambda: grid_topology(1 << (a.log2 // 2)))):
        t0 = time.perf_counter()
        topo = build()
        assert topo[0].size - 1 == n
        out = {"build": a.build, "workload": f"{name}, N = 2^{a.log2}, pushpull k = {K}, R = {R} (W = 1)", "nodes": n,
               "edges": int(topo[1].size), "fanout": K, "rumors": R, "max_rounds": a.rounds,
               "topo_peers": measure("pushpull", gh.FLAG_TOPO_PEERS, topo, n, a.rounds),
               "uniform_direct": measure("pushpull", gh.FLAG_DIRECT, None, n, a.rounds),
               "flood": measure("flood", 0, topo, n, a.rounds)}
        out["topo_over_uniform_direct"] = out["topo_peers"]["us_per_round"] / out["uniform_direct"]["us_per_round"]
        out["topo_over_flood"] = out["topo_peers"]["us_per_round"] / out["flood"]["us_per_round"]
        out["wall_s"] = time.perf_counter() - t0
        with open(os.path.join(a.out, f"{name}_2p{a.log2}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
