"""Generates tests/golden/shard_trace.json: per rank, [plan kind, link bytes] of every round of
gossip_hip.sharded.sharded_run at world 3 over gloo on oracle shards, for the runs of
tests/test_shard_trace.py.  TEST INFRASTRUCTURE: the recording pins the per-rank driver to what it
did before a change, so it is taken from a checkout of the parent commit, never from the tree under
test:

    git worktree add /tmp/parent HEAD~ && make -C /tmp/parent/oracle
    python tests/golden/make_shard_trace.py /tmp/parent
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_shard_trace as ts  # noqa: E402  (the runs and their worker; the code they drive comes from argv[1])

if __name__ == "__main__":
    tree = os.path.abspath(sys.argv[1])
    assert os.path.samefile(tree, ts.ROOT) is False, "record from a checkout of the parent commit"
    out = {ts.run_id(plan, direct): ts.record(tree, plan, direct) for plan, direct in ts.RUNS}
    with open(os.path.join(HERE, "shard_trace.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print({k: [len(r) for r in v] for k, v in out.items()})
