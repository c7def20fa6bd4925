"""CPU: the sharded round planner (csrc/plan.h, through oracle_sharded_plan) picks the kind recorded in
tests/golden/plan_grid.json at every point of a grid of shapes, knob sets and global totals.  The
recording comes from the commit before the planner moved into the shared header
(tests/golden/make_plan_grid.py); tests/test_gpu_plan_grid.py holds the engine to the same grid."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, SEED, FLAGS = 2, 7, 1
NS = (65536, (1 << 22) + 4099)
GS = (2, 3, 8, 16)
KS = (2, 9)
MODES = ("push", "pull", "pushpull")
# every knob set starts from these; sparse_frac comes last: once set it stays set
DEFAULTS = (("xd_shards", 6), ("link_gbps", 76), ("replicate", -1), ("cc_frac", 0.75))
KNOBS = ((), (("xd_shards", 2),), (("link_gbps", 0),), (("replicate", 1),), (("replicate", 0),), (("cc_frac", 0),),
         (("sparse_frac", 0.1),))
TOTALS = ((1e-4, 0), (0.02, 0), (0.05, 0), (0.3, 0), (0.6, 0.1), (0.9, 0.5), (1, 0.8), (1, 0.97), (1, 0.9999),
          (0.5, 0.5), (0.99, 0),
          # ... and two with few holders per rumor under many mixed nodes: entering replication pays only over
          # the third and later rounds ahead (the first two are predicted class-coded), so a shorter look-ahead
          # plans kind 0 where 8 rounds plan kind 5
          (0.9, 0.1, (0.02, 0.001)), (1, 0.2, (0.01, 0.01)))
# (nonzero nodes / N, full nodes / N[, holders / N per rumor: else (nonzero + full) // 2 of every rumor])
SHAPES = [(N, G) for N in NS for G in GS]


def key(N, G, k, mode):
    return f"{N}-{G}-{k}-{mode}"


def totals(N, plen):
    for nz_frac, full_frac, *holders in TOTALS:
        nz, full = int(nz_frac * N), int(full_frac * N)
        tot = np.zeros(plen, dtype=np.uint64)
        tot[0], tot[1], tot[4 + R] = full, N, nz
        tot[4:4 + R] = [int(h * N) for h in holders[0]] if holders else (nz + full) // 2
        yield tot


def walk(e, N):
    """Plans two rounds at every (knob set, totals) point on engine e: the plan, a commit with no compute between
    (host bookkeeping only: how a plan reaches kind 6), the plan again.  Returns the kinds as a digit string, and
    from an engine with plan_model() the plan letters and [ms, link ms after the first plan, after the second]."""
    model = hasattr(e, "plan_model")
    kinds, letters, ms = [], [], []
    for knobs in KNOBS:
        for name, v in DEFAULTS + knobs:
            e.set_param(name, v)
        for tot in totals(N, e.partial_len()):
            if model:
                e.reset_timing()
            kinds.append(e.sharded_plan(tot))
            first = e.plan_model()[:2] if model else ()
            e.round_commit(tot)
            kinds.append(e.sharded_plan(tot))
            if model:
                second = e.plan_model()
                ms.append([*first, *second[:2]])
                letters.append(second[3])
            e.reset()
    assert all(0 <= k <= 7 for k in kinds)
    return "".join(map(str, kinds)), "".join(letters), ms


def shape_engines(make, N, G):
    """(key, engine) of every fanout and mode at one (N, G): rank 0 of G shards"""
    for k in KS:
        for mode in MODES:
            with make(N, R, mode, k, SEED, flags=FLAGS, shard_rank=0, shard_count=G) as e:
                yield key(N, G, k, mode), e


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "plan_grid.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("N,G", SHAPES, ids=[f"{N}-{G}" for N, G in SHAPES])
def test_oracle_plans_recorded_kinds(recorded, N, G):
    import oracle_py as op
    for name, e in shape_engines(op.OracleEngine, N, G):
        assert walk(e, N)[0] == recorded["oracle"][name], name
