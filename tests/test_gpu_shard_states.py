"""GPU: the bodies of test_shard_states.py with HIP Engine shards on one device (device copies stand in
for the RCCL collectives).  The reference is the C oracle, one engine, never another HIP engine: an
error shared by the sharded and the one-engine HIP paths cannot cancel.  Hand-built states
(tests/states.py), the 8-slot plan carousel that changes the round's kind every round, inject /
set_faults / reset while the image is whole, and multi-word shards (tests/shard_cases.py)."""
import pytest

import shard_cases as sc
from gossip_hip import FLAG_SHARD_DIRECT, Engine
from gossip_hip.sharded import REP, REP_CLASSCODED, lockstep_run
from shard_cases import OFFSETS, RUNS, SLOTS_CC
from test_shard_states import BUILT, CAROUSEL, CAROUSEL_IDS, FORCED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_equals_oracle(run, G, offset):
    sc.body_carousel(Engine, run, G, offset)


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("run", [RUNS[0], RUNS[2]], ids=sc.run_id)  # one run per mode: push, pushpull (with faults)
def test_carousel_direct_kernels_equal_oracle(run, offset):
    """FLAG_SHARD_DIRECT: dense sharded rounds on the direct kernels instead of the binned passes."""
    sc.body_carousel(Engine, run, 3, offset, flags=FLAG_SHARD_DIRECT)


@pytest.mark.parametrize("run", [RUNS[0], RUNS[4]], ids=sc.run_id)
def test_carousel_enters_replication_class_coded(run):
    kinds = sc.body_carousel(Engine, run, 4, 0, SLOTS_CC)
    assert kinds[2:4] == [REP_CLASSCODED, REP]


def test_replicate_with_cc_frac_1_is_7_6_6():
    states, want = sc.reference(RUNS[1])
    engines = sc.make_engines(Engine, RUNS[1], 4, params={"sparse_frac": -1, "replicate": 1, "cc_frac": 1})
    try:
        stats, kinds = lockstep_run(engines, 3)
        assert kinds == [REP_CLASSCODED, REP, REP] and stats == list(want[:3])
        sc.assert_shards_hold(engines, states[3])
    finally:
        sc.close_all(engines)


def test_forced_replicated_inject_faults_reset():
    """An inject and a reset drop the whole image (kind 5 again), set_faults keeps it; stats equal the
    oracle's after every chunk; after reset every shard is all zero with hash 0."""
    sc.body_replicated_sequence(Engine, sc.REP_PARAMS, want_kinds=sc.REP_KINDS)


def test_auto_plan_inject_faults_reset():
    """The same sequence with no knob set: whatever the engine plans, the rounds are the oracle's."""
    sc.body_replicated_sequence(Engine, None)


@pytest.mark.parametrize("kind", list(FORCED), ids=lambda k: f"kind{k}")
@pytest.mark.parametrize("run", BUILT, ids=sc.run_id)
def test_built_state_under_one_forced_kind(run, kind):
    """The first round of each kind sees a class mix that gossip from Philox origins never produces."""
    sc.body_forced_kind(Engine, run, FORCED[kind], kind)


@pytest.mark.parametrize("case", range(len(sc.MULTIWORD)), ids=sc.MULTIWORD_IDS)
def test_multiword_shards_equal_oracle(case):
    """W > 1 at G > 1: push, ragged Nl, an empty last shard, faults with the stall mode."""
    sc.body_multiword(Engine, case)

