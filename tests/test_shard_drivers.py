"""CPU only: the driver seam of tests/shard_cases.py against the references alone.  OrderedDevComm,
the comm that test_gpu_shard_devvalues.py runs HIP shards through, is rehearsed here over oracle host
shards (they have no *_dev calls, so it takes the host forms): the bodies must pass through it as they
do through the copy comm.  The rest pins what test_gpu_group_states.py reads a round's kind from (the
plan string's letters) and the preconditions that keep both GPU files from going vacuous."""
import numpy as np
import pytest

import oracle_py as op
import shard_cases as sc
from gossip_hip import sharded
from gossip_hip.sharded import REP, REP_CLASSCODED
from shard_cases import PHILOX, RUNS, SLOTS, SLOTS_CC
from test_shard_states import CAROUSEL, CAROUSEL_IDS, test_carousel_visits_every_kind_and_both_filter_states as visits

OFFSETS = (0, 3, 5)  # the fewest offsets that reach every kind (pinned below)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_through_the_ordered_comm(run, G, offset):
    made = []

    def driver(*args, **kw):
        made.append(sc.OrderedDevDriver(*args, **kw))
        return made[0]

    sc.body_carousel(op.OracleEngine, run, G, offset, driver=driver)
    (d,) = made
    # host shards: every value through the host forms, no stream bound, no flag set
    assert d.comm.called["round_compute"] and not any(name.endswith("_dev") for name in d.comm.called)
    assert not d.device_engines and not d.ordered


def test_wire_through_the_recording_ordered_comm():
    """RecordingOrderedComm logs what RecordingComm logs: every product equals the numpy references."""
    sc.body_carousel_wire(op.OracleEngine, PHILOX, sc.PHILOX_G, 0, driver=sc.OrderedDevDriver)


def test_default_driver_is_the_lockstep_driver():
    """driver=None and LockstepDriver are one path: equal kinds from the same body."""
    a = sc.body_carousel(op.OracleEngine, RUNS[1], 3, 0)
    b = sc.body_carousel(op.OracleEngine, RUNS[1], 3, 0, driver=sc.LockstepDriver)
    assert a == b


def test_plan_letters_name_the_kinds():
    """The plan string's letter of a round is "DSAXCRrQ"[kind] (csrc/engine.hip gossip_sharded_plan)."""
    assert sc.PLAN_LETTERS == sharded.KIND_LETTERS == "DSAXCRrQ"
    want = {"D": sharded.DENSE, "S": sharded.SPARSE, "A": sharded.ANTIENTROPY, "X": sharded.EXCHANGE,
            "C": sharded.CLASSCODED, "R": sharded.REP_GATHER, "r": sharded.REP, "Q": sharded.REP_CLASSCODED}
    assert {c: sc.PLAN_LETTERS.index(c) for c in sc.PLAN_LETTERS} == want
    assert sorted(want.values()) == list(range(8))


@pytest.mark.parametrize("run", RUNS + [PHILOX], ids=sc.run_id)
def test_three_offsets_reach_every_kind(run):
    """expected_kinds(SLOTS, o, rounds) over o in {0, 3, 5} covers ALL_KINDS (and both filter states):
    the precondition test of test_shard_states.py, whose offsets are the ones used here."""
    visits(run)
    want = sc.reference(run)[1]
    assert set().union(*(sc.expected_kinds(SLOTS, o, len(want)) for o in OFFSETS)) == sc.ALL_KINDS


@pytest.mark.parametrize("run", RUNS + [PHILOX], ids=sc.run_id)
def test_every_offset_has_the_rounds_a_dev_call_needs(run):
    """Over the three offsets every run has a sparse and an exchange round (the *_dev calls other than
    round_compute_dev), and every single offset a round that ends in round_compute."""
    want = sc.reference(run)[1]
    seen = set()
    for o in OFFSETS:
        kinds = set(sc.expected_kinds(SLOTS, o, len(want)))
        assert kinds - {sharded.SPARSE, sharded.EXCHANGE}
        seen |= kinds
    assert {sharded.SPARSE, sharded.EXCHANGE} <= seen


def test_slots_cc_enters_replication_class_coded():
    for rounds in (4, 11):
        assert sc.expected_kinds(SLOTS_CC, 0, rounds)[2:4] == [REP_CLASSCODED, REP]
    assert REP_CLASSCODED not in sc.expected_kinds(SLOTS, 0, 16)


def test_antientropy_write_case_converges_on_the_references():
    """test_gpu_group_states.py's ANTIENTROPY case on the references alone: no round of the first chunk
    converges, the run after the three writes does within 400 rounds (9, pinned there), and every write
    raises the global max vector, so the driver has to reduce the shards' targets again."""
    import test_gpu_group_states as tg
    for loss, (_, rounds) in tg.AE_RUNS.items():
        first, second = tg._ae_reference(loss)
        assert first[0].rounds == 4 and second[0].rounds == rounds == 9 and second[0].converged


@pytest.mark.parametrize("run", RUNS + [PHILOX], ids=sc.run_id)
def test_reference_infected_counts_the_bits_of_the_states(run):
    """The per-rumor counts the Group tests compare are the column sums of S_{t+1}."""
    states, _ = sc.reference(run)
    _, R = sc.run_shape(run)
    for S, inf in zip(states[1:], sc.reference_infected(run)):
        bits = (S[:, None] >> np.arange(R, dtype=np.uint64)[None, :]) & np.uint64(1)
        assert np.array_equal(bits.sum(axis=0, dtype=np.uint64), inf)
