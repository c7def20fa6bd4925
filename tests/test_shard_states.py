"""CPU only: oracle host shards through the sharded round bodies (gossip_hip.sharded._round) against
one oracle engine, on the hand-built states and the plan carousel of tests/shard_cases.py, and the
numpy references of the wire products against what the oracle shards put on the wire.  This is the
check that the references alone satisfy every condition the GPU files (test_gpu_shard_states.py,
test_gpu_shard_wire.py) then hold the HIP engine to through the same bodies, and it pins the
preconditions that keep those tests from going vacuous."""
import pytest

import oracle_py as op
import shard_cases as sc
from gossip_hip.sharded import CLASSCODED, DENSE, EXCHANGE, REP, REP_CLASSCODED, REP_GATHER, SPARSE, lockstep_run
from shard_cases import GS, OFFSETS, PHILOX, PHILOX_G, RUNS, SLOTS, SLOTS_CC
from states import N0, SEED

CAROUSEL = [(run, G) for run in RUNS for G in GS] + [(PHILOX, PHILOX_G)]
CAROUSEL_IDS = [f"{sc.run_id(run)}-G{G}" for run, G in CAROUSEL]
# one run per builder, and the plan knobs that force the first round's kind
BUILT = [RUNS[0], RUNS[2], RUNS[3], RUNS[4]]
FORCED = {SPARSE: SLOTS[0][1], DENSE: SLOTS[1][1], CLASSCODED: SLOTS[5][1], EXCHANGE: SLOTS[4][1],
          REP_GATHER: SLOTS[2][1]}


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_equals_one_engine(run, G, offset):
    """Every round another kind, every knob set each round."""
    sc.body_carousel(op.OracleEngine, run, G, offset)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_wire_equals_numpy(run, G, offset):
    """Rare lists, sparse messages, class bitmaps, exchange items and replies, class-coded slots and
    mixed words, state slices: each is what the numpy restatement derives from S_t alone."""
    sc.body_carousel_wire(op.OracleEngine, run, G, offset)


@pytest.mark.parametrize("run", [RUNS[0], RUNS[4]], ids=sc.run_id)
def test_carousel_enters_replication_class_coded(run):
    """The table whose first rep slot has cc_frac = 1: that round is kind 7, the next kind 6."""
    kinds = sc.body_carousel(op.OracleEngine, run, 4, 0, SLOTS_CC)
    assert kinds[2:4] == [REP_CLASSCODED, REP]


def test_replicate_with_cc_frac_1_is_7_6_6():
    states, want = sc.reference(RUNS[1])
    engines = sc.make_engines(op.OracleEngine, RUNS[1], 4, params={"sparse_frac": -1, "replicate": 1, "cc_frac": 1})
    stats, kinds = lockstep_run(engines, 3)
    assert kinds == [REP_CLASSCODED, REP, REP] and stats == list(want[:3])
    sc.assert_shards_hold(engines, states[3])


def test_forced_replicated_inject_faults_reset():
    """An inject and a reset drop the whole image (the next round gathers it again: kind 5);
    set_faults keeps it."""
    sc.body_replicated_sequence(op.OracleEngine, sc.REP_PARAMS, want_kinds=sc.REP_KINDS)


@pytest.mark.parametrize("kind", list(FORCED), ids=lambda k: f"kind{k}")
@pytest.mark.parametrize("run", BUILT, ids=sc.run_id)
def test_built_state_under_one_forced_kind(run, kind):
    sc.body_forced_kind(op.OracleEngine, run, FORCED[kind], kind)


@pytest.mark.parametrize("case", range(len(sc.MULTIWORD)), ids=sc.MULTIWORD_IDS)
def test_multiword_shards_equal_one_engine(case):
    """W > 1 sharded: push, ragged Nl, an empty last shard (N = 12 at G = 5: 3, 3, 3, 3, 0), faults
    with the stall mode (12 rounds: that run never converges)."""
    owned = sc.body_multiword(op.OracleEngine, case)
    if case == 0:
        assert owned == [3, 3, 3, 3, 0]


# -- preconditions, so that a later change cannot make a GPU test vacuous -----------------------

# builder -> mixed nodes per shard at G = 4 (shards of 4113, 4113, 4113 and 4110 nodes) in round 0
CC_COUNTS_G4 = {"clustered": [0, 0, 0, 0], "thirds": [1371, 1371, 1371, 1370], "holes": [43, 42, 43, 42],
                "disjoint": [4113, 4113, 4113, 4110]}


@pytest.mark.parametrize("name", list(CC_COUNTS_G4))
def test_round0_class_mixes_at_G4(name):
    run = next(r for r in RUNS if r[0] == name)
    engines = sc.make_engines(op.OracleEngine, run, 4, params=dict(SLOTS[5][1]))
    assert [e.hi - e.lo for e in engines] == [4113, 4113, 4113, 4110]
    comm = sc.RecordingComm(engines)
    kinds = []
    sc.drive_round(engines, comm, kinds)
    assert kinds == [CLASSCODED]
    assert sc.wire(CLASSCODED, comm.take())["cc_counts"] == CC_COUNTS_G4[name]
    S0 = sc.reference(run)[0][0]
    if name == "clustered":  # no mixed node anywhere (the class-coded stride is 0), two shards wholly empty
        assert sum(not S0[e.lo:e.hi].any() for e in engines) == 2
    if name == "disjoint":  # every node mixed: the rare list fills rare_send to its capacity Nl
        rare = sc.ref_wire(SPARSE, S0, N0, 4, 64, "pushpull", 2, SEED, 0)["rare_counts"]
        assert rare == [4113, 4113, 4113, 4110]
        assert sc.dense_filter(S0, N0, 64, "pushpull", 2, 0.0) == 0  # nothing for the exchange filter to drop
    if name == "holes":  # not-full is the rare class from round 0 on
        assert sc.rare_is_not_full(S0, N0, 3)


# run -> the filter words (bit 0: pulls from empty peers dropped, bit 1: pushes into full ones) of its
# "exchange" slot rounds at offsets {0, 3, 5}; 0 = xd_classes returns bytes == 0.  Every run has a round
# with bytes > 0 and one with 0: the exchange_unfiltered slot (xd_filter_frac 1) never filters.
FILTER_WORDS = {RUNS[0]: {0, 2}, RUNS[1]: {0, 2}, RUNS[2]: {0, 2}, RUNS[3]: {2}, RUNS[4]: {0, 2}, PHILOX: {0, 1, 2}}


@pytest.mark.parametrize("run", RUNS + [PHILOX], ids=sc.run_id)
def test_carousel_visits_every_kind_and_both_filter_states(run):
    """Over the offsets {0, 3, 5}, the fewest a GPU file uses, every run visits each of the kinds
    0, 1, 3, 4, 5, 6 and has exchange rounds with and without the class all-gather."""
    states, want = sc.reference(run)
    _, mode, k, _, _ = run
    N, R = sc.run_shape(run)
    seen, words, unfiltered = set(), set(), set()
    for offset in (0, 3, 5):
        kinds = sc.expected_kinds(SLOTS, offset, len(want))
        seen |= set(kinds)
        for i, kind in enumerate(kinds):
            if kind == EXCHANGE:
                name, knobs = SLOTS[(offset + i) % 8]
                f = sc.dense_filter(states[i], N, R, mode, k, knobs["xd_filter_frac"])
                (words if name == "exchange" else unfiltered).add(f)
    assert seen == sc.ALL_KINDS
    assert words == FILTER_WORDS[run] and unfiltered == {0} and words - {0}
