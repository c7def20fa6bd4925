"""GPU: the library's own round driver (csrc/multi.hip: Driver::plan / dense / sparse / exchange /
antientropy / round and sharded_step, behind gossip_group_step) through the bodies of
tests/shard_cases.py.  The reference is the C oracle, one engine, never another HIP engine: an error
shared by the sharded and the one-engine HIP paths cannot cancel.  Against test_gpu_group.py this
adds hand-built states, a plan that changes the round's kind every round (sparse -> exchange, rep ->
sparse -> rep with the whole image dropped, kind 7 -> 6), the kind of every round asserted from the
plan string, per-rumor counts every round, and inject / set_faults / reset between library-driven
rounds while the image is whole.  A Group of G shards on one device runs over the copy transport;
the driver above it (the plan, the order of the collectives, the *_dev values, publish_kernel, no
publishing sync: e->driven) is the one an RCCL run uses."""
import functools

import numpy as np
import pytest

import ae_faults_ref as fr
import oracle_py as op
import shard_cases as sc
from gossip_hip import FLAG_SHARD_DIRECT, FLAG_TIMING
from gossip_hip.engine import Group, churn_threshold as ct, loss_threshold as lt
from gossip_hip.sharded import REP, REP_CLASSCODED, SPARSE
from shard_cases import OFFSETS, RUNS, SLOTS_CC, GroupDriver
from test_shard_states import BUILT, CAROUSEL, CAROUSEL_IDS, FORCED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_equals_oracle(run, G, offset):
    sc.body_carousel(None, run, G, offset, driver=GroupDriver)


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("run", [RUNS[0], RUNS[2]], ids=sc.run_id)  # one run per mode: push, pushpull (with faults)
def test_carousel_direct_kernels_equal_oracle(run, offset):
    """FLAG_SHARD_DIRECT: dense sharded rounds on the direct kernels instead of the binned passes."""
    sc.body_carousel(None, run, 3, offset, flags=FLAG_SHARD_DIRECT, driver=GroupDriver)


@pytest.mark.parametrize("run", [RUNS[0], RUNS[4]], ids=sc.run_id)
def test_carousel_enters_replication_class_coded(run):
    kinds = sc.body_carousel(None, run, 4, 0, SLOTS_CC, driver=GroupDriver)
    assert kinds[2:4] == [REP_CLASSCODED, REP]


@pytest.mark.parametrize("kind", list(FORCED), ids=lambda k: f"kind{k}")
@pytest.mark.parametrize("run", BUILT, ids=sc.run_id)
def test_built_state_under_one_forced_kind(run, kind):
    """The first library-driven round of each kind on a class mix that gossip from Philox origins never
    produces: two shards wholly empty and a class-coded stride of 0 (clustered), the rare list at its
    capacity (disjoint), not-full as the rare class from round 0 (holes)."""
    sc.body_forced_kind(None, run, FORCED[kind], kind, driver=GroupDriver)


def test_forced_replicated_inject_faults_reset():
    """An inject and a reset drop the whole image (kind 5 again), set_faults keeps it; stats and
    per-rumor counts equal the oracle's after every round; after reset every shard is all zero."""
    sc.body_replicated_sequence(None, sc.REP_PARAMS, want_kinds=sc.REP_KINDS, driver=GroupDriver)


def test_auto_plan_inject_faults_reset():
    """The same sequence with no knob set: Driver::plan sums the shards' own totals (kind -1) after the
    build, after the injects and after the reset."""
    sc.body_replicated_sequence(None, None, driver=GroupDriver)


@pytest.mark.parametrize("case", range(len(sc.MULTIWORD)), ids=sc.MULTIWORD_IDS)
def test_multiword_shards_equal_oracle(case):
    """W > 1 at G > 1: push, ragged Nl, an empty last shard (N = 12, G = 5), faults with the stall
    mode; the shards are read after every round."""
    owned = sc.body_multiword(None, case, driver=GroupDriver)
    if case == 0:
        assert owned == [3, 3, 3, 3, 0]


def test_carousel_with_timing():
    """FLAG_TIMING: pub_ready syncs and collects the timers, engine_wall_end waits on its event.  The
    bits are the untimed run's (the body's own asserts), and every shard counted each round once in
    its class: sparse rounds in round_wall(1), all others in round_wall(0)."""
    made = []

    class Kept(GroupDriver):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            made.append(self)

        def close(self):  # the counters are read below
            pass

    try:
        kinds = sc.body_carousel(None, RUNS[2], 4, 0, flags=FLAG_TIMING, driver=Kept)
        sparse = kinds.count(SPARSE)
        assert 0 < sparse < len(kinds)
        for e in made[0].engines:
            assert e.round_wall(1)[1] == sparse and e.round_wall(0)[1] == len(kinds) - sparse
            assert e.round_wall(2)[1] == 0
            assert e.kernel_time(0)[1] > 0
    finally:
        for d in made:
            GroupDriver.close(d)


# -- ANTIENTROPY with client writes between library-driven rounds -----------------------------------
# 12289 nodes over 3 shards of 4160, 4160 and 3969 (ANTIENTROPY shards are whole 64-node words of the
# alive / stale image); churn 0.01 / 0.1; inject_random, 4 rounds, one write
# in each shard, then to convergence.  After the writes Driver::plan finds the global max vector
# stale (kind -2) and all-reduces the shards' targets (MAX) before it can plan.
AE_N, AE_K, AE_FANOUT, AE_G, AE_SEED = 12289, 5, 2, 3, 0x5EED0031
# (node, component), one in each shard; each node holds its component's global max after round 3 (in
# both references below), so its write raises the max vector
AE_WRITES = ((5, 1), (4214, 2), (AE_N - 2, 3))
AE_KW = dict(flags=1, churn_fail=ct(0.01), churn_recover=ct(0.1))
# edge_loss -> (the reference, rounds to convergence after the writes).  The C oracle has no ANTIENTROPY
# under faults (oracle_create answers ENOTSUP), so the run with edge_loss 0.1 is held to the numpy
# restatement that test_ae_faults_ref.py holds to the C oracle; without loss the C oracle itself is
# the reference.  The round counts were taken from the references alone, on the CPU.
AE_RUNS = {0: (op.OracleEngine, 9), lt(0.1): (fr.RefEngine, 9)}


@functools.lru_cache(maxsize=None)
def _ae_reference(loss):
    factory, rounds = AE_RUNS[loss]
    ref = factory(AE_N, AE_K, "antientropy", AE_FANOUT, AE_SEED, edge_loss=loss, **AE_KW)
    ref.inject_random()
    chunks = [(ref.step(4), ref.read_rows().copy())]
    for node, comp in AE_WRITES:
        ref.inject(node, comp)
    chunks.append((ref.step(400), ref.read_rows().copy()))
    assert not any(s["converged"] for s in chunks[0][0].stats)
    assert chunks[1][0].converged and chunks[1][0].rounds == rounds
    # every write raised the global max of its component, each from another shard: the all-reduce MAX
    # of Driver::plan needs every shard's vector
    before, after = chunks[0][1].max(axis=0), chunks[1][1].max(axis=0)
    assert all(after[comp] > before[comp] for _, comp in AE_WRITES)
    return chunks


@pytest.mark.parametrize("loss", list(AE_RUNS), ids=["no_loss-oracle", "loss0.1-restatement"])
def test_antientropy_writes_between_group_rounds(loss):
    want = _ae_reference(loss)
    with Group(AE_N, AE_K, "antientropy", AE_FANOUT, AE_SEED, n_shards=AE_G, devices=[0] * AE_G, transport=2,
               edge_loss=loss, **AE_KW) as g:
        assert [e.hi - e.lo for e in g.shards] == [4160, 4160, 3969]
        assert [sum(e.lo <= n < e.hi for n, _ in AE_WRITES) for e in g.shards] == [1, 1, 1]
        g.inject_random()
        for i, (res, rows) in enumerate(want):
            if i == 1:
                for node, comp in AE_WRITES:
                    g.inject(node, comp)  # (on every shard: its owner takes it)
            got = g.step(4 if i == 0 else 400)
            assert got.stats == res.stats, i
            assert np.array_equal(got.infected, res.infected), i
            for e in g.shards:
                assert np.array_equal(e.read_rows(), rows[e.lo:e.hi]), (i, e.cfg.shard_rank)
