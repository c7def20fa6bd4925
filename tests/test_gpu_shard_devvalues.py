"""GPU: the device-value calls (gossip_round_compute_dev, gossip_sparse_rare_dev, gossip_sparse_scan_dev,
gossip_sparse_commit_dev, gossip_xd_requests_dev, gossip_xd_finish_dev) the way the RCCL transport and
torch-RCCL run them: ordered_collectives = 1, every engine bound to the collectives' stream, and no
stream sync between an engine call and the collective that consumes its buffer or value.  HIP Engine
shards on one device go through the product's round bodies (sharded._round) over OrderedDevComm
(tests/shard_cases.py): every copy a torch op on that stream, counts and partials combined on the
device from publish_kernel's slots and read with one .cpu().  The reference is the C oracle and the
numpy wire references, never another HIP engine.

This shows the engine's calls correct when the host orders its collectives on the engine's stream;
that RCCL does so needs two devices and stays unverified."""
import pytest

import shard_cases as sc
from gossip_hip import Engine
from gossip_hip.sharded import EXCHANGE, SPARSE, _CopyComm
from shard_cases import PHILOX, PHILOX_G, RUNS, SLOTS, OrderedDevDriver
from test_shard_states import CAROUSEL, CAROUSEL_IDS

pytestmark = pytest.mark.gpu

OFFSETS = (0, 3, 5)  # test_shard_drivers.py: they reach every kind, sparse and exchange rounds included
DEV_STEMS = ("sparse_rare", "sparse_scan", "sparse_commit", "xd_requests", "xd_finish")


class _Kept(OrderedDevDriver):
    """close() releases the engines (no flag, the null stream) and leaves them open for the test."""

    def close(self):
        self.release()


@pytest.mark.parametrize("run,G", CAROUSEL, ids=CAROUSEL_IDS)
def test_carousel_equals_oracle(run, G):
    states, want = sc.reference(run)
    called = set()
    for offset in OFFSETS:
        made = []

        def driver(*args, **kw):
            made.append(_Kept(*args, **kw))
            return made[0]

        try:
            sc.body_carousel(Engine, run, G, offset, driver=driver)
            (d,) = made
            # no silent fallback: the partials of every dense round came from the published values,
            # and no count or partial of a sparse or exchange round through a host form
            assert d.comm.called["round_compute_dev"] >= 1
            assert not any(d.comm.called[stem] for stem in DEV_STEMS + ("round_compute",))
            called |= {name for name, n in d.comm.called.items() if n}
            # released: the flag did not outlive the rounds, every engine is back on the null stream,
            # and a host driver with its own syncs takes them over (the state is full: it stays)
            assert len(d.device_engines) == G
            assert d.ordered == {r: 0 for r in range(G)} and all(e._stream == 0 for e in d.engines)
            stats = sc.drive_round(d.engines, _CopyComm(d.engines))
            assert stats["converged"] and stats["round"] == len(want)
            sc.assert_shards_hold(d.engines, states[-1])
        finally:
            for d in made:
                sc.close_all(d.engines)
    assert {stem + "_dev" for stem in DEV_STEMS} <= called


@pytest.mark.parametrize("run,G", [(PHILOX, PHILOX_G), (RUNS[4], 4)], ids=["philox-G5", "disjoint-G4"])
def test_wire_products_equal_numpy(run, G):
    """Rare lists, sparse messages, exchange items and replies, class-coded slots: what the rounds put
    on the wire with their counts taken through the device values, against ref_wire."""
    sc.body_carousel_wire(Engine, run, G, 0, driver=OrderedDevDriver)


@pytest.mark.parametrize("kind", [SPARSE, EXCHANGE], ids=lambda k: f"kind{k}")
@pytest.mark.parametrize("run", [RUNS[3], RUNS[4]], ids=sc.run_id)
def test_built_state_under_one_forced_kind(run, kind):
    """holes: not-full is the rare class from round 0; disjoint: the rare list at its capacity."""
    knobs = {SPARSE: SLOTS[0][1], EXCHANGE: SLOTS[4][1]}[kind]
    sc.body_forced_kind(Engine, run, knobs, kind, driver=OrderedDevDriver)
