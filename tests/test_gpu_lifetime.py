"""GPU: an engine owns its device memory (csrc/devmem.h).  Every engine kind is created, run far
enough to reach its lazy allocations and destroyed, over and over: free device memory does not
drift and every cycle computes the same bits; a create that cannot fit returns an error and holds
nothing; receive buffers regrown from a smaller first use change no result."""
import ctypes as C

import numpy as np
import pytest
import torch

import topologies as tp
from conftest import inject_case
from gossip_hip import FLAG_DIRECT, Engine, Group, loss_threshold
from gossip_hip import engine as eng_mod
from gossip_hip.engine import churn_threshold as ct
from gossip_hip.sharded import _as_tensor, lockstep_run

pytestmark = pytest.mark.gpu

SEED = 0x5EED0004
CHURN = dict(churn_fail=ct(0.01), churn_recover=ct(0.1))
N_FLOOD = 30011


def _last_hash(res):
    return res.stats[-1]["state_hash"]


def binned_pushpull(after_first_step):
    """W == 1: a record slab under 512 MiB, so place_tries 2 takes placement's early-out."""
    with Engine(1 << 21, 64, "pushpull", 2, SEED, flags=1) as e:
        e.set_param("place_tries", 2)
        e.inject_random()
        e.step(1)
        after_first_step()
        return _last_hash(e.step(64))


def direct_two_words(after_first_step):
    with Engine(1 << 20, 65, "pushpull", 2, SEED, flags=1 | FLAG_DIRECT) as e:
        e.inject_random()
        e.step(1)
        after_first_step()
        return _last_hash(e.step(64))


def flood_faults(after_first_step):
    with Engine(N_FLOOD, 3, "flood", 0, 0, flags=1, edge_loss=loss_threshold(0.1), stall_rounds=3) as e:
        e.set_topology(tp.ragged(N_FLOOD, 7))
        e.set_topology(tp.symmetrize(*tp.ragged(N_FLOOD, 7), N_FLOOD))
        inject_case(e, [(0, 0), (N_FLOOD - 1, 1), (12345, 2)])
        e.step(1)
        after_first_step()
        return _last_hash(e.step(40))


def random_stall(after_first_step):
    with Engine(1 << 21, 64, "pushpull", 2, SEED, flags=1, stall_rounds=3) as e:
        e.inject_random()
        e.step(1)
        after_first_step()
        return _last_hash(e.step(64))


def antientropy(after_first_step):
    with Engine(1 << 20, 16, "antientropy", 1, 0x5EED0005, flags=1, **CHURN) as e:
        e.set_param("ae_cap", 1 << 18)  # the edge lists are freed and allocated again
        e.inject_random()
        e.step(1)
        after_first_step()
        return _last_hash(e.step(12))


def _group(mode, R, k, seed, params=None, rounds=300, N=1 << 20, **kw):
    def run(after_first_step):
        with Group(N, R, mode, k, seed, flags=1, n_shards=3, devices=[0] * 3, params=params, **kw) as g:
            g.inject_random()
            g.step(1)
            after_first_step()
            return _last_hash(g.step(rounds))
    return run


class _DevValues(Engine):
    """round_compute through gossip_round_compute_dev: the partials read from the published device values."""

    def round_compute(self):
        p = self.round_compute_dev()
        return _as_tensor(p, self.partial_len() * 8, True, self.device).cpu().numpy().view(np.uint64)


def lockstep_dev_pair(after_first_step):
    dense = {"sparse_frac": -1, "xd_shards": 0, "cc_frac": 0, "replicate": 0}
    engines = [_DevValues(1 << 20, 64, "pushpull", 2, SEED, flags=1, shard_rank=r, shard_count=2, params=dense)
               for r in range(2)]
    try:
        for e in engines:
            e.inject_random()
        lockstep_run(engines, 1)
        after_first_step()
        stats, kinds = lockstep_run(engines, 64)
        assert set(kinds) == {0}
        return stats[-1]["state_hash"]
    finally:
        for e in engines:
            e.close()


KINDS = {
    "binned_pushpull": binned_pushpull,
    "direct_R65": direct_two_words,
    "flood_faults": flood_faults,
    "random_stall": random_stall,
    "antientropy": antientropy,
    "group_exchange": _group("pushpull", 64, 2, SEED, {"xd_shards": 2}),
    "group_classcoded": _group("pushpull", 64, 2, SEED, {"sparse_frac": -1, "xd_shards": 0, "cc_frac": 1}),
    "group_antientropy": _group("antientropy", 16, 1, 0x5EED0005, rounds=400, N=1 << 16, **CHURN),
    "lockstep_dev_pair": lockstep_dev_pair,
}


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_run_destroy_cycles(kind):
    """Seven cycles of one engine kind.  The footprint is the drop in free device memory from before
    the create to after the first step of cycle 1; cycles 2-7 may lower free memory by less than half
    of it (mem_get_info is device-wide and the runtime keeps small pools of its own: a leaked main
    buffer would show as several footprints), and every cycle ends on the same state hash."""
    run = KINDS[kind]
    seen = {}
    before = _free()
    first = run(lambda: seen.setdefault("after_step", _free()))
    footprint = before - seen["after_step"]
    after_cycle1 = _free()
    hashes = [run(lambda: None) for _ in range(6)]
    drift = after_cycle1 - _free()
    print(f"{kind}: footprint {footprint / 2**20:.1f} MiB, drift over 6 cycles {drift / 2**20:.2f} MiB")
    assert footprint > 0
    assert drift < footprint / 2
    assert hashes == [first] * 6


def test_create_that_cannot_fit_holds_nothing(golden):
    """2^32 - 1 nodes x 4096 rumors: the first state image is 2 TiB, so gossip_create fails at its
    first large allocation with the totals and scratch buffers already held.  An API error return:
    GOSSIP_ENOMEM, a null handle, the allocation named; an engine created right after is sound."""
    lib = eng_mod.load_library()
    cfg = eng_mod.make_config(2**32 - 1, 4096, "push", 1, 1)
    h = C.c_void_p()
    assert lib.gossip_create(C.byref(cfg), C.byref(h)) == -3
    assert not h.value
    msg = lib.gossip_last_error(None)
    assert b"hipMalloc of" in msg and b"bytes failed" in msg, msg
    c = golden["random"][0]
    with Engine(c["N"], c["R"], c["mode"], c["k"], c["seed"], flags=1) as e:
        inject_case(e, c["inject"])
        res = e.step(256)
        assert [s["state_hash"] for s in res.stats] == [r["hash"] for r in c["rounds"]]
        assert e.state_hash() == c["final_hash"]


def test_regrown_buffers_keep_results():
    """A 3-shard group runs a few-rumor case to convergence, is reset and runs inject_random: the
    receive buffers sized by the first run's small rounds are freed and allocated larger.  Every
    round's stats equal one engine's, as does the final state."""
    N, R, k, seed, G = 200003, 3, 2, 9, 3
    with Engine(N, R, "pushpull", k, seed, flags=1) as ref, \
            Group(N, R, "pushpull", k, seed, flags=1, n_shards=G, devices=[0] * G, params={"xd_shards": 2}) as g:
        for pattern in ([(5, 0), (N - 1, 1), (77, 2)], "random"):
            for x in (ref, g):
                x.reset()
                inject_case(x, pattern)
            want, got = ref.step(100), g.step(100)
            assert got.converged and got.stats == want.stats
            assert np.array_equal(got.infected, want.infected)
            full = ref.read_shard()
            for e in g.shards:
                assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])
