"""GPU: wide states, up to the configuration maxima, on every multi-word path, against the C oracle
bit for bit (tests/test_wide_state.py holds the oracle to the numpy restatement at these widths).
257 rumors are the first count past one 256-lane block (a second block of inject_random, a second
trip of the stats kernel's last loop), 1024 are the Maelstrom front-end's default page (W = 16),
4033 are W = 64 with one bit in the last word, 4096 the maximum (16 KB of counters in the stats
kernel).  Two workloads: inject_random, and states.sparse_words, which leaves most words of every
node empty for good.  Every comparison is of the per-round stats with the state hash, the per-rumor
counts and the whole state; no bit at or above R is ever set.  41037 nodes are three 16384-node
tiles with a ragged last one; the FLOOD walks keep 9 bytes per (value, node), so their engines have
3001 nodes at 1024 values and 1000 at 4096 (28 and 37 MB)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import numpy_ref as nr
import oracle_py as op
import shard_cases as sc
import states as st
import topo_ref as tr
import topologies as tp
from gossip_hip import FLAG_HASH, FLAG_TOPO_PEERS, Engine, _abi, loss_threshold
from shard_cases import GroupDriver, LockstepDriver
from states import SEED

pytestmark = pytest.mark.gpu

N = 41037
WIDTHS = [257, 1024, 4033, 4096]
MODES = [("push", 5), ("pull", 2), ("pushpull", 3)]
PATHS = ["auto", "direct"]
SPARSE_ROUNDS = 6
THREADS = min(16, os.cpu_count() or 1)
LOSSY = dict(edge_loss=loss_threshold(0.2), partitions=3, stall_rounds=3)


def fill(x, work, R):
    if work == "random":
        x.inject_random()
    else:
        st.sparse_words(x, R)


@functools.lru_cache(maxsize=None)
def oracle(R, mode, k, work, rounds, faults=()):
    """(step result, final state) of one oracle run, computed once per session and shared (read only)."""
    o = op.OracleEngine(N, R, mode, k, SEED, flags=1, threads=THREADS, **dict(faults))
    fill(o, work, R)
    res, shard = o.step(rounds), o.read_shard()
    o.close()
    shard.setflags(write=False)
    return res, shard


def top_mask(R):
    return ~nr.full_masks(R)[-1]


def short_read(e, node):
    """gossip_read_bitset with room for W - 1 words: (status, message)"""
    out = np.zeros(e.n_words, dtype=np.uint64)
    rc = e._fn("read_bitset")(e._h, C.c_uint64(node), out.ctypes.data_as(_abi.U64P), C.c_uint32(e.n_words - 1))
    return rc, e._fn("last_error")(e._h).decode()


def check_reads(e, shard):
    """read_bitset of the first, a middle and the last node: nwords == W, and W - 1 (GOSSIP_EINVAL)."""
    for n in (0, N // 2 + 1, N - 1):
        assert np.array_equal(e.read_bitset(n), shard[:, n])
        rc, msg = short_read(e, n)
        assert rc == -1 and f"need {e.n_words} words" in msg


def compare(R, mode, k, path, work, rounds, faults=()):
    """One gossip_step call for the whole run, then the same run one round per call: both equal the
    oracle after every round, state_hash between the steps included."""
    want, shard = oracle(R, mode, k, work, rounds, faults)
    flags, params = st.path_of(path)
    top = top_mask(R)
    with Engine(N, R, mode, k, SEED, flags=FLAG_HASH | flags, params=params, **dict(faults)) as e:
        fill(e, work, R)
        got = e.step(rounds)
        assert got.rounds == want.rounds
        assert got.stats == want.stats
        assert np.array_equal(got.infected, want.infected)
        assert np.array_equal(e.read_shard(), shard)
        assert e.state_hash() == want.stats[-1]["state_hash"]
        check_reads(e, shard)
    with Engine(N, R, mode, k, SEED, flags=FLAG_HASH | flags, params=params, **dict(faults)) as e:
        fill(e, work, R)
        for t in range(want.rounds):
            one = e.step(1)
            assert one.rounds == 1 and one.stats[0] == want.stats[t], t
            assert np.array_equal(one.infected[0], want.infected[t]), t
            assert e.state_hash() == want.stats[t]["state_hash"], t
            assert not (e.read_shard()[-1] & top).any(), t
        assert np.array_equal(e.read_shard(), shard)
    return want, shard


# --- random modes -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode,k", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_inject_random(R, mode, k, path):
    want, shard = compare(R, mode, k, path, "random", 64)
    assert want.converged and (shard == nr.full_masks(R)[:, None]).all()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode,k", MODES)
@pytest.mark.parametrize("R", WIDTHS)
def test_sparse_words(R, mode, k, path):
    """Rumors in the first, the 18th (or middle) and the last word only: every other word of every
    node is empty after every round, so the stats kernel skips it in every wave."""
    want, shard = compare(R, mode, k, path, "sparse", SPARSE_ROUNDS)
    assert want.rounds == SPARSE_ROUNDS and not want.converged
    ids = st.sparse_word_ids(R)
    assert not shard[[w for w in range(shard.shape[0]) if w not in ids]].any()
    assert int(want.infected[-1][R - 1]) > 3 and int(want.infected[-1][1]) == 0


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("R,mode", [(1024, "pull"), (4096, "pushpull")])
def test_fanout_64(R, mode, path):
    """Sixteen Philox blocks of peer draws per node and round."""
    assert compare(R, mode, 64, path, "random", 64)[0].converged


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("R,mode,k,work", [(257, "pushpull", 2, "random"), (4033, "push", 3, "sparse"),
                                          (1024, "pull", 2, "sparse")])
def test_loss_partitions_stall(R, mode, k, work, path):
    """20 % loss, three partition blocks, stall_rounds = 3: stall_update_kernel beside the W > 1
    round kernel.  No rumor leaves its block, so the run goes its whole 24 rounds."""
    want, _ = compare(R, mode, k, path, work, 24, tuple(LOSSY.items()))
    assert want.rounds == 24 and not want.converged


# --- FLOOD ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def topo(name, n):
    if name == "ragged_sym":   # node 1 is a hub with a row of 300 entries (and more at 30011 nodes)
        return tp.symmetrize(*tp.ragged(n, 7), n)
    if name == "hubs":         # hubs of 60 every 256 nodes; odd nodes hear from nodes they do not send to
        return tp.symmetrize(*tp.ragged(n, 7, hub_every=256, hub_deg=60), n, every=2)
    if name == "banded":
        return tp.symmetrize(*tp.banded(n, 7, hub_every=256, hub_deg=60), n)
    raise KeyError(name)


def flood_script(name, n, R):
    """The even slots injected (up to R - 2: past 2^8 and, at 4096, past 2^11), three rounds; at a hub
    a new high slot and a held one, five rounds; new rows (which end every walk) and
    64 odd slots from R - 3 down, twelve rounds or until nothing is sent."""
    hub = int(np.argmax(np.diff(topo(name, n)[0].astype(np.int64))))

    def script(x, after_step=lambda: None):
        x.set_topology(topo(name, n))
        for i in range(0, R, 2):
            x.inject((431 * i) % n, i)
        out = [x.step(3)]
        after_step()
        x.inject(hub, R - 1)
        x.inject(0, 0)   # held
        out.append(x.step(5))
        after_step()
        x.set_topology(topo("banded", n))
        for j in range(64):
            x.inject((977 * j + 5) % n, R - 3 - 2 * j)
        out.append(x.step(12))
        after_step()
        return out
    return script


_FLOOD = {}


def flood_oracle(name, n, R, faults=()):
    key = (name, n, R, faults)
    if key not in _FLOOD:
        o = op.OracleEngine(n, R, "flood", 0, 5, flags=1, threads=THREADS, **dict(faults))
        _FLOOD[key] = (flood_script(name, n, R)(o), o.read_shard())
        o.close()
    return _FLOOD[key]


def flood_compare(name, n, R, faults=()):
    want, shard = flood_oracle(name, n, R, faults)
    with Engine(n, R, "flood", 0, 5, flags=FLAG_HASH, **dict(faults)) as e:
        hashes = []
        got = flood_script(name, n, R)(e, lambda: hashes.append(e.state_hash()))
        assert len(got) == len(want) == 3
        for a, b, h in zip(got, want, hashes):
            assert a.rounds == b.rounds
            assert a.stats == b.stats   # messages per round among them
            assert np.array_equal(a.infected, b.infected)
            assert h == b.stats[-1]["state_hash"]
        got_shard = e.read_shard()
        assert np.array_equal(got_shard, shard)
        assert not (got_shard[-1] & top_mask(R)).any()
        for node in (0, n // 2, n - 1):
            assert np.array_equal(e.read_bitset(node), shard[:, node])
    return want


@pytest.mark.parametrize("name,n", [("ragged_sym", 30011), ("hubs", 3001)])
@pytest.mark.parametrize("R", [1024, 4096])
def test_flood(R, name, n):
    want = flood_compare(name, n, R)
    assert all(s["messages"] > 0 for s in want[0].stats + want[1].stats)
    assert int(want[2].infected[-1][R - 1]) > n // 2 and int(want[2].infected[-1][R - 3]) > n // 2


@pytest.mark.parametrize("D", [1, 16])
@pytest.mark.parametrize("name", ["ragged_sym", "hubs"])
@pytest.mark.parametrize("R,n", [(1024, 3001), (4096, 1000)])
def test_flood_walks(R, n, name, D):
    """The walk kernels: R x n walks, the loss draw of a message carries its value's slot in the
    counter word (x << 16, up to 4095 << 16).  D = 1: a walk whose neighbour lost one attempt stays
    on it for good; D = 16: walks wait, and move on once delivered."""
    faults = (("edge_loss", loss_threshold(0.15)), ("partitions", 2), ("stall_rounds", D))
    want = flood_compare(name, n, R, faults)
    assert [r.rounds for r in want] == [3, 5, 12] and want[2].stats[-1]["messages"] > 0
    assert want[2].stats != flood_oracle(name, n, R)[0][2].stats


# --- random gossip over the topology ----------------------------------------------------------------

NT = 1500
TOPO_FAULTS = (("edge_loss", loss_threshold(0.25)), ("partitions", 3), ("stall_rounds", 2))


@functools.lru_cache(maxsize=None)
def peer_rows():
    """One hub (node 1, a row of 300 entries and its listings back), empty rows, self-loops, repeated entries."""
    rp, col = tp.symmetrize(*tp.ragged(NT, 7), NT, every=2)
    deg = np.diff(rp.astype(np.int64))
    src = np.repeat(np.arange(NT), deg)
    assert deg.max() >= 300 and (deg >= 40).sum() == 1 and (deg == 0).sum() > 5 and (src == col).any()
    return rp, col


def topo_run(x, R):
    x.set_topology(peer_rows())
    deg = np.diff(peer_rows()[0].astype(np.int64))
    for i in range(R):
        x.inject((431 * i) % NT, i)
    x.inject(int(np.argmax(deg)), R - 1)
    x.inject(int(np.nonzero(deg == 0)[0][2]), R // 2)
    return x.step(12), x.read_shard()


@functools.lru_cache(maxsize=None)
def topo_ref(R, mode, k, faults):
    return topo_run(tr.TopoSim(NT, R, mode, k, 9, **dict(faults)), R)


@pytest.mark.parametrize("faults", [(), TOPO_FAULTS], ids=["clean", "faults"])
@pytest.mark.parametrize("mode,k", [("push", 5), ("pull", 4), ("pushpull", 2)])
@pytest.mark.parametrize("R", [1024, 4096])
def test_topo_peers(R, mode, k, faults):
    (want, shard) = topo_ref(R, mode, k, faults)
    assert want.rounds == 12 and want.stats[-1]["messages"] > 0
    with Engine(NT, R, mode, k, 9, flags=FLAG_HASH | FLAG_TOPO_PEERS, **dict(faults)) as e:
        got, got_shard = topo_run(e, R)
        assert e.state_hash() == want.stats[-1]["state_hash"]
    assert got.rounds == want.rounds
    for a, b in zip(got.stats, want.stats):
        assert a == b
    assert np.array_equal(got.infected, want.infected)
    assert np.array_equal(got_shard, shard)


# --- sharded, all shards on one GPU ---------------------------------------------------------------

@pytest.mark.parametrize("driver", ["lockstep", "group"])
@pytest.mark.parametrize("case", range(len(sc.WIDE)), ids=sc.WIDE_IDS)
def test_sharded(case, driver):
    """shard_cases.WIDE through the lockstep host driver and through gossip_group_step over device
    copies (transport 2): a [G][W][Nl] image of up to 64 words per node, 5 + R totals per round;
    stats, per-rumor counts and every rank's words after every round."""
    if driver == "lockstep":
        owned = sc.body_multiword(Engine, case, driver=LockstepDriver, wide=True)
    else:
        owned = sc.body_multiword(None, case, driver=GroupDriver, wide=True)
    Nc, G = sc.WIDE[case][0], sc.WIDE[case][4]
    assert owned == [min(-(-Nc // G), max(0, Nc - r * -(-Nc // G))) for r in range(G)]
    assert (owned[-1] == 0) == (Nc == 16)
