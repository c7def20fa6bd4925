"""GPU: the fanout and rumor-count classes of the dense emit that no other test runs, against the
C oracle bit for bit.  make_bin_geom halves the sender tile until ts * k <= 16384:

    k    4     7     8     16    17   32   33   34   63   64
    ts   4096  2048  2048  1024  512  512  256  256  256  256

with exactly full regions (ts * k == 16384) at k = 4, 8, 16, 32 and at the maximum fanout, 64; from
k = 33 up the tile stays at 256 senders.  The binned sparse scan takes k <= 4; loss draws with
j >> 2 above 1 start at k = 9 and reach Philox block 15 at k = 64.  41037 nodes are three
destination tiles with a ragged last one."""
import functools
import os

import numpy as np
import pytest

import oracle_py as op
import states as st
from gossip_hip import Engine, loss_threshold
from states import N0, SEED

pytestmark = pytest.mark.gpu

N = 41037
MAX_ROUNDS = 64
PATHS = ["auto", "dense", "dense_filter", "sparse", "sparse_bscan", "direct"]
THREADS = min(16, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def _oracle(N_, R, mode, k, loss=0, parts=0, work="random", rounds=MAX_ROUNDS):
    """Oracle run of one case, computed once per session and shared by every path (read only)."""
    o = op.OracleEngine(N_, R, mode, k, SEED, flags=1, edge_loss=loss, partitions=parts, threads=THREADS)
    _fill(o, work, R)
    res = o.step(rounds)
    return res, o.read_shard()


def _fill(x, work, R):
    if work == "random":
        x.inject_random()
    else:
        st.BUILDERS[work][0](x, R)


def _compare(N_, R, mode, k, path, loss=0, parts=0, work="random", rounds=MAX_ROUNDS, converges=True):
    want, shard = _oracle(N_, R, mode, k, loss, parts, work, rounds)
    assert converges is None or want.converged == converges
    flags, params = path
    e = Engine(N_, R, mode, k, SEED, flags=1 | flags, edge_loss=loss, partitions=parts, params=params)
    _fill(e, work, R)
    got = e.step(rounds)
    assert got.stats == want.stats
    assert np.array_equal(got.infected, want.infected)
    assert np.array_equal(e.read_shard(), shard)
    e.close()
    return want, shard


# the issue's rotation push / pull / pushpull over k = 4 .. 33 gives pull no power-of-two fanout and
# push-pull none that is not; the next two cases add them; the last five are the classes above 33, up
# to the maximum fanout in every mode
SWEEP = [("push", 4), ("pull", 7), ("pushpull", 8), ("push", 16), ("pull", 17), ("pushpull", 32), ("push", 33),
         ("pull", 16), ("pushpull", 7),
         ("pull", 34), ("pushpull", 63), ("push", 64), ("pull", 64), ("pushpull", 64)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode,k", SWEEP)
def test_fanout_sweep(mode, k, path):
    _compare(N, 64, mode, k, st.path_of(path))


@pytest.mark.parametrize("path", PATHS)
def test_fanout4_one_rumor(path):
    """k = 4, the largest fanout of the binned scan, with the one-bit full mask."""
    _compare(N, 1, "pushpull", 4, st.path_of(path))


@pytest.mark.parametrize("path", list(st.FAULT_PATHS))
@pytest.mark.parametrize("mode,k,loss,parts", [("push", 4, 0.2, 5), ("pushpull", 8, 0.3, 0), ("pull", 17, 0.25, 2),
                                               ("push", 64, 0.9, 0)])
def test_fanout_faults(mode, k, loss, parts, path):
    """Loss draws of edge j come from Philox block j >> 2: k = 8 reaches block 1, k = 17 block 4,
    k = 64 block 15 (nine edges in ten lost, so that the run still takes several rounds).
    With partitions no rumor leaves its block, so those runs go the whole 64 rounds unconverged."""
    want, _ = _compare(N, 64, mode, k, st.FAULT_PATHS[path], loss=loss_threshold(loss), parts=parts, converges=None)
    assert want.converged == (parts == 0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("R", [63, 64])
def test_one_word_rumor_counts(R, path):
    """The full mask of a partial word (63 bits) and of a whole one."""
    _, shard = _compare(N, R, "pushpull", 2, st.path_of(path))
    assert (shard[0] == np.uint64((1 << R) - 1)).all()


@pytest.mark.parametrize("path", ["auto", "direct"])
@pytest.mark.parametrize("mode,k", [("push", 3), ("pull", 2)])
@pytest.mark.parametrize("R", [65, 127, 128, 129])
def test_multi_word_rumor_counts(R, mode, k, path):
    """W = 2 with one bit in the last word, W = 2 ending one bit short of a word and exactly on a
    word, W = 3: such engines are not binned (bin_path_ok needs W == 1).  No bit at or above R is
    ever set: after every round the last word of every node stays inside the mask of R % 64 bits."""
    want, shard = _compare(N, R, mode, k, st.path_of(path))
    W, top = (R + 63) // 64, np.uint64((1 << (R % 64 or 64)) - 1)
    assert shard.shape == (W, N) and (shard[-1] == top).all()
    flags, params = st.path_of(path)
    e = Engine(N, R, mode, k, SEED, flags=1 | flags, params=params)
    e.inject_random()
    for _ in range(want.rounds):
        e.step(1)
        assert not (e.read_shard()[-1] & ~top).any()
    assert np.array_equal(e.read_shard(), shard)
    e.close()


@pytest.mark.parametrize("path", ["auto", "dense", "sparse"])
@pytest.mark.parametrize("parts", [N0, N0 - 1, 257])
def test_partition_extremes(parts, path):
    """State `thirds`, push-pull k=2.  N0 partitions: every node is alone, nothing may move.
    N0 - 1 and 257 (64 nodes and a bit per block): blocks that cut through groups; five rounds."""
    want, shard = _compare(N0, 3, "pushpull", 2, st.path_of(path), parts=parts, work="thirds", rounds=5,
                           converges=False)
    assert want.rounds == 5
    if parts == N0:
        o = op.OracleEngine(N0, 3, "pushpull", 2, SEED, flags=1)
        st.thirds(o, 3)
        assert np.array_equal(shard, o.read_shard())
        assert all(s["state_hash"] == o.state_hash() for s in want.stats)
