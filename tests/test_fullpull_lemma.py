"""CPU: the premise of the full-majority pull shortcut, held against the C oracle.

In PULL and PUSHPULL every read of a round is of S_t, so a node that pulls from a
full peer over an edge that is not lost ends the round with the full mask, whatever else reaches
it.  Here the peers and the lost edges come from oracle/numpy_ref.py and the next state from the C
oracle: nothing of the HIP engine runs, so this pins the lemma itself, not the code that uses it.
"""
import functools

import numpy as np
import pytest

import numpy_ref as nr
import oracle_py as op
from gossip_hip import loss_threshold

N = 4099
SEED = 0x5EED0F11
LOSS = loss_threshold(0.25)
FAULTS = {"none": (0, 0), "loss": (LOSS, 0), "parts": (0, 3), "loss_parts": (LOSS, 3)}


def full_mask(R):
    return np.uint64((1 << R) - 1) if R < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def state_words(kind, R):
    """S_t as one u64 word per node (read only)."""
    rng = np.random.default_rng(0xF011 + R)
    fm = full_mask(R)
    S = np.zeros(N, dtype=np.uint64)
    n = np.arange(N)
    if kind == "random":  # a third full, the rest empty or holding up to three rumors
        for _ in range(3):
            S |= np.where(rng.random(N) < 0.5, np.uint64(1) << rng.integers(0, R, N).astype(np.uint64), np.uint64(0))
        S[rng.random(N) < 0.33] = fm
    elif kind == "blocks":  # full and non-full nodes in alternating 64-node groups, the ragged last group full
        S[:] = np.uint64(1) << (n % R).astype(np.uint64)
        S[(n // 64) % 2 == 0] = fm
        S[4096:] = fm
    elif kind == "few_full":  # 16 full nodes: almost nobody is resolved
        S[:] = np.uint64(1) << (n % R).astype(np.uint64)
        S[7::257] = fm
    else:
        raise KeyError(kind)
    return S


def inject_words(engine, S, R):
    for node in np.flatnonzero(S):
        w = int(S[node])
        for r in range(R):
            if (w >> r) & 1:
                engine.inject(int(node), r)


def live_full_pull(S, R, k, t, loss, parts):
    """nodes that are not full and pull from a full peer over an edge that is not lost"""
    fm = full_mask(R)
    p = nr.peers(SEED, N, t, k).astype(np.int64)
    n = np.arange(N, dtype=np.int64)
    hit = np.zeros(N, dtype=bool)
    for j in range(k):
        lost = nr.edge_lost(SEED, N, loss, parts, n, p[:, j], t, j)
        hit |= ~lost & (S[p[:, j]] == fm)
    return hit & (S != fm)


@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("R", [64, 37])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("mode", ["pull", "pushpull"])
def test_random_state(mode, k, R, faults):
    _check("random", mode, k, R, faults, rounds=2)


@pytest.mark.parametrize("faults", list(FAULTS))
@pytest.mark.parametrize("kind,mode,k,R", [("blocks", "pull", 2, 37), ("blocks", "pushpull", 1, 64),
                                           ("few_full", "pushpull", 3, 37), ("few_full", "pull", 3, 64)])
def test_hand_made_state(kind, mode, k, R, faults):
    _check(kind, mode, k, R, faults, rounds=1)


def _check(kind, mode, k, R, faults, rounds):
    loss, parts = FAULTS[faults]
    fm = full_mask(R)
    o = op.OracleEngine(N, R, mode, k, SEED, flags=1, edge_loss=loss, partitions=parts)
    S = state_words(kind, R)
    inject_words(o, S, R)
    assert np.array_equal(o.read_shard()[0], S)
    seen = 0
    for t in range(rounds):
        S = o.read_shard()[0].copy()
        assert o.round_index == t
        must = live_full_pull(S, R, k, t, loss, parts)
        o.step(1)
        Sn = o.read_shard()[0]
        assert np.all(Sn[must] == fm), (kind, mode, k, R, faults, t)
        assert np.all(Sn & ~fm == 0) and np.all(Sn & S == S)  # no bit past R, no bit lost
        seen += int(must.sum())
    assert seen > 0  # the premise was exercised
    o.close()
