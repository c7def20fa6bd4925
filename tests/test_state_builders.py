"""CPU only: the preconditions that test_gpu_states.py relies on, pinned on the oracle alone, so a
later change to a builder of tests/states.py cannot quietly make a GPU test vacuous.  The figures
were measured with the C oracle (seed states.SEED, N0 = 16449 nodes)."""
import numpy as np
import pytest

import oracle_py as op
import states as st
from states import N0, SEED

# builder -> (R, inject calls, empty nodes, full nodes, empty share, full share to 3 places)
ROUND0 = {
    "thirds": (3, 21932, 5483, 5483, 0.333, 0.333),
    "clustered": (64, 12352, N0 - 193, 193, 0.988, 0.012),
    "holes": (3, 49153, 8, N0 - 8 - 170, 0.0, 0.989),
    "disjoint": (64, 16449, 0, 0, 0.0, 0.0),
}

# (builder, mode, k, edge_loss, partitions) -> rounds to convergence (every run converges, so
# the GPU tests may step with max_rounds = 64)
ROUNDS = {
    ("thirds", "pushpull", 2, 0, 0): 3,
    ("thirds", "push", 1, 0, 0): 11,
    ("thirds", "pull", 1, 0, 0): 5,
    ("thirds", "pushpull", 2, 1 << 31, 2): 11,
    ("clustered", "push", 1, 0, 0): 16,
    ("clustered", "pull", 1, 0, 0): 10,
    ("clustered", "pushpull", 2, 0, 0): 5,
    ("clustered", "pushpull", 1, 0, 0): 7,
    ("holes", "push", 1, 0, 0): 5,
    ("disjoint", "pushpull", 2, 0, 0): 5,
}

# rounds that start with more than 0.3 of the nodes empty and more than 0.3 full (plan_dense_filter()'s
# default threshold): (empty, full) shares to 3 places at the start of the round
BOTH_CLASSES = {
    ("thirds", "pushpull", 2, 0, 0): {0: (0.333, 0.333)},
    ("thirds", "push", 1, 0, 0): {0: (0.333, 0.333)},
    ("thirds", "pull", 1, 0, 0): {0: (0.333, 0.333)},
    ("thirds", "pushpull", 2, 1 << 31, 2): {0: (0.333, 0.333)},
    ("clustered", "push", 1, 0, 0): {6: (0.524, 0.476), 7: (0.325, 0.675)},
    ("clustered", "pull", 1, 0, 0): {6: (0.496, 0.504)},
    ("clustered", "pushpull", 1, 0, 0): {4: (0.422, 0.578)},
}


def _oracle(name, mode="pushpull", k=2, loss=0, parts=0):
    b, R = st.BUILDERS[name]
    o = op.OracleEngine(N0, R, mode, k, SEED, flags=1, edge_loss=loss, partitions=parts)
    return o, b(o, R), R


@pytest.mark.parametrize("name", list(ROUND0))
def test_round0_classes_and_inject_counts(name):
    R, calls, empty, full, es, fs = ROUND0[name]
    assert st.BUILDERS[name][1] == R
    o, got_calls, _ = _oracle(name)
    assert got_calls == calls
    w = o.read_shard()[0]
    fm = np.uint64((1 << R) - 1)
    assert int((w == 0).sum()) == empty and int((w == fm).sum()) == full
    e, f = st.shares(o.read_shard(), R)
    assert (round(e, 3), round(f, 3)) == (es, fs)
    # the bits themselves, restated
    n = np.arange(N0, dtype=np.uint64)
    if name == "thirds":
        want = np.where(n % 3 == 1, fm, np.where(n % 3 == 2, np.uint64(1) << (n % 3), np.uint64(0)))
    elif name == "clustered":
        want = np.where((n < 64) | (n >= 16320), fm, np.uint64(0))
    elif name == "holes":
        want = np.where(n % 97 == 5, fm & ~(np.uint64(1) << (n % 3)), fm)
        want[list(st.HOLES)] = 0
    else:
        want = np.uint64(1) << (n % 64)
    o2, _, _ = _oracle(name)
    assert np.array_equal(o2.read_shard()[0], want.astype(np.uint64))


def test_holes_sit_on_group_and_tile_boundaries():
    assert st.HOLES == (0, 63, 64, 8191, 8192, 16383, 16384, N0 - 1)
    assert all(h % 97 != 5 for h in st.HOLES)
    assert N0 == 16384 + 64 + 1


@pytest.mark.parametrize("name", list(ROUND0))
def test_noisy_builds_the_same_state(name):
    o, calls, R = _oracle(name)
    q, noisy_calls, _ = _oracle("noisy_" + name)
    assert noisy_calls == calls + calls // 10  # every 10th call repeated: +10 %
    assert np.array_equal(q.read_shard(), o.read_shard())
    assert q.state_hash() == o.state_hash() != 0
    # really another order, really with duplicates
    rec, ref = st._Recorder(), st._Recorder()
    st.BUILDERS["noisy_" + name][0](rec, R)
    st.BUILDERS[name][0](ref, R)
    assert rec.calls[:50] != ref.calls[:50] and sorted(set(rec.calls)) == sorted(ref.calls)
    assert rec.calls[9] == rec.calls[10] and len(rec.calls) - len(set(rec.calls)) == calls // 10
    # the shuffle is fixed: two builds give the same order
    rec2 = st._Recorder()
    st.BUILDERS["noisy_" + name][0](rec2, R)
    assert rec2.calls == rec.calls


@pytest.mark.parametrize("run", list(ROUNDS), ids=lambda r: "-".join(str(x) for x in r))
def test_rounds_to_convergence_and_mixed_rounds(run):
    name, mode, k, loss, parts = run
    o, _, R = _oracle(name, mode, k, loss, parts)
    both = {}
    rounds = 0
    while rounds < 64:
        e, f = st.shares(o.read_shard(), R)
        if e > 0.3 and f > 0.3:
            both[rounds] = (round(e, 3), round(f, 3))
        res = o.step(1)
        rounds += 1
        if res.converged:
            break
    assert res.converged and rounds == ROUNDS[run] <= 64
    assert both == BOTH_CLASSES.get(run, {})


def test_path_tables_are_consistent():
    assert len(st.PATHS) == 9 and set(st.PATH_FLAGS) == set(st.PATHS)
    assert set(st.PATH_PARAMS) <= set(st.PATHS) and len(st.FAULT_PATHS) == 7
    for params in list(st.PATH_PARAMS.values()) + [p for _, p in st.FAULT_PATHS.values()]:
        assert set(params) <= set(st.PARAM_DEFAULTS)
