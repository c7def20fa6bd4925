"""CPU: the ragged topology builders pinned, and the C oracle's FLOOD held to two restatements
that share no text with it, at sizes the goldens never reach (30011 nodes, rows of 300 entries,
directed rows with repeats, self-loops, empty rows and unreachable nodes): plain FLOOD against
the BFS restatement of DESIGN.md §2.4-2.6 (tests/topologies.py), the walks of FLOOD with faults
(§2.9) against numpy_ref.Sim on rows of 40 and 45 entries (loss-draw counter words up to 11).
tests/test_gpu_flood.py holds the HIP kernels to this oracle on the same topologies."""
import functools
import os

import numpy as np
import pytest

import numpy_ref as nr
import oracle_py as op
import topologies as tp
from gossip_hip import loss_threshold

THREADS = min(16, os.cpu_count() or 1)
N = 30011
INJ3 = [(0, 0), (N - 1, 1), (12345, 2)]


def injects(n, R):
    return [((431 * i) % n, i) for i in range(R)]


@functools.lru_cache(maxsize=None)
def topo(name):
    if name == "ragged":
        return tp.ragged(N, 7)
    if name == "ragged_sym":
        return tp.symmetrize(*tp.ragged(N, 7), N)
    if name == "banded_sym":
        return tp.symmetrize(*tp.banded(N, 7), N)
    if name == "ragged_half":   # odd nodes hear from nodes they do not send to, and from nodes they do
        return tp.symmetrize(*tp.ragged(N, 7), N, every=2)
    raise KeyError(name)


def _degrees(row_ptr, col, n):
    return np.diff(row_ptr.astype(np.int64)), np.bincount(col, minlength=n)


def test_builders_pinned():
    rp, col = topo("ragged")
    assert rp.dtype == np.uint32 and col.dtype == np.uint32 and rp.size == N + 1 and rp[-1] == col.size
    out, inn = _degrees(rp, col, N)
    assert (col.size, int((out == 0).sum()), int((inn == 0).sum())) == (123036, 3360, 502)
    assert out.max() >= 300 and out[1] == 300 and out[4100] == 300
    src = np.repeat(np.arange(N), out)
    assert (src == col).any()                                        # self-loops
    assert np.unique(src.astype(np.int64) * N + col).size < col.size  # repeated entries
    srp, scol = topo("ragged_sym")
    sout, sinn = _degrees(srp, scol, N)
    assert (scol.size, int((sout == 0).sum()), int(sinn.max())) == (246072, 55, 308)
    assert sout.max() >= 300 and np.array_equal(sout, sinn)
    # row u: its own list in order, then the nodes that list u, ascending
    for u in (0, 1, 4100, N - 1):
        own = col[rp[u]:rp[u + 1]]
        row = scol[srp[u]:srp[u + 1]]
        assert np.array_equal(row[:own.size], own)
        assert np.array_equal(row[own.size:], np.sort(src[col == u]))
    # banded keeps ragged's degrees and every 8th entry; the others lie within 64 after u
    brp, bcol = tp.banded(N, 7)
    assert np.array_equal(brp, rp)
    j = np.arange(col.size) - rp[:-1].astype(np.int64)[src]
    far = j % 8 == 7
    assert np.array_equal(bcol[far], col[far])
    gap = (bcol.astype(np.int64) - src - 1) % N
    assert gap[~far].max() == 63 and gap[~far].min() == 0
    # small arguments, the mix itself
    assert [int(x) for x in tp.mix(np.array([0, 1], dtype=np.uint64))] == [0, 0x5692161D100B05E5]
    drp, dcol = tp.dedupe(srp, scol, N)
    assert dcol.size == np.unique(np.repeat(np.arange(N), sout).astype(np.int64) * N + scol).size
    assert all(np.array_equal(dcol[drp[u]:drp[u + 1]], np.unique(scol[srp[u]:srp[u + 1]])) for u in (0, 1, 77, N - 1))


def _oracle_flood(name, R, inj):
    o = op.OracleEngine(N, R, "flood", 0, 0, flags=1, threads=THREADS)
    o.set_topology(topo(name))
    for n, r in inj:
        o.inject(n, r)
    return o.step(256)


# topology, rounds, total messages, nodes holding each value at the end
# ragged_half: a sender skip that took any sender in the row for the first one sends 493,959
FLOOD3 = [("ragged", 15, 362538, 29468), ("ragged_sym", 9, 648153, 29956), ("banded_sym", 12, 615105, 29951),
          ("ragged_half", 11, 495122, 29890)]


@pytest.mark.parametrize("name,rounds,total,reached", FLOOD3, ids=[c[0] for c in FLOOD3])
def test_oracle_flood_equals_bfs(name, rounds, total, reached):
    res = _oracle_flood(name, 3, INJ3)
    want = tp.flood_bfs(*topo(name), N, INJ3, 3)
    assert res.rounds == len(want) == rounds
    assert [s["messages"] for s in res.stats] == [m for m, _ in want]
    assert [[int(x) for x in row] for row in res.infected] == [inf for _, inf in want]
    assert sum(s["messages"] for s in res.stats) == total
    assert [int(x) for x in res.infected[-1]] == [reached] * 3
    assert res.stats[-1]["messages"] == 0 and not res.converged  # the quiescent round is reported


def test_oracle_flood_equals_bfs_first_sender_among_many():
    """Eight values in one word reach the same node in the same round from different senders,
    some in its row and some not: the skip belongs to each value's own first sender."""
    inj = injects(N, 8)
    res = _oracle_flood("ragged_half", 8, inj)
    want = tp.flood_bfs(*topo("ragged_half"), N, inj, 8)
    assert res.rounds == len(want) == 11 and sum(s["messages"] for s in res.stats) == 1320012
    assert [s["messages"] for s in res.stats] == [m for m, _ in want]
    assert [[int(x) for x in row] for row in res.infected] == [inf for _, inf in want]


def test_oracle_flood_equals_bfs_70_values():
    """Two words per node; the restatement follows every 10th value."""
    inj = injects(N, 70)
    res = _oracle_flood("ragged_sym", 70, inj)
    assert res.rounds == 10 and sum(s["messages"] for s in res.stats) == 15123570
    sub = [(n, r // 10) for n, r in inj if r % 10 == 0]
    want = tp.flood_bfs(*topo("ragged_sym"), N, sub, 7, rounds=res.rounds)
    assert [[int(x) for x in row[::10]] for row in res.infected] == [inf for _, inf in want]


def _rows(row_ptr, col):
    return [[int(v) for v in col[row_ptr[u]:row_ptr[u + 1]]] for u in range(row_ptr.size - 1)]


def _bulk_draws(monkeypatch):
    """numpy_ref.Sim asks numpy_ref.edge_lost about one message at a time, a Philox call each.
    The same function answers for every node at once here: its loss draws of (round, position,
    value) are taken for all nodes on first use and kept, its partition rule is asked per message."""
    one, kept = nr.edge_lost, {}

    def edge_lost(seed, n_nodes, loss, parts, n, p, t, j, value=0):
        lost = one(seed, n_nodes, 0, parts, n, p, t, j, value)
        if loss:
            if (t, j, value) not in kept:
                if kept and next(iter(kept))[0] != t:
                    kept.clear()
                every = np.arange(n_nodes)
                kept[(t, j, value)] = one(seed, n_nodes, loss, 0, every, every, t, j, value)
            lost = lost | kept[(t, j, value)][np.asarray(n)]
        return lost

    monkeypatch.setattr(nr, "edge_lost", edge_lost)


def _walks_case(monkeypatch, n, R, topology, loss, D, parts, rounds):
    _bulk_draws(monkeypatch)
    o = op.OracleEngine(n, R, "flood", 0, 5, flags=1, edge_loss=loss, partitions=parts, stall_rounds=D)
    o.set_topology(topology)
    sim = nr.Sim(n, R, "flood", 0, 5, topology=_rows(*topology), edge_loss=loss, partitions=parts, stall_rounds=D)
    for node, r in injects(n, R):
        o.inject(node, r)
        sim.inject(node, r)
    got, want = o.step(rounds), sim.run(rounds)
    assert got.rounds == len(want) and got.rounds > 5
    assert [(s["messages"], s["state_hash"], s["full_nodes"]) for s in got.stats] == \
        [(s["messages"], s["hash"], s["full"]) for s in want]
    assert [[int(x) for x in row] for row in got.infected] == [s["infected"] for s in want]


@pytest.mark.parametrize("parts", [0, 3])
@pytest.mark.parametrize("D", [0, 1, 3])
@pytest.mark.parametrize("sym", [False, True], ids=["directed", "symmetrized"])
def test_oracle_walks_equal_numpy(monkeypatch, sym, D, parts):
    """numpy_ref.Sim is slow on stuck walks: the first 20 rounds with a deadline, 40 without."""
    n = 1201
    t = tp.ragged(n, 3, max_deg=7, hub_every=97, hub_deg=40)
    if sym:
        t = tp.symmetrize(*t, n)
    assert np.diff(t[0].astype(np.int64)).max() == (45 if sym else 40)
    _walks_case(monkeypatch, n, 5, t, loss_threshold(0.2), D, parts, 20 if D else 40)


def test_oracle_walks_equal_numpy_70_values(monkeypatch):
    n = 301
    t = tp.symmetrize(*tp.ragged(n, 9, max_deg=7, hub_every=53, hub_deg=20), n)
    _walks_case(monkeypatch, n, 70, t, loss_threshold(0.3), 2, 0, 12)
