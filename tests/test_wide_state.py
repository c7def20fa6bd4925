"""CPU: the C oracle against the numpy restatement at the widths no golden vector has: 257 rumors
(the first count past one 256-lane block), 1024 (the Maelstrom front-end's default page, W = 16),
4033 (W = 64 with one bit in the last word) and 4096 (the configuration maximum), and fanout 64.
Computed live, round by round: stats, hash, messages, the per-rumor counts, then the whole state.
tests/test_gpu_wide_state.py judges the HIP engine by the oracle at these widths; this file is
what licenses that."""
import numpy as np
import pytest

import numpy_ref as nr
import oracle_py as op
import shard_cases as sc
import states as st
import topologies as tp
from gossip_hip import loss_threshold
from gossip_hip.maelstrom import grid_topology

SEED = st.SEED
WIDTHS = [257, 1024, 4033, 4096]
SPARSE_ROUNDS = 6


def rows_of(topo):
    """(row_ptr, col) -> list of neighbour lists"""
    rp, col = topo
    return [[int(v) for v in col[rp[u]:rp[u + 1]]] for u in range(rp.size - 1)]


def grid_rows(n):
    g = grid_topology(n)
    return [[int(v[1:]) for v in g[f"n{i}"]] for i in range(n)]


def check(o, s, rounds, stop=True):
    """Steps the oracle one round at a time beside the numpy Sim; returns the rounds run."""
    for t in range(rounds):
        res = o.step(1)
        want = s.round()
        assert res.rounds == 1
        got = res.stats[0]
        assert (got["round"], got["full_nodes"], got["converged"], got["messages"], got["state_hash"]) == \
            (want["round"], want["full"], want["converged"], want["messages"], want["hash"]), t
        assert [int(x) for x in res.infected[0]] == want["infected"], t
        if stop and (want["converged"] or (s.mode == "flood" and want["messages"] == 0)):
            break
    assert np.array_equal(o.read_shard(), s.S)
    assert o.state_hash() == nr.state_hash(s.S)
    return t + 1


def fill(x, work, R, N):
    if work == "random":
        x.inject_random()
    else:
        st.sparse_words(x, R, N)


def random_pair(N, R, mode, k, work, **faults):
    o = op.OracleEngine(N, R, mode, k, SEED, flags=1, **faults)
    s = nr.Sim(N, R, mode, k, SEED, **faults)
    fill(o, work, R, N)
    fill(s, work, R, N)
    assert np.array_equal(o.read_shard(), s.S)
    return o, s


@pytest.mark.parametrize("work", ["random", "sparse"])
@pytest.mark.parametrize("mode,k", [("push", 5), ("pull", 2), ("pushpull", 3)])
@pytest.mark.parametrize("R", WIDTHS)
def test_random_modes(R, mode, k, work):
    N = {257: 1200, 1024: 777, 4033: 1021, 4096: 1500}[R]
    o, s = random_pair(N, R, mode, k, work)
    if work == "random":
        rounds = check(o, s, 64)
        assert rounds < 64 and (s.S == nr.full_masks(R)[:, None]).all()
    else:
        check(o, s, SPARSE_ROUNDS, stop=False)
        untouched = [w for w in range(s.W) if w not in st.sparse_word_ids(R)]
        assert untouched and not s.S[untouched].any() and s.S[st.sparse_word_ids(R)].any(axis=1).all()


@pytest.mark.parametrize("R,mode", [(1024, "pull"), (4096, "pushpull")])
def test_fanout_64(R, mode):
    """Peer draws from sixteen Philox blocks per node and round."""
    o, s = random_pair(777, R, mode, 64, "random")
    assert check(o, s, 64) < 64


@pytest.mark.parametrize("work", ["random", "sparse"])
def test_fanout_64_loss(work):
    """Loss draws up to Philox block 15."""
    o, s = random_pair(1021, 257, "push", 64, work, edge_loss=loss_threshold(0.6))
    check(o, s, 64 if work == "random" else SPARSE_ROUNDS, stop=work == "random")


@pytest.mark.parametrize("R,mode,k,work", [(257, "pushpull", 2, "random"), (4033, "push", 3, "sparse"),
                                          (1024, "pull", 2, "sparse")])
def test_loss_partitions_stall(R, mode, k, work):
    """20 % loss, three partition blocks and stall_rounds = 3: no rumor leaves its block, so the
    runs go their whole 24 rounds unconverged, and nodes stall on the way."""
    o, s = random_pair(1200, R, mode, k, work, edge_loss=loss_threshold(0.2), partitions=3, stall_rounds=3)
    assert check(o, s, 24) == 24
    assert (s.streak >= 3).any()


def flood_injects(N, R, count):
    """`count` values with slots spread over every word, the first and last slot among them."""
    slots = sorted({(i * (R - 1)) // (count - 1) for i in range(count)})
    return [((431 * x + 3) % N, x) for x in slots]


FLOOD_TOPOS = {"grid": lambda: grid_rows(100),
               "ragged": lambda: rows_of(tp.symmetrize(*tp.ragged(150, 7, max_deg=5, hub_every=64, hub_deg=30), 150,
                                                       every=2))}


@pytest.mark.parametrize("R", [1024, 4096])
@pytest.mark.parametrize("name", list(FLOOD_TOPOS))
def test_flood(name, R):
    """Plain FLOOD, messages included: every slot injected (inject_random) on the grid; on the
    ragged rows (self-loops, repeated entries, empty rows, hubs, one-way listings) 200 values spread
    over all words, so most bits of most words stay empty."""
    rows = FLOOD_TOPOS[name]()
    N = len(rows)
    o = op.OracleEngine(N, R, "flood", 0, SEED, flags=1)
    o.set_topology(rows)
    s = nr.Sim(N, R, "flood", 0, SEED, topology=rows)
    for x in (o, s):
        if name == "grid":
            x.inject_random()
        else:
            for n, r in flood_injects(N, R, 200):
                x.inject(n, r)
    rounds = check(o, s, 64)
    assert 3 < rounds < 64
    if name == "grid":
        assert (s.S == nr.full_masks(R)[:, None]).all()


@pytest.mark.parametrize("D,parts,loss,R", [(0, 0, 0.3, 300), (3, 2, 0.2, 300), (1, 0, 0.25, 300),
                                            (2, 2, 0.2, 2200)])
def test_flood_walks(D, parts, loss, R):
    """FLOOD with faults: 40 values of a 300-slot state (five words, the last partial) walking
    a 5 x 5 grid, the loss draw carrying the slot, up to 299; once of a 2200-slot state, with slots
    past 2^11 in the draw's counter word."""
    N = 25
    rows = grid_rows(N)
    kw = dict(edge_loss=loss_threshold(loss), partitions=parts, stall_rounds=D)
    o = op.OracleEngine(N, R, "flood", 0, SEED, flags=1, **kw)
    o.set_topology(rows)
    s = nr.Sim(N, R, "flood", 0, SEED, topology=rows, **kw)
    for x in (o, s):
        for n, r in flood_injects(N, R, 40):
            x.inject(n, r)
    check(o, s, 14, stop=False)
    assert s.S.any(axis=1).all()


@pytest.mark.parametrize("case", range(len(sc.WIDE)), ids=sc.WIDE_IDS)
def test_sharded_oracle_shards(case):
    """shard_cases.WIDE over oracle shards in lockstep: the sharded protocol at 16 and 64 words per node
    equals one engine (test_gpu_wide_state.py runs the same cases over HIP shards)."""
    owned = sc.body_multiword(op.OracleEngine, case, wide=True)
    assert sum(owned) == sc.WIDE[case][0] and (owned[-1] == 0) == (sc.WIDE[case][0] == 16)
