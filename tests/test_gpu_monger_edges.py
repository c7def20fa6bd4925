"""GPU: the three mongering engines (GOSSIP_FLAG_MONGER, _MONGER_PULL, _MONGER_PUSHPULL; DESIGN.md
§2.13 - §2.16) at the edges of tests/monger_edges.py, against their numpy restatements, bit for bit: per
round the stats with the state hash and the messages, and the per-rumor counts; at the end the known and
the hot bitsets, the count of every node and rumor, the number of hot nodes, the round index and the hash.
No tolerance anywhere.

SEEDS: seeds whose high word is not zero (the coin of monger_close.h takes both key words).  MAXIMA:
4096 rumors, fanout 61, 63 and 64, bit 63 a rumor, counts that climb to 15.  GRID: 2^21 - 1, 2^21 and
2^21 + 1 nodes under a launch of 2^21 lanes.  PARTS and LOSS: the ends of values.PARTS and values.LOSS
through the FAULTS kernels.  LATE: coins and peers drawn at t >= 300.
tests/test_monger_edge_tables.py shows from the restatements alone that no case here is vacuous; the GRID
guards are asserted here, from the restatement's run."""
import pytest

import monger_edges as me

pytestmark = pytest.mark.gpu


def ids(cases):
    return [me.case_id(c) for c in cases]


@pytest.mark.parametrize("c", me.SEEDS, ids=ids(me.SEEDS))
def test_seeds(c):
    want = me.ref(c)
    assert c.seed >> 32 and me.guard(want, "cooled") > 0 and want.steps[0].rounds == c.rounds
    me.same(me.gpu(c), want)


@pytest.mark.parametrize("c", me.MAXIMA, ids=ids(me.MAXIMA))
def test_maxima(c):
    want = me.ref(c)
    assert want.steps[0].stats[0]["messages"] > 0 and me.guard(want, "cooled") > 0
    me.same(me.gpu(c), want)


@pytest.mark.parametrize("c", me.GRID, ids=ids(me.GRID))
def test_grid(c):
    """The 64 nodes below 2^21 and the nodes from 2^21 on (the second trip of the stride loops of both passes,
    at 2^21 + 1 one lane whose ballot writes a bitmap word with one bit) each hold, after two rounds, cooled
    rumors, rumors counted once and still hot, and at R = 65 a hot bit in the second word."""
    want = me.ref(c)
    assert want.steps[0].rounds == 2 and me.guard(want, "cooled") > 0 and me.guard(want, "kept") > 0
    regions = me.grid_guards(c, want)
    assert len(regions) == (2 if c.N > me.GRID_EDGE else 1)
    for cooled, counted, hot, last_word in regions:
        assert cooled > 0 and counted > 0 and hot > 0
        assert c.R != 65 or last_word > 0
    me.same(me.gpu(c), want)


@pytest.mark.parametrize("c", me.PARTS, ids=ids(me.PARTS))
def test_parts(c):
    want = me.ref(c)
    assert me.guard(want, "lost") > 0 and want.steps[0].rounds == c.rounds
    me.same(me.gpu(c), want)


@pytest.mark.parametrize("c", me.LOSS, ids=ids(me.LOSS))
def test_loss(c):
    want = me.ref(c)
    assert want.steps[0].rounds == c.rounds and want.hot_nodes > 0
    me.same(me.gpu(c), want)


@pytest.mark.parametrize("c", me.LATE, ids=ids(me.LATE))
def test_late(c):
    """300 rounds under cool = 0, then feedback 1/2 with a limit of 3: every coin and every peer draw that
    decides the second step has t >= 300; it ends before its cap with no node hot."""
    want = me.ref(c)
    first, second = want.steps
    assert first.rounds == 300 and second.stats[0]["round"] == 300 and second.rounds < 200 and want.hot_nodes == 0
    got = me.gpu(c)
    me.same(got, want)
    last = got.steps[1].stats[-1]
    assert got.round_index == last["round"] + 1 == 300 + second.rounds
    assert got.state_hash == last["state_hash"] == second.stats[-1]["state_hash"]
