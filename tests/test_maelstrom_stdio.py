"""Maelstrom JSON wire format (gossip_hip.maelstrom_stdio): the reference's
handler set (main.go:102-153) answered for a whole cluster.  CPU tests drive
the oracle engine through the same front-end; the GPU test drives the HIP
engine.  Mirrors what Maelstrom's broadcast checker asserts: every
acknowledged value is in every node's read."""
import io
import json

import pytest

import oracle_py as op
from gossip_hip.maelstrom import grid_topology, line_topology
from gossip_hip.maelstrom_stdio import ERR_CRASH, ERR_NOT_SUPPORTED, MaelstromServer


def _script(n, values):
    ids = [f"n{i}" for i in range(n)]
    msgs = [{"src": "c0", "dest": i, "body": {"type": "init", "msg_id": 1, "node_id": i, "node_ids": ids}}
            for i in ids]
    topo = grid_topology(n)
    msgs += [{"src": "c1", "dest": i, "body": {"type": "topology", "msg_id": 2, "topology": topo}} for i in ids]
    mid = 10
    for node, v in values:
        msgs.append({"src": "c2", "dest": node, "body": {"type": "broadcast", "message": v, "msg_id": mid}})
        mid += 1
    msgs += [{"src": "c3", "dest": i, "body": {"type": "read", "msg_id": 99}} for i in ids]
    return msgs


def _run(server, msgs):
    inp = io.StringIO("".join(json.dumps(m) + "\n" for m in msgs))
    out = io.StringIO()
    server.serve(inp, out)
    return [json.loads(line) for line in out.getvalue().splitlines()]


def _check_cluster(server, n=25):
    values = [("n0", 1000), ("n24", -7), ("n12", 42), ("n0", 1000)]  # last one: dedupe (main.go:113)
    replies = _run(server, _script(n, values))
    kinds = [r["body"]["type"] for r in replies]
    assert kinds.count("init_ok") == n and kinds.count("topology_ok") == n
    assert kinds.count("broadcast_ok") == len(values) and kinds.count("read_ok") == n
    for r in replies:
        assert "in_reply_to" in r["body"] and r["src"].startswith("n") and r["dest"].startswith("c")
    for r in replies:
        if r["body"]["type"] == "read_ok":
            assert sorted(r["body"]["messages"]) == [-7, 42, 1000]
    # three distinct values flooded over a 5x5 grid; the repeat moved nothing
    assert server.stats["broadcasts"] == 4 and server.stats["gossip_messages"] > 0
    return replies


def test_stdio_cluster_oracle():
    _check_cluster(MaelstromServer(max_values=8, engine_factory=lambda **kw: op.OracleEngine(**kw)))


def test_stdio_errors_oracle():
    s = MaelstromServer(max_values=2, engine_factory=lambda **kw: op.OracleEngine(**kw))
    out = s.handle({"src": "c", "dest": "n0", "body": {"type": "read", "msg_id": 1}})
    assert out[0]["body"]["code"] == ERR_CRASH  # not initialised
    s.handle({"src": "c", "dest": "n0", "body": {"type": "init", "msg_id": 1, "node_id": "n0",
                                                 "node_ids": ["n0", "n1"]}})
    out = s.handle({"src": "c", "dest": "n0", "body": {"type": "cas", "msg_id": 2}})
    assert out[0]["body"]["code"] == ERR_NOT_SUPPORTED and out[0]["body"]["in_reply_to"] == 2
    out = s.handle({"src": "c", "dest": "n0", "body": {"type": "broadcast", "msg_id": 3, "message": "x"}})
    assert out[0]["body"]["code"] == ERR_CRASH  # body does not decode (main.go:104-106)
    assert s.handle({"src": "n1", "dest": "n0", "body": {"type": "broadcast_ok", "in_reply_to": 5}}) == []
    for v in (1, 2):
        s.handle({"src": "c", "dest": "n1", "body": {"type": "broadcast", "msg_id": 4, "message": v}})
    out = s.handle({"src": "c", "dest": "n1", "body": {"type": "broadcast", "msg_id": 5, "message": 3}})
    assert out[0]["body"]["code"] == ERR_CRASH  # more distinct values than slots


@pytest.mark.gpu
def test_stdio_cluster_gpu():
    _check_cluster(MaelstromServer(max_values=8))


def _oracle_factory(**kw):
    return op.OracleEngine(**kw)


def test_stdio_many_values_pages_oracle():
    """A standard broadcast workload sends thousands of distinct values (the reference's
    MessageKeeper has no limit, main.go:35-39): they spill over engine pages."""
    s = MaelstromServer(engine_factory=_oracle_factory, page_values=64)
    n = 9
    values = [(f"n{i % n}", 10_000 + i) for i in range(300)]
    replies = _run(s, _script(n, values))
    assert len(s.cluster.pages) == 5  # ceil(300 / 64)
    for r in replies:
        if r["body"]["type"] == "read_ok":
            assert sorted(r["body"]["messages"]) == [v for _, v in values]
    assert [r["body"]["type"] for r in replies].count("broadcast_ok") == 300


def test_broadcast_before_topology_is_never_forwarded():
    """main.go:72 ranges over a nil Topology for a broadcast that arrives before `topology`:
    the value is recorded and acked but never forwarded, also not after the topology
    arrives; later values flood as usual."""
    n = 9
    ids = [f"n{i}" for i in range(n)]
    s = MaelstromServer(engine_factory=_oracle_factory)
    msgs = [{"src": "c0", "dest": i, "body": {"type": "init", "msg_id": 1, "node_id": i, "node_ids": ids}}
            for i in ids]
    msgs.append({"src": "c2", "dest": "n4", "body": {"type": "broadcast", "message": 5, "msg_id": 3}})
    msgs += [{"src": "c1", "dest": i, "body": {"type": "topology", "msg_id": 2, "topology": grid_topology(n)}}
             for i in ids]
    msgs.append({"src": "c2", "dest": "n0", "body": {"type": "broadcast", "message": 6, "msg_id": 4}})
    msgs += [{"src": "c3", "dest": i, "body": {"type": "read", "msg_id": 99}} for i in ids]
    reads = {r["src"]: sorted(r["body"]["messages"]) for r in _run(s, msgs) if r["body"]["type"] == "read_ok"}
    assert reads["n4"] == [5, 6]
    assert all(reads[i] == [6] for i in ids if i != "n4")


# --- the front-end as shipped: default pages of 1024 slots (FLOOD engines of 16 words per node) -----
#
# A scenario is (server keywords, script, pages, check(replies, server)).  The CPU test runs it on the
# oracle engine and checks what a Maelstrom client would; the GPU twin runs the identical script through
# the HIP engine and through the oracle and compares every reply and the server's counters.

def _ids(n):
    return [f"n{i}" for i in range(n)]


def _inits(n):
    return [{"src": "c0", "dest": i, "body": {"type": "init", "msg_id": 1, "node_id": i, "node_ids": _ids(n)}}
            for i in _ids(n)]


def _topologies(n, topo, mid=2):
    return [{"src": "c1", "dest": i, "body": {"type": "topology", "msg_id": mid, "topology": topo}} for i in _ids(n)]


def _broadcast(node, v, mid):
    return {"src": "c2", "dest": node, "body": {"type": "broadcast", "message": v, "msg_id": mid}}


def _reads(n, mid=99):
    return [{"src": "c3", "dest": i, "body": {"type": "read", "msg_id": mid}} for i in _ids(n)]


def _read_sets(replies):
    """per read_ok reply, in order: (node, sorted messages)"""
    return [(r["src"], sorted(r["body"]["messages"])) for r in replies if r["body"]["type"] == "read_ok"]


def _all_hold(values):
    def check(replies, server):
        reads = _read_sets(replies)
        assert reads and all(got == sorted(set(values)) for _, got in reads)
    return check


def _many(n, count, first=10_000):
    values = [(f"n{i % n}", first + 7 * i) for i in range(count)]
    return _script(n, values), _all_hold([v for _, v in values])


def _scenario_cluster25():
    values = [("n0", 1000), ("n24", -7), ("n12", 42), ("n0", 1000)]
    return _script(25, values), _all_hold([1000, -7, 42])


def _scenario_before_topology():
    n = 9
    msgs = _inits(n) + [_broadcast("n4", 5, 3)] + _topologies(n, grid_topology(n)) + [_broadcast("n0", 6, 4)]

    def check(replies, server):
        reads = dict(_read_sets(replies))
        assert reads["n4"] == [5, 6] and all(reads[i] == [6] for i in _ids(n) if i != "n4")
    return msgs + _reads(n), check


def _scenario_repeated_value():
    """The same value again at its node, at another node, and after other values (dedupe, main.go:113)."""
    n = 9
    sends = [("n0", 11), ("n0", 11), ("n8", 11), ("n3", -4), ("n5", 11), ("n3", -4), ("n7", 1 << 40)]
    msgs = _inits(n) + _topologies(n, grid_topology(n)) + [_broadcast(d, v, 10 + i) for i, (d, v) in enumerate(sends)]

    def check(replies, server):
        _all_hold([11, -4, 1 << 40])(replies, server)
        assert server.stats["broadcasts"] == len(sends) and len(server.cluster.values) == 3
    return msgs + _reads(n), check


def _scenario_reads_between_broadcasts():
    """After every broadcast a read at every node: the value is there already, with all earlier ones."""
    n, count = 9, 40
    msgs = _inits(n) + _topologies(n, grid_topology(n))
    for i in range(count):
        msgs.append(_broadcast(f"n{(5 * i) % n}", 3 * i - 50, 10 + i))
        msgs += _reads(n, 1000 + i)

    def check(replies, server):
        reads = _read_sets(replies)
        assert len(reads) == n * count
        for j, (_, got) in enumerate(reads):
            assert got == sorted(3 * i - 50 for i in range(j // n + 1))
    return msgs, check


def _scenario_second_topology():
    """A grid, three values, then a line in place of the grid, three more: every flood reaches every
    node, over the rows in force when it was sent (a 16-node line takes more rounds than the grid)."""
    n = 16
    msgs = _inits(n) + _topologies(n, grid_topology(n))
    msgs += [_broadcast(f"n{d}", v, 10 + v) for d, v in ((0, 1), (15, 2), (6, 3))] + _reads(n, 50)
    msgs += _topologies(n, line_topology(n), mid=3)
    msgs += [_broadcast(f"n{d}", v, 10 + v) for d, v in ((0, 4), (15, 5), (6, 6))] + _reads(n, 51)

    def check(replies, server):
        reads = _read_sets(replies)
        assert all(got == [1, 2, 3] for _, got in reads[:n]) and all(got == [1, 2, 3, 4, 5, 6] for _, got in reads[n:])
        # a line forwards 2 (n - 1) - 1 messages per value less the sender skips; the grid sent more
        assert server.stats["gossip_rounds"] > 3 * 7 + 2 * 16
    return msgs, check


SCENARIOS = {
    "cluster25": ({}, _scenario_cluster25, 1),
    "two_pages_1100_values": ({}, lambda: _many(9, 1100), 2),   # the second page holds 76 values
    "five_pages_of_64": ({"page_values": 64}, lambda: _many(9, 300), 5),
    "one_page_of_4096": ({"page_values": 4096}, lambda: _many(9, 2100), 1),   # slots past 2^11, word 32
    "before_topology": ({}, _scenario_before_topology, 1),
    "repeated_value": ({}, _scenario_repeated_value, 1),
    "reads_between_broadcasts": ({}, _scenario_reads_between_broadcasts, 1),
    "second_topology": ({}, _scenario_second_topology, 1),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_stdio_scenario_oracle(name):
    kw, build, pages = SCENARIOS[name]
    msgs, check = build()
    s = MaelstromServer(engine_factory=_oracle_factory, **kw)
    replies = _run(s, msgs)
    assert len(replies) == len(msgs) and not any(r["body"]["type"] == "error" for r in replies)
    assert len(s.cluster.pages) == pages and s.cluster.page_values == kw.get("page_values", 1024)
    assert s.cluster.pages[0].n_words == s.cluster.page_values // 64
    check(replies, s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_stdio_scenario_gpu(name):
    """The identical script through a MaelstromServer with the HIP engine, as shipped, and through one
    with the oracle engine: the replies are equal message for message, and so are the counters
    (broadcasts, gossip rounds, gossip messages)."""
    kw, build, pages = SCENARIOS[name]
    msgs, check = build()
    hip, ora = MaelstromServer(**kw), MaelstromServer(engine_factory=_oracle_factory, **kw)
    got, want = _run(hip, msgs), _run(ora, msgs)
    assert len(got) == len(want) == len(msgs)
    for a, b in zip(got, want):
        assert a == b
    assert hip.stats == ora.stats and hip.stats["gossip_messages"] > 0
    assert len(hip.cluster.pages) == len(ora.cluster.pages) == pages
    assert all(e.on_device for e in hip.cluster.pages) and not any(e.on_device for e in ora.cluster.pages)
    check(got, hip)
