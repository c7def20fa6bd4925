"""Deterministic ragged topologies for the FLOOD tests, and a BFS restatement of plain FLOOD.

Builders return (row_ptr, col) as uint32 arrays and use integer arithmetic only (uint64 with
wraparound, no numpy RNG), so pinned figures do not depend on the numpy version.  `flood_bfs`
restates DESIGN.md §2.4-2.6 (the reference's (*NodeState).Gossip, main.go:65-89: forward once
to Topology[self], :72, minus the sender, :73-75) by level-synchronous BFS per value; it shares
no code with oracle/.
"""
import numpy as np

_U = np.uint64


def mix(z):
    """splitmix64's finalizer over a uint64 array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> _U(30))
        z = z * _U(0xBF58476D1CE4E5B9)
        z = z ^ (z >> _U(27))
        z = z * _U(0x94D049BB133111EB)
        z = z ^ (z >> _U(31))
    return z


def _rows(N, seed, max_deg, hub_every, hub_deg):
    """(row_ptr, source u and position j of every entry, ragged's value of every entry)."""
    u = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        deg = mix(_U(2) * u + _U(seed)) % _U(max_deg)
        deg[u % _U(hub_every) == _U(1)] = _U(hub_deg)
        row_ptr = np.zeros(N + 1, dtype=np.uint64)
        row_ptr[1:] = np.cumsum(deg, dtype=np.uint64)
        src = np.repeat(u, deg.astype(np.int64))
        j = np.arange(int(row_ptr[-1]), dtype=np.uint64) - row_ptr[:-1][src.astype(np.int64)]
        far = mix((src << _U(20)) + j + (_U(seed) << _U(44))) % _U(N)
    return row_ptr, src, j, far


def ragged(N, seed, max_deg=9, hub_every=4099, hub_deg=300):
    """Directed rows of mix(2u + seed) % max_deg entries (hub_deg where u % hub_every == 1), entry j
    of row u = mix((u << 20) + j + (seed << 44)) % N: self-loops, repeated entries, empty rows and
    nodes nobody points at."""
    row_ptr, _, _, far = _rows(N, seed, max_deg, hub_every, hub_deg)
    return row_ptr.astype(np.uint32), far.astype(np.uint32)


def banded(N, seed, max_deg=9, hub_every=4099, hub_deg=300, span=64, far_every=8):
    """ragged's degrees; entry j of row u lies within span after u, except every far_every-th,
    which keeps ragged's value: contiguous blocks (partitions) cut few of the edges."""
    row_ptr, src, j, far = _rows(N, seed, max_deg, hub_every, hub_deg)
    with np.errstate(over="ignore"):
        near = (src + _U(1) + mix((src << _U(20)) + j + (_U(seed + 1) << _U(44))) % _U(span)) % _U(N)
    col = np.where(j % _U(far_every) == _U(far_every - 1), far, near)
    return row_ptr.astype(np.uint32), col.astype(np.uint32)


def _sources(row_ptr, N):
    return np.repeat(np.arange(N, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))


def symmetrize(row_ptr, col, N, every=1):
    """Row u = its own list in order, then every v that lists u, in ascending v, one entry per
    listing (repeated entries and self-loops stay).  every > 1: only the rows u % every == 0 get
    the listings back, so the other nodes hear from nodes they do not send to as well as from
    nodes they do (the sender skip, main.go:73, then depends on which of them was first)."""
    src = _sources(row_ptr, N)
    dst = col.astype(np.int64)
    back = dst % every == 0
    s2 = np.concatenate([src, dst[back]])
    d2 = np.concatenate([dst, src[back]])
    order = np.argsort(s2, kind="stable")
    rp = np.zeros(N + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(s2, minlength=N))
    return rp.astype(np.uint32), d2[order].astype(np.uint32)


def dedupe(row_ptr, col, N):
    """Every row as a sorted set."""
    key = np.unique(_sources(row_ptr, N) * N + col.astype(np.int64))
    rp = np.zeros(N + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(key // N, minlength=N))
    return rp.astype(np.uint32), (key % N).astype(np.uint32)


def flood_bfs(row_ptr, col, N, injects, R, rounds=None):
    """Plain FLOOD, per value by level-synchronous BFS over rows as sets.

    dist = BFS distance from the value's origins; the first sender of v is its lowest-id
    in-neighbour at dist(v) - 1; round t sends, over the v with dist(v) = t, deg(v) messages minus
    one where v's first sender is in Adj(v); after round t value x is held by the nodes with
    dist <= t + 1.  Returns the per-round list of (messages, infected[R]), ending at convergence
    or with the first round that sends nothing — or after exactly `rounds` rounds, when given
    (for a subset of the values of a longer run)."""
    key = np.unique(_sources(row_ptr, N) * N + col.astype(np.int64))  # edges u -> v as u * N + v
    src, dst = key // N, key % N
    deg = np.bincount(src, minlength=N)
    big = np.iinfo(np.int64).max
    sent = {}                                   # round -> messages
    level = np.zeros((0, R), dtype=np.int64)    # level[d, x] = nodes at distance d of value x
    far = np.zeros(N, dtype=np.int64)           # per node, max over values of dist (big: never)
    for x in range(R):
        origins = sorted({n for n, r in injects if r == x})
        dist = np.full(N, -1, dtype=np.int64)
        dist[origins] = 0
        front = np.zeros(N, dtype=bool)
        front[origins] = True
        skipped = np.zeros(N, dtype=np.int64)   # 1 where the node's first sender is in its own row
        d = 0
        while front.any():
            if level.shape[0] <= d:
                level = np.vstack([level, np.zeros((1, R), dtype=np.int64)])
            level[d, x] = int(front.sum())
            sent[d] = sent.get(d, 0) + int((deg[front] - skipped[front]).sum())
            e = front[src] & (dist[dst] < 0)
            first = np.full(N, big, dtype=np.int64)
            np.minimum.at(first, dst[e], src[e])
            new = first != big
            v = np.nonzero(new)[0]
            skipped[v] = np.isin(v * N + first[v], key)
            d += 1
            dist[v] = d
            front = new
        far = np.maximum(far, np.where(dist < 0, big, dist))
    held = np.cumsum(level, axis=0)
    out, t = [], 0
    while True:
        inf = held[min(t + 1, held.shape[0] - 1)] if held.shape[0] else np.zeros(R, dtype=np.int64)
        m = sent.get(t, 0)
        out.append((m, [int(c) for c in inf]))
        t += 1
        if rounds is not None:
            if t >= rounds:
                break
        elif m == 0 or bool((far <= t).all()):
            break
    return out
