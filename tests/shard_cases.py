"""Sharded-round cases shared by test_shard_states.py and test_shard_drivers.py (CPU, oracle host
shards), test_gpu_shard_states.py and test_gpu_shard_wire.py (HIP shards on one device, the Python
round bodies with the copy comm), test_gpu_group_states.py (the library's own driver, csrc/multi.hip)
and test_gpu_shard_devvalues.py (the device-value calls with no sync); WIDE, the shards of 16 and 64
words per node, by test_wide_state.py and test_gpu_wide_state.py.  A plain module in the style
of states.py and ae_cases.py: tables and helpers, no tests.

  SLOTS / SLOTS_CC   the 8-slot plan carousel: every slot sets all six plan knobs, so a round's kind
                     is a function of the table and of what ran before it (expected_kinds);
  RUNS / PHILOX      the carousel runs, taken from test_state_builders.ROUNDS (hand-built states of
                     N0 nodes) plus one Philox run with shards of more than one 16384-node tile;
  SHAPES / register  runs of any other shape: a run whose first field is registered names its own
                     (N, R) and builder (tests/shard_sizes.py: shard edges on and beside the units);
  LockstepDriver, GroupDriver, OrderedDevDriver
                     who runs a round: sharded._round with the copy comm, gossip_group_step, or
                     sharded._round with OrderedDevComm (every copy a torch op on the engines' stream,
                     counts and partials through the *_dev calls, no sync in the comm);
  RecordingComm      the copy comm of gossip_hip.sharded with a copy of every collective's send
                     buffers, counts and receive buffers, per rank (RecordingOrderedComm: the same
                     over OrderedDevComm);
  wire / ref_wire    what a round put on the wire, normalised, and the same from S_t alone in numpy
                     (peers and lost edges from oracle/numpy_ref.py; the oracle's sharded code is
                     not used there: it is the second check).

Every reference is exact: the comparisons have no tolerance.
"""
import collections
import functools

import numpy as np
import torch

import numpy_ref as nr
import oracle_py as op
import states as st
import topologies as tp
from gossip_hip import sharded
from gossip_hip.engine import Group, loss_threshold
from gossip_hip.sharded import (CLASSCODED, DENSE, EXCHANGE, REP, REP_CLASSCODED, REP_GATHER, SPARSE, _CopyComm,
                                _width)
from states import N0, SEED
from test_state_builders import ROUNDS

NO_PUSH, NO_PULL = 1 << 30, 1 << 31  # include/gossip_shard.h GOSSIP_XD_NO_PUSH / GOSSIP_XD_NO_PULL
KNOBS = ("sparse_frac", "alld_frac", "replicate", "xd_shards", "cc_frac", "xd_filter_frac")


def _slot(sparse_frac, alld_frac, replicate, xd_shards, cc_frac, xd_filter_frac):
    return dict(zip(KNOBS, (sparse_frac, alld_frac, replicate, xd_shards, cc_frac, xd_filter_frac)))


# (name, knobs): S D R r X C S X
SLOTS = [
    ("sparse", _slot(1.0, 1e30, 0, 0, 0, 0.6)),
    ("dense", _slot(-1, 1 / 128, 0, 0, 0, 0.6)),
    ("rep", _slot(-1, 1 / 128, 1, 0, 0, 0.6)),
    ("rep", _slot(-1, 1 / 128, 1, 0, 0, 0.6)),
    ("exchange", _slot(-1, 1 / 128, 0, 2, 0, 0.6)),
    ("classcoded", _slot(-1, 1 / 128, 0, 0, 1, 0.6)),
    ("sparse_alld", _slot(1.0, 0, 0, 0, 0, 0.6)),
    ("exchange_unfiltered", _slot(-1, 1 / 128, 0, 2, 0, 1.0)),
]
# the first rep slot enters replication over the class-coded all-gather (kind 7)
SLOTS_CC = [(n, dict(p, cc_frac=1) if i == 2 else p) for i, (n, p) in enumerate(SLOTS)]
_SLOT_KIND = {"sparse": SPARSE, "sparse_alld": SPARSE, "dense": DENSE, "exchange": EXCHANGE,
              "exchange_unfiltered": EXCHANGE, "classcoded": CLASSCODED}
ALL_KINDS = {DENSE, SPARSE, EXCHANGE, CLASSCODED, REP_GATHER, REP}

# (builder, mode, k, edge_loss, partitions), each a key of test_state_builders.ROUNDS, where "converges
# within 64 rounds" and the round count are pinned on the oracle alone
RUNS = [("clustered", "push", 1, 0, 0), ("thirds", "push", 1, 0, 0), ("thirds", "pushpull", 2, 1 << 31, 2),
        ("holes", "push", 1, 0, 0), ("disjoint", "pushpull", 2, 0, 0)]
assert all(r in ROUNDS for r in RUNS)
# inject_random at 100003 nodes, 64 rumors, G = 5: Nl = 20001 is more than one 16384-node tile, the
# last shard owns 19999
PHILOX = ("philox", "pushpull", 2, 0, 0)
PHILOX_N, PHILOX_G = 100003, 5
GS = (2, 3, 4, 5)  # G = 3: no ragged shard (16449 = 3 x 5483, and 5483 is no multiple of 64)
OFFSETS = tuple(range(8))

# multi-word shards (W > 1: every round the plain state all-gather): (N, R, mode, k, G, faults, rounds or
# None = to convergence)
MULTIWORD = [
    (12, 130, "push", 1, 5, {}, None),
    (N0, 129, "pull", 2, 4, {}, None),
    # never converges (partitions): a fixed number of rounds
    (30011, 65, "pushpull", 3, 3, dict(edge_loss=loss_threshold(0.1), partitions=3, stall_rounds=3), 12),
]
MULTIWORD_IDS = [f"N{c[0]}-R{c[1]}-{c[2]}-G{c[4]}" for c in MULTIWORD]

# wide multi-word shards (test_gpu_wide_state.py): the same tuple plus the workload, "random" (inject_random),
# "sparse" (states.sparse_words: most words of every node empty) or "flood" (ragged rows, one value in each of
# 200 slots spread over all words).  1024 rumors (W = 16) at G = 3 with a ragged Nl (1001, 1001, 999 nodes);
# 4096 rumors (W = 64) at G = 5 with a ragged last shard (201 x 4 + 199) and with an empty one: only N < 20
# leaves the fifth shard nothing (16 nodes: 4, 4, 4, 4, 0)
WIDE_NODES = 3001
WIDE = [
    (WIDE_NODES, 1024, "push", 2, 3, {}, None, "random"),
    (16, 4096, "pull", 1, 5, {}, None, "random"),
    (1003, 4096, "pull", 3, 5, {}, 6, "sparse"),
    (WIDE_NODES, 1024, "flood", 0, 3, {}, 9, "flood"),  # the ninth round sends nothing
    (WIDE_NODES, 1024, "pushpull", 2, 3, dict(edge_loss=loss_threshold(0.2), partitions=3, stall_rounds=3), 10,
     "sparse"),
    (1003, 4096, "push", 2, 5, dict(edge_loss=loss_threshold(0.2), partitions=2, stall_rounds=2), 8, "random"),
]
WIDE_IDS = [f"N{c[0]}-R{c[1]}-{c[2]}-G{c[4]}-{c[7]}" + ("-faults" if c[5] else "") for c in WIDE]


@functools.lru_cache(maxsize=None)
def wide_topology():
    """Symmetrised ragged rows over WIDE_NODES nodes: hubs of 40 entries at 1, 1025 and 2049, empty rows,
    self-loops and repeated entries."""
    return tp.symmetrize(*tp.ragged(WIDE_NODES, 7, hub_every=1024, hub_deg=40), WIDE_NODES)


def fill_work(engine, work, R):
    """Builds one engine's (or one shard's) state for a workload of WIDE."""
    if work == "random":
        engine.inject_random()
    elif work == "sparse":
        st.sparse_words(engine, R)
    else:
        engine.set_topology(wide_topology())
        for i in range(200):
            x = i * (R - 1) // 199
            engine.inject((431 * x + 3) % engine.n_nodes, x)


def run_id(run):
    return "-".join(str(x) for x in run)


# runs that name their own shape and builder (tests/shard_sizes.py): run[0] -> (N, R, build(engine))
SHAPES = {}


def register(name, N, R, build):
    """Makes `name` the first field of runs of N nodes and R rumors whose state is build(engine); the
    name must say everything the state depends on, since reference() is cached by the run."""
    assert name != "philox" and name not in st.BUILDERS and SHAPES.get(name, (N, R))[:2] == (N, R)
    SHAPES[name] = (N, R, build)
    return name


def run_shape(run):
    """(N, R) of a run"""
    if run[0] in SHAPES:
        return SHAPES[run[0]][:2]
    return (PHILOX_N, 64) if run[0] == "philox" else (N0, st.BUILDERS[run[0]][1])


def build_state(engine, run):
    if run[0] in SHAPES:
        SHAPES[run[0]][2](engine)
    elif run[0] == "philox":
        engine.inject_random()
    else:
        b, R = st.BUILDERS[run[0]]
        b(engine, R)


def make_engines(factory, run, G, flags=0, params=None, seed=SEED):
    """G shard engines (G = 1: one engine) of a run, built; factory: Engine or op.OracleEngine."""
    _, mode, k, loss, parts = run
    N, R = run_shape(run)
    if G == 1:
        engines = [factory(N, R, mode, k, seed, flags=1 | flags, edge_loss=loss, partitions=parts)]
    else:
        engines = [factory(N, R, mode, k, seed, flags=1 | flags, shard_rank=r, shard_count=G, edge_loss=loss,
                           partitions=parts, params=params) for r in range(G)]
    for e in engines:
        build_state(e, run)
    return engines


def close_all(engines):
    for e in engines:
        e.close()


@functools.lru_cache(maxsize=None)
def _reference(run, seed=SEED):
    (ref,) = make_engines(op.OracleEngine, run, 1, seed=seed)
    states, stats, infected = [ref.read_shard()[0].copy()], [], []
    for _ in range(64):
        res = ref.step(1)
        stats.append(res.stats[0])
        infected.append(res.infected[0].copy())
        states.append(ref.read_shard()[0].copy())
        if res.converged:
            break
    for s in states + infected:
        s.setflags(write=False)
    assert seed != SEED or len(stats) == ROUNDS.get(run, len(stats))
    return tuple(states), tuple(stats), tuple(infected)


def reference(run, seed=SEED):
    """One oracle engine over a run, a round at a time until it converges (at most 64 rounds):
    (S_0 .. S_T as read-only [N] uint64 arrays, the per-round stats).  Computed once, shared."""
    return _reference(run, seed)[:2]


def reference_infected(run, seed=SEED):
    """The same run's per-rumor node counts after every round ([R] uint64 each), as gossip_step and
    gossip_group_step hand them out beside the stats."""
    return _reference(run, seed)[2]


# -- the carousel -----------------------------------------------------------------------------

def expected_kinds(table, offset, rounds, whole=False):
    """The kind of each of `rounds` rounds from slot `offset` on.  A rep slot enters replication
    (kind 5, or 7 where its cc_frac is 1) when the image is not whole: the previous round was not
    replicated, or an inject or reset came since (whole=False at the start); else it is kind 6."""
    kinds = []
    for i in range(rounds):
        name, knobs = table[(offset + i) % len(table)]
        if name == "rep":
            kinds.append(REP if whole else REP_CLASSCODED if knobs["cc_frac"] == 1 else REP_GATHER)
            whole = True
        else:
            kinds.append(_SLOT_KIND[name])
            whole = False
    return kinds


def set_knobs(engines, knobs):
    for e in engines:
        for name, value in knobs.items():
            e.set_param(name, value)


def drive_round(engines, comm, kinds=None):
    """One round through the product's round bodies (sharded._round): host and device engines alike.
    Returns the stats every shard agreed on."""
    _, stats = sharded._round(engines, comm, kinds)
    assert all(s == stats[0] for s in stats)
    return stats[0]


def carousel(driver, table, offset, rounds, after_round=None):
    """`rounds` rounds (fewer if the run converges), round i with the knobs of slot offset + i set on
    every shard.  after_round(i, kind, knobs): called after each round.  Returns (per-round stats,
    kinds)."""
    stats, kinds = [], []
    for i in range(rounds):
        knobs = table[(offset + i) % len(table)][1]
        set_knobs(driver.engines, knobs)
        st_, kind = driver.round()
        stats.append(st_)
        kinds.append(kind)
        if after_round is not None:
            after_round(i, kind, knobs)
        if st_["converged"]:
            break
    return stats, kinds


def assert_shards_hold(engines, state):
    """every shard's words are its slice of the [N] reference state"""
    for e in engines:
        assert np.array_equal(e.read_shard()[0], state[e.lo:e.hi]), f"shard {e.cfg.shard_rank}"


# -- the recording comm -----------------------------------------------------------------------

class OrderedDevComm(_CopyComm):
    """Stands in for RCCL's ordering on one device: every engine launches on torch's current stream
    (OrderedDevDriver binds them), every slice copy is a torch op on that stream, and nothing here
    synchronizes.  Counts and partials come from engine.<stem>_dev where the library has that form:
    the published device values are combined on the device and read with one .cpu(), the only host
    wait of that exchange (as in gossip_hip.sharded._Comm.dev_*).  Host engines (the oracle's) have
    no *_dev calls and take the host forms, so the comm can be rehearsed on the CPU.  self.called
    counts the engine calls made, by name (stem + "_dev" or the bare stem)."""

    direct = True

    def __init__(self, engines):
        super().__init__(engines)
        self.called = collections.Counter()

    def _sync(self):  # never: the copies and the engines' kernels are ordered by the one stream
        pass

    def all_gather_async(self, recv, send, nbytes: int):
        """Enqueued at once, before the engines' own-slice kernels (the order RCCL's launch has)."""
        self.all_gather(recv, send, nbytes)
        return None

    def wait(self, work):
        pass

    def _values(self, L, stem, *args, each=None):
        """(every engine's results, whether their last one is a pointer to device values)"""
        dev = all(e.on_device and e.supports(stem + "_dev") for e in L)
        name = stem + "_dev" if dev else stem
        self.called[name] += 1
        return sharded._calls(L, name, *args, each=each), dev

    def _read(self, ptrs, n):
        """[len(ptrs), n] int64 on the device from n values at each pointer (no host wait yet)"""
        return torch.stack(self._views(ptrs, [n * 8] * len(ptrs)))

    def gather_counts(self, L, stem: str):
        res, dev = self._values(L, stem)
        if not dev:
            return [r[:-1] for r in res], [r[-1] for r in res]
        counts = self._read([r[-1] for r in res], 1).cpu()
        return [r[:-1] for r in res], [int(c) for c in counts[:, 0]]

    def exchange_counts(self, L, stem: str, *args):
        res, dev = self._values(L, stem, *args)
        if dev:
            counts = [[int(c) for c in row] for row in self._read([r[-1] for r in res], self.world).cpu()]
        else:
            counts = [[int(c) for c in r[-1]] for r in res]
        return [r[:-1] for r in res], counts, [[c[r] for c in counts] for r in range(self.world)]

    def sum(self, L, stem: str, each=None) -> np.ndarray:
        parts, dev = self._values(L, stem, each=each)
        if dev:  # the all-reduce: an int64 sum on the device wraps like RCCL's
            return self._read(parts, L[0].partial_len()).sum(dim=0).cpu().numpy().view(np.uint64)
        tot = np.zeros_like(parts[0])
        for p in parts:
            tot = tot + p
        return tot


class _Recording:
    """Mixin over a copy comm, keeping for every collective of a round a copy of what each rank sent,
    the counts, and what each rank received: self.log has one entry per collective, in the order the
    round body issued them, with per-rank payloads (uint64 words, uint32 for the exchange ids).  It
    waits for the device before it copies a buffer (it records); the comm under it is left as it is."""

    def __init__(self, engines):
        super().__init__(engines)
        self.log = []

    def _grab(self, ptrs, nbytes, width=8):
        for d in {e.device for e in self.engines if e.on_device}:
            torch.cuda.synchronize(d)
        ut = np.uint64 if width == 8 else np.uint32
        return [v.cpu().numpy().copy().view(ut) for v in self._views(ptrs, nbytes, width)]

    def take(self):
        log, self.log = self.log, []
        return log

    def all_gather(self, recv, send, nbytes):  # (all_gather_async of the copy comm ends here too)
        G = self.world
        sent = self._grab(send, [nbytes] * G)
        super().all_gather(recv, send, nbytes)
        self.log.append(dict(op="all_gather", nbytes=nbytes, send=sent, recv=self._grab(recv, [nbytes * G] * G)))

    def all_to_all(self, recv, send, recv_counts, send_counts, item_bytes):
        width = _width(item_bytes)
        sent = self._grab(send, [sum(c) * item_bytes for c in send_counts], width)
        super().all_to_all(recv, send, recv_counts, send_counts, item_bytes)
        got = self._grab(recv, [sum(c) * item_bytes for c in recv_counts], width)
        self.log.append(dict(op="all_to_all", item_bytes=item_bytes, send=sent, recv=got,
                             send_counts=[[int(x) for x in c] for c in send_counts],
                             recv_counts=[[int(x) for x in c] for c in recv_counts]))

    def gather_counts(self, L, stem):
        head, counts = super().gather_counts(L, stem)
        self.log.append(dict(op="counts", stem=stem, counts=[int(c) for c in counts]))
        return head, counts

    def exchange_counts(self, L, stem, *args):
        head, counts, in_counts = super().exchange_counts(L, stem, *args)
        self.log.append(dict(op="counts", stem=stem, counts=[list(c) for c in counts]))
        return head, counts, in_counts


class RecordingComm(_Recording, _CopyComm):
    """The recording copy comm of gossip_hip.sharded."""


class RecordingOrderedComm(_Recording, OrderedDevComm):
    """The recording comm over the device-value path."""


# -- who runs a round -------------------------------------------------------------------------
# A driver has `engines` (the shard views: inject, set_param, set_faults, reset, read_shard,
# state_hash), round() -> (the stats every shard agreed on, the round's kind), close(), and
# `infected`: the per-rumor counts of the last round where the driver hands them out, else None.
# Every driver is made as driver(factory, N, R, mode, k, seed, G, flags=, params=, **faults) with
# its shards empty; the bodies build the state through `engines`.

PLAN_LETTERS = "DSAXCRrQ"  # csrc/engine.hip gossip_sharded_plan: the plan string's letter of kind i


class LockstepDriver:
    """The product's round bodies (sharded._round) over the copy comm, on shards made by `factory`
    (Engine or op.OracleEngine)."""

    comm_class, recording_class = _CopyComm, RecordingComm
    infected = None

    def __init__(self, factory, N, R, mode, k, seed, G, flags=0, params=None, recording=False, **faults):
        self.engines = [factory(N, R, mode, k, seed, flags=flags, shard_rank=r, shard_count=G, params=params, **faults)
                        for r in range(G)]
        self.comm = (self.recording_class if recording else self.comm_class)(self.engines)

    def round(self):
        kinds = []
        stats = drive_round(self.engines, self.comm, kinds)
        return stats, kinds[0]

    def close(self):
        close_all(self.engines)


class OrderedDevDriver(LockstepDriver):
    """The same round bodies over OrderedDevComm: device engines are bound to torch's current stream
    and run with ordered_collectives = 1 for the duration of each round (as sharded_round does for
    RCCL), so no call of the round synchronizes to publish a buffer or a value.  Host engines run
    unbound: the rehearsal of the comm on the CPU."""

    comm_class, recording_class = OrderedDevComm, RecordingOrderedComm

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.device_engines = [e for e in self.engines if e.on_device]
        self.ordered = {}  # engine rank -> the last ordered_collectives value this driver set

    def _ordered(self, value):
        for e in self.device_engines:
            e.set_param("ordered_collectives", value)
            self.ordered[e.cfg.shard_rank] = value

    def round(self):
        for e in self.device_engines:
            e.set_stream(torch.cuda.current_stream().cuda_stream)
        self._ordered(1)
        try:
            return super().round()
        finally:  # the flag must not outlive the round that bound the stream
            self._ordered(0)

    def release(self):
        """Hands the engines back to a host driver: no flag left, bound to the null stream."""
        self._ordered(0)
        for e in self.device_engines:
            e.set_stream(0)

    def close(self):
        self.release()
        super().close()


class GroupDriver:
    """The library's own driver (csrc/multi.hip behind gossip_group_step): a gossip_hip.Group of G
    shards on device 0 over the copy transport, a round = group.step(1).  The kind of the round just
    run is the last letter of every shard's plan string (gossip_plan_model; the string restarts at
    round 0 after a reset, so only its last letter is read), and every shard's count of planned
    rounds must have gone up by one, so a stale letter cannot pass.  Multi-word shards have no
    planner (every round is the state all-gather): their plan string stays empty."""

    def __init__(self, factory, N, R, mode, k, seed, G, flags=0, params=None, **faults):
        assert factory is None, "the group makes its own engines"
        self.group = Group(N, R, mode, k, seed, flags=flags, n_shards=G, devices=[0] * G, transport=2, params=params,
                           **faults)
        assert self.group.transport == 2
        self.engines = self.group.shards
        self.infected = None
        self.planned = [e.plan_model()[2] for e in self.engines]

    def _kind(self):
        models = [e.plan_model() for e in self.engines]
        if self.engines[0].n_words > 1:
            assert all(m[2] == 0 and m[3] == "" for m in models)
            return DENSE
        planned = [m[2] for m in models]
        assert planned == [p + 1 for p in self.planned], "not one planned round per shard"
        self.planned = planned
        letters = {m[3][-1] for m in models}
        assert len(letters) == 1, f"shards report different kinds: {letters}"
        return PLAN_LETTERS.index(letters.pop())

    def round(self):
        res = self.group.step(1)
        assert res.rounds == 1
        self.infected = res.infected[0]
        return res.stats[0], self._kind()

    def close(self):
        self.group.close()


def open_driver(driver, factory, run, G, flags=0, params=None, seed=SEED, **kw):
    """The driver (None: LockstepDriver) over the G shards of a run, built."""
    _, mode, k, loss, parts = run
    N, R = run_shape(run)
    d = (driver or LockstepDriver)(factory, N, R, mode, k, seed, G, flags=1 | flags, params=params, edge_loss=loss,
                                   partitions=parts, **kw)
    try:
        for e in d.engines:
            build_state(e, run)
    except BaseException:
        d.close()
        raise
    return d


def run_to_convergence(driver, max_rounds):
    """sharded.lockstep_run through a driver: (per-round stats, kinds)"""
    stats, kinds = [], []
    for _ in range(max_rounds):
        st_, kind = driver.round()
        stats.append(st_)
        kinds.append(kind)
        if st_["converged"]:
            break
    return stats, kinds


def assert_infected(driver, want):
    """the last round's per-rumor counts, where the driver hands them out"""
    if driver.infected is not None:
        assert np.array_equal(driver.infected, want), "per-rumor counts"


def _sorted_rows(a, b):
    """rows (a[i], b[i]) as a [n, 2] uint64 array in lexicographic order: a multiset"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    order = np.lexsort((b, a))
    return np.stack([a[order], b[order]], axis=1)


def _split(flat, counts):
    """the per-owner groups of one rank's send buffer (rows), owner q first"""
    at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [flat[at[q]:at[q + 1]] for q in range(len(counts))]


def wire(kind, log):
    """What one round put on the wire, from the RecordingComm log of that round, normalised so that two
    implementations and the numpy reference compare with == (groups whose order is not defined are
    sorted).  Keys by kind:
      SPARSE      rare_counts [G]; rare: per rank its [count, 2] items {global id, S_t};
                  msgs: {(sender, owner): sorted [n, 2] rows {node at owner, delta}} (non-empty groups)
      EXCHANGE    class_bytes; classes: per rank its own slot words (None without the all-gather);
                  items: {(sender, owner): sorted rows {id | flags, value}}; recv_ids: per rank the
                  ids it received, in the received order; replies: per rank what it sent back
      CLASSCODED, REP_CLASSCODED   cc_counts [G]; cc_bytes; cc_bits: per rank its slot words;
                  cc_vals: per rank its mixed words in id order
      DENSE, REP_GATHER            slices: per rank the S_t words it sent;  REP: nothing."""
    G = None
    out = {}
    log = list(log)
    if kind == SPARSE:
        c = log.pop(0)
        assert c["op"] == "counts" and c["stem"] == "sparse_rare"
        counts = out["rare_counts"] = c["counts"]
        G = len(counts)
        if max(counts):
            g = log.pop(0)
            assert g["op"] == "all_gather" and g["nbytes"] == 16 * max(counts)
            out["rare"] = [g["send"][q].reshape(-1, 2)[:counts[q]] for q in range(G)]
            for r in range(G):  # every rank received every list
                for q in range(G):
                    got = g["recv"][r].reshape(G, -1, 2)[q, :counts[q]]
                    assert np.array_equal(got, out["rare"][q])
        else:
            out["rare"] = [np.zeros((0, 2), np.uint64)] * G
        c = log.pop(0)
        assert c["op"] == "counts" and c["stem"] == "sparse_scan"
        a = log.pop(0)
        assert a["op"] == "all_to_all" and a["item_bytes"] == 16 and a["send_counts"] == c["counts"]
        out["msgs"] = {}
        for r in range(G):
            for q, grp in enumerate(_split(a["send"][r].reshape(-1, 2), c["counts"][r])):
                if len(grp):
                    out["msgs"][(r, q)] = _sorted_rows(grp[:, 0], grp[:, 1])
        assert not log
    elif kind == EXCHANGE:
        out["class_bytes"], out["classes"] = 0, None
        if log[0]["op"] == "all_gather":
            g = log.pop(0)
            out["class_bytes"], out["classes"] = g["nbytes"], g["send"]
        c = log.pop(0)
        assert c["op"] == "counts" and c["stem"] == "xd_requests"
        G = len(c["counts"])
        ids, vals, rep = log.pop(0), log.pop(0), log.pop(0)
        assert (ids["item_bytes"], vals["item_bytes"], rep["item_bytes"]) == (4, 8, 8) and not log
        assert ids["send_counts"] == vals["send_counts"] == c["counts"] == rep["recv_counts"]
        out["items"] = {}
        for r in range(G):
            gi, gv = _split(ids["send"][r], c["counts"][r]), _split(vals["send"][r], c["counts"][r])
            for q in range(G):
                if len(gi[q]):
                    out["items"][(r, q)] = _sorted_rows(gi[q], gv[q])
        out["recv_ids"] = ids["recv"]
        out["replies"] = rep["send"]
        # the all-to-all back returns every reply to the sender of its item
        assert [len(x) for x in rep["send"]] == [len(x) for x in ids["recv"]]
    elif kind in (CLASSCODED, REP_CLASSCODED):
        c = log.pop(0)
        assert c["op"] == "counts" and c["stem"] == "cc_send"
        counts = out["cc_counts"] = c["counts"]
        G = len(counts)
        g = log.pop(0)
        assert g["op"] == "all_gather"
        out["cc_bytes"], out["cc_bits"] = g["nbytes"], g["send"]
        if max(counts):
            v = log.pop(0)
            assert v["op"] == "all_gather" and v["nbytes"] == 8 * max(counts)
            out["cc_vals"] = [v["send"][q][:counts[q]] for q in range(G)]
        else:
            out["cc_vals"] = [np.zeros(0, np.uint64)] * G
        assert not log
    elif kind in (DENSE, REP_GATHER):
        (g,) = log
        out["slices"] = g["send"]
    else:
        assert kind == REP and not log
    return out


# -- numpy references of the wire products ----------------------------------------------------

def full_mask(R):
    return np.uint64((1 << R) - 1) if R < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)


def shard_geometry(N, G):
    """(Nl, [lo of every rank], [nodes owned]): contiguous shards of ceil(N / G) nodes"""
    Nl = -(-N // G)
    lo = [min(q * Nl, N) for q in range(G)]
    return Nl, lo, [min(N, l + Nl) - l for l in lo]


@functools.lru_cache(maxsize=64)
def _edges(seed, N, k, loss, parts, t):
    """(peers [N, k], live [N, k]) of round t, from oracle/numpy_ref.py"""
    P = nr.peers(seed, N, t, k).astype(np.int64)
    n = np.arange(N, dtype=np.int64)
    lost = np.stack([nr.edge_lost(seed, N, loss, parts, n, P[:, j], t, j) for j in range(k)], axis=1)
    P.setflags(write=False)
    return P, ~lost


def _bitmap(bits):
    """bit i of word w = bits[64 w + i]; len(bits) a multiple of 64"""
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def dense_filter(S, N, R, mode, k, frac):
    """The class filter of an exchange round, restated from the exact global totals of S_t: bit 0 drops
    pull-only edges into empty peers once more than frac of the nodes are empty, bit 1 push-only edges
    into full peers once more than frac are full; fanouts above 8 never filter."""
    if k > 8:
        return 0
    nz, full = int((S != 0).sum()), int((S == full_mask(R)).sum())
    empty_share, full_share = 1.0 - nz / N, full / N
    return (1 if mode != "push" and empty_share > frac else 0) | (2 if mode != "pull" and full_share > frac else 0)


def rare_is_not_full(S, N, R):
    """plan_choose_sparse: the rare class is not-full iff N - full < nonzero, else nonzero"""
    return N - int((S == full_mask(R)).sum()) < int((S != 0).sum())


def _groups(r, q, a, b):
    """{(sender, owner): sorted rows} of the kept edges"""
    out = {}
    if len(r) == 0:
        return out
    order = np.lexsort((b, a, q, r))
    r, q, a, b = r[order], q[order], a[order], b[order]
    key = r * (int(q.max()) + 1) + q
    cuts = np.flatnonzero(np.diff(key)) + 1
    for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(key)]])):
        out[(int(r[lo]), int(q[lo]))] = np.stack([a[lo:hi], b[lo:hi]], axis=1).astype(np.uint64)
    return out


def ref_wire(kind, S, N, G, R, mode, k, seed, t, loss=0, parts=0, xd_filter_frac=0.6):
    """The wire products of round t of the given kind from S_t ([N] uint64) alone: the keys of wire()
    that do not depend on the received order (replies: ref_replies)."""
    Nl, los, nown = shard_geometry(N, G)
    fm = full_mask(R)
    nwl = (Nl + 63) // 64
    n = np.arange(N, dtype=np.int64)
    owner = n // Nl
    out = {}

    def padded(q):
        own = np.zeros(nwl * 64, dtype=np.uint64)
        own[:nown[q]] = S[los[q]:los[q] + nown[q]]
        return own

    if kind == SPARSE:
        maj = rare_is_not_full(S, N, R)
        rare = (S != fm) if maj else (S != 0)
        majv = fm if maj else np.uint64(0)
        out["rare"] = [np.stack([n[l:l + c][rare[l:l + c]].astype(np.uint64), S[l:l + c][rare[l:l + c]]], axis=1)
                       for l, c in zip(los, nown)]
        out["rare_counts"] = [len(x) for x in out["rare"]]
        rs, qs, as_, bs = [], [], [], []
        if mode != "pull":
            P, live = _edges(seed, N, k, loss, parts, t)
            for j in range(k):
                p = P[:, j]
                v = np.where(rare[p], S[p], majv)
                delta = S & ~v
                send = live[:, j] & (rare | rare[p]) & (owner[p] != owner) & (delta != 0)
                rs.append(owner[send]); qs.append(owner[p[send]])
                as_.append(p[send] - owner[p[send]] * Nl); bs.append(delta[send])
        cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
        out["msgs"] = _groups(cat(rs, np.int64), cat(qs, np.int64), cat(as_, np.uint64), cat(bs, np.uint64))
    elif kind == EXCHANGE:
        filt = dense_filter(S, N, R, mode, k, xd_filter_frac)
        out["class_bytes"] = 2 * nwl * 8 if filt else 0
        out["classes"] = None
        if filt:
            out["classes"] = [np.concatenate([_bitmap(padded(q) != 0), _bitmap(padded(q) == fm)]) for q in range(G)]
        push = (S != 0) if mode != "pull" else np.zeros(N, dtype=bool)
        pull = (S != fm) if mode != "push" else np.zeros(N, dtype=bool)
        P, live = _edges(seed, N, k, loss, parts, t)
        rs, qs, as_, bs = [], [], [], []
        for j in range(k):
            p = P[:, j]
            keep = live[:, j] & (push | pull)
            if filt & 1:
                keep &= ~(~push & pull & (S[p] == 0))
            if filt & 2:
                keep &= ~(push & ~pull & (S[p] == fm))
            ids = (p - owner[p] * Nl) | np.where(push, 0, NO_PUSH) | np.where(pull, 0, NO_PULL)
            rs.append(owner[keep]); qs.append(owner[p[keep]])
            as_.append(ids[keep].astype(np.uint64)); bs.append(np.where(push, S, np.uint64(0))[keep])
        out["items"] = _groups(np.concatenate(rs), np.concatenate(qs), np.concatenate(as_), np.concatenate(bs))
    elif kind in (CLASSCODED, REP_CLASSCODED):
        out["cc_bytes"] = (2 * nwl + (nwl + 1) // 2) * 8  # cc_slot_words
        out["cc_bits"], out["cc_vals"] = [], []
        for q in range(G):
            own = padded(q)
            nz, full = own != 0, own == fm
            mixed = nz & ~full
            pre = np.zeros(2 * ((nwl + 1) // 2), dtype=np.uint32)
            per_word = mixed.reshape(nwl, 64).sum(axis=1)
            nwo = (nown[q] + 63) // 64  # the prefix of the words that hold an own node; the rest zero
            pre[:nwo] = (np.cumsum(per_word) - per_word)[:nwo]
            out["cc_bits"].append(np.concatenate([_bitmap(nz), _bitmap(full), pre.view(np.uint64)]))
            out["cc_vals"].append(own[mixed])
        out["cc_counts"] = [len(v) for v in out["cc_vals"]]
    elif kind in (DENSE, REP_GATHER):
        out["slices_own"] = [S[l:l + c] for l, c in zip(los, nown)]
    return out


def ref_replies(S, N, G, recv_ids):
    """Per rank, the reply to every received item in the received order: S_t of the node, 0 for an
    item flagged NO_PULL (gossip_shard.h)."""
    _, los, _ = shard_geometry(N, G)
    out = []
    for q, ids in enumerate(recv_ids):
        node = los[q] + (ids.astype(np.int64) & (NO_PUSH - 1))
        out.append(np.where(ids & np.uint32(NO_PULL), np.uint64(0), S[np.minimum(node, N - 1)]))
    return out


def _same_groups(got, want, what):
    assert sorted(got) == sorted(want), f"{what}: (sender, owner) groups differ"
    for key in want:
        assert got[key].shape == want[key].shape, f"{what} {key}: {len(got[key])} items, {len(want[key])} expected"
        assert np.array_equal(got[key], want[key]), f"{what} {key}"


def _same_lists(got, want, what):
    assert len(got) == len(want)
    for q, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what} of rank {q}"


def assert_wire_equal(kind, got, want, N, G):
    """got: wire() of a run; want: ref_wire() or another run's wire()."""
    _, _, nown = shard_geometry(N, G)
    if kind == SPARSE:
        assert got["rare_counts"] == want["rare_counts"]
        _same_lists(got["rare"], want["rare"], "rare list")
        _same_groups(got["msgs"], want["msgs"], "sparse messages")
        for (r, q), rows in got["msgs"].items():  # never to the own shard, in range, no empty delta
            assert r != q and int(rows[:, 0].max()) < nown[q] and int(rows[:, 1].min()) != 0
    elif kind == EXCHANGE:
        assert got["class_bytes"] == want["class_bytes"]
        if want["class_bytes"]:
            _same_lists(got["classes"], want["classes"], "class bitmaps")
        _same_groups(got["items"], want["items"], "exchange items")
        for (r, q), rows in got["items"].items():
            assert int((rows[:, 0] & np.uint64(NO_PUSH - 1)).max()) < nown[q]
    elif kind in (CLASSCODED, REP_CLASSCODED):
        assert got["cc_counts"] == want["cc_counts"] and got["cc_bytes"] == want["cc_bytes"]
        _same_lists(got["cc_bits"], want["cc_bits"], "class-coded slot")
        _same_lists(got["cc_vals"], want["cc_vals"], "mixed words")
    elif kind in (DENSE, REP_GATHER):
        own = want["slices_own"] if "slices_own" in want else [s[:c] for s, c in zip(want["slices"], nown)]
        _same_lists([s[:c] for s, c in zip(got["slices"], nown)], own, "state slice")


def check_round_wire(kind, log, S, run, G, t, knobs):
    """Every wire product of one recorded round against the numpy references.  Returns wire()."""
    _, mode, k, loss, parts = run
    N, R = run_shape(run)
    got = wire(kind, log)
    want = ref_wire(kind, S, N, G, R, mode, k, SEED, t, loss, parts, knobs["xd_filter_frac"])
    assert_wire_equal(kind, got, want, N, G)
    if kind == EXCHANGE:
        _same_lists(got["replies"], ref_replies(S, N, G, got["recv_ids"]), "exchange replies")
    return got


# -- test bodies shared by the CPU file (factory = op.OracleEngine) and the GPU files (Engine) ------

def body_carousel(factory, run, G, offset, table=SLOTS, flags=0, driver=None, seed=SEED):
    """Per-round stats (and per-rumor counts where the driver has them), the kind sequence exactly as
    the table gives it, every shard's final state."""
    states, want = reference(run, seed)
    infected = reference_infected(run, seed)
    d = open_driver(driver, factory, run, G, flags, seed=seed)
    try:
        stats, kinds = carousel(d, table, offset, len(want),
                                after_round=lambda i, kind, knobs: assert_infected(d, infected[i]))
        assert stats == list(want)
        assert kinds == expected_kinds(table, offset, len(want))
        assert_shards_hold(d.engines, states[-1])
    finally:
        d.close()
    return kinds


def body_carousel_wire(factory, run, G, offset, other=None, driver=None):
    """Every wire product of every round against the numpy references; other: a second factory whose
    shards run the same carousel, every product compared with theirs too (counts per owner included).
    driver: LockstepDriver (None) or OrderedDevDriver, made with its recording comm."""
    states, want = reference(run)
    N, _ = run_shape(run)
    d = open_driver(driver, factory, run, G, recording=True)
    theirs = make_engines(other, run, G) if other else None
    try:
        comm = d.comm
        comm2 = RecordingComm(theirs) if other else None
        stats = []
        for i in range(len(want)):
            knobs = SLOTS[(offset + i) % len(SLOTS)][1]
            set_knobs(d.engines, knobs)
            st_, kind = d.round()
            stats.append(st_)
            got = check_round_wire(kind, comm.take(), states[i], run, G, i, knobs)
            if other:
                kinds2 = []
                set_knobs(theirs, knobs)
                assert drive_round(theirs, comm2, kinds2) == stats[-1] and kinds2 == [kind]
                assert_wire_equal(kind, got, wire(kind, comm2.take()), N, G)
        assert stats == list(want)
    finally:
        d.close()
        close_all(theirs or [])


def body_forced_kind(factory, run, knobs, kind, G=4, driver=None):
    """A built state before any round under one forced plan: the first round is of that kind and equals
    the oracle, then the run goes to convergence."""
    states, want = reference(run)
    infected = reference_infected(run)
    d = open_driver(driver, factory, run, G, params=knobs)
    try:
        assert d.round() == (want[0], kind)
        assert_infected(d, infected[0])
        assert_shards_hold(d.engines, states[1])
        if len(want) > 1:
            stats, kinds = run_to_convergence(d, 64)
            assert stats == list(want[1:])
            assert_infected(d, infected[-1])
            assert set(kinds) == {REP if kind == REP_GATHER else kind}
        assert_shards_hold(d.engines, states[-1])
    finally:
        d.close()


REP_PARAMS = {"sparse_frac": -1, "replicate": 1, "cc_frac": 0, "xd_shards": 0}
REP_KINDS = [5, 6, 6, 5, 6, 6, 6, 6, 6, 5, 6, 6]
REP_RUN = RUNS[1]  # thirds, push, k = 1: 11 rounds to convergence, so no chunk runs on a full state


def body_replicated_sequence(factory, params, G=4, want_kinds=None, driver=None):
    """3 rounds, eight injects, 2 rounds, set_faults(0.3, 5 partitions), 2 rounds, healed, 2 rounds, reset
    and the thirds state again, 3 rounds: stats (and per-rumor counts where the driver has them) equal
    one oracle engine's after every chunk, every shard is all zero with hash 0 right after the reset,
    the final states are equal, and the kinds so far are want_kinds' after every chunk (None: whatever
    the engine plans)."""
    (ref,) = make_engines(op.OracleEngine, REP_RUN, 1)
    d = open_driver(driver, factory, REP_RUN, G, params=params)
    engines = d.engines
    everyone = [ref] + list(engines)
    kinds = []

    def chunk(n, what):
        for _ in range(n):  # (run_to_convergence would stop at convergence)
            res = ref.step(1)
            assert not res.converged
            got, kind = d.round()
            kinds.append(kind)
            assert got == res.stats[0], what
            assert_infected(d, res.infected[0])
        assert want_kinds is None or kinds == want_kinds[:len(kinds)], what

    try:
        chunk(3, "from the built state")
        for e in everyone:
            for node in range(6000, 6024, 3):  # nodes that thirds leaves empty (n % 3 == 0), in shard 1
                e.inject(node, 1)
        chunk(2, "after the injects")
        for e in everyone:
            e.set_faults(loss_threshold(0.3), 5)
        chunk(2, "with faults")
        for e in everyone:
            e.set_faults(0, 0)
        chunk(2, "healed")
        for e in everyone:
            e.reset()
        for e in engines:
            assert not e.read_shard().any() and e.state_hash() == 0
        for e in everyone:
            st.thirds(e, 3)
        chunk(3, "after reset and rebuild")
        assert_shards_hold(engines, ref.read_shard()[0])
    finally:
        d.close()
    return kinds


@functools.lru_cache(maxsize=None)
def multiword_reference(case, wide=False):
    """(per-round stats, the final [W, N] state, the per-round per-rumor counts) of one oracle engine"""
    N, R, mode, k, G, faults, rounds, work = (WIDE if wide else MULTIWORD)[case] + (() if wide else ("random",))
    ref = op.OracleEngine(N, R, mode, k, SEED, flags=1, **faults)
    fill_work(ref, work, R)
    res = ref.step(rounds or 64)
    return res.stats, ref.read_shard(), res.infected


def body_multiword(factory, case, driver=None, wide=False):
    """W > 1 sharded: every round the plain state all-gather, equal to one oracle engine; no bit at or
    above R in any shard after any round.  wide: a case of WIDE, and after every round the per-rumor
    counts of the shards' own words equal the oracle's."""
    N, R, mode, k, G, faults, rounds, work = (WIDE if wide else MULTIWORD)[case] + (() if wide else ("random",))
    want, full, infected = multiword_reference(case, wide)
    assert bool(want[-1]["converged"]) == (rounds is None) and len(want) == (rounds or len(want))
    d = (driver or LockstepDriver)(factory, N, R, mode, k, SEED, G, flags=1, **faults)
    engines = d.engines
    top = ~nr.full_masks(R)[-1]
    try:
        for e in engines:
            fill_work(e, work, R)
        if wide and hasattr(d, "comm"):  # a lockstep driver: the round's summed partials carry the shards' counts
            comm_sum = d.comm.sum

            def keep(L, stem, each=None):
                total = comm_sum(L, stem, each=each)
                d.infected = total[4:4 + R]
                return total
            d.comm.sum = keep
        kinds = []
        for i, w in enumerate(want):
            got, kind = d.round()
            kinds.append(kind)
            assert got == w
            assert_infected(d, infected[i])
            shards = [e.read_shard() for e in engines]
            for s in shards:
                assert not (s[-1] & top).any()
            if wide:
                assert nr.stats_of(np.concatenate(shards, axis=1), R)[1] == [int(x) for x in infected[i]]
        assert set(kinds) == {DENSE}
        for e in engines:
            assert np.array_equal(e.read_shard(), full[:, e.lo:e.hi])
        return [e.hi - e.lo for e in engines]
    finally:
        d.close()
