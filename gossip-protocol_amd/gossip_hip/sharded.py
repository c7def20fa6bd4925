"""Sharded rounds across ranks: one engine per GPU, node ids
split into contiguous shards.

Reference anchor: the only cross-node traffic of the reference is the
per-neighbour SyncRPC of (*NodeState).Gossip (main.go:81).  Here each round is
one of two exchanges over RCCL (torch.distributed backend "nccl" is RCCL on
ROCm; on CPU the same code runs over gloo, which is how the N>1 path is tested
without a GPU):

  dense round   all-gather of every shard's state slice (the exchange image),
                then an all-reduce of the stats partials;
  sparse round  (the engine's plan, when one class of nodes is rare) all-gather
                of each shard's rare nodes {id, value}, all-to-all of the pushes
                that land on another shard, all-reduce of the partials;
  exchange      (kind 3, DESIGN.md §5.2: dense rounds at G >= the "xd_shards" param) no
                image: all-to-all of one item per live edge {p at its owner | flags,
                S_t[n]} to p's owner, all-to-all of the pull replies back, all-reduce of
                the partials; when many nodes are empty or full, first an all-gather of
                every shard's occupancy bitmaps, so the one-way edges that move nothing
                (into an empty / full peer) are never sent;
  class-coded   (kind 4, DESIGN.md §5.1: dense rounds while few nodes are mixed) the
                state all-gather as each shard's two occupancy bitmaps (empty / full)
                plus the words of its mixed nodes, expanded into the image on arrival;
  replicated    (kinds 5 / 6, DESIGN.md §5.7: dense rounds where the links cost more than the
                extra device time, e.g. G = 2 at 2^27 nodes) every rank runs the whole round over
                the whole image in place: kind 5 after the state all-gather (as a dense round),
                kind 7 after the class-coded all-gather, kind 6 with no collective before it
                (the previous round left every node's S_{t+1} in the image); then the
                all-reduce of the own-slice partials;
  ANTIENTROPY   ("Design B") all-gather of the alive and stale bits,
                all-to-all of request items {p, n, V_t[n]} to p's owner and of its
                replies V_t[p], all-reduce of the partials; the global max vector
                by an all-reduce MAX (ncclMax) after any injection.

The engine decides the kind from the global totals it was last given, so every
rank takes the same branch.

Each kind is written once, over the local engines L and a comm, in the shape of the library's
own driver (csrc/multi.hip, struct Driver): sharded_round runs it on the one engine of a rank
with the torch.distributed comm, lockstep_round on all G engines of one process with the copy comm.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

# plan kinds (gossip_sharded_plan).  Below zero the engine needs something before it can plan:
NEED_TARGET, NEED_TOTALS = -2, -1  # ANTIENTROPY's global max vector; the global totals
# ... from zero on, the coming round: dense, sparse, ANTIENTROPY, exchange dense, class-coded dense, and
# replicated dense after the state all-gather / with no collective / after the class-coded all-gather
DENSE, SPARSE, ANTIENTROPY, EXCHANGE, CLASSCODED, REP_GATHER, REP, REP_CLASSCODED = range(8)
KIND_LETTERS = "DSAXCRrQ"  # one letter per kind, in that order


class _DevPtr:
    """Zero-copy view of engine-owned device memory for torch collectives."""

    def __init__(self, ptr: int, nbytes: int, width: int = 8):
        self.__cuda_array_interface__ = {
            "shape": (nbytes // width,), "typestr": f"<i{width}", "data": (ptr, False), "version": 3, "strides": None,
        }


def _as_tensor(ptr: int, nbytes: int, on_device: bool, device: int | None = None, width: int = 8) -> torch.Tensor:
    """int64 (width 8) or int32 (width 4) view of nbytes at ptr."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device) if on_device else "cpu"
    dt = torch.int64 if width == 8 else torch.int32
    if nbytes == 0:
        return torch.empty(0, dtype=dt, device=dev)
    if on_device:
        return torch.as_tensor(_DevPtr(ptr, nbytes, width), device=dev)
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64 if width == 8 else C.c_int32)),
                                shape=(nbytes // width,))
    return torch.from_numpy(arr)


def _device_collectives(group) -> bool:
    return dist.get_backend(group) == "nccl"


def _calls(L, stem: str, *args, each=None) -> list:
    """One engine call on every local engine; each: one further argument per engine."""
    return [getattr(e, stem)(*args, *(() if each is None else (each[i],))) for i, e in enumerate(L)]


def _width(item_bytes: int) -> int:
    """Items travel as int64s where they are whole ones, else as int32s (the exchange round's ids)."""
    return 4 if item_bytes % 8 else 8


# A comm has the collectives of a round on engine memory, given one pointer (and for an
# all-to-all one list of item counts per rank) per local engine:
#   all_gather(recv, send, nbytes), all_gather_async(...) -> work, wait(work),
#   all_to_all(recv, send, recv_counts, send_counts, item_bytes), max(vectors),
# and the exchanges of what an engine call hands out as values, named by the call's stem:
#   gather_counts(L, stem)         -> (the call's other results per engine, the count of every rank)
#   exchange_counts(L, stem, ...)  -> (the other results, counts sent per rank, counts received)
#   sum(L, stem, ...)              -> the sum of every rank's partials
# Whether those values pass through the host or stay on the device (engine.<stem>_dev) is the
# comm's business.  world: ranks; link: the bytes a rank put on its links this round; direct:
# collectives on the device, ordered on torch's current stream.

class _Comm:
    """torch.distributed among ranks of one engine each (L = [engine]): in place over RCCL for
    device engines, staged through host tensors over gloo."""

    def __init__(self, engine, group, direct: bool | None = None):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        # the model of gossip_round_wall: an all-gather sends the slice to world - 1 ranks, an
        # all-to-all what goes to other ranks, a ring all-reduce 2 (world - 1) / world of the vector
        self.link = 0
        self.on_device = engine.on_device
        self.direct = engine.on_device and _device_collectives(group)
        if direct is not None:  # tests: the collectives on engine memory as RCCL would run them
            self.direct = direct
        # counts and partials as device values (RCCL on device engines with the ABI v9 calls)
        self.dev = self.direct and engine.on_device and engine.supports("round_compute_dev")

    def _sync(self):
        if self.on_device:
            torch.cuda.synchronize()

    def _t(self, ptr: int, nbytes: int, width: int = 8) -> torch.Tensor:
        return _as_tensor(ptr, nbytes, self.on_device, width=width)

    def _lb_gather(self, send: torch.Tensor):
        self.link += send.numel() * send.element_size() * (self.world - 1)

    def _lb_a2a(self, send: torch.Tensor, send_splits):
        el = send.element_size()
        self.link += sum(int(c) * el for q, c in enumerate(send_splits) if q != self.rank)

    def _lb_reduce(self, t: torch.Tensor):
        self.link += 2 * (self.world - 1) * t.numel() * t.element_size() // max(self.world, 1)

    def all_gather(self, recv, send, nbytes: int):
        recv, send = self._t(recv[0], nbytes * self.world), self._t(send[0], nbytes)
        self._lb_gather(send)
        if self.direct:
            dist.all_gather_into_tensor(recv, send, group=self.group)
            return
        host = torch.empty(recv.numel(), dtype=torch.int64)
        dist.all_gather_into_tensor(host, send.cpu() if self.on_device else send.clone(), group=self.group)
        recv.copy_(host)
        self._sync()

    def all_gather_async(self, recv, send, nbytes: int):
        """Device collectives: returns the pending work (the caller's stream waits on wait());
        staged collectives complete before returning None."""
        if self.direct:
            recv, send = self._t(recv[0], nbytes * self.world), self._t(send[0], nbytes)
            self._lb_gather(send)
            return dist.all_gather_into_tensor(recv, send, group=self.group, async_op=True)
        self.all_gather(recv, send, nbytes)
        return None

    def wait(self, work):
        if work is not None:
            work.wait()

    def all_to_all(self, recv, send, recv_counts, send_counts, item_bytes: int):
        width = _width(item_bytes)
        recv_splits = [c * item_bytes // width for c in recv_counts[0]]
        send_splits = [c * item_bytes // width for c in send_counts[0]]
        recv = self._t(recv[0], sum(recv_splits) * width, width)
        send = self._t(send[0], sum(send_splits) * width, width)
        self._lb_a2a(send, send_splits)
        if self.direct:
            dist.all_to_all_single(recv, send, output_split_sizes=recv_splits, input_split_sizes=send_splits,
                                   group=self.group)
            return
        host = torch.empty(recv.numel(), dtype=recv.dtype)
        dist.all_to_all_single(host, send.cpu() if self.on_device else send.clone(), output_split_sizes=recv_splits,
                               input_split_sizes=send_splits, group=self.group)
        recv.copy_(host)
        self._sync()

    def small(self, values) -> torch.Tensor:
        t = torch.as_tensor(np.asarray(values, dtype=np.int64).copy())
        return t.cuda() if self.direct and self.on_device else t

    def max(self, vectors) -> np.ndarray:
        t = self.small(np.asarray(vectors[0], dtype=np.int64))
        self._lb_reduce(t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return t.cpu().numpy()

    def all_reduce_sum(self, partial: np.ndarray) -> np.ndarray:
        t = self.small(partial.view(np.int64))
        self._lb_reduce(t)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy().view(np.uint64)

    def all_gather_small(self, value: int) -> list:
        self.link += 8 * (self.world - 1)
        out = self.small(np.zeros(self.world))
        dist.all_gather_into_tensor(out, self.small([value]), group=self.group)
        return [int(x) for x in out.cpu()]

    def all_to_all_small(self, values) -> list:
        self.link += 8 * (self.world - 1)
        out = self.small(np.zeros(self.world))
        dist.all_to_all_single(out, self.small(values), group=self.group)
        return [int(x) for x in out.cpu()]

    # device-resident values (engine.*_dev, RCCL): the collective reads engine memory on the
    # engine's (= torch's current) stream and one host read of its result is the round's only
    # sync for that exchange
    def dev_all_gather_one(self, ptr: int) -> list:
        self.link += 8 * (self.world - 1)
        out = torch.empty(self.world, dtype=torch.int64, device="cuda")
        dist.all_gather_into_tensor(out, _as_tensor(ptr, 8, True), group=self.group)
        return [int(x) for x in out.cpu()]

    def dev_all_to_all_counts(self, ptr: int):
        """(sent counts, received counts) from the G counts at ptr."""
        send = _as_tensor(ptr, self.world * 8, True)
        self.link += 8 * (self.world - 1)
        recv = torch.empty_like(send)
        dist.all_to_all_single(recv, send, group=self.group)
        both = [int(x) for x in torch.cat([send, recv]).cpu()]
        return both[:self.world], both[self.world:]

    def dev_all_reduce_sum(self, ptr: int, n: int) -> np.ndarray:
        t = _as_tensor(ptr, n * 8, True).clone()  # (the engine keeps its own partials)
        self._lb_reduce(t)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy().view(np.uint64)

    def _values(self, L, stem: str, *args, each=None):
        """(the engine call's results, whether its last one is a device pointer): engine.<stem>_dev
        where this comm takes device values and the call has that form."""
        dev = self.dev and hasattr(L[0], stem + "_dev")
        return _calls(L, stem + "_dev" if dev else stem, *args, each=each)[0], dev

    def gather_counts(self, L, stem: str):
        (*head, count), dev = self._values(L, stem)
        return [head], self.dev_all_gather_one(count) if dev else self.all_gather_small(count)

    def exchange_counts(self, L, stem: str, *args):
        (*head, counts), dev = self._values(L, stem, *args)
        if dev:
            counts, in_counts = self.dev_all_to_all_counts(counts)
        else:
            counts = [int(c) for c in counts]
            in_counts = self.all_to_all_small(counts)
        return [head], [counts], [in_counts]

    def sum(self, L, stem: str, each=None) -> np.ndarray:
        part, dev = self._values(L, stem, each=each)
        return self.dev_all_reduce_sum(part, L[0].partial_len()) if dev else self.all_reduce_sum(part)


class _CopyComm:
    """The engines of one process, device or host, one per rank in rank order (L = all of
    them; also the one engine of a world of 1): slice copies in place of the collectives."""

    link, direct = 0, False

    def __init__(self, engines):
        self.engines, self.world = engines, len(engines)

    def _sync(self):
        for d in {e.device for e in self.engines if e.on_device}:
            torch.cuda.synchronize(d)

    def _views(self, ptrs, nbytes, width: int = 8) -> list:
        return [_as_tensor(p, n, e.on_device, e.device if e.on_device else None, width)
                for e, p, n in zip(self.engines, ptrs, nbytes)]

    def all_gather(self, recv, send, nbytes: int):
        G, n = self.world, nbytes // 8
        src = self._views(send, [nbytes] * G)
        for r, dst in enumerate(self._views(recv, [nbytes * G] * G)):
            for q in range(G):
                if recv[r] + q * nbytes != send[q]:  # (else the own slot of an in-place gather)
                    dst[q * n:(q + 1) * n].copy_(src[q])
        self._sync()

    def all_gather_async(self, recv, send, nbytes: int):
        """The copies run at wait(): after the engines' own-slice kernels are on their streams."""
        return lambda: self.all_gather(recv, send, nbytes)

    def wait(self, work):
        work()

    def all_to_all(self, recv, send, recv_counts, send_counts, item_bytes: int):
        width = _width(item_bytes)
        w = item_bytes // width
        src = self._views(send, [sum(c) * item_bytes for c in send_counts], width)
        for r, dst in enumerate(self._views(recv, [sum(c) * item_bytes for c in recv_counts], width)):
            at = 0  # rank r receives from q = 0 .. G - 1 in order
            for q, cnt in enumerate(send_counts):
                if cnt[r]:
                    off = sum(cnt[:r])
                    dst[at * w:(at + cnt[r]) * w].copy_(src[q][off * w:(off + cnt[r]) * w])
                    at += cnt[r]
        self._sync()

    def max(self, vectors) -> np.ndarray:
        return np.maximum.reduce(vectors)

    def gather_counts(self, L, stem: str):
        res = _calls(L, stem)
        return [r[:-1] for r in res], [r[-1] for r in res]

    def exchange_counts(self, L, stem: str, *args):
        res = _calls(L, stem, *args)
        counts = [[int(c) for c in r[-1]] for r in res]
        return [r[:-1] for r in res], counts, [[c[r] for c in counts] for r in range(self.world)]

    def sum(self, L, stem: str, each=None) -> np.ndarray:
        parts = _calls(L, stem, each=each)
        tot = np.zeros_like(parts[0])
        for p in parts:
            tot = tot + p  # uint64 wraps like the RCCL int64 sum
        return tot


def _plan(L, comm) -> int:
    if not L[0].supports("sharded_plan"):
        return DENSE
    ks = _calls(L, "sharded_plan")
    if ks[0] == NEED_TARGET:  # after an injection (ncclMax over the shards)
        _calls(L, "ae_set_target", comm.max(_calls(L, "ae_local_target")))
        ks = _calls(L, "sharded_plan")
    if ks[0] < 0:  # NEED_TOTALS (after reset / inject): all-reduce the shards' own
        ks = _calls(L, "sharded_plan", comm.sum(L, "local_totals"))
    assert len(set(ks)) == 1, "shards planned different rounds"
    return ks[0]


# -- the rounds: each returns the global sum of the partials ------------------------------------

def _dense_round(L, comm) -> np.ndarray:
    """DENSE, and REP_GATHER (the engine then computes every node of the image)."""
    send, recv, nbytes = zip(*_calls(L, "exchange_buffers"))
    if comm.world > 1:
        # in place (a device engine's send slice lies inside its image), in flight while the
        # engine runs the part of the round that reads only its own slice
        work = comm.all_gather_async(recv, send, nbytes[0])
        _calls(L, "dense_prepare")
        comm.wait(work)
    return comm.sum(L, "round_compute")


def _sparse_round(L, comm) -> np.ndarray:
    rare, counts = comm.gather_counts(L, "sparse_rare")
    stride = max(counts)
    recv = _calls(L, "sparse_rare_recv", stride)
    if stride:
        comm.all_gather(recv, [p for p, in rare], stride * 16)
    out, out_counts, in_counts = comm.exchange_counts(L, "sparse_scan", counts)
    n_in = [sum(c) for c in in_counts]
    inbox = _calls(L, "sparse_msg_recv", each=n_in)
    # every rank joins the collective, also one with nothing to send or receive (G > 2)
    comm.all_to_all(inbox, [p for p, in out], in_counts, out_counts, 16)  # items {uint64 node, uint64 value}
    return comm.sum(L, "sparse_commit", each=n_in)


def _xd_round(L, comm, items: list | None = None) -> np.ndarray:
    """items gets each local shard's item counts per owner."""
    cls, img, nb = zip(*_calls(L, "xd_classes"))
    if nb[0] and comm.world > 1:  # every shard's class bitmaps (in place): the edge filter of this round
        comm.all_gather(img, cls, nb[0])
    reqs, counts, in_counts = comm.exchange_counts(L, "xd_requests")
    if items is not None:
        items.append([list(c) for c in counts])
    ids, vals = zip(*reqs)
    rid, rval = zip(*_calls(L, "xd_request_recv", each=[sum(c) for c in in_counts]))
    comm.all_to_all(rid, ids, in_counts, counts, 4)
    comm.all_to_all(rval, vals, in_counts, counts, 8)
    rep = _calls(L, "xd_serve")  # replies in the received order
    back = _calls(L, "xd_response_recv")
    comm.all_to_all(back, rep, counts, in_counts, 8)  # what a shard received from q returns to q
    return comm.sum(L, "xd_finish")


def _rep_round(L, comm) -> np.ndarray:
    """REP: the image already holds S_t of every node (the last round was replicated)."""
    return comm.sum(L, "round_compute")


def _cc_round(L, comm) -> np.ndarray:
    """CLASSCODED, and REP_CLASSCODED (the engine then computes every node of the image)."""
    sends, counts = comm.gather_counts(L, "cc_send")
    bits, nbytes, vals = zip(*sends)
    stride = max(counts)
    img, rvals = zip(*_calls(L, "cc_recv", stride))
    if comm.world > 1:
        # the bitmaps in place (the own slot lies inside the image); the mixed words padded to
        # the stride.  Both in flight while the engine runs the own-slice part of the round.
        works = [comm.all_gather_async(img, bits, nbytes[0])]
        if stride:
            works.append(comm.all_gather_async(rvals, vals, stride * 8))
        _calls(L, "dense_prepare")
        for work in works:
            comm.wait(work)
    elif stride:
        comm.all_gather(rvals, vals, stride * 8)
    _calls(L, "cc_expand", counts)
    return comm.sum(L, "round_compute")


def _ae_round(L, comm) -> np.ndarray:
    rw, pw = L[0].ae_item_words(0), L[0].ae_item_words(1)  # uint32 words, even: whole int64s
    send, recv, nbytes = zip(*_calls(L, "exchange_buffers"))  # own stale words -> every shard's image
    if comm.world > 1:
        comm.all_gather(recv, send, nbytes[0])
    reqs, counts, in_counts = comm.exchange_counts(L, "ae_requests")
    inbox = _calls(L, "ae_request_recv", each=[sum(c) for c in in_counts])
    # (every rank joins, also one with nothing to send or receive; a shard sends itself nothing)
    comm.all_to_all(inbox, [p for p, in reqs], in_counts, counts, rw * 4)
    resp = _calls(L, "ae_serve")  # replies in the received order
    back = _calls(L, "ae_response_recv")
    comm.all_to_all(back, resp, counts, in_counts, pw * 4)
    return comm.sum(L, "ae_finish")


_ROUNDS = {DENSE: _dense_round, SPARSE: _sparse_round, ANTIENTROPY: _ae_round, EXCHANGE: _xd_round,
           CLASSCODED: _cc_round, REP_GATHER: _dense_round, REP: _rep_round, REP_CLASSCODED: _cc_round}


def _round(L, comm, kinds: list | None = None, items: list | None = None):
    """Plan, the round of that kind, commit -> (kind, every local engine's stats)."""
    kind = _plan(L, comm)
    if kinds is not None:
        kinds.append(kind)
    total = _xd_round(L, comm, items) if kind == EXCHANGE else _ROUNDS[kind](L, comm)
    return kind, _calls(L, "round_commit", total)


def _bind_stream(engine, comm) -> bool:
    """Device collectives are enqueued on torch's current stream (the RCCL stream waits for
    it, and work.wait() / a synchronous collective make it wait in turn): the engine must
    launch on that same stream, or its kernels could read the image before the all-gather
    wrote it.  torch's default stream is the null stream (cuda_stream 0), which
    gossip_set_stream binds as such.  Returns True when it also set ordered_collectives (torch's
    collectives wait for this stream, so the per-kind calls skip their publishing sync); the
    caller clears it when the round ends (sharded_round), so the flag never outlives the round
    that bound the stream (a later host driver, staged collectives or another stream get the
    sync back)."""
    if comm.direct and engine.on_device:
        engine.set_stream(torch.cuda.current_stream().cuda_stream)
        engine.set_param("ordered_collectives", 1)
        return True
    return False


def sharded_round(engine, group=None, kinds: list | None = None, direct: bool | None = None,
                  trace: list | None = None) -> dict:
    """Runs one round of a sharded engine; every rank must call it.  With RCCL the engine is
    bound to the caller's current torch stream, so every kernel is ordered after the
    collectives that feed it.  kinds: the round's plan kind is appended to it.  direct (tests):
    force the in-place collective path that RCCL takes, also for host engines over gloo.
    trace: gets {"kind", "link_bytes"} of the round (the bytes this rank sent over its links)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    comm = _Comm(engine, group, direct) if world > 1 else _CopyComm([engine])
    ordered = _bind_stream(engine, comm)
    try:
        kind, (st,) = _round([engine], comm, kinds)
        if trace is not None:
            trace.append({"kind": kind, "link_bytes": comm.link})
        return st
    finally:
        if ordered:  # scoped to this round (the flag must not outlive the binding)
            engine.set_param("ordered_collectives", 0)


def _all_ranks(ok: bool, group=None) -> bool:
    """True iff `ok` holds on every rank (an all-reduce MIN: every rank learns the same answer)."""
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
    return bool(t.item())


def init_engine_comm(engine, group=None) -> str | None:
    """Hands a shard engine its own RCCL communicator (gossip_comm_init_rank): rank 0
    makes the unique id, torch.distributed carries it; engine.step then runs every sharded round
    inside the library (plan, collectives on the engine's stream, kernels).

    Collective, and so is its outcome: every rank joins every step, also after a failure, and
    every rank returns the same thing — None when every rank has its communicator, else the
    reason (then the caller drives the rounds over torch.distributed on every rank).  Rank 0
    broadcasts the id or None; each rank first loads RCCL itself (a rank that could not would
    leave the others waiting inside ncclCommInitRank), and the init's success is agreed on by
    an all-reduce MIN."""
    from .engine import comm_unique_id
    rank0 = dist.get_rank(group) == 0
    box, err = [None], None
    try:  # rank 0: the id; every rank: RCCL loads and answers (a throwaway id elsewhere)
        uid = comm_unique_id()
        if rank0:
            box[0] = uid
    except Exception as exc:  # noqa: BLE001 - reported in the return value
        err = f"RCCL unavailable on rank {dist.get_rank(group)}: {exc}"
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if not _all_ranks(err is None and box[0] is not None, group):
        return err or "RCCL unavailable on another rank"
    try:
        engine.comm_init_rank(box[0])
    except Exception as exc:  # noqa: BLE001
        err = f"gossip_comm_init_rank on rank {dist.get_rank(group)}: {exc}"
    if not _all_ranks(err is None, group):
        return err or "gossip_comm_init_rank failed on another rank"
    return None


def sharded_run(engine, max_rounds: int, group=None, kinds: list | None = None, direct: bool | None = None,
                trace: list | None = None) -> list:
    """Rounds until converged (same stop rule as gossip_step); kinds collects the plan kinds.
    trace: one entry per round, {"kind", "link_bytes"} and, on a device engine, "events" = a
    timing torch.cuda.Event pair on the current stream around the whole round (plan,
    collectives, kernels, host reads: the RCCL collectives are ordered on that stream)."""
    on_dev = engine.on_device and torch.cuda.is_available()
    if on_dev:
        engine.set_stream(torch.cuda.current_stream().cuda_stream)
    out = []
    for _ in range(max_rounds):
        ev = None
        if trace is not None and on_dev:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        st = sharded_round(engine, group, kinds, direct, trace)
        if ev is not None:
            ev[1].record()
            trace[-1]["events"] = ev
        out.append(st)
        if st["converged"] or (engine.cfg.mode == 0 and st["messages"] == 0):
            break
    return out


# -- single-process driver ---------------------------------------------------

def lockstep_round(engines, items: list | None = None):
    """One round of G shard engines in one process (one per GPU, several on one, or host
    engines), in rank order: the round of sharded_round with copies in place of the collectives.
    Returns (kind, stats).  items (exchange rounds): gets each shard's item counts per owner."""
    kind, st = _round(engines, _CopyComm(engines), items=items)
    assert all(s == st[0] for s in st)
    return kind, st[0]


def lockstep_run(engines, max_rounds: int, items: list | None = None):
    """lockstep_round until converged.  Returns (per-round stats, per-round kind: DENSE ..
    REP_CLASSCODED above).  items: as for lockstep_round, one entry per exchange round."""
    stats, kinds = [], []
    for _ in range(max_rounds):
        kind, st = lockstep_round(engines, items)
        kinds.append(kind)
        stats.append(st)
        if st["converged"]:
            break
    return stats, kinds
