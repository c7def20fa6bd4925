"""GPU: what HIP Engine shards put on the wire, collective by collective (the recording comm of
tests/shard_cases.py), against the numpy restatement of every product from S_t alone and against the
oracle shards' buffers of the same round.  Errors that cancel end to end and cost only link bytes (a
full node sent as mixed, an edge the filter should have dropped, an extra rare-list member, garbage
in tail bits or prefix words) fail here; the plan model and every DESIGN.md §5 figure rest on these
bytes, and so would a second host implementation of include/gossip_shard.h."""
import numpy as np
import pytest

import oracle_py as op
import shard_cases as sc
from gossip_hip import Engine
from gossip_hip.sharded import _as_tensor
from shard_cases import PHILOX, PHILOX_G, RUNS, SLOTS

pytestmark = pytest.mark.gpu

WIRE = [(run, G) for run in RUNS for G in (4, 5)] + [(PHILOX, PHILOX_G)]


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("run,G", WIRE, ids=[f"{sc.run_id(run)}-G{G}" for run, G in WIRE])
def test_wire_products_equal_numpy_and_oracle(run, G, offset):
    """Every product of every round: equal to the numpy reference, and to the oracle shards' (sparse
    messages and exchange items as sorted multisets per (sender, owner), so with equal counts)."""
    sc.body_carousel_wire(Engine, run, G, offset, other=op.OracleEngine)


class _DevForms(Engine):
    """The five calls with a _dev form routed through it, the values read from the returned device
    pointer (as an RCCL collective on the engine's stream would consume them)."""

    def _read(self, ptr, n):
        return _as_tensor(ptr, n * 8, True, self.device).cpu().numpy().view(np.uint64).copy()

    def sparse_rare(self):
        ptr, cnt = self.sparse_rare_dev()
        return ptr, int(self._read(cnt, 1)[0])

    def sparse_scan(self, counts):
        ptr, cnt = self.sparse_scan_dev(counts)
        return ptr, self._read(cnt, self.cfg.shard_count)

    def sparse_commit(self, items):
        return self._read(self.sparse_commit_dev(items), self.partial_len())

    def xd_requests(self):
        ids, vals, cnt = self.xd_requests_dev()
        return ids, vals, [int(x) for x in self._read(cnt, self.cfg.shard_count)]

    def xd_finish(self):
        return self._read(self.xd_finish_dev(), self.partial_len())


def test_dev_forms_equal_oracle():
    """One carousel run at G = 3 with the counts and partials taken from the device values."""
    kinds = sc.body_carousel(_DevForms, RUNS[1], 3, 0)
    assert {1, 3} <= set(kinds) and SLOTS[0][0] == "sparse"
