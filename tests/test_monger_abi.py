"""CPU: GOSSIP_FLAG_MONGER at the C ABI — what gossip_create refuses, decided
before any device is touched (as test_abi.py::test_bad_config_rejected's cases), and the two entry
points the flag adds, exported by the library and bound in Python and Go."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from gossip_hip import FLAG_HASH, FLAG_MONGER, FLAG_TIMING, FLAG_TOPO_PEERS, Engine, _abi
from gossip_hip import engine as eng_mod


def create(mode, flags=FLAG_MONGER, **kw):
    lib = eng_mod.load_library()
    cfg = eng_mod.make_config(1000, 3, mode, 2, 1, flags=flags, **kw)
    h = C.c_void_p()
    rc = lib.gossip_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.gossip_destroy(h)
    return rc, lib.gossip_last_error(None)


def test_flag_value():
    assert FLAG_MONGER == 1 << 8
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert re.search(r"GOSSIP_FLAG_MONGER = 1u << 8\b", hdr)


@pytest.mark.parametrize("mode", ["pull", "pushpull", "flood", "antientropy"])
def test_flag_needs_push(mode):
    rc, msg = create(mode)
    assert rc == -1 and b"GOSSIP_FLAG_MONGER" in msg   # GOSSIP_EINVAL


def test_flag_with_stall_or_shards_is_not_supported():
    rc, msg = create("push", stall_rounds=2, edge_loss=1 << 30)
    assert rc == -6 and b"GOSSIP_FLAG_MONGER" in msg   # GOSSIP_ENOTSUP
    rc, msg = create("push", shard_count=2)
    assert rc == -6 and b"GOSSIP_FLAG_MONGER" in msg
    rc, msg = create("push", shard_count=2, shard_rank=1)
    assert rc == -6


def test_accepted_configs_get_past_validation():
    """The flag with PUSH, alone or with the flags it composes with and with faults, is refused only
    for want of a device (or not at all)."""
    for flags in (0, FLAG_HASH | FLAG_TIMING, FLAG_TOPO_PEERS, 1 << 2, 1 << 3):
        rc, _ = create("push", FLAG_MONGER | flags, edge_loss=1 << 30, partitions=3)
        assert rc in (0, -5, -2)


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(eng_mod.LIB_PATH)
    sigs = {n: (res, args) for n, res, args in _abi.SIGNATURES}
    for name in ("set_monger", "read_hot_shard"):
        assert hasattr(lib, "gossip_" + name)
        assert name in sigs and sigs[name][0] is C.c_int
    assert sigs["set_monger"][1] == [C.c_void_p, C.c_uint32, C.c_uint32]
    assert sigs["read_hot_shard"][1] == [C.c_void_p, _abi.U64P, C.c_uint64]
    assert callable(Engine.set_monger) and callable(Engine.read_hot)
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    assert "C.gossip_set_monger(" in go and "C.gossip_read_hot_shard(" in go and "C.GOSSIP_FLAG_MONGER" in go
