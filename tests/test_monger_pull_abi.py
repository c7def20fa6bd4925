"""CPU: pull rumor mongering at the C ABI — the flag has one value in the header,
in Python and in Go, gossip_create refuses what item 10 says before a device is touched and names
the flag, and the call the feature adds is exported, bound and documented inside ABI v10."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from gossip_hip import FLAG_DENSE, FLAG_DIRECT, FLAG_MONGER, FLAG_MONGER_PULL, FLAG_TOPO_PEERS, Engine, _abi
from gossip_hip import engine as eng_mod

EINVAL, ENODEV, ENOTSUP = -1, -5, -6


def create(mode, flags=FLAG_MONGER_PULL, **kw):
    lib = eng_mod.load_library()
    cfg = eng_mod.make_config(1000, 3, mode, 2, 1, flags=flags, **kw)
    h = C.c_void_p()
    rc = lib.gossip_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.gossip_destroy(h)
    return rc, lib.gossip_last_error(None)


def test_flag_value_in_header_python_and_go():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert re.search(r"\bGOSSIP_FLAG_MONGER_PULL = 1u << 9\b", hdr)
    assert re.search(r"\bGOSSIP_FLAG_MONGER = 1u << 8,", hdr)
    assert FLAG_MONGER_PULL == _abi.FLAG_MONGER_PULL == 1 << 9 and FLAG_MONGER == 1 << 8
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    assert "FlagMongerPull Flags = Flags(C.GOSSIP_FLAG_MONGER_PULL)" in go
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u\b", hdr) and _abi.ABI_VERSION == 10
    assert C.sizeof(_abi.Config) == 64


@pytest.mark.parametrize("mode", ["push", "pushpull", "flood", "antientropy"])
def test_flag_needs_pull(mode):
    rc, msg = create(mode)
    assert rc == EINVAL and b"GOSSIP_FLAG_MONGER_PULL" in msg


def test_flag_with_the_push_flag_is_refused():
    for mode in ("pull", "push", "pushpull"):
        rc, msg = create(mode, FLAG_MONGER | FLAG_MONGER_PULL)
        assert rc == EINVAL and b"GOSSIP_FLAG_MONGER_PULL" in msg
    rc, msg = create("pull", FLAG_MONGER)     # bit 8 with PULL stays refused
    assert rc == EINVAL and b"GOSSIP_FLAG_MONGER" in msg and b"GOSSIP_FLAG_MONGER_PULL" not in msg


def test_flag_with_stall_or_shards_is_not_supported():
    rc, msg = create("pull", stall_rounds=2, edge_loss=1 << 30)
    assert rc == ENOTSUP and b"GOSSIP_FLAG_MONGER_PULL" in msg
    for kw in (dict(shard_count=2), dict(shard_count=2, shard_rank=1)):
        rc, msg = create("pull", **kw)
        assert rc == ENOTSUP and b"GOSSIP_FLAG_MONGER_PULL" in msg


@pytest.mark.parametrize("extra", [0, FLAG_TOPO_PEERS, FLAG_DIRECT | FLAG_DENSE, 3],
                         ids=["alone", "topo_peers", "direct_dense", "hash_timing"])
def test_what_composes_passes_validation(extra):
    """Past validation the next stop is the device: OK with an MI355X, GOSSIP_ENODEV without one."""
    rc, msg = create("pull", FLAG_MONGER_PULL | extra, edge_loss=1 << 30, partitions=3)
    assert rc in (0, ENODEV), msg


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(eng_mod.LIB_PATH)
    sigs = {n: (res, args) for n, res, args in _abi.SIGNATURES}
    assert hasattr(lib, "gossip_monger_hot_nodes")
    assert sigs["monger_hot_nodes"] == (C.c_int, [C.c_void_p, _abi.U64P]) and "monger_hot_nodes" in _abi.ENGINE_ONLY
    assert callable(Engine.hot_nodes)
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    assert "C.gossip_monger_hot_nodes(" in go and "func (e *Engine) HotNodes(" in go


def test_header_documents_the_call():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert re.search(r"^int gossip_monger_hot_nodes\(gossip_engine_t\* \w+, uint64_t\* out\);", hdr, re.M)
    doc = hdr[:hdr.index("int gossip_monger_hot_nodes(")].rsplit("/*", 1)[1]
    assert "GOSSIP_ESTATE" in doc and "GOSSIP_EINVAL" in doc and "*/" in doc
    flag = hdr[hdr.index("GOSSIP_FLAG_MONGER_PULL = 1u << 9"):].split("*/", 1)[0]
    for word in ("DESIGN.md §2.15", "GOSSIP_EINVAL", "GOSSIP_ENOTSUP", "stats.messages", "gossip_step"):
        assert word in flag, word


def test_null_arguments_are_refused():
    lib = eng_mod.load_library()
    out = C.c_uint64()
    assert lib.gossip_monger_hot_nodes(None, C.byref(out)) == EINVAL
