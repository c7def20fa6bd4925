"""CPU: push-pull rumor mongering at the C ABI — the flag has one value in the
header, in Python and in Go, gossip_create refuses what item 10 says before a device is touched and
names the flag, what bits 8 and 9 answered with PUSHPULL before they still answer, and the flag is
documented inside ABI v10."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from gossip_hip import (FLAG_DENSE, FLAG_DIRECT, FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER_PUSHPULL, FLAG_TOPO_PEERS,
                        _abi)
from gossip_hip import engine as eng_mod

EINVAL, ENODEV, ENOTSUP = -1, -5, -6
NAME = b"GOSSIP_FLAG_MONGER_PUSHPULL"


def create(mode, flags=FLAG_MONGER_PUSHPULL, **kw):
    lib = eng_mod.load_library()
    cfg = eng_mod.make_config(1000, 3, mode, 2, 1, flags=flags, **kw)
    h = C.c_void_p()
    rc = lib.gossip_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.gossip_destroy(h)
    return rc, lib.gossip_last_error(None)


def test_flag_value_in_header_python_and_go():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert re.search(r"\bGOSSIP_FLAG_MONGER_PUSHPULL = 1u << 10\b", hdr)
    assert re.search(r"\bGOSSIP_FLAG_MONGER_PULL = 1u << 9,", hdr)
    assert FLAG_MONGER_PUSHPULL == _abi.FLAG_MONGER_PUSHPULL == 1 << 10
    assert FLAG_MONGER_PULL == 1 << 9 and FLAG_MONGER == 1 << 8
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    assert "FlagMongerPushPull Flags = Flags(C.GOSSIP_FLAG_MONGER_PUSHPULL)" in go
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u\b", hdr) and _abi.ABI_VERSION == 10
    assert C.sizeof(_abi.Config) == 64


@pytest.mark.parametrize("mode", ["push", "pull", "flood", "antientropy"])
def test_flag_needs_pushpull(mode):
    rc, msg = create(mode)
    assert rc == EINVAL and NAME in msg


@pytest.mark.parametrize("other", [FLAG_MONGER, FLAG_MONGER_PULL, FLAG_MONGER | FLAG_MONGER_PULL])
def test_flag_with_another_mongering_flag_is_refused(other):
    for mode in ("pushpull", "push", "pull"):
        rc, msg = create(mode, FLAG_MONGER_PUSHPULL | other)
        assert rc == EINVAL and NAME in msg


def test_bits_8_and_9_with_pushpull_answer_as_before():
    rc, msg = create("pushpull", FLAG_MONGER)
    assert rc == EINVAL and b"GOSSIP_FLAG_MONGER applies to PUSH" in msg and b"_PULL" not in msg and NAME not in msg
    rc, msg = create("pushpull", FLAG_MONGER_PULL)
    assert rc == EINVAL and b"GOSSIP_FLAG_MONGER_PULL applies to PULL" in msg and NAME not in msg
    rc, msg = create("pushpull", FLAG_MONGER | FLAG_MONGER_PULL)
    assert rc == EINVAL and b"GOSSIP_FLAG_MONGER_PULL" in msg and NAME not in msg


def test_flag_with_stall_or_shards_is_not_supported():
    rc, msg = create("pushpull", stall_rounds=2, edge_loss=1 << 30)
    assert rc == ENOTSUP and NAME in msg
    for kw in (dict(shard_count=2), dict(shard_count=2, shard_rank=1)):
        rc, msg = create("pushpull", **kw)
        assert rc == ENOTSUP and NAME in msg


@pytest.mark.parametrize("extra", [0, FLAG_TOPO_PEERS, FLAG_DIRECT | FLAG_DENSE, 3],
                         ids=["alone", "topo_peers", "direct_dense", "hash_timing"])
def test_what_composes_passes_validation(extra):
    """Past validation the next stop is the device: OK with an MI355X, GOSSIP_ENODEV without one."""
    rc, msg = create("pushpull", FLAG_MONGER_PUSHPULL | extra, edge_loss=1 << 30, partitions=3)
    assert rc in (0, ENODEV), msg


def test_header_documents_the_flag_and_the_calls():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    flag = hdr[hdr.index("GOSSIP_FLAG_MONGER_PUSHPULL = 1u << 10"):].split("*/", 1)[0]
    for word in ("DESIGN.md §2.16", "GOSSIP_EINVAL", "GOSSIP_ENOTSUP", "stats.messages", "gossip_step"):
        assert word in flag, word
    stats = hdr[hdr.index("typedef struct gossip_round_stats"):hdr.index("} gossip_round_stats_t;")]
    assert "GOSSIP_FLAG_MONGER_PUSHPULL" in stats and "§2.16" in stats
    for call in ("gossip_set_monger", "gossip_set_monger_limit", "gossip_read_hot_shard", "gossip_read_monger_counts",
                 "gossip_monger_hot_nodes"):
        doc = hdr[:hdr.index("int %s(" % call)].rsplit("/*", 1)[1]
        assert "_MONGER_PUSHPULL" in doc and "GOSSIP_ESTATE" in doc, call
