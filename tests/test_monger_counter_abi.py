"""CPU: the counter rule of rumor mongering at the C ABI — the two entry points it
adds are exported by the library, bound in Python and Go and documented in the header, inside ABI
v10, and everything test_monger_abi.py sees refused is still refused."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from gossip_hip import FLAG_MONGER, Engine, _abi
from gossip_hip import engine as eng_mod

NEW = ("set_monger_limit", "read_monger_counts")


def create(mode, flags=FLAG_MONGER, **kw):
    lib = eng_mod.load_library()
    cfg = eng_mod.make_config(1000, 3, mode, 2, 1, flags=flags, **kw)
    h = C.c_void_p()
    rc = lib.gossip_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.gossip_destroy(h)
    return rc, lib.gossip_last_error(None)


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(eng_mod.LIB_PATH)
    sigs = {n: (res, args) for n, res, args in _abi.SIGNATURES}
    for name in NEW:
        assert hasattr(lib, "gossip_" + name)
        assert name in sigs and sigs[name][0] is C.c_int and name in _abi.ENGINE_ONLY
    assert sigs["set_monger_limit"][1] == [C.c_void_p, C.c_uint32]
    assert sigs["read_monger_counts"][1] == [C.c_void_p, _abi.U64P, C.c_uint64]
    assert callable(Engine.set_monger_limit) and callable(Engine.read_counts)
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    assert "C.gossip_set_monger_limit(" in go and "C.gossip_read_monger_counts(" in go
    assert "func (e *Engine) SetMongerLimit(" in go and "func (e *Engine) ReadMongerCounts(" in go


def test_header_documents_them_inside_v10():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert re.search(r"^int gossip_set_monger_limit\(gossip_engine_t\* \w+, uint32_t limit\);", hdr, re.M)
    assert re.search(r"^int gossip_read_monger_counts\(gossip_engine_t\* \w+, uint64_t\* out, uint64_t n_words\);",
                     hdr, re.M)
    for name in NEW:   # a comment that names the call's errors stands right above each prototype
        doc = hdr[:hdr.index("int gossip_" + name + "(")].rsplit("/*", 1)[1]
        assert "GOSSIP_ESTATE" in doc and "GOSSIP_EINVAL" in doc and "*/" in doc
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u\b", hdr) and _abi.ABI_VERSION == 10
    assert C.sizeof(_abi.Config) == 64


@pytest.mark.parametrize("mode", ["pull", "pushpull", "flood", "antientropy"])
def test_flag_still_needs_push(mode):
    rc, msg = create(mode)
    assert rc == -1 and b"GOSSIP_FLAG_MONGER" in msg   # GOSSIP_EINVAL


def test_flag_with_stall_or_shards_is_still_not_supported():
    rc, msg = create("push", stall_rounds=2, edge_loss=1 << 30)
    assert rc == -6 and b"GOSSIP_FLAG_MONGER" in msg   # GOSSIP_ENOTSUP
    for kw in (dict(shard_count=2), dict(shard_count=2, shard_rank=1)):
        rc, _ = create("push", **kw)
        assert rc == -6


def test_null_engine_is_refused():
    lib = eng_mod.load_library()
    out = (C.c_uint64 * 4)()
    assert lib.gossip_set_monger_limit(None, 2) == -1
    assert lib.gossip_read_monger_counts(None, out, 4) == -1
