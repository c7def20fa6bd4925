"""CPU: connection limits and hunting at the C ABI — the two calls and the host probe
are exported, declared and bound (Python and Go) inside ABI v10, refuse what can be refused before a
device is touched, and the probe's words are numpy_ref's Philox.  (The refusals that need an engine —
GOSSIP_ESTATE without a mongering flag, GOSSIP_EINVAL out of range — are in test_gpu_monger_conn.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import monger_conn_ref as mc
import numpy_ref as nr
from conftest import ROOT
from gossip_hip import _abi
from gossip_hip import engine as eng_mod

EINVAL = -1
CALLS = ("gossip_set_monger_connections", "gossip_monger_connections", "gossip_monger_conn_words")


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(eng_mod.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    go = open(os.path.join(ROOT, "gossipgpu", "gossipgpu.go")).read()
    bound = {"gossip_" + n for n, _, _ in _abi.SIGNATURES}
    for call in CALLS:
        assert hasattr(lib, call), call
        assert re.search(r"\bint %s\(" % call, hdr), call
        assert call in bound, call
        assert "C.%s(" % call in go, call
    assert re.search(r"#define GOSSIP_ABI_VERSION 10u\b", hdr)
    assert eng_mod.load_library().gossip_abi_version() == _abi.ABI_VERSION == 10
    assert C.sizeof(_abi.Config) == 64
    for method in ("func (e *Engine) SetMongerConnections(", "func (e *Engine) MongerConnections("):
        assert method in go, method
    assert hasattr(eng_mod.Engine, "set_monger_connections") and hasattr(eng_mod.Engine, "connections")


def test_null_arguments_are_refused():
    lib = eng_mod.load_library()
    out = (C.c_uint64 * 4)()
    assert lib.gossip_set_monger_connections(None, 1, 0) == EINVAL
    assert lib.gossip_monger_connections(None, out) == EINVAL
    assert lib.gossip_monger_conn_words(1, 0, 0, 0, 0, None) == EINVAL
    words = (C.c_uint32 * 2)()
    assert lib.gossip_monger_conn_words(1, 0, 0, 16, 0, words) == EINVAL     # stages are 0 .. 15
    assert lib.gossip_monger_conn_words(1, 0, 0, 0, 64, words) == EINVAL     # k <= 64
    assert lib.gossip_monger_conn_words(1, 0, 0, 15, 63, words) == 0


@pytest.mark.parametrize("seed", [1, 0x5EED0516, 0xFEDCBA9876543210, 2 ** 64 - 1])
def test_probe_words_are_numpy_refs_philox(seed):
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for n, t, s, j in [(0, 0, 0, 0), (4097, 11, 15, 63), (2 ** 32 - 2, 2 ** 32 - 1, 1, 5), (30010, 3, 7, 34)]:
        pw, hw = eng_mod.monger_conn_words(seed, n, t, s, j)
        tag = 6 | (s << 16)
        assert pw == int(nr.philox4x32_10(n, t, tag, j >> 2, k0, k1)[j & 3])
        assert hw == int(nr.philox4x32_10(n, t, tag, 16 + (j >> 2), k0, k1)[j & 3])
        a, b = mc.conn_words(seed, np.array([n]), t, s, j)
        assert (pw, hw) == (int(a[0]), int(b[0]))


def test_header_documents_the_calls():
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    doc = hdr[:hdr.index("int gossip_set_monger_connections(")].rsplit("\n\n", 1)[1]
    for word in ("DESIGN.md §2.17", "GOSSIP_ESTATE", "GOSSIP_EINVAL", "GOSSIP_ENOMEM", "gossip_reset", "1..8", "0..15"):
        assert word in doc, word
    doc = hdr[:hdr.index("int gossip_monger_connections(")].rsplit("/*", 1)[1]
    for word in ("attempts", "accepted", "refused", "hunt", "GOSSIP_ESTATE"):
        assert word in doc, word
