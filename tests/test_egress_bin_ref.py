"""CPU tests of per-peer egress (hb_egress_bin; no GPU calls).

- the ABI: version 8, HB_EGRESS_MAX_PEERS mirrored, the three exports, and each
  refusing a NULL handle before any device work;
- etcd_amd/csrc/hipbatch_bin.h under AddressSanitizer + UBSan:
  tests/asan/bin_asan.cpp is a stand-alone program (its own main, includes only
  that header) and is run directly;
- tests/egress_bin_util.bin_reference, the reference of the GPU tests, on
  hand-written cases.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from etcd_amd import abi

from .egress_bin_util import ASAN_SIZES, asan_probes, asan_table, bin_reference, bins_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = abi.hb_info(abi.HB_MSG_VOTE_RESP, abi.HB_REF_OTHER)
SLOT = abi.hb_info(abi.HB_MSG_APP_RESP, 1)


def test_abi_version_and_peer_limit():
    assert abi.HB_ABI_VERSION == 8
    assert abi.HB_EGRESS_MAX_PEERS == 255
    txt = open(os.path.join(ROOT, "include", "hipbatch.h")).read()
    assert re.search(r"^#define\s+HB_ABI_VERSION\s+8\b", txt, re.M)
    assert re.search(r"^#define\s+HB_EGRESS_MAX_PEERS\s+255\b", txt, re.M)


def test_library_exports_and_refuses_a_null_handle():
    from etcd_amd import hipbatch
    L = hipbatch.lib()  # loads without touching the GPU
    assert L.hb_abi_version() == 8
    for name in ("hb_set_egress_peers", "hb_egress_bin", "hb_peer_spans"):
        assert hasattr(L, name), name
    ids = (C.c_uint64 * 3)(1, 2, 3)
    w = (C.c_uint64 * 8)()
    b = abi.hb_out_batch()
    assert L.hb_set_egress_peers(None, C.addressof(ids), 3) == abi.HB_EINVAL
    assert L.hb_set_egress_peers(None, None, 0) == abi.HB_EINVAL
    assert L.hb_egress_bin(None, C.byref(b), 0, None, C.byref(b), None, C.addressof(w)) == abi.HB_EINVAL
    assert L.hb_egress_bin(None, None, 0, None, None, None, None) == abi.HB_EINVAL
    assert L.hb_peer_spans(None, C.addressof(w), C.addressof(w), C.addressof(w)) == abi.HB_EINVAL
    assert L.hb_peer_spans(None, None, None, None) == abi.HB_EINVAL


def test_bin_lookup_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "bin_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "bin_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "bin ok" in out, out[-3000:]
    # the probes the program reports are the ones asan_probes restates for the GPU test
    want = sum(len(asan_probes(asan_table(n))) for n in ASAN_SIZES)
    assert f"bin ok: {want} probes" in out, out[-300:]


def test_asan_tables_are_legal_tables():
    for n in ASAN_SIZES:
        ids = asan_table(n)
        assert len(ids) == n and len(set(ids.tolist())) == n and (ids != 0).all()
    ids = asan_table(255).tolist()
    assert {1, 1 << 32, 1 << 63, (1 << 64) - 1} <= set(ids)
    assert any(a != b and (a ^ b) >> 32 == 0 for a in ids[:12] for b in ids[:12])  # differ only in the low half
    assert any(a != b and (a ^ b) & 0xFFFFFFFF == 0 for a in ids[:12] for b in ids[:12])  # only in the high half


def _ref(to, info, ids):
    order, off = bin_reference(np.array(to, np.uint64), np.array(info, np.uint32), np.array(ids, np.uint64))
    return order.tolist(), off.tolist()


def test_bin_reference_hand_written_cases():
    # empty batch: every offset zero, n_peers + 2 of them
    assert _ref([], [], [5, 6, 7]) == ([], [0, 0, 0, 0, 0])
    # one bin: the identity, and "other" is empty
    assert _ref([9, 9, 9, 9], [SLOT] * 4, [9]) == ([0, 1, 2, 3], [0, 4, 4])
    # every record "other": unknown ids, a zero id, HB_REF_OTHER with a known id
    assert _ref([4, 0, 7, 8], [SLOT, OTHER, OTHER, SLOT], [7, 9]) == ([0, 1, 2, 3], [0, 0, 0, 4])
    # ties keep their order; bins follow the caller's order of ids, not the ids' values
    to = [30, 10, 20, 10, 30, 99, 10, 20]
    order, off = _ref(to, [SLOT] * 8, [30, 10, 20])
    assert order == [0, 4, 1, 3, 6, 2, 7, 5] and off == [0, 2, 5, 7, 8]
    # all 64 bits of an id count
    ids = [1, 1 << 32, (1 << 32) | 1]
    assert bins_of([1, 1 << 32, (1 << 32) | 1, 2, 1 << 33], [SLOT] * 5, ids).tolist() == [0, 1, 2, 3, 3]
