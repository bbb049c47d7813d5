"""CPU tests of the role-ordered slot placement (no GPU calls).

- etcd_amd/csrc/hbslots.h, the slot-map bookkeeping of libhbnode, under
  AddressSanitizer + UBSan: tests/asan/slots_asan.cpp is a stand-alone program
  (its own main, includes only hbslots.h) that drives randomised create /
  remove / role-flip sequences against a brute-force model — capacities 1, 2
  and others that are no multiple of the 64-slot tile, a full slot space
  (capacity == live count), an adopted arrival-order layout — and checks the
  layout invariant, the read-before-write move list and the move bound after
  every re-pack plan.
- the new exports refuse bad arguments before any device work.
"""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_map_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "slots_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "slots_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "slots_asan ok" in out, out[-3000:]


def test_move_groups_rejects_bad_arguments_without_device_work():
    from etcd_amd import hipbatch
    L = hipbatch.lib()
    assert L.hb_move_groups(None, 0, None, None) == abi.HB_EINVAL
    a = (C.c_uint32 * 1)(0)
    assert L.hb_move_groups(None, 1, a, a) == abi.HB_EINVAL


def test_placement_rejects_bad_arguments_without_device_work():
    from etcd_amd import multinode as M
    L = M.lib()
    assert L.hbn_set_placement(None, M.HBN_PLACE_ROLE) == abi.HB_EINVAL
    assert L.hbn_set_placement(None, 1) == abi.HB_EINVAL
    s = M.hbn_placement()
    assert L.hbn_placement_stats(None, C.byref(s)) == abi.HB_EINVAL
    assert C.sizeof(M.hbn_placement) == 32
    assert (M.HBN_PLACE_ARRIVAL, M.HBN_PLACE_ROLE) == (0, 1)
