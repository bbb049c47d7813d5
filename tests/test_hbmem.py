"""CPU test of the engine's owning buffer type (no GPU calls).

etcd_amd/csrc/hbmem.h, the DevBuf every lazily allocated or grown scratch block
of the engine's host side goes through, under AddressSanitizer + UBSan:
tests/asan/hbmem_asan.cpp is a stand-alone program (its own main, includes only
hbmem.h) that instantiates it over malloc-backed traits which count live blocks
and fail a chosen allocation.  It writes cap() elements after every reserve, so
an undersized block is a sanitizer report, and checks the growth rules, the
failure contract (empty buffer, HB_ENOMEM, usable afterwards), release, both
moves, the hb_set_rand sequence, the hook's call count and that no block is
left at the end of any scenario.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "hbmem_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "hbmem_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "hbmem_asan ok" in out, out[-3000:]
