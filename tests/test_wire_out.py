"""CPU tests of wire egress's encoder core and entry points (no GPU calls).

- etcd_amd/csrc/hipbatch_wire_out.h under AddressSanitizer + UBSan:
  tests/asan/wire_out_asan.cpp is a stand-alone program (its own main,
  includes only that header) that checks wo_size and wo_write against
  tests/golden/wire_out/wire_out_vectors.npz (bytes of tests/wire_util.gogo_marshal:
  the four types, every varint-length edge of a u64 in every field, the 28-
  and the 91-byte record) and writes each record into a heap buffer of exactly
  wo_size bytes.
- the fixture is what its generator makes, and the oracle's Message.Unmarshal
  reads every vector's fields back.
- hb_set_egress / hb_egress / hb_encode refuse bad arguments before any
  device work.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from etcd_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_out", "wire_out_vectors.npz")


def test_wire_out_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_out_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_out_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_out ok" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes_and_unmarshals():
    from oracle.pyoracle import unmarshal_message
    from .golden.make_wire_out_vectors import EDGES, TYPES, vectors
    from .test_wire_gpu import EDGES as WIRE_EDGES
    from .wire_util import gogo_marshal
    assert EDGES == WIRE_EDGES
    z = np.load(FIXTURE)
    fields, off, data = z["fields"], z["off"], z["data"]
    rows = vectors()
    assert 200 <= len(rows) <= 1000 and np.array_equal(fields, np.array(rows, dtype=np.uint64))
    assert set(fields[:, 0].tolist()) == set(TYPES)
    for col in range(1, 9):
        if col != 7:  # every edge in every varint field
            assert set(EDGES) <= set(fields[:, col].tolist()), col
    lens = np.diff(off).astype(np.int64)
    assert lens.min() == 28 and lens.max() == 91 and int(off[-1]) == len(data)
    raw = data.tobytes()
    for i, (t, to, frm, term, lt, idx, com, rej, hint) in enumerate(rows):
        rec = raw[int(off[i]):int(off[i + 1])]
        assert rec == gogo_marshal(t, to=to, frm=frm, term=term, log_term=lt, index=idx, commit=com,
                                   reject=bool(rej), hint=hint), i
        rc, m = unmarshal_message(rec)
        assert rc == 0, i
        assert (m.type, m.to, m.from_, m.term, m.log_term, m.index, m.commit, m.reject, m.reject_hint, m.nentries) == \
            (t, to, frm, term, lt, idx, com, rej, hint, 0), i


def test_egress_rejects_bad_arguments_without_device_work():
    from etcd_amd import hipbatch
    L = hipbatch.lib()
    b = abi.hb_out_batch()  # every array NULL
    w = (C.c_uint64 * 2)()
    assert L.hb_set_egress(None, 1) == abi.HB_EINVAL
    assert L.hb_set_egress(None, 0) == abi.HB_EINVAL
    assert L.hb_egress(None, 1, None, 0, None) == abi.HB_EINVAL
    assert L.hb_egress(None, 1, C.byref(b), 1, C.addressof(w)) == abi.HB_EINVAL
    assert L.hb_encode(None, None, 0, None, 1, None, 0, None, None, None) == abi.HB_EINVAL
    assert L.hb_encode(None, C.byref(b), 1, None, 1, None, 0, C.addressof(w), C.addressof(w),
                       C.addressof(w)) == abi.HB_EINVAL
    assert C.sizeof(abi.hb_out_batch) == 64 and [n for n, _ in abi.hb_out_batch._fields_] == \
        [n for n, _ in abi.OUT_BATCH_FIELDS]
