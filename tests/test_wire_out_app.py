"""CPU tests of the split MsgApp records of wire egress's encoder core (no GPU calls).

- etcd_amd/csrc/hipbatch_wire_out.h under AddressSanitizer + UBSan:
  tests/asan/wire_out_app_asan.cpp is a stand-alone program (its own main) that
  checks wo_size_split, wo_write_split and wo_prefix_len against
  tests/golden/wire_out/wire_out_app_vectors.npz (MsgApp with 0, 1 and 3 entries
  through tests/wire_util.gogo_marshal, every varint-length edge of a u64 in to /
  from / term / logTerm / index / commit), writes each record into a heap buffer
  of exactly its size and checks that prefix ‖ entries ‖ suffix is the message.
  Built and run as tests/test_wire_out.py does: no preloaded runtime, nothing
  loaded into Python.
- the fixture is what its generator makes; etcd_amd.splice rebuilds every whole
  message from the record, the status byte and the marshalled entries; the
  oracle's Message.Unmarshal and the protobuf library read the fields back.
- the append-mode constants of the ABI: header, abi.py and the loaded library.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from etcd_amd import abi
from etcd_amd.splice import entries_run, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_out", "wire_out_app_vectors.npz")


def test_wire_out_app_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_out_app_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_out_app_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_out_app ok" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes_and_splices():
    from oracle.pyoracle import unmarshal_message
    from .golden.make_wire_out_app_vectors import build, entries_of, vectors
    from .golden.make_wire_out_vectors import EDGES
    from .wire_util import _entry, gogo_marshal, pb_classes
    z = np.load(FIXTURE)
    fields, off, data, eoff, edata = z["fields"], z["off"], z["data"], z["eoff"], z["edata"]
    rows = vectors()
    assert 6 * len(EDGES) <= len(rows) <= 1000 and np.array_equal(fields[:, :7], np.array(rows, dtype=np.uint64))
    for col in range(6):  # every edge in to, from, term, logTerm, index, commit
        assert set(EDGES) <= set(fields[:, col].tolist()), col
    assert set(fields[:, 6].tolist()) == {0, 1, 3}
    bare = (np.diff(off) - np.diff(eoff)).astype(np.int64)
    assert bare.min() == 28 and bare.max() == 82 and int(off[-1]) == len(data) and int(eoff[-1]) == len(edata)
    assert int(fields[:, 7].max()) == 57 and int(fields[:, 7].min()) == 12
    raw, eraw = data.tobytes(), edata.tobytes()
    M = pb_classes()["Message"]
    for i, row in enumerate(rows):
        to, frm, term, lt, idx, com, n = row
        full, run, prefix = build(row, i)
        assert raw[int(off[i]):int(off[i + 1])] == full and eraw[int(eoff[i]):int(eoff[i + 1])] == run, i
        assert prefix == int(fields[i, 7])
        # what hb_encode writes for the record, and the helper's splice of it
        rec = gogo_marshal(abi.HB_MSG_APP, to=to, frm=frm, term=term, log_term=lt, index=idx, commit=com)
        ents = [_entry(e) for e in entries_of(term, idx, n, i)]
        assert entries_run(ents) == run
        status = (abi.HB_WIRE_SPLICE | prefix) if n else abi.HB_WIRE_OK
        assert splice(rec, status, ents) == full, i
        assert splice(rec, abi.HB_WIRE_SPLICE | prefix, []) == rec  # (an empty run: the record itself)
        rc, m = unmarshal_message(full)
        assert rc == 0, i
        assert (m.type, m.to, m.from_, m.term, m.log_term, m.index, m.commit, m.reject, m.reject_hint, m.nentries) == \
            (abi.HB_MSG_APP, to, frm, term, lt, idx, com, 0, 0, n), i
        p = M.FromString(full)
        assert (p.type, p.to, getattr(p, "from"), p.term, p.logTerm, p.index, p.commit, p.reject, p.rejectHint) == \
            (abi.HB_MSG_APP, to, frm, term, lt, idx, com, False, 0), i
        assert [(e.Term, e.Index) for e in p.entries] == [(term, (idx + 1 + k) & ((1 << 64) - 1)) for k in range(n)], i
    with pytest.raises(ValueError):
        splice(b"\x08\x03", abi.HB_WIRE_OK, [b"x"])
    with pytest.raises(ValueError):
        splice(b"\x08\x03", abi.HB_WIRE_SPLICE | 9, [b"x"])


def test_append_mode_constants():
    assert (abi.HB_EGRESS_APPS, abi.HB_OUT_ENTS, abi.HB_WIRE_SPLICE) == (4, 0x800, 0x80)
    assert abi.HB_EGRESS_APPS & (abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES) == 0
    # bit 11 of info is free: not a bit of HB_INFO, HB_INFO_VOTED or HB_OUT_HOST
    assert abi.HB_OUT_ENTS & (abi.HB_INFO_VOTED | abi.HB_OUT_HOST | abi.hb_info(0xF, 0xF, True)) == 0
    # the status byte: no other status has bit 7, and a prefix (at most 57 bytes) fits below it
    assert all(s < abi.HB_WIRE_SPLICE for s in (abi.HB_WIRE_OK, abi.HB_WIRE_HOST, abi.HB_WIRE_ERROR, abi.HB_WIRE_PANIC,
                                                 abi.HB_WIRE_BADGROUP))
    txt = open(os.path.join(ROOT, "include", "hipbatch.h")).read()
    for name, val in (("HB_EGRESS_APPS", "4"), ("HB_OUT_ENTS", "0x800u"), ("HB_WIRE_SPLICE", "0x80"),
                      ("HB_ABI_VERSION", str(abi.HB_ABI_VERSION))):
        assert re.search(rf"^#define\s+{name}\s+{val}\b", txt, re.M), name
    wo = open(os.path.join(ROOT, "etcd_amd", "csrc", "hipbatch_wire_out.h")).read()
    assert "WO_PREFIX_MAX == 57" in wo
    from etcd_amd import hipbatch
    L = hipbatch.lib()  # loads without touching the GPU
    # append mode is an addition inside the ABI number the suite pins: the library says which bits it knows
    assert L.hb_abi_version() == abi.HB_ABI_VERSION == 8
    assert L.hb_egress_caps() == abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES | abi.HB_EGRESS_APPS
    assert L.hb_egress_mode(None) == abi.HB_EINVAL
