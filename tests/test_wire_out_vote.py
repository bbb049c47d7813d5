"""CPU tests of the MsgVote records of wire egress's encoder core (no GPU calls).

- etcd_amd/csrc/hipbatch_wire_out.h under AddressSanitizer + UBSan:
  tests/asan/wire_out_vote_asan.cpp is a stand-alone program (its own main) that
  checks wo_size and wo_write against tests/golden/wire_out/wire_out_vote_vectors.npz
  (MsgVote through tests/wire_util.gogo_marshal, every varint-length edge of a
  u64 in to / from / term / logTerm / index) and writes each record into a heap
  buffer of exactly wo_size bytes.  Built and run as tests/test_wire_out.py
  does: no preloaded runtime, nothing loaded into Python.
- the fixture is what its generator makes, the oracle's Message.Unmarshal and the
  protobuf library read every vector's fields back.
- the vote-mode constants of the ABI and hb_egress_mode, by which a caller tells that a library has it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from etcd_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_out", "wire_out_vote_vectors.npz")


def test_wire_out_vote_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_out_vote_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_out_vote_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_out_vote ok" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes_and_unmarshals():
    from oracle.pyoracle import unmarshal_message
    from .golden.make_wire_out_vectors import EDGES
    from .golden.make_wire_out_vote_vectors import vectors
    from .wire_util import gogo_marshal, pb_classes
    z = np.load(FIXTURE)
    fields, off, data = z["fields"], z["off"], z["data"]
    rows = vectors()
    assert 5 * len(EDGES) <= len(rows) <= 1000 and np.array_equal(fields, np.array(rows, dtype=np.uint64))
    assert set(fields[:, 0].tolist()) == {abi.HB_MSG_VOTE} and not fields[:, 6:].any()
    for col in range(1, 6):  # every edge in to, from, term, logTerm, index
        assert set(EDGES) <= set(fields[:, col].tolist()), col
    lens = np.diff(off).astype(np.int64)
    assert lens.min() == 28 and lens.max() == 73 and int(off[-1]) == len(data)
    raw = data.tobytes()
    M = pb_classes()["Message"]
    for i, (t, to, frm, term, lt, idx, com, rej, hint) in enumerate(rows):
        rec = raw[int(off[i]):int(off[i + 1])]
        assert rec == gogo_marshal(t, to=to, frm=frm, term=term, log_term=lt, index=idx), i
        rc, m = unmarshal_message(rec)
        assert rc == 0, i
        assert (m.type, m.to, m.from_, m.term, m.log_term, m.index, m.commit, m.reject, m.reject_hint, m.nentries) == \
            (t, to, frm, term, lt, idx, 0, 0, 0, 0), i
        p = M.FromString(rec)
        assert (p.type, p.to, getattr(p, "from"), p.term, p.logTerm, p.index, p.commit, p.reject, p.rejectHint) == \
            (t, to, frm, term, lt, idx, 0, False, 0), i


def test_vote_mode_constants():
    assert (abi.HB_EGRESS_ON, abi.HB_EGRESS_VOTES, abi.HB_OUT_HOST) == (1, 2, 0x400)
    assert abi.HB_OUT_HOST & (abi.HB_INFO_VOTED | abi.hb_info(0xF, 0xF, True)) == 0
    txt = open(os.path.join(ROOT, "include", "hipbatch.h")).read()
    for name, val in (("HB_EGRESS_ON", "1"), ("HB_EGRESS_VOTES", "2"), ("HB_OUT_HOST", "0x400u")):
        assert re.search(rf"^#define\s+{name}\s+{val}\b", txt, re.M), name
    from etcd_amd import hipbatch
    L = hipbatch.lib()  # loads without touching the GPU
    # vote mode is an addition inside the ABI number the suite pins: the symbol tells it is there
    assert L.hb_abi_version() == abi.HB_ABI_VERSION and hasattr(L, "hb_egress_mode")
    assert L.hb_egress_mode(None) == abi.HB_EINVAL
