"""CPU tests of forwarded proposals on the wire path (no GPU calls).

- the contract of hb_set_wire_props: the three symbols, the constants in the header and in
  abi.py, HB_EINVAL without a handle or with a bit the library does not know, and the values
  that must not move (the library loads without touching the GPU);
- the proposal rule of etcd_amd/csrc/hipbatch_wire_in.h under AddressSanitizer + UBSan:
  tests/asan/wire_props_asan.cpp is a stand-alone program (its own main) over
  tests/golden/wire_in/wire_props_vectors.npz and the follower fixture, built and run as
  tests/test_wire_in.py does: no preloaded runtime, nothing loaded into Python;
- the fixture is what its generator makes, and the decode reference
  (tests/props_util.props_reference) gives it the verdicts and entries it records.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from etcd_amd import abi, hipbatch

from . import props_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "hipbatch.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_in", "wire_props_vectors.npz")
FOLLOW_FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_in", "wire_in_vectors.npz")


def test_symbols_constants_and_invalid_arguments():
    L = hipbatch.lib()
    for sym in ("hb_set_wire_props", "hb_wire_props", "hb_wire_props_caps"):
        assert hasattr(L, sym), sym
    assert (abi.HB_WIRE_PROPS_IN, abi.HB_WIRE_PROPS_OUT) == (1, 2)
    assert L.hb_wire_props_caps() == 3 == abi.HB_WIRE_PROPS_IN | abi.HB_WIRE_PROPS_OUT
    for bits in (0, 1, 2, 3, 4, 8, -1):
        assert L.hb_set_wire_props(None, bits) == abi.HB_EINVAL
    assert L.hb_wire_props(None) == abi.HB_EINVAL
    # a knob of its own: the caps of the calls it changes and the version are what they were
    assert L.hb_decode_caps() == 1 == abi.HB_DECODE_FOLLOW
    assert L.hb_egress_caps() == 7 == abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES | abi.HB_EGRESS_APPS
    assert L.hb_abi_version() == abi.HB_ABI_VERSION == 8
    assert L.hb_egress_limit_caps() == 1 == abi.HB_EGRESS_LIMIT_V1


def test_header_and_abi_agree():
    txt = open(HDR).read()
    for name, val in (("HB_WIRE_PROPS_IN", abi.HB_WIRE_PROPS_IN), ("HB_WIRE_PROPS_OUT", abi.HB_WIRE_PROPS_OUT),
                      ("HB_ABI_VERSION", abi.HB_ABI_VERSION), ("HB_DECODE_FOLLOW", abi.HB_DECODE_FOLLOW)):
        assert re.search(rf"^#define\s+{name}\s+{val}\b", txt, re.M), name
    for proto in (r"int\s+hb_set_wire_props\(hb_handle\* h, int bits\);", r"int\s+hb_wire_props\(hb_handle\* h\);",
                  r"int\s+hb_wire_props_caps\(void\);"):
        assert re.search(proto, txt), proto
    assert hasattr(hipbatch.Engine, "set_wire_props") and hasattr(hipbatch.Engine, "wire_props")


def test_wire_props_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_props_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_props_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE, FOLLOW_FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_props ok" in out and "wire_in unchanged" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes():
    from .golden.make_wire_props_vectors import build
    z = np.load(FIXTURE)
    made = build()
    assert set(z.files) == set(made)
    for k, a in made.items():
        assert z[k].dtype == a.dtype and np.array_equal(z[k], a), k
    assert os.path.getsize(FIXTURE) < 1 << 20
    cases = PU.rule_cases()
    assert len(cases) == len(z["accept"]) and [int(c[1]) for c in cases.values()] == z["accept"].tolist()
    ne = np.diff(z["eoff"])
    assert [c[2] for c in cases.values()] == ne.tolist() and {1, 3, 300} <= set(ne.tolist())
    has = (z["edesc"] >> np.uint32(31)).astype(bool)
    lens = z["edesc"] & np.uint32(abi.HB_ENT_MAX_DATA)
    assert (~has).any() and (has & (lens == 0)).any() and 128 in lens.tolist() and not (z["edesc"] >> 30 & 1).any()


def test_decode_reference_on_the_fixture():
    """props_reference = follow_reference + the rule: the fixture's verdicts and entries with the
    bit on, all HB_WIRE_HOST with it off; a record for a group past the capacity stays the host's."""
    from .ingest_util import follow_reference
    z = np.load(FIXTURE)
    n = len(z["accept"])
    off, data = z["off"][:-1], z["data"]
    length = np.diff(z["off"]).astype(np.uint32)
    peers = np.zeros((2, abi.HB_MAX_REPLICAS), np.uint64)
    peers[:, :3] = (1, 2, 3)
    group = np.zeros(n, np.uint32)
    args = (data, off, length, group, 2, [3, 3], peers)
    base = follow_reference(*args)
    names = list(PU.rule_cases())
    # without the bit no MsgProp is a batch record: the host's, or what Unmarshal makes of a broken one
    assert (base["status"] != abi.HB_WIRE_OK).all() and base["n_ent"] == 0
    assert (base["status"][z["accept"].astype(bool)] == abi.HB_WIRE_HOST).all()
    assert {abi.HB_WIRE_HOST, abi.HB_WIRE_ERROR, abi.HB_WIRE_PANIC} == set(base["status"].tolist())
    assert base["status"][names.index("truncated")] == abi.HB_WIRE_ERROR
    off_ref = PU.props_reference(*args, props=False)
    assert all(np.array_equal(off_ref[k], base[k]) for k in base)
    ref = PU.props_reference(*args)
    acc = z["accept"].astype(bool)
    assert (ref["status"][acc] == abi.HB_WIRE_OK).all() and np.array_equal(ref["status"][~acc], base["status"][~acc])
    assert np.array_equal(ref["eoff"], z["eoff"]) and ref["n_ent"] == len(z["edesc"])
    assert np.array_equal(ref["edesc"], z["edesc"]) and not ref["eterm"].any()
    pos = np.repeat(off, np.diff(z["eoff"]).astype(np.int64)) + z["epos"]
    assert np.array_equal(ref["edata"], np.where(z["epos"] != 0, pos, 0))
    assert np.array_equal(ref["index"][:n][acc], np.diff(z["eoff"])[acc]) and not ref["index"][:n][~acc].any()
    assert not ref["term"].any() and not ref["hint"].any() and not ref["commit"].any()
    slots = (ref["info"][:n][acc] >> 4) & 0xF
    want = [abi.HB_SLOT_NONE if names[i] in ("from a non-member", "from node 0") else 1 for i in np.nonzero(acc)[0]]
    assert slots.tolist() == want and ((ref["info"][:n][acc] & 0xF) == abi.HB_MSG_PROP).all()
    assert (ref["group"][:n][acc] == 0).all() and (ref["group"][:n][~acc] == 0xFFFFFFFF).all() and ref["group"][n] == 0xFFFFFFFF
    far = PU.props_reference(data, off, length, np.full(n, 2, np.uint32), 2, [3, 3], peers)
    assert (far["status"] == base["status"]).all() and far["n_ent"] == 0
