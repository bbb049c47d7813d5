"""CPU tests of the canonical-shape parser of wire ingestion's follower side (no GPU calls).

- etcd_amd/csrc/hipbatch_wire_in.h under AddressSanitizer + UBSan:
  tests/asan/wire_in_asan.cpp is a stand-alone program (its own main) that runs
  wi_message / wi_header / wi_entry / wi_tail over
  tests/golden/wire_in/wire_in_vectors.npz, each record in a heap buffer of exactly
  its length, and over every truncation of a dozen records (refused, and no read
  past the buffer).  Built and run as tests/test_wire_out_app.py does: no preloaded
  runtime, nothing loaded into Python.
- the fixture is what its generator makes, holds the cases the contract names, and
  the Python reference parser (tests/ingest_util.canonical_entries) reads the same
  entries from it as the fixture records.
"""
import os
import subprocess

import numpy as np
import pytest

from etcd_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_in", "wire_in_vectors.npz")


def test_wire_in_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_in_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_in_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_in ok" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes():
    from .golden.make_wire_in_vectors import DATA_LENS, EDGES, build
    from .ingest_util import canonical_entries
    from .wire_util import varint
    z = np.load(FIXTURE)
    made = build()
    assert set(z.files) == set(made)
    for k, a in made.items():
        assert z[k].dtype == a.dtype and np.array_equal(z[k], a), k
    assert os.path.getsize(FIXTURE) < 1 << 20
    fields, off, eoff = z["fields"], z["off"], z["eoff"]
    canon = fields[:, 9] == 1
    app = canon & (fields[:, 0] == abi.HB_MSG_APP)
    assert {len(varint(v)) for v in EDGES} == set(range(1, 11))
    for col in (3, 4, 5, 6):  # every edge in term, logTerm, index, commit
        assert set(EDGES) <= set(fields[app, col].tolist()), col
    assert set(EDGES) <= set(z["eterm"].tolist())
    ne = np.diff(eoff)
    assert {0, 1, 3, 300} <= set(ne[canon].tolist()) and not ne[~canon].any()
    lens = (z["edesc"] & np.uint32(abi.HB_ENT_MAX_DATA)).tolist()
    has = (z["edesc"] >> np.uint32(31)).astype(bool)
    assert {x for x in DATA_LENS if x is not None} <= set(lens) and (~has).any() and (has & (z["edesc"] << 2 == 0)).any()
    assert set(((z["edesc"] >> np.uint32(30)) & np.uint32(1)).tolist()) == {0, 1}
    assert {abi.HB_MSG_APP, abi.HB_MSG_HEARTBEAT, abi.HB_MSG_VOTE} <= set(fields[canon, 0].tolist())
    raw = z["data"].tobytes()
    for i in range(len(fields)):
        ents = canonical_entries(raw[int(off[i]):int(off[i + 1])])
        if not canon[i]:
            assert ents is None, i
            continue
        assert ents is not None and len(ents) == ne[i], i
        e0 = int(eoff[i])
        for k, (term, desc, pos) in enumerate(ents):
            assert (term, desc, pos) == (z["eterm"][e0 + k], z["edesc"][e0 + k], z["epos"][e0 + k]), (i, k)
