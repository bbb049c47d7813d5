"""CPU tests of hb_encode_ents' encoder core and host side (no GPU calls).

- etcd_amd/csrc/hipbatch_wire_out.h under AddressSanitizer + UBSan:
  tests/asan/wire_out_ents_asan.cpp is a stand-alone program (its own main) that checks
  wo_entry_size / wo_entry_head and whole messages against
  tests/golden/wire_out/wire_out_ents_vectors.npz, wo_ents_covered on a table of window
  and range cases, and the payload copy plan lane by lane.  Built and run as
  tests/test_wire_out_app.py runs its harness: no preloaded runtime, nothing loaded
  into Python.
- the fixture is what its generator makes; etcd_amd.splice.entry_bytes equals
  wire_util._entry; the oracle's Message.Unmarshal and the protobuf library read every
  whole message back.
- the reference of the GPU tests (tests/encode_ents_util.py) against the oracle's own
  r.msgs through the scenarios of tests/egress_app_cases.py.
- constants, the layout of hb_ent_source, and the argument checks a call without a
  handle reaches.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from etcd_amd import abi
from etcd_amd.splice import entry_bytes, source_covers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wire_out", "wire_out_ents_vectors.npz")
HDR = os.path.join(ROOT, "include", "hipbatch.h")


def test_wire_out_ents_under_asan_ubsan():
    exe = os.path.join(ROOT, "oracle", "build", "wire_out_ents_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "wire_out_ents_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0 and "wire_out_ents ok" in out, out[-3000:]
    assert "coverage ok" in out and "copy plan ok: 21760 cases" in out, out[-3000:]


def test_fixture_is_what_the_generator_makes_and_reads_back():
    from oracle.pyoracle import unmarshal_message
    from .golden.make_wire_out_ents_vectors import DATA_LENS, arrays, build
    from .golden.make_wire_out_vectors import EDGES
    from .wire_util import _entry, pb_classes
    z = np.load(FIXTURE)
    want = arrays()
    assert set(z.files) == set(want)
    for k, v in want.items():
        assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k
    assert os.path.getsize(FIXTURE) < 1 << 20
    pd, ents, msgs, raw, heads, whole = build()
    # coverage of the table
    for col in (1, 2):  # every edge in Term and in Index
        assert set(EDGES) <= {e[col] for e in ents}, col
    assert {e[3] for e in ents} == set(DATA_LENS) and {e[0] for e in ents} == {0, 1}
    assert {None, 0, 1, 15, 16, 17, 16383, 16384, 70000} | set(range(117, 131)) == set(DATA_LENS)
    sizes = {len(r) for r in raw}
    assert 127 in sizes and 128 in sizes  # both sides of the 1 / 2-byte edge of varint(Entry.Size())
    assert sorted({m[7] - m[6] for m in msgs}) == [0, 1, 3, 300]
    # etcd_amd.splice.entry_bytes is Entry.MarshalTo
    for (t, term, index, ln, poff), r, h in zip(ents, raw, heads):
        data = None if ln is None else pd[poff:poff + ln].tobytes()
        assert r == _entry((t, term, index, data))
        desc = abi.hb_ent_desc(ln or 0, t, ln is not None)
        assert entry_bytes(desc, term, index, b"" if data is None else data) == r
        assert abi.entry_size(desc, term, index) == len(r)
        assert h == b"\x3a" + _varint(len(r)) + r[:len(r) - (ln or 0)]
    with pytest.raises(ValueError):
        entry_bytes(abi.hb_ent_desc(4, 0, True), 1, 1, b"abc")
    # the oracle's Unmarshal and the protobuf library read every whole message back
    M = pb_classes()["Message"]
    for (to, frm, term, lt, idx, com, e0, e1), full in zip(msgs, whole):
        rc, m = unmarshal_message(full)
        assert rc == 0
        assert (m.type, m.to, m.from_, m.term, m.log_term, m.index, m.commit, m.reject, m.reject_hint, m.nentries) == \
            (abi.HB_MSG_APP, to, frm, term, lt, idx, com, 0, 0, e1 - e0)
        p = M.FromString(full)
        assert (p.type, p.to, getattr(p, "from"), p.term, p.logTerm, p.index, p.commit, p.reject, p.rejectHint) == \
            (abi.HB_MSG_APP, to, frm, term, lt, idx, com, False, 0)
        assert len(p.entries) == e1 - e0
        for e, (t, eterm, index, ln, poff) in zip(p.entries, ents[e0:e1]):
            assert (e.Type, e.Term, e.Index) == (t, eterm, index)
            assert e.HasField("Data") == (ln is not None)
            assert e.Data == (b"" if ln is None else pd[poff:poff + ln].tobytes())


def _varint(v):
    from etcd_amd.splice import varint
    return varint(v)


def test_source_covers_boundaries():
    """The host's restatement of the coverage rule, on the boundaries the GPU tests use."""
    desc = [abi.hb_ent_desc(16, 0, True)] * 12
    at = [16 * k for k in range(12)]
    cov = lambda *a, **kw: source_covers(*a, **dict(dict(edesc=desc, edata=at, data_len=192), **kw))  # noqa: E731
    assert cov(10, 13, 11, 3, 4, 12) == 4           # exact fit
    assert cov(10, 12, 9, 6, 2, 12) == 4            # inside a longer window
    assert cov(10, 11, 11, 0, 0, 12) is None        # count 0
    assert cov(10, 13, 12, 3, 0, 12) is None        # the window starts at index + 2
    assert cov(10, 13, 11, 2, 0, 12) is None        # the window ends at hint - 1
    assert cov(10, 13, 11, 3, 9, 12) == 9           # start + count == n_ent
    assert cov(10, 13, 11, 3, 10, 12) is None       # one past
    assert cov(10, 13, 11, 3, 9, 12, data_len=191) is None  # the last payload ends one past data_len
    assert cov(10, 10, 11, 3, 0, 12) is None and cov(10, 9, 5, 8, 0, 12) is None  # hint <= index
    big = (1 << 64) - 1
    assert cov(big - 1, big, big, 1, 0, 12) == 0 and cov(10, 11, 11, 1, big, 12) is None
    nil = [abi.hb_ent_desc(0, 1, False)] * 2
    assert source_covers(7, 9, 8, 2, 0, 2, nil, [big, big], 0) == 0  # no Data: edata is not looked at


def test_reference_equals_the_oracles_messages():
    """encode_ents_reference with a source that covers every log, on the scenario step: every
    HB_OUT_ENTS record that is not flagged comes out HB_WIRE_OK and is gogo_marshal of the oracle's
    message with its entries; the flagged counts are the ones each case states."""
    from . import egress_app_cases as AC
    from .egress_app_util import entry_tuple, is_app, replay_apps
    from .egress_util import by_group
    from .egress_vote_util import oracle_older_runs
    from .encode_ents_util import encode_ents_reference, log_source
    from .test_egress_app_replay import _oracle_groups, _step_all
    from .wire_util import gogo_marshal
    cases = AC.scenarios()
    rafts = [AC.build(c) for c in cases]
    og, peers, batch = _oracle_groups(rafts, cases)
    before, older = og.groups(), oracle_older_runs(og)
    ev, _ = og.step(batch)
    got = by_group(replay_apps(ev, before, older, peers, 1))
    want = _step_all(rafts, cases)  # (the Raft objects are stepped here: log_source reads the logs after it)
    assert len(got) == len(want)
    src = log_source(rafts)
    recs, off, st = encode_ents_reference(got, src)
    assert int(off[-1]) == sum(len(r) for r in recs)
    flagged, whole = {}, 0
    for rec, raw, s, w in zip(got, recs, st, want):
        g = rec[0]
        if rec[11]:
            assert s == abi.HB_WIRE_HOST and raw == b""
            if is_app(rec):
                flagged[cases[g]["name"]] = flagged.get(cases[g]["name"], 0) + 1
            continue
        if rec[2] == abi.HB_REF_OTHER:
            assert s == abi.HB_WIRE_HOST
            continue
        assert s == abi.HB_WIRE_OK, (cases[g]["name"], rec)  # no HB_WIRE_SPLICE is left
        _, mtype, to_ref, to, frm, term, lt, index, commit, reject, hint, lo, hi = w
        ents = [entry_tuple(g, j, rafts[g].term(j)) for j in range(lo, hi + 1)] if hi else []
        assert raw == gogo_marshal(mtype, to=to, frm=frm, term=term, log_term=lt, index=index, entries=ents,
                                   commit=commit, reject=reject, hint=hint), (cases[g]["name"], rec)
        whole += bool(rec[12])
    assert flagged == {c["name"]: c["flagged"] for c in cases if c["flagged"]}
    assert whole > 30
    # without a window every such record keeps the split form
    src["count"][:] = 0
    _, _, st0 = encode_ents_reference(got, src)
    assert sum(bool(s & abi.HB_WIRE_SPLICE) for s in st0) == whole


def test_encode_ents_constants_and_layout():
    assert abi.HB_ENCODE_ENTS == 1
    txt = open(HDR).read()
    for name, val in (("HB_ENCODE_ENTS", "1"), ("HB_ABI_VERSION", "8")):
        assert re.search(rf"^#define\s+{name}\s+{val}\b", txt, re.M), name
    from etcd_amd import hipbatch
    L = hipbatch.lib()  # loads without touching the GPU
    assert L.hb_abi_version() == abi.HB_ABI_VERSION == 8
    assert L.hb_encode_caps() == abi.HB_ENCODE_ENTS
    assert L.hb_egress_caps() == abi.HB_EGRESS_ON | abi.HB_EGRESS_VOTES | abi.HB_EGRESS_APPS
    assert L.hb_decode_caps() == abi.HB_DECODE_FOLLOW
    fields = [f for f, _ in abi.hb_ent_source._fields_]
    assert fields == ["first", "count", "start", "n_ent", "eterm", "edesc", "edata", "data", "data_len"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "hipbatch.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(hb_ent_source));\n' +
           "".join(f'  printf(" %zu", offsetof(hb_ent_source, {f}));\n' for f in fields) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HDR), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.hb_ent_source)] + [getattr(abi.hb_ent_source, f).offset for f in fields]
    # the encoder core's constants the kernels rely on
    wo = open(os.path.join(ROOT, "etcd_amd", "csrc", "hipbatch_wire_out.h")).read()
    assert "WO_ENTRY_HEAD_MAX = 1 + 5 + 2 + 11 + 11 + 6" in wo


def test_encode_ents_without_a_handle_is_invalid():
    """The handle is checked before anything is read or launched: HB_EINVAL with valid-looking
    arguments and no handle.  (The other HB_EINVAL cases need a handle: tests/test_encode_ents_gpu.py.)"""
    from etcd_amd import hipbatch
    L = hipbatch.lib()
    z = np.zeros(4, np.uint64)
    b = abi.hb_out_batch()
    for name, _ in abi.OUT_BATCH_FIELDS:
        setattr(b, name, z.ctypes.data)
    s = abi.hb_ent_source()
    s.first = s.count = s.start = z.ctypes.data
    assert L.hb_encode_ents(None, C.byref(b), 1, None, 1, C.byref(s), None, 0, z.ctypes.data, z.ctypes.data,
                            z.ctypes.data) == abi.HB_EINVAL
    assert L.hb_encode_ents(None, None, 0, None, 0, None, None, 0, None, None, None) == abi.HB_EINVAL
