"""CPU tests of framed peer streams (no GPU calls).

- etcd_amd/csrc/hipbatch_frame.h under AddressSanitizer + UBSan: tests/asan/frame_asan.cpp is a
  stand-alone program (its own main) that checks the frame sizes, the hand frame, the validation
  table and the directory in exactly sized heap buffers.  Built and run as
  tests/test_wire_out_ents.py runs its harness: no preloaded runtime, nothing loaded into Python.
- etcd_amd/frame.py (the GPU tests' reference) against a hand-written frame, against the C core's
  bytes and rows, and against the C core's directory tables.
- constants, struct layouts, hb_frame_size / hb_frame_rows of the library, and the argument
  checks a call without a handle reaches.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from etcd_amd import abi, frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "hipbatch.h")

# node 0x1111 to node 0x2222, seq 7, 75 bytes; rows: (gid C..3, 30 bytes), (gid A..1, 0 bytes, hole),
# (gid B..2, 45 bytes); one pad word because the count is odd
HAND = bytes.fromhex(
    "48424631" "00000000"            # magic "HBF1", flags
    "1111000000000000"               # from
    "2222000000000000"               # to
    "0700000000000000"               # seq
    "4b00000000000000"               # bytes = 75
    "03000000" "01000000"            # count, holes
    "03000000000000c0" "01000000000000a0" "02000000000000b0"   # gid[3]
    "1e000000" "00000080" "2d000000"                           # len[3], bit 31 = hole
    "00000000")                                                # padding
HAND_IN = dict(group=[2, 0, 1], off=[100, 130, 130, 175], status=[abi.HB_WIRE_OK, abi.HB_WIRE_HOST, abi.HB_WIRE_OK],
               gid=[0xA000000000000001, 0xB000000000000002, 0xC000000000000003])


@pytest.fixture(scope="module")
def asan_exe():
    exe = os.path.join(ROOT, "oracle", "build", "frame_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                         os.path.join(ROOT, "tests", "asan", "frame_asan.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in (cc.stderr or "").lower() and "cannot find" in (cc.stderr or "").lower():
        pytest.skip("gcc sanitizer runtimes not installed")
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert "runtime error:" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert r.returncode == 0, out[-3000:]
    return dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())


def test_frame_core_under_asan_ubsan(asan_exe):
    out = _run(asan_exe)
    assert out["frame"] == "ok" and out["directory"] == "ok"
    assert out["sizes"].startswith("ok:") and out["validation"].startswith("ok:")
    # the C core's hand frame is the hex literal, and its rows are the Python reference's
    assert bytes.fromhex(out["hand"]) == HAND
    d = frame.Directory([0xD00D, HAND_IN["gid"][1], 0], 64)
    boff = (1 << 33) + 5
    off, ln, grp, fst, unk = frame.unframe(HAND, [(0, len(HAND), boff, 75, 0x1111)], 0x2222, d.lookup)
    want = "%d %d " % (fst[0], unk) + " ".join("%d:%d:%d" % (o, l, g) for o, l, g in zip(off, ln, grp))
    assert out["rows"] == want
    assert list(ln) == [0, 0, 45] and list(grp) == [frame.NO_SLOT, frame.NO_SLOT, 1] and unk == 1
    assert list(off) == [boff, boff + 30, boff + 30]


def test_isize_rows_round_trip():
    for c in list(range(301)) + [2 ** 32 - 1]:
        s = frame.isize(c)
        assert s % 8 == 0 and frame.rows(s) == c
        if c:
            assert s == 48 + 12 * c + 4 * (c & 1)
    made = set()
    c = 0
    while frame.isize(c) < 4096:
        made.add(frame.isize(c))
        c += 1
    assert all(frame.rows(l) == frame.IMPOSSIBLE for l in range(4096) if l not in made)
    assert frame.rows(frame.isize(2 ** 32 - 1) + 12) == frame.IMPOSSIBLE
    from etcd_amd import hipbatch
    L = hipbatch.lib()
    assert L.hb_frame_caps() == abi.HB_FRAME_V1
    for l in range(4096):
        assert L.hb_frame_rows(l) == frame.rows(l), l
    for c in (0, 1, 2, 3, 300, 2 ** 32 - 1):
        assert L.hb_frame_size(c) == frame.isize(c) and L.hb_frame_rows(frame.isize(c)) == c
    assert L.hb_frame_size(2 ** 32) == 2 ** 64 - 1


def test_hand_frame_build_and_parse():
    h = HAND_IN
    index, ispan, fstat = frame.build_index(h["group"], [0x2222] * 3, h["off"], h["status"], [0, 3, 3], [100, 175, 175],
                                            h["gid"], 3, 0x1111, 7)
    assert index == HAND and list(ispan) == [0, 88, 88] and list(fstat) == [1, 0]
    p = frame.parse_index(HAND)
    assert (p["magic"], p["flags"], p["from_id"], p["to"], p["seq"], p["bytes"], p["count"], p["holes"]) == \
        (frame.MAGIC, 0, 0x1111, 0x2222, 7, 75, 3, 1)
    assert list(p["gid"]) == [h["gid"][2], h["gid"][0], h["gid"][1]]
    assert list(p["len"]) == [30, 0, 45] and list(p["hole"]) == [False, True, False]
    for bad in (HAND[:-1], HAND + b"\0", b""):
        with pytest.raises(ValueError):
            frame.parse_index(bad)
    # the hole rule's other sources and the oversize bin
    g, w, over = frame.row(abi.HB_WIRE_SPLICE | 20, 1, 3, h["gid"], 50)
    assert (g, w, over) == (h["gid"][1], 50 | frame.HOLE, False)
    assert frame.row(abi.HB_WIRE_OK, 3, 3, h["gid"], 50) == (0, 50 | frame.HOLE, False)
    assert frame.row(abi.HB_WIRE_OK, 0, 3, [0, 1, 2], 50) == (0, 50 | frame.HOLE, False)
    assert frame.row(abi.HB_WIRE_OK, 1, 3, h["gid"], 2 ** 31)[2] and not frame.row(0, 1, 3, h["gid"], 2 ** 31 - 1)[2]
    f, st = frame.build_frame([0], [0, 2 ** 31], [0], 0, 1, [9], 1, 1, 2, 0, 2 ** 31)
    assert st == frame.OVERSIZE and frame.parse_index(f)["magic"] == 0
    assert frame.validate(f, 1, 2, 1, 2 ** 31) == abi.HB_FRAME_BAD_MAGIC


def _flip(buf, at, x):
    b = bytearray(buf)
    b[at] ^= x
    return bytes(b)


@pytest.mark.parametrize("name,at,x,self_id,from_id,blen,want", [
    ("good", None, 0, 0x2222, 0x1111, 75, abi.HB_FRAME_OK),
    ("magic", 0, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_MAGIC),
    ("flags", 4, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_MAGIC),
    ("count", 40, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_COUNT),
    ("to", 16, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_ROUTE),
    ("self", None, 0, 0x2223, 0x1111, 75, abi.HB_FRAME_BAD_ROUTE),
    ("from", 8, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_ROUTE),
    ("sender", None, 0, 0x2222, 0x1112, 75, abi.HB_FRAME_BAD_ROUTE),
    ("bytes field", 32, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_LENGTH),
    ("bytes_len + 1", None, 0, 0x2222, 0x1111, 76, abi.HB_FRAME_BAD_LENGTH),
    ("sum + 1", 72, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_LENGTH),
    ("sum - 1", 72, 3, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_LENGTH),
    ("a hole's length counts", 76, 1, 0x2222, 0x1111, 75, abi.HB_FRAME_BAD_LENGTH),
])
def test_validation_table(name, at, x, self_id, from_id, blen, want):
    """The same one-field changes frame_asan.cpp makes to the same frame."""
    f = HAND if at is None else _flip(HAND, at, x)
    assert frame.validate(f, 3, self_id, from_id, blen) == want
    off, ln, grp, fst, unk = frame.unframe(f, [(0, 88, 500, blen, from_id)], self_id, lambda g: 7)
    assert fst[0] == want
    if want != abi.HB_FRAME_OK:
        assert not off.any() and not ln.any() and (grp == frame.NO_SLOT).all() and unk == 0
    else:
        assert list(off) == [500, 530, 530] and list(ln) == [30, 0, 45] and list(grp) == [7, frame.NO_SLOT, 7]


def _bucket(cap, bucket, want, start):
    out, i = [], start
    while len(out) < want:
        if frame.mix(i) & (cap - 1) == bucket:
            out.append(i)
        i += 1
    return out


@pytest.mark.parametrize("case", ["high bits", "one bucket, wrapping", "zero and duplicates", "load 0.5", "full"])
def test_directory_matches_the_c_core(asan_exe, case):
    cap = 64
    if case == "high bits":
        ids = [7] + [(k << 32) | 7 for k in range(1, 32)]
    elif case == "one bucket, wrapping":
        ids = _bucket(cap, cap - 1, 5, 1000)
    elif case == "zero and duplicates":
        ids = [5, 0, 9, 5, 0, 9, 11]
    elif case == "load 0.5":
        ids = [(k * 0x9E3779B97F4A7C15) & (2 ** 64 - 1) for k in range(1, 33)]
    else:
        ids = [(k * 0x9E3779B97F4A7C15) & (2 ** 64 - 1) for k in range(1, 67)]
    out = _run(asan_exe, "dir", str(cap), *(str(i) for i in ids))
    d = frame.Directory(ids, cap)
    assert [int(v) for v in out["key"].split()] == d.key
    assert [int(v) for v in out["slot"].split()] == [s if k else 0 for k, s in zip(d.key, d.slot)]
    first = {}
    for i, g in enumerate(ids):
        if g:
            first.setdefault(g, i)
    placed = set(d.key) - {0}
    dups = sum(1 for i, g in enumerate(ids) if g and first[g] != i)
    assert out["dups"].split() == [str(dups), "full", str(len(first) - len(placed))]
    assert d.dups == dups
    for g, i in first.items():
        assert d.lookup(g) == (i if g in placed else frame.NO_SLOT)
    for g in (1, 2 ** 63, (33 << 32) | 7, 123456789):
        if g not in first:
            assert d.lookup(g) == frame.NO_SLOT  # (the full table: after cap probes)
    if case == "one bucket, wrapping":
        assert d.key[cap - 1] == ids[0] and d.key[:4] == ids[1:] and d.key[4] == 0
    if case == "load 0.5":
        assert len(placed) == cap // 2
    if case == "full":
        assert len(placed) == cap and 0 not in d.key
    assert frame.dir_cap(1) == 64 and frame.dir_cap(32) == 64 and frame.dir_cap(33) == 128


def test_constants_and_layouts():
    assert frame.MAGIC == int.from_bytes(b"HBF1", "little") and abi.HB_FRAME_V1 == 1
    assert (abi.HB_FRAME_OK, abi.HB_FRAME_BAD_MAGIC, abi.HB_FRAME_BAD_COUNT, abi.HB_FRAME_BAD_ROUTE,
            abi.HB_FRAME_BAD_LENGTH) == (0, 1, 2, 3, 4)
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "hipbatch.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(hb_gid_dir), offsetof(hb_gid_dir, slot), offsetof(hb_gid_dir, cap),
         sizeof(hb_frame_in), offsetof(hb_frame_in, from));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HDR), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.hb_gid_dir), abi.hb_gid_dir.slot.offset, abi.hb_gid_dir.cap.offset,
                   C.sizeof(abi.hb_frame_in), abi.hb_frame_in.from_.offset]


def test_argument_checks_without_a_handle():
    from etcd_amd import hipbatch
    L = hipbatch.lib()
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf)
    b = abi.hb_out_batch()
    for name, _ in abi.OUT_BATCH_FIELDS:
        setattr(b, name, p)
    d = abi.hb_gid_dir(p, p, 64)
    f = (abi.hb_frame_in * 1)()
    assert L.hb_gid_dir_build(None, p, 1, p, p, 64, p) == abi.HB_EINVAL
    assert L.hb_frame(None, C.byref(b), p, p, p, p, p, 1, 0, p, 64, p, p) == abi.HB_EINVAL
    assert L.hb_unframe(None, p, 64, f, 1, 1, C.byref(d), 0, p, p, p, 0, p, p) == abi.HB_EINVAL
