"""GPU parity of framed peer streams: hb_gid_dir_build, hb_frame and hb_unframe
compared bit for bit with etcd_amd/frame.py, which tests/test_frame.py pins to a hand-written
frame and to the C core; then two engines that hold every group at different slots talk through
their frames alone.
"""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import abi, frame, hipbatch

from .cluster_util import receive as _receive, send_chain as _send_chain  # noqa: F401  (the device chain lives there)

pytestmark = pytest.mark.gpu

FILL = 0xAA
GUARD = 64
M64 = (1 << 64) - 1
_TV = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_TV[a.dtype])).cuda()


def _full(n, dt, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=dt, device="cuda")


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _engine(monkeypatch, capacity=8, max_batch=2048, small=True):
    """small=False: HB_SMALL_STEP=0 at hb_create forces the tiled launches."""
    if small:
        monkeypatch.delenv("HB_SMALL_STEP", raising=False)
    else:
        monkeypatch.setenv("HB_SMALL_STEP", "0")
    return hipbatch.Engine(capacity, max_replicas=3, max_batch=max_batch)


def _ids(rng, k):
    """k distinct non-zero 64-bit ids, every one with high bits set."""
    out = set()
    while len(out) < k:
        out.update(int(v) | (1 << 63) for v in rng.integers(1, 1 << 62, size=k - len(out), dtype=np.uint64))
    return np.array(sorted(out), dtype=np.uint64)[rng.permutation(k)]


def _frame_np(gid, length, hole, from_id, to_id, seq=0, nbytes=None):
    """A frame from its columns (numpy; the sender's side of frame.parse_index)."""
    c = len(gid)
    if c == 0:
        return b""
    w = (np.asarray(length, np.uint32) & np.uint32(frame.LEN_MASK)) | (np.asarray(hole, bool).astype(np.uint32) << 31)
    nbytes = int(np.asarray(length, np.uint64).sum()) if nbytes is None else nbytes
    head = frame._HDR.pack(frame.MAGIC, 0, from_id, to_id, seq, nbytes, c, int(np.asarray(hole, bool).sum()))
    return head + np.asarray(gid, "<u8").tobytes() + w.astype("<u4").tobytes() + (b"\0" * 4 if c & 1 else b"")


def _build_dir(eng, gid, cap=None):
    """hb_gid_dir_build of a numpy id column: (GidDir, dups)."""
    import torch
    cap = frame.dir_cap(len(gid)) if cap is None else cap
    d = hipbatch.GidDir(_full(cap, torch.int64, -1), _full(cap, torch.int32, -1), cap)
    dups = _full(1, torch.int32, -1)
    eng.gid_dir_build(_dev(gid), d, dups)
    eng.sync()
    return d, int(_host(dups, np.uint32)[0])


def _unframe(eng, index, frames, d, self_id, bytes_size, n):
    """hb_unframe into pre-filled arrays; host views."""
    import torch
    off, ln, grp = _full(n + 8, torch.int64, -7), _full(n + 8, torch.int32, -7), _full(n + 8, torch.int32, -7)
    fst, unk = _full(len(frames) + 1, torch.int32, -7), _full(1, torch.int64, -7)
    pad = np.frombuffer(bytes(index) + b"\0" * (-len(index) % 8 + 8), np.uint8)
    eng.unframe(self_id, _dev(pad), frames, d, bytes_size, off if n else None, ln if n else None, grp if n else None,
                fst, unk, n=n, index_size=len(index))
    eng.sync()
    off, ln, grp = _host(off, np.uint64), _host(ln, np.uint32), _host(grp, np.uint32)
    for a in (off, ln, grp):  # nothing past row n
        assert (a[n:] == a.dtype.type((1 << 8 * a.itemsize) - 7)).all()
    fs = _host(fst, np.uint32)
    assert fs[len(frames)] == np.uint32(-7 % (1 << 32))
    return off[:n], ln[:n], grp[:n], fs[:len(frames)], int(_host(unk, np.uint64)[0])


# ---- 1. the directory ------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 100000])
def test_gid_dir_build_and_lookup(monkeypatch, count):
    """Every id is found at its slot and 1,000 absent ids are found absent: hb_unframe of one frame
    that lists them all is the device lookup."""
    rng = np.random.default_rng(count)
    ids = _ids(rng, count + 1000)
    col, absent = ids[:count].copy(), ids[count:]
    if count >= 64:
        col[rng.choice(count, 5, replace=False)] = 0  # empty slots are skipped
    eng = _engine(monkeypatch, max_batch=1 << 17)
    d, dups = _build_dir(eng, col)
    assert d.cap == frame.dir_cap(count) and dups == 0
    ask = np.concatenate([col, absent])[rng.permutation(count + 1000)]
    n = len(ask)
    fr = _frame_np(ask, np.ones(n, np.uint32), np.zeros(n, bool), 5, 9)
    off, ln, grp, fst, unk = _unframe(eng, fr, [(0, len(fr), 0, n, 5)], d, 9, n, n)
    slot = {int(g): i for i, g in enumerate(col) if g}
    want = np.array([slot.get(int(g), frame.NO_SLOT) for g in ask], np.uint32)
    assert fst[0] == abi.HB_FRAME_OK
    assert np.array_equal(grp, want) and unk == 1000
    assert np.array_equal(ln, (want != frame.NO_SLOT).astype(np.uint32)) and np.array_equal(off, np.arange(n, dtype=np.uint64))
    # the table itself: every key once, at a place its probe run reaches (frame.Directory.lookup on the device's table)
    if count <= 4097:
        ref = frame.Directory([], d.cap)
        ref.key = [int(v) for v in _host(d.key, np.uint64)]
        ref.slot = [int(v) for v in _host(d.slot, np.uint32)]
        assert sorted(k for k in ref.key if k) == sorted(slot)
        assert all(ref.lookup(g) == s for g, s in slot.items())
    eng.close()


def test_gid_dir_dups_and_cap_checks(monkeypatch):
    eng = _engine(monkeypatch, max_batch=4096)
    rng = np.random.default_rng(3)
    col = _ids(rng, 300)
    col[[10, 200, 299]] = col[[7, 7, 150]]  # three repeats (one id three times)
    d, dups = _build_dir(eng, col)
    assert dups == 3
    fr = _frame_np(col, np.ones(300, np.uint32), np.zeros(300, bool), 5, 9)
    _, _, grp, fst, unk = _unframe(eng, fr, [(0, len(fr), 0, 300, 5)], d, 9, 300, 300)
    assert fst[0] == 0 and unk == 0
    for i, s in enumerate(grp):
        assert col[s] == col[i] and (s == i or i in (7, 10, 200, 150, 299))
    L = hipbatch.lib()
    z = _dev(np.zeros(1024, np.uint64))
    p = z.data_ptr()
    call = lambda count, cap: L.hb_gid_dir_build(eng.h, p, count, p + 2048, p + 4096, cap, p + 6144)  # noqa: E731
    assert call(1, 64) == abi.HB_OK and call(32, 64) == abi.HB_OK and call(0, 64) == abi.HB_OK
    assert call(1, 32) == call(1, 96) == call(33, 64) == call(1, 0) == call(1, 63) == abi.HB_EINVAL
    assert L.hb_gid_dir_build(eng.h, None, 1, p, p, 64, p) == L.hb_gid_dir_build(eng.h, p, 1, None, p, 64, p) == \
        L.hb_gid_dir_build(eng.h, p, 1, p, None, 64, p) == L.hb_gid_dir_build(eng.h, p, 1, p, p, 64, None) == abi.HB_EINVAL
    eng.sync()
    eng.close()


# ---- 2. hb_frame -----------------------------------------------------------------------------
CAPACITY = 300
BIN_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257)


def _binned(rng, peers, sizes, other=5, gap_at=None):
    """A hand-made binned batch: sizes[b] records for ids[b], `other` records behind them; off[] is
    synthetic (no message bytes are needed).  Hole sources are mixed in: HB_WIRE_HOST records of
    length 0, HB_WIRE_SPLICE records, groups past capacity, groups whose id is 0."""
    ids = _ids(rng, peers)
    n = int(sum(sizes)) + other
    bin_off = np.concatenate([[0], np.cumsum(list(sizes) + [other])]).astype(np.uint64)
    to = np.concatenate([np.full(s, ids[b], np.uint64) for b, s in enumerate(sizes)] + [np.zeros(other, np.uint64)])
    group = rng.integers(0, CAPACITY, n).astype(np.uint32)
    group[rng.random(n) < 0.05] = CAPACITY + 3
    group[rng.random(n) < 0.02] = 0xFFFFFFFF
    status = np.zeros(n, np.uint8)
    r = rng.random(n)
    status[r < 0.1] = abi.HB_WIRE_HOST
    status[(r >= 0.1) & (r < 0.2)] = abi.HB_WIRE_SPLICE | 23
    length = rng.integers(28, 92, n).astype(np.uint64)
    length[status == abi.HB_WIRE_HOST] = 0
    if gap_at is not None:
        length[gap_at] = 1 << 31
    off = np.concatenate([[1000], 1000 + np.cumsum(length)]).astype(np.uint64)
    gid = _ids(rng, CAPACITY)
    gid[rng.random(CAPACITY) < 0.1] = 0
    span = off[bin_off.astype(np.int64)]
    return dict(ids=ids, n=n, bin_off=bin_off, to=to, group=group, status=status, off=off, gid=gid, span=span)


def _index_np(b, self_id, seq):
    """frame.build_index's bytes with numpy columns (for batches too large for its loops)."""
    g = b["group"]
    ok = g < CAPACITY
    gid = np.where(ok, b["gid"][np.minimum(g, CAPACITY - 1)], np.uint64(0))
    hole = (b["status"] != abi.HB_WIRE_OK) | ~ok | (gid == 0)
    length = np.diff(b["off"])
    out = b""
    for k in range(len(b["ids"])):
        lo, hi = int(b["bin_off"][k]), int(b["bin_off"][k + 1])
        out += _frame_np(gid[lo:hi], length[lo:hi], hole[lo:hi], self_id, int(b["ids"][k]), seq,
                         int(b["span"][k + 1]) - int(b["span"][k]))
    return out


def _frame(eng, b, self_id=77, seq=0x0102030405060708, index_cap=None, ref=None):
    """hb_frame of a _binned batch into a pre-filled buffer of index_cap bytes (default: exact) that is
    followed by GUARD bytes."""
    import torch
    ref = ref or frame.build_index(b["group"], b["to"], b["off"], b["status"], b["bin_off"], b["span"], b["gid"],
                                   CAPACITY, self_id, seq)
    index_cap = len(ref[0]) if index_cap is None else index_cap
    np_ = len(b["ids"])
    eng.set_egress_peers(b["ids"])
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # noqa: E731  (never an empty tensor: its pointer is NULL)
    batch = {name: _dev(pad(b[name]) if name in b else np.zeros(b["n"] + 1, dt)) for name, dt in abi.OUT_BATCH_FIELDS}
    index = torch.full((index_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ispan, fstat = _full(np_ + 3, torch.int64, -7), _full(np_ + 2, torch.int32, -7)
    eng.frame(self_id, seq, batch, _dev(b["off"]), _dev(pad(b["status"])), _dev(b["bin_off"]), _dev(b["span"]),
              _dev(b["gid"]), index[:index_cap] if index_cap else None, ispan, fstat, index_cap=index_cap)
    eng.sync()
    ispan, fstat = _host(ispan, np.uint64), _host(fstat, np.uint32)
    assert ispan[np_ + 2] == np.uint64(-7 % (1 << 64)) and fstat[np_ + 1] == np.uint32(-7 % (1 << 32))
    return dict(index=index.cpu().numpy(), ispan=ispan[:np_ + 2], fstat=fstat[:np_ + 1], cap=index_cap), ref


def _check_frame(res, ref, ctx, skip_rows_of=()):
    index, ispan, fstat = ref
    assert np.array_equal(res["ispan"], ispan), f"{ctx}: ispan"
    assert np.array_equal(res["fstat"], fstat), f"{ctx}: fstat {res['fstat'][:8]} expected {fstat[:8]}"
    got = res["index"]
    if len(index) > res["cap"]:
        assert (got == FILL).all(), f"{ctx}: bytes written although the total exceeds index_cap"
        return
    assert (got[len(index):] == FILL).all(), f"{ctx}: bytes written past the total"
    for b in range(len(ispan) - 2):
        lo, hi = int(ispan[b]), int(ispan[b + 1])
        if b in skip_rows_of:  # an oversize bin: its rows are unspecified, its header is not
            lo, hi = lo, lo + frame.HEADER
        assert got[lo:hi].tobytes() == index[lo:hi], f"{ctx}: frame of bin {b} ({hi - lo} bytes)"


def _sizes(peers):
    if peers <= 2:
        return None
    # 255 peers: three rounds of the sizes, then short bins (every bin boundary falls in mid-wave)
    return [BIN_SIZES[b % 9] if b < 27 else (0, 1, 2, 3)[b % 4] for b in range(peers)]


@pytest.mark.parametrize("peers", [1, 2, 255])
def test_frame_bins_holes_and_both_paths(monkeypatch, peers):
    rng = np.random.default_rng(100 + peers)
    cases = [_binned(rng, peers, _sizes(peers))] if peers > 2 else \
        [_binned(rng, peers, [s] if peers == 1 else [s, BIN_SIZES[(k + 4) % 9]]) for k, s in enumerate(BIN_SIZES)]
    outs = []
    for small in (True, False):
        eng = _engine(monkeypatch, CAPACITY, 2048, small)  # 2048 x 7 records at most: the small-step rule's side
        got = []
        for k, b in enumerate(cases):
            res, ref = _frame(eng, b)
            _check_frame(res, ref, f"peers {peers} case {k} small {small}")
            assert ref[0] == _index_np(b, 77, 0x0102030405060708)  # (the vectorised reference of the large test)
            got.append(res["index"].tobytes())
        outs.append(got)
        eng.close()
    assert outs[0] == outs[1]


def test_grid_stride_sizes(monkeypatch):
    """Past 2,048 workgroups' worth of rows, ids and keys the launches loop: 600,000 records in two
    bins, and a directory of 600,000 ids."""
    rng = np.random.default_rng(7)
    eng = _engine(monkeypatch, CAPACITY, 1 << 20)
    b = _binned(rng, 2, [350001, 249000], other=999)
    index = _index_np(b, 77, 0x0102030405060708)
    holes = [int(((np.frombuffer(index[lo:hi], "<u4", c, frame.HEADER + 8 * c) >> 31) & 1).sum())
             for lo, hi, c in ((0, frame.isize(350001), 350001), (frame.isize(350001), len(index), 249000))]
    ref = (index, np.array([0, frame.isize(350001), len(index), len(index)], np.uint64), np.array(holes + [0], np.uint32))
    res, ref = _frame(eng, b, ref=ref)
    _check_frame(res, ref, "600,000 records")
    count = 600000
    ids = _ids(rng, count + 1000)
    d, dups = _build_dir(eng, ids[:count])
    assert dups == 0 and d.cap == 1 << 21
    ask = ids[rng.permutation(count + 1000)]
    fr = _frame_np(ask, np.ones(len(ask), np.uint32), np.zeros(len(ask), bool), 5, 9)
    _, ln, grp, fst, unk = _unframe(eng, fr, [(0, len(fr), 0, len(ask), 5)], d, 9, len(ask), len(ask))
    slot = dict(zip(ids[:count].tolist(), range(count)))
    want = np.array([slot.get(g, frame.NO_SLOT) for g in ask.tolist()], np.uint32)
    assert fst[0] == 0 and unk == 1000 and np.array_equal(grp, want)
    eng.close()


def test_frame_oversize_bin(monkeypatch):
    rng = np.random.default_rng(11)
    for small in (True, False):
        eng = _engine(monkeypatch, CAPACITY, 2048, small)
        b = _binned(rng, 3, [65, 70, 66], gap_at=65 + 31)
        b["status"][65 + 31] = abi.HB_WIRE_OK
        res, ref = _frame(eng, b)
        assert ref[2][1] == frame.OVERSIZE and res["fstat"][1] == 0xFFFFFFFF
        assert ref[2][0] != frame.OVERSIZE and ref[2][2] != frame.OVERSIZE
        _check_frame(res, ref, f"oversize small {small}", skip_rows_of=(1,))
        lo = int(ref[1][1])
        assert res["index"][lo:lo + 4].tobytes() == b"\0\0\0\0"  # magic 0: a receiver rejects the frame
        eng.close()


def test_frame_index_cap_one_short_and_exact(monkeypatch):
    rng = np.random.default_rng(13)
    for small in (True, False):
        eng = _engine(monkeypatch, CAPACITY, 2048, small)
        b = _binned(rng, 2, [130, 7])
        total = len(_index_np(b, 77, 0x0102030405060708))
        res, ref = _frame(eng, b, index_cap=total - 1)
        _check_frame(res, ref, "one short")  # nothing written: buffer and guard intact, ispan and fstat written
        res, ref = _frame(eng, b, index_cap=total)
        _check_frame(res, ref, "exact")
        assert res["index"][total - 1] != FILL or ref[0][-1] == FILL
        res, ref = _frame(eng, b, index_cap=0)
        _check_frame(res, ref, "no buffer")
        eng.close()


def test_frame_empty_batch_and_bad_bin_off(monkeypatch):
    import torch
    rng = np.random.default_rng(17)
    for small in (True, False):
        eng = _engine(monkeypatch, CAPACITY, 2048, small)
        b = _binned(rng, 2, [0, 0], other=0)
        res, ref = _frame(eng, b)
        assert len(ref[0]) == 0 and not res["ispan"].any() and not res["fstat"].any()
        # a bin_off that descends, or ends past the handle's largest batch, is read as an empty batch
        b = _binned(rng, 2, [10, 10], other=0)
        for bad in ([0, 10, 5, 5], [0, 10, 20, 2048 * 7 + 1]):
            index = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
            ispan, fstat = _full(4, torch.int64, -7), _full(3, torch.int32, -7)
            batch = {name: _dev(b[name] if name in b else np.zeros(b["n"], dt)) for name, dt in abi.OUT_BATCH_FIELDS}
            eng.set_egress_peers(b["ids"])
            eng.frame(1, 2, batch, _dev(b["off"]), _dev(b["status"]), _dev(np.array(bad, np.uint64)), _dev(b["span"]),
                      _dev(b["gid"]), index, ispan, fstat)
            eng.sync()
            assert (index.cpu().numpy() == FILL).all()
            assert not _host(ispan, np.uint64).any() and not _host(fstat, np.uint32).any()
        eng.close()


# ---- 3. hb_unframe ---------------------------------------------------------------------------
KNOWN = 500


def _rows(rng, n, ids, strangers):
    """n rows: mostly known gids, some unknown, some 0, some holes (with and without bytes)."""
    r = rng.random(n)
    gid = ids[rng.integers(0, len(ids), n)].copy()
    unknown = r < 0.07
    gid[unknown] = strangers[rng.integers(0, len(strangers), int(unknown.sum()))]
    gid[(r >= 0.07) & (r < 0.12)] = 0
    hole = (r >= 0.12) & (r < 0.2)
    length = rng.integers(28, 4000, n).astype(np.uint32)
    length[hole & (rng.random(n) < 0.5)] = 0
    return gid, length, hole


def _stream(rng, n, nf, ids, strangers, self_id=9, edges=None):
    """nf frames that hold n rows between them (empty frames among them when nf > 1), laid out in an
    index buffer with gaps; their byte ranges lie anywhere, one of them above 2^32."""
    cuts = np.sort(rng.integers(0, n + 1, nf - 1)) if nf > 1 else np.zeros(0, np.int64)
    if nf >= 3:
        cuts[0] = cuts[1]  # at least one empty frame
    edges = np.concatenate([[0], np.sort(cuts), [n]]).astype(np.int64) if edges is None else edges
    gid, length, hole = _rows(rng, n, ids, strangers)
    index, frames, boff = b"", [], 64
    for k in range(nf):
        lo, hi = int(edges[k]), int(edges[k + 1])
        sender = 100 + k
        f = _frame_np(gid[lo:hi], length[lo:hi], hole[lo:hi], sender, self_id, seq=k)
        index += b"\xEE" * (8 * int(rng.integers(0, 3)))
        nb = int(length[lo:hi].astype(np.uint64).sum())
        if k == nf // 2:
            boff += (1 << 32) + 12345
        frames.append((len(index), len(f), boff, nb, sender))
        index += f
        boff += nb + int(rng.integers(0, 50))
    return index, frames, boff + 99


N_ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 16384, 16385)


@pytest.mark.parametrize("small", [True, False], ids=["default", "HB_SMALL_STEP=0"])
@pytest.mark.parametrize("n", N_ROWS)
def test_unframe_rows_and_frames(monkeypatch, n, small):
    rng = np.random.default_rng(1000 + n)
    allids = _ids(rng, KNOWN + 50)
    ids, strangers = allids[:KNOWN], allids[KNOWN:]
    eng = _engine(monkeypatch, 8, 1 << 15, small)
    d, dups = _build_dir(eng, ids)
    slot = {int(g): i for i, g in enumerate(ids)}
    assert dups == 0
    for nf in (1, 3, 256):
        index, frames, bsize = _stream(rng, n, nf, ids, strangers)
        ref = frame.unframe(index, frames, 9, lambda g: slot.get(g, frame.NO_SLOT))
        got = _unframe(eng, index, frames, d, 9, bsize, n)
        ctx = f"n {n} frames {nf} small {small}"
        assert np.array_equal(got[3], ref[3]) and not ref[3].any(), f"{ctx}: fstatus {got[3]}"
        for k, name in enumerate(("off", "len", "group")):
            bad = np.nonzero(got[k] != ref[k])[0]
            assert len(bad) == 0, f"{ctx}: {name} at {bad[:5]}: dev {got[k][bad[:5]]} expected {ref[k][bad[:5]]}"
        assert got[4] == ref[4], f"{ctx}: n_unknown {got[4]} expected {ref[4]}"
        if n >= 255:
            assert ref[4] > 0 and (ref[1] == 0).any() and int(ref[0].max()) > 1 << 32
    if n == 0:  # no frame at all
        got = _unframe(eng, b"", [], d, 9, 0, 0)
        assert got[4] == 0
    eng.close()


def _mutations():
    return [("magic", 0, 1, None, abi.HB_FRAME_BAD_MAGIC), ("flags", 5, 0x80, None, abi.HB_FRAME_BAD_MAGIC),
            ("count", 40, 1, None, abi.HB_FRAME_BAD_COUNT), ("to", 23, 0x40, None, abi.HB_FRAME_BAD_ROUTE),
            ("from", 8, 1, None, abi.HB_FRAME_BAD_ROUTE), ("sender", None, 0, "from", abi.HB_FRAME_BAD_ROUTE),
            ("bytes field", 32, 1, None, abi.HB_FRAME_BAD_LENGTH), ("bytes_len + 1", None, 0, "+1", abi.HB_FRAME_BAD_LENGTH),
            ("bytes_len - 1", None, 0, "-1", abi.HB_FRAME_BAD_LENGTH), ("sum + 1", "len", 1, None, abi.HB_FRAME_BAD_LENGTH),
            ("sum - 1", "len", -1, None, abi.HB_FRAME_BAD_LENGTH), ("hole + 1", "hole", 1, None, abi.HB_FRAME_BAD_LENGTH)]


@pytest.mark.parametrize("small", [True, False], ids=["default", "HB_SMALL_STEP=0"])
def test_unframe_bad_frame_beside_good_neighbours(monkeypatch, small):
    """Each fstatus by a one-field change of the middle frame: all its rows are dropped, and the
    neighbours' rows are what they were."""
    rng = np.random.default_rng(5)
    allids = _ids(rng, KNOWN + 50)
    ids, strangers = allids[:KNOWN], allids[KNOWN:]
    eng = _engine(monkeypatch, 8, 1 << 15, small)
    d, _ = _build_dir(eng, ids)
    slot = {int(g): i for i, g in enumerate(ids)}
    look = lambda g: slot.get(g, frame.NO_SLOT)  # noqa: E731
    n = 700
    index, frames, bsize = _stream(rng, n, 4, ids, strangers, edges=[0, 200, 200, 450, 700])  # frame 1 is empty
    mid = 2
    ioff, ilen, boff, blen, sender = frames[mid]
    c = frame.rows(ilen)
    assert c == 250 and frame.rows(frames[0][1]) == 200 and frame.rows(frames[3][1]) == 250
    good = frame.unframe(index, frames, 9, look)
    p = frame.parse_index(index[ioff:ioff + ilen])
    jh = int(np.nonzero(p["hole"])[0][0])
    jl = int(np.nonzero(~p["hole"] & (p["len"] > 1))[0][0])
    base = sum(frame.rows(f[1]) for f in frames[:mid])
    for name, at, x, arg, want in _mutations():
        buf, fr = bytearray(index), list(frames)
        if at == "len" or at == "hole":
            j = jl if at == "len" else jh
            pos = ioff + frame.HEADER + 8 * c + 4 * j
            w = int.from_bytes(buf[pos:pos + 4], "little")
            buf[pos:pos + 4] = ((w & frame.HOLE) | ((w & frame.LEN_MASK) + x)).to_bytes(4, "little")
        elif at is not None:
            buf[ioff + at] ^= x
        if arg == "from":
            fr[mid] = (ioff, ilen, boff, blen, sender + 1)
        elif arg in ("+1", "-1"):
            fr[mid] = (ioff, ilen, boff, blen + int(arg), sender)
        ref = frame.unframe(bytes(buf), fr, 9, look)
        assert ref[3][mid] == want and not np.delete(ref[3], mid).any(), name
        got = _unframe(eng, bytes(buf), fr, d, 9, bsize + 1, n)
        assert np.array_equal(got[3], ref[3]), f"{name}: fstatus {got[3]}"
        for k in range(3):
            assert np.array_equal(got[k], ref[k]), name
            assert np.array_equal(np.delete(got[k], np.s_[base:base + c]), np.delete(good[k], np.s_[base:base + c])), name
        assert not got[0][base:base + c].any() and not got[1][base:base + c].any()
        assert (got[2][base:base + c] == frame.NO_SLOT).all() and got[4] == ref[4], name
    eng.close()


def test_unframe_host_checks(monkeypatch):
    eng = _engine(monkeypatch, 8, 512)
    L = hipbatch.lib()
    z = _dev(np.zeros(8192, np.uint64))
    p = z.data_ptr()
    fr3 = _frame_np([5, 6, 7], [10, 20, 30], [0, 0, 0], 4, 9)
    idx = _dev(np.frombuffer(b"\0" * 8 + fr3 + b"\0" * 8, np.uint8))
    ip = idx.data_ptr()
    good = dict(index=ip, index_size=8 + 88, frames=[(8, 88, 16, 60, 4)], nf=1, dirp=(p, p + 4096, 64), bytes_size=76,
                off=p + 8192, ln=p + 16384, grp=p + 24576, n=3, fst=p + 32768, unk=p + 40000, h=eng.h)

    def call(**kw):
        a = dict(good, **kw)
        f = (abi.hb_frame_in * max(len(a["frames"] or ()), 1))()
        for k, v in enumerate(a["frames"] or ()):
            f[k].index_off, f[k].index_len, f[k].bytes_off, f[k].bytes_len, f[k].from_ = v
        dr = abi.hb_gid_dir(*a["dirp"]) if a["dirp"] else None
        return L.hb_unframe(a["h"], a["index"], a["index_size"], f if a["frames"] is not None else None, a["nf"], 9,
                            C.byref(dr) if dr else None, a["bytes_size"], a["off"], a["ln"], a["grp"], a["n"], a["fst"],
                            a["unk"])

    assert call() == abi.HB_OK
    for name in ("index", "off", "ln", "grp", "fst", "unk", "h", "dirp"):
        assert call(**{name: None}) == abi.HB_EINVAL, name
    assert call(frames=None) == abi.HB_EINVAL
    assert call(dirp=(None, p, 64)) == call(dirp=(p, None, 64)) == call(dirp=(p, p, 96)) == call(dirp=(p, p, 0)) == abi.HB_EINVAL
    assert call(frames=[(4, 88, 16, 60, 4)]) == abi.HB_EINVAL                       # index_off % 8
    assert call(index_size=8 + 87) == abi.HB_EINVAL                                 # the frame ends past the index
    assert call(frames=[(M64 - 7, 88, 16, 60, 4)]) == abi.HB_EINVAL                 # index_off + index_len wraps
    assert call(bytes_size=75) == abi.HB_EINVAL and call(frames=[(8, 88, M64, 60, 4)]) == abi.HB_EINVAL
    assert call(frames=[(8, 80, 16, 60, 4)]) == abi.HB_EINVAL                       # no row count gives 80 bytes
    assert call(n=2) == call(n=4) == abi.HB_EINVAL                                  # n != the rows
    assert call(index=ip + 4) == abi.HB_EINVAL                                      # index not at a multiple of 8
    assert call(frames=[(0, 0, 0, 0, 0)] * 257, nf=257, n=0) == abi.HB_EINVAL       # more than 256 frames
    assert call(frames=[(0, 0, 0, 0, 0)] * 256, nf=256, n=0) == abi.HB_OK
    assert call(frames=[], nf=0, n=0, index=None, off=None, ln=None, grp=None, fst=None, index_size=0) == abi.HB_OK
    big = frame.isize(513)                                                          # n > max_batch
    assert call(frames=[(0, big, 0, 0, 4)], index_size=big, n=513) == abi.HB_EINVAL
    eng.sync()
    eng.close()


# ---- 4. two hops through frames, the slots permuted --------------------------------------------
def test_two_hops_through_frames_with_permuted_slots(monkeypatch):
    """tests/test_encode_ents_gpu.py::test_loopback_device_to_device's scenario, but the receiver gets
    nothing of the sender's arrays: node 2 holds group g at slot perm[g], the two nodes share only the
    64-bit group ids, and each hop is (index span, byte span) into hb_unframe -> hb_decode_follow ->
    step.  Both engines equal their oracles after each hop and the leader's commit advances."""
    from etcd_amd import synth
    from . import wire_util as W
    from .encode_ents_util import encode_ents_reference, records_of
    from .ingest_util import follow_reference
    from .parity_util import Pair, assert_events_equal, assert_groups_equal
    from .test_egress_gpu import _peers, _tap
    from .test_encode_ents_gpu import _source
    from .test_ingest_gpu import _with_sentinel
    monkeypatch.delenv("HB_SMALL_STEP", raising=False)
    G, n, PL = 512, 3, 16
    rng = np.random.default_rng(20240)
    perm = rng.permutation(G).astype(np.uint32)  # node 2's slot of the group node 1 holds at slot g
    inv = np.argsort(perm)
    gid = _ids(rng, G)                           # the MultiNode group ids, by node 1's slots
    gid2 = gid[inv]                              # node 2's column
    g, runs = synth.steady_groups(G, n, seed=231, last_hi=1 << 14)
    lead = _tap(Pair(g, runs, n, 256, max_batch=8 * G, term_runs=True))
    lpeers = _peers(G, n)
    lead.eng.load_peers(lpeers)
    lead.eng.set_egress(True, apps=True)
    lead.eng.set_egress_peers(np.array([2, 3], dtype=np.uint64))
    fg, fruns = synth.follow_groups(G, n, seed=231, last_hi=1 << 14, with_runs=True)
    fol = _tap(Pair(fg[inv], [fruns[int(i)] for i in inv], n, 256, max_batch=8 * G, term_runs=True))
    fpeers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    fpeers[:, :3] = (2, 1, 3)
    fol.eng.load_peers(fpeers)
    fol.eng.set_egress(True)
    fol.eng.set_egress_peers(np.array([1, 3], dtype=np.uint64))
    ldir, ldups = _build_dir(lead.eng, gid)
    fdir, fdups = _build_dir(fol.eng, gid2)
    assert ldups == 0 and fdups == 0
    src = synth.cfg2_entry_source(g, 0, PL)
    before = lead.og.groups()["committed"].copy()
    lead.step(synth.cfg2_batch(g, 0, seed=232), ctx="frames propose")

    # hop 1: node 1 -> node 2
    ch = _send_chain(lead.eng, 1, 41, 8 * G, 2, _dev(gid), dsrc=_source(src), bytes_per=91 + 40 + PL)
    lead.eng.sync()
    nrec = 2 * G
    # the oracle's side, on the CPU: the reference encoder's bytes of the same records, for node 2's slots
    lo, hi = (int(v) for v in _host(ch["bin_off"], np.uint64)[:2])
    assert hi - lo == nrec and int(ch["count"].item()) == 4 * G
    recs_np = {name: ch["out"][name][lo:hi].cpu().numpy().view(dt) for name, dt in abi.OUT_BATCH_FIELDS}
    ref = encode_ents_reference(records_of(recs_np, nrec, 1), src)
    assert (ref[2] == abi.HB_WIRE_OK).all()      # the condition: no hole on this hop
    rdata, roff, rln = W.pack(ref[0])
    fref = follow_reference(rdata, roff, rln, perm[recs_np["group"]], G, np.full(G, n, np.uint32), fpeers)
    assert (fref["status"] == abi.HB_WIRE_OK).all() and fref["n_ent"] == G
    ob = _with_sentinel(None, fref)
    fol.reserve(ob)
    rx = _receive(fol, 2, ch, 0, 1, fdir, nrec, 2 * G)
    dev_ev, dev_st = fol.eng.events(), fol.eng.stats()
    ora_ev, ora_st = fol.og.step(ob)
    assert_events_equal(dev_ev, ora_ev, "frames follower")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_ENTRIES] == G
    assert_groups_equal(fol.eng.get_groups(), fol.og.groups(), "frames follower")
    assert _host(ch["fstat"], np.uint32).tolist() == [0, 0, 0]
    assert int(_host(rx["fst"], np.uint32)[0]) == abi.HB_FRAME_OK and int(rx["unk"].item()) == 0
    assert (rx["dstatus"].cpu().numpy() == abi.HB_WIRE_OK).all() and int(rx["n_ent"].item()) == G
    assert np.array_equal(_host(rx["grp"], np.uint32), perm[recs_np["group"]])
    # the frame on the wire is the host reference's, and the host reference reads it as the device did
    p = frame.parse_index(ch["index"].cpu().numpy()[rx["frames"][0][0]:rx["frames"][0][0] + rx["frames"][0][1]].tobytes())
    assert (p["from_id"], p["to"], p["seq"], p["count"], p["holes"]) == (1, 2, 41, nrec, 0)
    assert np.array_equal(p["gid"], gid[recs_np["group"]]) and np.array_equal(p["len"], rln)

    # hop 2: node 2's MsgAppResp -> node 1
    ch2 = _send_chain(fol.eng, 2, 42, 8 * G, 2, _dev(gid2))
    fol.eng.sync()
    lo2, hi2 = (int(v) for v in _host(ch2["bin_off"], np.uint64)[:2])  # bin 0: node 1
    assert hi2 - lo2 == nrec
    back = {name: ch2["out"][name][lo2:hi2].cpu().numpy().view(dt) for name, dt in abi.OUT_BATCH_FIELDS}
    assert ((back["info"] & 0xF) == abi.HB_MSG_APP_RESP).all() and (back["to"] == 1).all()
    st2 = ch2["status"].cpu().numpy()[lo2:hi2]
    assert (st2 == abi.HB_WIRE_OK).all()         # the condition, checked here before it is relied on
    hoff = _host(ch2["off"], np.uint64)
    hdata = ch2["data"].cpu().numpy()
    msgs = [hdata[int(hoff[i]):int(hoff[i + 1])].tobytes() for i in range(lo2, hi2)]
    bdata, boff, bln = W.pack(msgs)
    lgrp = inv[back["group"]].astype(np.uint32)  # node 1's slots of node 2's records
    lref = follow_reference(bdata, boff, bln, lgrp, G, np.full(G, n, np.uint32), lpeers)
    assert (lref["status"] == abi.HB_WIRE_OK).all() and lref["n_ent"] == 0
    assert (lref["info"][:-1] == abi.hb_info(abi.HB_MSG_APP_RESP, 1, False)).all()
    ob2 = _with_sentinel(None, lref)
    lead.reserve(ob2)
    rx2 = _receive(lead, 1, ch2, 0, 2, ldir, nrec, 0)
    dev_ev, dev_st = lead.eng.events(), lead.eng.stats()
    ora_ev, ora_st = lead.og.step(ob2)
    assert_events_equal(dev_ev, ora_ev, "frames leader ack")
    assert np.array_equal(dev_st, ora_st) and dev_st[abi.HB_STAT_APPRESP] == nrec
    now = lead.og.groups()
    assert_groups_equal(lead.eng.get_groups(), now, "frames leader ack")
    assert (now["committed"] > before).all()
    assert _host(ch2["fstat"], np.uint32).tolist() == [0, 0, 0]
    assert int(_host(rx2["fst"], np.uint32)[0]) == abi.HB_FRAME_OK and int(rx2["unk"].item()) == 0
    assert (rx2["dstatus"].cpu().numpy() == abi.HB_WIRE_OK).all()
    assert np.array_equal(_host(rx2["grp"], np.uint32), lgrp)
    lead.eng.close()
    fol.eng.close()


# ---- 5. hb_frame's argument checks that need a handle ---------------------------------------------
def test_frame_invalid_arguments_with_a_handle(monkeypatch):
    eng = _engine(monkeypatch, 8, 16)
    L = hipbatch.lib()
    z = _dev(np.zeros(8192, np.uint64))
    p = z.data_ptr()
    names = ("batch", "off", "status", "bin_off", "span", "gid", "index", "ispan", "fstat")

    def call(drop=None, index_cap=64, field=None, index=None):
        b = abi.hb_out_batch()
        for name, _ in abi.OUT_BATCH_FIELDS:
            setattr(b, name, None if field == name else p)
        a = {k: p + 4096 * (i + 1) for i, k in enumerate(names)}
        if index is not None:
            a["index"] = index
        if drop:
            a[drop] = None
        return L.hb_frame(eng.h, C.byref(b) if drop != "batch" else None, a["off"], a["status"], a["bin_off"], a["span"],
                          a["gid"], 1, 2, a["index"], index_cap, a["ispan"], a["fstat"])

    assert call() == abi.HB_EINVAL  # no node table yet, as hb_peer_spans
    eng.set_egress_peers(np.array([2, 3], np.uint64))
    assert call() == abi.HB_OK
    for name in names:
        assert call(drop=name) == abi.HB_EINVAL, name
    assert call(drop="index", index_cap=0) == abi.HB_OK
    assert call(field="group") == call(field="to") == abi.HB_EINVAL
    assert call(field="term") == abi.HB_OK  # only group and to are read
    assert call(index=p + 4) == abi.HB_EINVAL
    eng.set_egress_peers(np.zeros(0, np.uint64))
    assert call() == abi.HB_EINVAL
    eng.sync()
    eng.close()
