"""GPU tests of per-peer egress: hb_set_egress_peers, hb_egress_bin, hb_peer_spans
 against tests/egress_bin_util.bin_reference.

The split is stable, so its output is a pure function of its input and every
comparison is exact: all eight arrays of `out` are `in[order]`, src is `order`,
bin_off is the reference's, nothing at or past n is written and `in` is not
written.  The end-to-end tests chain hb_egress -> hb_egress_bin -> hb_encode ->
hb_peer_spans with no host synchronisation in between and check each peer's
records against the replay of the oracle's events and each peer's byte span
against the reference encoder's restatement.
"""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import abi, synth

from .egress_bin_util import ASAN_SIZES, asan_probes, asan_table, bin_reference, bins_of
from .egress_util import marshal, out_arrays, replay
from .parity_util import Pair
from .test_egress_gpu import DRAWS, _TDT, _follower_steps, _tap

pytestmark = pytest.mark.gpu

FIELDS = abi.OUT_BATCH_FIELDS
CAP_MAX = 4096 * 7  # the handle of the synthetic tests: 256 groups x 3, max_batch 4,096
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 16384, 16385, 5 * 2048 + 777)
TILED_SIZES = (1, 65, 2049, 5 * 2048 + 777)
MIXES = ("uniform", "one-bin", "all-other", "descending")
SENT = {"<u4": 0xA5A5A5A5, "<u8": 0xA5A5A5A5A5A5A5A5}
PAD = 9
M64 = (1 << 64) - 1


def _engine(monkeypatch, small):
    from etcd_amd.hipbatch import Engine
    monkeypatch.setenv("HB_SMALL_STEP", small)
    return Engine(256, max_replicas=3, max_inflight=8, max_batch=4096)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {"uint32": np.int32, "uint64": np.int64}.get(a.dtype.name)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _table(np_ids, seed):
    """A node table of np_ids ids: the sanitizer program's (64-bit edges included), shuffled."""
    return np.random.default_rng(seed).permutation(asan_table(np_ids))


def _unknown(ids, rng, k):
    """k node ids that are not in the table, some one bit away from an id of it."""
    have = set(ids.tolist()) | {0}
    out = []
    while len(out) < k:
        v = int(ids[rng.integers(len(ids))]) ^ (1 << int(rng.integers(64))) if rng.random() < 0.5 \
            else int(rng.integers(1, 1 << 62))
        if v not in have:
            out.append(v)
    return np.array(out, dtype=np.uint64)


def _records(n, ids, mix, seed):
    """n synthetic records (numpy arrays by field) whose destinations follow `mix`."""
    rng = np.random.default_rng(seed)
    nb = len(ids)
    slot = rng.integers(0, 7, n).astype(np.uint32)
    to = np.zeros(n, np.uint64)
    if mix == "uniform":  # 90 % over the table, 5 % unknown ids, 5 % HB_REF_OTHER (to = 0)
        u = rng.random(n)
        to[:] = ids[rng.integers(0, nb, n)]
        unk = (u >= 0.90) & (u < 0.95)
        to[unk] = _unknown(ids, rng, int(unk.sum()))
        oth = u >= 0.95
        to[oth] = 0
        slot[oth] = abi.HB_REF_OTHER
    elif mix == "one-bin":
        to[:] = ids[nb // 2]
    elif mix == "all-other":
        k = n // 2
        to[:k] = _unknown(ids, rng, k)
        slot[k:] = abi.HB_REF_OTHER  # (their `to` is an id of the table: the ref decides)
        to[k:] = ids[rng.integers(0, nb, n - k)]
    elif mix == "descending":  # "other" first, then the table's bins from the last to the first
        b = (nb - (np.arange(n, dtype=np.int64) * (nb + 1)) // max(n, 1)).clip(0, nb)
        known = b < nb
        to[known] = ids[b[known]]
        to[~known] = _unknown(ids, rng, int((~known).sum()))
        assert (np.diff(bins_of(to, np.zeros(n, np.uint32), ids)) <= 0).all()
    typ = rng.choice([abi.HB_MSG_APP_RESP, abi.HB_MSG_HEARTBEAT_RESP, abi.HB_MSG_VOTE_RESP, abi.HB_MSG_HEARTBEAT], n)
    info = (typ.astype(np.uint32) | (slot << np.uint32(4)) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(8)))
    rec = dict(group=rng.integers(0, 256, n).astype(np.uint32), info=info.astype(np.uint32), to=to)
    for name in ("term", "log_term", "index", "commit", "hint"):
        rec[name] = rng.integers(0, 1 << 63, n).astype(np.uint64) << np.uint64(rng.integers(0, 2))
    return rec


def _bin(eng, rec, n, cap, n_dev=None, with_src=True):
    """One hb_egress_bin of the numpy records `rec` (at least cap of them are uploaded);
    returns the host copies of out, src, bin_off and of the input after the call."""
    import torch
    alloc = cap + PAD
    inp, out = {}, {}
    for name, dt in FIELDS:
        a = np.full(alloc, SENT[dt] ^ 0x0F0F0F0F, dtype=dt)
        a[:len(rec[name])] = rec[name]
        inp[name] = _dev(a)
        out[name] = _dev(np.full(alloc, SENT[dt], dtype=dt))
    src = _dev(np.full(alloc, SENT["<u4"], dtype=np.uint32)) if with_src else None
    bin_off = torch.full((abi.HB_EGRESS_MAX_PEERS + 2 + PAD,), -1, dtype=torch.int64, device="cuda")
    before = {name: _host(inp[name], dt).copy() for name, dt in FIELDS}
    eng.egress_bin(inp, cap, out, bin_off, src=src, n_dev=n_dev)
    eng.sync()
    res = {name: _host(out[name], dt) for name, dt in FIELDS}
    res["src"] = _host(src, "<u4") if with_src else None
    res["bin_off"] = _host(bin_off, "<u8")
    for name, dt in FIELDS:
        assert np.array_equal(_host(inp[name], dt), before[name]), f"`in` written: {name}"
    return res


def _check_bin(res, rec, n, ids, ctx):
    order, off = bin_reference(rec["to"][:n], rec["info"][:n], ids)
    nb = len(ids)
    assert np.array_equal(res["bin_off"][:nb + 2], off), f"{ctx}: bin_off {res['bin_off'][:nb + 2]} expected {off}"
    assert (res["bin_off"][nb + 2:] == M64).all(), f"{ctx}: bin_off written past n_peers + 2"
    for name, dt in FIELDS:
        bad = np.nonzero(res[name][:n] != rec[name][:n][order])[0]
        assert len(bad) == 0, f"{ctx}: {name} differs at output records {bad[:5]}"
        assert (res[name][n:] == SENT[dt]).all(), f"{ctx}: {name} written at or past n"
    if res["src"] is not None:
        assert np.array_equal(res["src"][:n], order.astype(np.uint32)), f"{ctx}: src"
        assert (res["src"][n:] == SENT["<u4"]).all(), f"{ctx}: src written at or past n"
    return order, off


# ---- 1. synthetic batches against bin_reference ---------------------------------------------
@pytest.mark.parametrize("np_ids", [1, 3, 64, 255])
@pytest.mark.parametrize("small", ["1", "0"])
def test_synthetic_batches(small, np_ids, monkeypatch):
    """small = "1": sizes up to 16,384 run in one workgroup, 16,385 in the tiled kernels;
    small = "0" (HB_SMALL_STEP=0): the tiled kernels at one tile, ragged tiles, several tiles."""
    import torch
    eng = _engine(monkeypatch, small)
    ids = _table(np_ids, 1000 + np_ids)
    eng.set_egress_peers(ids)
    for n in (SIZES if small == "1" else TILED_SIZES):
        for m, mix in enumerate(MIXES):
            ctx = f"small={small} ids={np_ids} n={n} {mix}"
            rec = _records(n, ids, mix, seed=7 * n + m)
            res = _bin(eng, rec, n, n)
            order, off = _check_bin(res, rec, n, ids, ctx)
            if mix == "uniform":
                cnt = np.diff(off.astype(np.int64))
                if np_ids == 255 and n == 16385:
                    assert (cnt > 0).all(), "every bin of the reference holds a record"
                if np_ids == 255 and n == 65:
                    assert (cnt == 0).any(), "some bins of the reference are empty"
                # the same records behind a device count, the capacity a little larger
                cap = min(n + 5, CAP_MAX)
                more = _records(cap, ids, mix, seed=7 * n + m)  # (a longer draw of the same stream differs: its own check)
                count = torch.tensor([n], dtype=torch.int64, device="cuda")
                _check_bin(_bin(eng, more, n, cap, n_dev=count, with_src=(n % 2 == 0)), more, n, ids, ctx + " n_dev")
    eng.close()


# ---- 2. 64-bit ids: the sanitizer program's tables and probes as a batch --------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_64_bit_ids(small, monkeypatch):
    eng = _engine(monkeypatch, small)
    slot, other = abi.hb_info(abi.HB_MSG_APP_RESP, 2), abi.hb_info(abi.HB_MSG_VOTE_RESP, abi.HB_REF_OTHER, True)
    for np_ids in ASAN_SIZES:
        ids = asan_table(np_ids)
        eng.set_egress_peers(ids)
        p = asan_probes(ids)
        to = np.concatenate([p, p])
        n = len(to)
        rec = {name: np.arange(n, dtype=dt) for name, dt in FIELDS}
        rec["to"] = to
        rec["info"] = np.concatenate([np.full(len(p), slot, np.uint32), np.full(len(p), other, np.uint32)])
        res = _bin(eng, rec, n, n)
        _, off = _check_bin(res, rec, n, ids, f"small={small} asan table {np_ids}")
        b = bins_of(p, rec["info"][:len(p)], ids)
        assert (b[0:4 * np_ids:4] == np.arange(np_ids)).all()  # every id lands in its own bin
        assert int(off[np_ids + 1] - off[np_ids]) >= len(p) + 1  # the HB_REF_OTHER half and the probe 0
    eng.close()


# ---- 3. n_dev -------------------------------------------------------------------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_n_dev(small, monkeypatch):
    import torch
    from etcd_amd.hipbatch import lib
    eng = _engine(monkeypatch, small)
    ids = _table(3, 31)
    eng.set_egress_peers(ids)
    cap = 3000
    rec = _records(cap, ids, "uniform", seed=33)
    # a device count above cap clamps
    count = torch.tensor([cap + 12345], dtype=torch.int64, device="cuda")
    _check_bin(_bin(eng, rec, cap, cap, n_dev=count), rec, cap, ids, "clamped")
    count = torch.tensor([-1], dtype=torch.int64, device="cuda")  # 2^64 - 1
    _check_bin(_bin(eng, rec, cap, cap, n_dev=count), rec, cap, ids, "clamped from 2^64 - 1")
    # NULL means cap
    _check_bin(_bin(eng, rec, cap, cap, n_dev=None), rec, cap, ids, "NULL")
    # a count, and bin_off, in hb_alloc_pinned memory
    p = C.c_void_p()
    assert lib().hb_alloc_pinned(8 * 8, C.byref(p)) == 0
    try:
        n = 2500
        C.c_uint64.from_address(p.value).value = n
        inp = {name: _dev(rec[name]) for name, _ in FIELDS}
        out = {name: _dev(np.full(cap, SENT[dt], dtype=dt)) for name, dt in FIELDS}
        bi, bo = eng._out_batch(inp), eng._out_batch(out)
        assert lib().hb_egress_bin(eng.h, C.byref(bi), cap, p.value, C.byref(bo), None, p.value + 8) == 0
        eng.sync()
        order, off = bin_reference(rec["to"][:n], rec["info"][:n], ids)
        got = np.array([C.c_uint64.from_address(p.value + 8 + 8 * k).value for k in range(5)], dtype=np.uint64)
        assert np.array_equal(got, off)
        for name, dt in FIELDS:
            o = _host(out[name], dt)
            assert np.array_equal(o[:n], rec[name][:n][order]) and (o[n:] == SENT[dt]).all(), name
    finally:
        lib().hb_free_pinned(p)
    eng.close()


# ---- 4, 5. end to end -----------------------------------------------------------------------
def _chain(eng, self_id, cap, nb):
    """hb_egress -> hb_egress_bin -> hb_encode -> hb_peer_spans, one synchronisation at the end."""
    import torch
    t = lambda dt, fill, k=cap: torch.full((max(k, 1),), fill, dtype=dt, device="cuda")  # noqa: E731
    raw = {name: t(getattr(torch, _TDT[dt]), -1) for name, dt in FIELDS}
    out = {name: t(getattr(torch, _TDT[dt]), -1) for name, dt in FIELDS}
    count, total = t(torch.int64, -1, 1), t(torch.int64, -1, 1)
    src, bin_off, span = t(torch.int32, -1), t(torch.int64, -1, nb + 2), t(torch.int64, -1, nb + 2)
    data, off, status = t(torch.uint8, 0xAA, 91 * cap), t(torch.int64, -1, cap + 1), t(torch.uint8, 0xEE)
    eng.egress(self_id, raw, cap, count)
    eng.egress_bin(raw, cap, out, bin_off, src=src, n_dev=count)
    eng.encode(self_id, out, cap, data, off, status, total, n_dev=count)
    eng.peer_spans(off, bin_off, span)
    eng.sync()
    res = dict(raw={name: _host(raw[name], dt) for name, dt in FIELDS},
               out={name: _host(out[name], dt) for name, dt in FIELDS},
               n=int(count.item()), total=int(total.item()), src=_host(src, "<u4"), bin_off=_host(bin_off, "<u8"),
               span=_host(span, "<u8"), data=data.cpu().numpy(), off=_host(off, "<u8"), status=status.cpu().numpy())
    return res


def _tuples(a, n, self_id):
    """Records of out arrays as egress_util tuples."""
    info = a["info"][:n]
    return [(int(a["group"][i]), int(info[i] & 0xF), int((info[i] >> 4) & 0xF), int(a["to"][i]), self_id,
             int(a["term"][i]), int(a["log_term"][i]), int(a["index"][i]), int(a["commit"][i]),
             bool((info[i] >> 8) & 1), int(a["hint"][i])) for i in range(n)]


def _check_chain(res, want, ids, self_id, ctx):
    """want: the replay of the oracle's events, in event order (a group's records in r.msgs order)."""
    n, nb = res["n"], len(ids)
    assert n == len(want) and n <= len(res["src"]), f"{ctx}: count {n} expected {len(want)}"
    # the binned arrays are bin_reference of this call's unbinned records
    order, boff = bin_reference(res["raw"]["to"][:n], res["raw"]["info"][:n], ids)
    assert np.array_equal(res["bin_off"], boff), f"{ctx}: bin_off"
    assert np.array_equal(res["src"][:n], order.astype(np.uint32)), f"{ctx}: src"
    for name, _ in FIELDS:
        assert np.array_equal(res["out"][name][:n], res["raw"][name][:n][order]), f"{ctx}: {name}"
        assert (res["out"][name][n:].view(np.int64 if res["out"][name].itemsize == 8 else np.int32) == -1).all()
    # per peer, per group: the replayed sequence of the messages to that node
    idl = ids.tolist()
    wbin = [nb if (r[2] == abi.HB_REF_OTHER or r[3] not in idl) else idl.index(r[3]) for r in want]
    got = _tuples(res["out"], n, self_id)
    lens = []
    for b in range(nb + 1):
        lo, hi = int(boff[b]), int(boff[b + 1])
        exp = sorted((r for r, wb in zip(want, wbin) if wb == b), key=lambda r: r[0])  # stable: a group's in order
        dev = sorted(got[lo:hi], key=lambda r: r[0])
        assert dev == exp, f"{ctx}: bin {b}: the records of some group differ from the replay"
        # peer b's bytes
        blob = b"".join(marshal(r) for r in got[lo:hi])
        s0, s1 = int(res["span"][b]), int(res["span"][b + 1])
        assert s1 - s0 == len(blob), f"{ctx}: bin {b}: span of {s1 - s0} bytes expected {len(blob)}"
        assert res["data"][s0:s1].tobytes() == blob, f"{ctx}: bin {b}: bytes"
        lens.append(len(blob))
    assert int(res["span"][0]) == 0 and int(res["span"][nb + 1]) == res["total"] == sum(lens), f"{ctx}: total"
    assert (res["data"][res["total"]:] == 0xAA).all(), f"{ctx}: bytes written past total"
    # the "other" bin's HB_REF_OTHER records: nothing encoded, status HB_WIRE_HOST
    oth = ((res["out"]["info"][:n] >> 4) & 0xF) == abi.HB_REF_OTHER
    assert (np.nonzero(oth)[0] >= int(boff[nb])).all()
    ln = np.diff(res["off"][:n + 1].astype(np.int64))
    assert (ln[oth] == 0).all() and (res["status"][:n][oth] == abi.HB_WIRE_HOST).all()
    assert (ln[~oth] >= 28).all() and (res["status"][:n][~oth] == abi.HB_WIRE_OK).all()
    return np.diff(boff.astype(np.int64))


@pytest.mark.parametrize("small", ["1", "0"])
def test_end_to_end_follower_side(small, monkeypatch):
    """G = 600, n = 3, three steps of the follower-side fuzz; peer rows drawn per group from a
    pool of 7 node ids, 5 of them in the table: two pool ids land in "other"."""
    monkeypatch.setenv("HB_SMALL_STEP", small)
    G, self_id = 600, 99
    pool = np.array([11, (1 << 32) | 11, 13, 1 << 40, (1 << 63) | 5, 16, 17], dtype=np.uint64)
    ids = pool[[4, 0, 6, 1, 3]]
    rng = np.random.default_rng(404)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    for g in range(G):
        peers[g, :3] = pool[rng.permutation(7)[:3]]
    g, runs, ins = synth.random_groups(G, 3, seed=71, W=8)
    pair = _tap(Pair(g, runs, 3, 8, ins=ins, max_batch=1 << 13, term_runs=True))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True)
    pair.eng.set_egress_peers(ids)
    seen = np.zeros(len(ids) + 1, np.int64)
    for k, before in _follower_steps(pair, g, 74):
        want = replay(pair.ora_ev, before, peers, self_id)
        assert len(want) > 500
        res = _chain(pair.eng, self_id, 4096, len(ids))
        seen += _check_chain(res, want, ids, self_id, f"small={small} step {k}")
    assert (seen > 0).all(), "every table bin and \"other\" took records"


def test_end_to_end_tick():
    """Half the groups leaders: a tick's MsgHeartbeat to both followers of each, peer rows from a
    pool of 64 node ids, all 64 in the table: 64 per-peer streams and an empty "other"."""
    G, self_id = 600, 9999
    pool = _table(64, 64)
    rng = np.random.default_rng(505)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    for g in range(G):
        peers[g, :3] = pool[rng.permutation(64)[:3]]
    g, runs = synth.steady_groups(G, 3, seed=301, last_hi=1 << 16)
    f, _ = synth.follow_groups(G, 3, seed=301, last_hi=1 << 16, with_runs=True)
    g[1::2] = f[1::2]
    pair = _tap(Pair(g, runs, 3, 256, max_batch=4096))
    pair.eng.load_peers(peers)
    timers = np.zeros(G, dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"] = 10, 1
    pair.set_timers(timers, DRAWS)
    pair.eng.set_egress(True)
    pair.eng.set_egress_peers(pool)
    before = pair.og.groups()
    pair.tick(ctx="egress bin tick")
    want = replay(pair.ora_ev, before, peers, self_id)
    assert len(want) == 2 * (G // 2) and all(r[1] == abi.HB_MSG_HEARTBEAT for r in want)
    cnt = _check_chain(_chain(pair.eng, self_id, 2048, 64), want, pool, self_id, "tick")
    assert cnt[64] == 0 and (cnt[:64] > 0).sum() >= 60


# ---- 6. edges of the contract ---------------------------------------------------------------
def test_contract_edges(monkeypatch):
    import torch
    from etcd_amd.hipbatch import HipBatchError, lib
    eng = _engine(monkeypatch, "1")
    L = lib()
    n = 500
    tab_a, tab_b = np.array([5, 6, 7], np.uint64), np.array([7, 1 << 33, 5, 6], np.uint64)
    rec = _records(n, tab_a, "uniform", seed=61)
    inp = {name: _dev(rec[name]) for name, _ in FIELDS}
    mk = lambda: {name: _dev(np.full(n, SENT[dt], dtype=dt)) for name, dt in FIELDS}  # noqa: E731
    out, out_b = mk(), mk()
    boff, boff_b = (torch.full((8,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    span = torch.zeros(8, dtype=torch.int64, device="cuda")

    def einval(f, *a, **k):
        with pytest.raises(HipBatchError) as e:
            f(*a, **k)
        assert e.value.code == abi.HB_EINVAL

    einval(eng.egress_bin, inp, n, out, boff)  # no table
    einval(eng.peer_spans, boff, boff, span)
    einval(eng.set_egress_peers, np.arange(1, 257, dtype=np.uint64))  # a table of 256 ids
    einval(eng.set_egress_peers, [5, 0, 7])  # a zero id
    einval(eng.set_egress_peers, [5, 6, 5])  # a repeated id
    assert L.hb_set_egress_peers(eng.h, None, 3) == abi.HB_EINVAL
    einval(eng.egress_bin, inp, n, out, boff)  # still no table
    eng.set_egress_peers(np.arange(1, 256, dtype=np.uint64))  # 255 ids is the limit
    eng.set_egress_peers(tab_a)
    for name, _ in FIELDS:  # an `out` array aliasing `in`'s
        einval(eng.egress_bin, inp, n, dict(out, **{name: inp[name]}), boff)
    einval(eng.egress_bin, inp, CAP_MAX + 1, out, boff)  # cap above the handle's limit
    bi, bo = eng._out_batch(inp), eng._out_batch(out)
    assert L.hb_egress_bin(eng.h, C.byref(bi), n, None, C.byref(bo), None, None) == abi.HB_EINVAL
    assert L.hb_egress_bin(eng.h, None, n, None, C.byref(bo), None, boff.data_ptr()) == abi.HB_EINVAL
    for name, dt in FIELDS:  # nothing ran
        assert (_host(out[name], dt) == SENT[dt]).all()
    # cap = 0 is legal: bin_off all zeros
    eng.egress_bin(inp, 0, out, boff)
    eng.sync()
    assert (_host(boff, "<u8")[:5] == 0).all() and _host(boff, "<u8")[5] == M64
    # a table replaced between two calls: each call has its own table's result, no sync between
    eng.egress_bin(inp, n, out, boff)
    eng.set_egress_peers(tab_b)
    eng.egress_bin(inp, n, out_b, boff_b)
    eng.sync()
    for tab, o, bo_ in ((tab_a, out, boff), (tab_b, out_b, boff_b)):
        order, off = bin_reference(rec["to"], rec["info"], tab)
        assert np.array_equal(_host(bo_, "<u8")[:len(tab) + 2], off)
        for name, dt in FIELDS:
            assert np.array_equal(_host(o[name], dt), rec[name][order]), name
    # the table freed: the calls refuse again; freeing twice is fine
    eng.set_egress_peers([])
    eng.set_egress_peers([])
    einval(eng.egress_bin, inp, n, out, boff)
    einval(eng.peer_spans, boff, boff, span)
    eng.close()
