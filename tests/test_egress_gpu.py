"""GPU parity of wire egress: hb_egress + hb_encode against the replay rules
(tests/egress_util.py, pinned to the oracle's r.msgs by
tests/test_egress_replay.py) and the reference encoder's restatement
(tests/wire_util.gogo_marshal).

Every scenario goes through parity_util.Pair, so the engine's events are
already compared with the oracle's; the expected records are the replay of the
oracle's events from the oracle's groups before the step.  The record count,
every array of the out batch, status, off, total and the bytes are compared
exactly.  The engine promises a group's records in the order of its events and
no order across groups (a chunk interleaves its groups as they were emitted),
so records are matched after a stable sort by group, and off / the bytes are
the expected records' in the device's order.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth

from . import egress_cases as EC
from .egress_util import by_group, marshal, out_arrays, replay
from .lift_util import lifted
from .parity_util import Pair, assert_events_equal, assert_groups_equal

pytestmark = pytest.mark.gpu

SELF = 1  # this node's id: slot 0 of the destination's peer rows (ids are slot + 1)
DRAWS = np.arange(1, 64, dtype=np.uint64) * np.uint64(7919)
_TDT = {"<u4": "int32", "<u8": "int64"}


def _peers(G, n):
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :n] = np.arange(1, n + 1, dtype=np.uint64)
    return p


def _tap(pair):
    """Keep the oracle's events of the last step / tick (Pair compares them with the engine's)."""
    for name in ("step", "tick"):
        def wrap(*a, _f=getattr(pair.og, name), **k):
            r = _f(*a, **k)
            pair.ora_ev = r[0]
            return r
        setattr(pair.og, name, wrap)
    return pair


def _egress(eng, cap, enc_cap=None, bytes_cap=None):
    """hb_egress then hb_encode fed by its count through n_dev, no host sync between."""
    import torch
    enc_cap = cap if enc_cap is None else enc_cap
    bytes_cap = 91 * enc_cap if bytes_cap is None else bytes_cap
    alloc = max(cap, enc_cap, 1)
    out = {name: torch.full((alloc,), -1, dtype=getattr(torch, _TDT[dt]), device="cuda")
           for name, dt in abi.OUT_BATCH_FIELDS}
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    data = torch.full((max(bytes_cap, 1),), 0xAA, dtype=torch.uint8, device="cuda")[:bytes_cap]
    off = torch.full((enc_cap + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((max(enc_cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    eng.egress(SELF, out, cap, count)
    eng.encode(SELF, out, enc_cap, data if bytes_cap else None, off, status, total, n_dev=count)
    eng.sync()
    res = {name: out[name].cpu().numpy().view(dt) for name, dt in abi.OUT_BATCH_FIELDS}
    res.update(count=int(count.item()), total=int(total.item()), off=off.cpu().numpy().view(np.uint64),
               status=status.cpu().numpy(), data=data.cpu().numpy(), cap=cap, enc_cap=enc_cap, bytes_cap=bytes_cap)
    return res


def _expect(pair, before, peers):
    return by_group(replay(pair.ora_ev, before, peers, SELF))


def _check(res, want, ctx=""):
    """A complete egress + encode result (cap and bytes_cap sufficed) against the expected records."""
    n = len(want)
    assert res["count"] == n, f"{ctx}: count {res['count']} expected {n}"
    assert n <= res["cap"] and n <= res["enc_cap"]
    order = np.argsort(res["group"][:n], kind="stable")
    exp = out_arrays(want)
    for name, _ in abi.OUT_BATCH_FIELDS:
        d = res[name][:n][order]
        bad = np.nonzero(d != exp[name])[0]
        assert len(bad) == 0, f"{ctx}: {name} differs at sorted {bad[:5]}: dev {d[bad[:5]]} expected {exp[name][bad[:5]]}"
    recs = [None] * n
    for j, i in enumerate(order):
        recs[int(i)] = marshal(want[j])
    lens = np.array([len(r) for r in recs], dtype=np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    assert res["total"] == int(off[n]), f"{ctx}: total"
    assert np.array_equal(res["off"][:n + 1], off), f"{ctx}: off"
    st = np.where(lens == 0, abi.HB_WIRE_HOST, abi.HB_WIRE_OK).astype(np.uint8)
    assert np.array_equal(res["status"][:n], st), f"{ctx}: status"
    assert (res["status"][n:] == 0xEE).all() and (res["group"][n:].view(np.int32) == -1).all(), f"{ctx}: past n"
    blob = b"".join(recs)
    assert res["bytes_cap"] >= len(blob)
    got = res["data"][:len(blob)].tobytes()
    if got != blob:
        i = next(k for k in range(n) if got[int(off[k]):int(off[k + 1])] != recs[k])
        raise AssertionError(f"{ctx}: bytes of record {i} (group {res['group'][i]}): "
                             f"{got[int(off[i]):int(off[i + 1])].hex()} expected {recs[i].hex()}")
    assert (res["data"][len(blob):] == 0xAA).all(), f"{ctx}: bytes written past total"


def _round_trip(eng, res, want_types=()):
    """The bytes through hb_decode under the destination's peer rows (ids slot + 1): every
    response comes back HB_WIRE_OK with what it was built from; MsgHeartbeat goes to the host."""
    import torch
    from .test_wire_gpu import _decode_dev
    n = res["count"]
    ok = res["status"][:n] == abi.HB_WIRE_OK
    off = res["off"][:n][ok]
    ln = (res["off"][1:n + 1][ok] - off).astype(np.uint32)
    grp = res["group"][:n][ok]
    out, status = _decode_dev(eng, torch, res["data"], off, ln, grp)
    st = status.cpu().numpy()
    typ = res["info"][:n][ok] & 0xF
    hb = typ == abi.HB_MSG_HEARTBEAT
    assert (st[hb] == abi.HB_WIRE_HOST).all() and (st[~hb] == abi.HB_WIRE_OK).all()
    r = ~hb
    info = out["info"].cpu().numpy().view(np.uint32)[r]
    assert np.array_equal(info & 0xF, typ[r]) and ((info >> 4) & 0xF == SELF - 1).all()
    assert np.array_equal((info >> 8) & 1, (res["info"][:n][ok][r] >> 8) & 1)
    assert np.array_equal(out["group"].cpu().numpy().view(np.uint32)[r], grp[r])
    for k in ("term", "index", "hint"):
        assert np.array_equal(out[k].cpu().numpy().view(np.uint64)[r], res[k][:n][ok][r]), k
    assert set(want_types) <= set(typ.tolist())


def _follower_pair(nmax, lift=None, G=600, seed=71):
    g, runs, ins = synth.random_groups(G, nmax, seed=seed, W=8)
    g, runs, ins = lifted(lift, g, runs, ins, delta=24, eps=20)
    pair = _tap(Pair(g, runs, nmax, 8, ins=ins, max_batch=1 << 13, term_runs=True))
    pair.eng.load_peers(_peers(G, nmax))
    return pair, g


def _follower_steps(pair, g, seed, steps=3):
    """Three consecutive steps of the follower-side fuzz; yields (k, groups before the step)."""
    now = pair.og.groups()
    for k in range(steps):
        f = synth.follower_messages(now, pair.og.term, 1500, seed=seed + 13 * k)
        b = synth.merge_batches(synth.random_batch(g, 700, seed=seed + 7 * k), f, seed=seed + k)
        before = now
        _, _, now = pair.step(b, ctx=f"egress fuzz {seed} step {k}")
        yield k, before


# ---- 1. follower parity: a ragged last partition, chunk bases across chunks -----------------
@pytest.mark.parametrize("nmax,small", [(3, "1"), (5, "1"), (3, "0")])
def test_follower_parity(nmax, small, monkeypatch):
    """G = 600 (2 full partitions + 88 groups), three consecutive steps: the second and third
    start from a snapshot the previous step changed.  small = "0": HB_SMALL_STEP=0, the tiled
    kernels of both calls; n = 5 encodes through the tiled kernels by its capacity."""
    monkeypatch.setenv("HB_SMALL_STEP", small)
    pair, g = _follower_pair(nmax)
    pair.eng.set_egress(True)
    peers = _peers(len(g), nmax)
    for k, before in _follower_steps(pair, g, 71 + nmax):
        want = _expect(pair, before, peers)
        assert len(want) > 500
        res = _egress(pair.eng, 4096, enc_cap=20000 if nmax == 5 else None)
        _check(res, want, f"n={nmax} step {k}")
        if k == 0:  # 8. round trip
            _round_trip(pair.eng, res, (abi.HB_MSG_APP_RESP, abi.HB_MSG_VOTE_RESP, abi.HB_MSG_HEARTBEAT_RESP))
    terms = {r[5] for r in want}
    assert len(terms) > 10


# ---- 2. Term and lastIndex inside a step, hand-built ----------------------------------------
def test_term_and_last_inside_a_step():
    scs = EC.scenarios()
    rafts = [EC.build(sc) for sc in scs]
    groups, runs, peers, batch = EC.export(rafts, scs)
    pair = _tap(Pair(groups, runs, 5, 256, max_batch=4096, term_runs=True))
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True)
    before = pair.og.groups()
    _, _, after = pair.step(batch, ctx="egress hand-built")
    want = _expect(pair, before, peers)
    res = _egress(pair.eng, 1024)
    _check(res, want, "hand-built")
    name = {sc[0]: g for g, sc in enumerate(scs)}
    of = lambda n: [r for r in want if r[0] == name[n]]  # noqa: E731
    a, v = of("app-then-vote/0")
    assert (a[1], v[1]) == (abi.HB_MSG_APP_RESP, abi.HB_MSG_VOTE_RESP) and v[5] == a[5] + 1 == int(before[name["app-then-vote/0"]]["term"]) + 1
    ok, rej = of("append-then-reject/0")
    assert not ok[9] and rej[9] and rej[10] == ok[7] == int(before[name["append-then-reject/0"]]["last_index"]) + 2
    (rej,) = of("reject-alone/0")
    assert rej[9] and rej[10] == int(before[name["reject-alone/0"]]["last_index"])
    ok, rej = of("restore-then-reject/0")
    assert rej[9] and rej[10] == ok[7] == 10
    rej = of("leader-steps-down/0")[-1]
    g = name["leader-steps-down/0"]
    assert rej[9] and rej[10] == int(before[g]["last_index"]) + 2 and rej[5] == int(before[g]["term"]) + 1
    h0, vo, h1 = of("vote-outsider/0")
    assert vo[2] == abi.HB_REF_OTHER and vo[3] == 0 and h0[2] == h1[2] == 1
    assert len(of("fault-mid-batch/0")) == 1 and after[name["fault-mid-batch/0"]]["fault"] == abi.HB_FAULT_COMMIT_RANGE
    assert [r[1] for r in of("leader-beats/1")] == [abi.HB_MSG_HEARTBEAT] * 8
    _round_trip(pair.eng, res, (abi.HB_MSG_HEARTBEAT,))


# ---- 3. heartbeats: a tick (P chunks) and a MsgBeat batch, beside campaigns ------------------
def test_heartbeats_of_tick_and_beat_beside_campaigns():
    G = 600
    g, runs = synth.steady_groups(G, 3, seed=301, last_hi=1 << 16)
    f, _ = synth.follow_groups(G, 3, seed=301, last_hi=1 << 16, with_runs=True)
    g[1::2] = f[1::2]  # half leaders, half followers (the same logs)
    pair = _tap(Pair(g, runs, 3, 256, max_batch=4096))
    peers = _peers(G, 3)
    pair.eng.load_peers(peers)
    timers = np.zeros(G, dtype=abi.TIMER_DTYPE)
    timers["election_tick"], timers["heartbeat_tick"] = 10, 1
    timers["elapsed"][1::2] = 20  # the followers are past every randomized timeout: they campaign
    pair.set_timers(timers, DRAWS)
    pair.eng.set_egress(True)
    before = pair.og.groups()
    ev, _, now = pair.tick(ctx="egress tick")
    want = _expect(pair, before, peers)
    assert len(want) == 2 * (G // 2) and all(r[1] == abi.HB_MSG_HEARTBEAT for r in want)
    assert (ev["type"] == abi.HB_EV_VOTE).sum() == 2 * (G // 2) and (ev["type"] == abi.HB_EV_TERM).sum() == G // 2
    _, counts = pair.eng.event_words()
    assert counts[0::2].sum() > 0 and counts[1::2].sum() == 0  # a tick's events sit in the P chunks
    _check(_egress(pair.eng, 2048), want, "tick")
    # MsgBeat to every leader and MsgHup to every other group, one batch
    lead = now["state"] == abi.HB_STATE_LEADER
    info = np.where(lead, abi.hb_info(abi.HB_MSG_BEAT, 0), abi.hb_info(abi.HB_MSG_HUP, 0)).astype(np.uint32)
    z = np.zeros(G, np.uint64)
    b = dict(group=np.arange(G, dtype=np.uint32), info=info, term=z, index=z, hint=z, props=None)
    before = now
    ev, _, _ = pair.step(b, ctx="egress beat")
    want = _expect(pair, before, peers)
    assert len(want) == 2 * int(lead.sum()) and (ev["type"] == abi.HB_EV_VOTE).sum() == 2 * int((~lead).sum())
    res = _egress(pair.eng, 2048)
    _check(res, want, "beat")
    _round_trip(pair.eng, res, (abi.HB_MSG_HEARTBEAT,))


# ---- 4. a chunk longer than a tile ----------------------------------------------------------
def test_chunk_longer_than_a_tile():
    """G = 256, 40 MsgHeartbeat per group in one batch: one M chunk of more than 20,000 words,
    ten tiles of the egress kernel (2,048 words each), 10,240 records, each group's 40 in order."""
    G, K, TILE = 256, 40, 2048
    g, runs = synth.follow_groups(G, 3, seed=401, last_hi=1 << 14, with_runs=True)
    pair = _tap(Pair(g, runs, 3, 256, max_batch=1 << 14, term_runs=True))
    peers = _peers(G, 3)
    pair.eng.load_peers(peers)
    pair.eng.set_egress(True)
    rng = np.random.default_rng(402)
    grp = rng.permutation(np.repeat(np.arange(G, dtype=np.uint32), K))
    n = len(grp)
    b = dict(group=grp, info=np.full(n, abi.hb_info(abi.HB_MSG_HEARTBEAT, 1), np.uint32),
             term=g["term"][grp].astype(np.uint64), index=np.zeros(n, np.uint64), hint=np.zeros(n, np.uint64),
             commit=(g["committed"][grp] + rng.integers(0, 2, n).astype(np.uint64)).astype(np.uint64),
             eoff=np.zeros(n, np.uint64), eterm=np.zeros(0, np.uint64), props=None)
    before = pair.og.groups()
    pair.step(b, ctx="egress long chunk", check_inflights=False)
    _, counts = pair.eng.event_words()
    print("words per chunk:", counts.tolist())
    assert len(counts) == 2 and counts[1] >= 20000 and counts[1] >= 3 * TILE
    want = _expect(pair, before, peers)
    assert len(want) == n
    _check(_egress(pair.eng, n), want, "long chunk")
    _check(_egress(pair.eng, n, enc_cap=20000), want, "long chunk, tiled encode")


# ---- 5. wide values -------------------------------------------------------------------------
@pytest.mark.parametrize("lift", ["W32", "W40", "W62"])
def test_follower_parity_wide_values(lift):
    """Scenario 1 at n = 3 lifted to 2^32, to 2^40 / 2^24 (short words and continuation words
    in one chunk) and to 2^61 / 2^50 (9- and 10-byte varints)."""
    pair, g = _follower_pair(3, lift=lift)
    pair.eng.set_egress(True)
    peers = _peers(len(g), 3)
    longest = 0
    for k, before in _follower_steps(pair, g, 74):
        want = _expect(pair, before, peers)
        res = _egress(pair.eng, 4096)
        _check(res, want, f"{lift} step {k}")
        longest = max(longest, int(np.diff(res["off"][:res["count"] + 1].astype(np.int64)).max()))
        x = pair.ora_ev["x"]
        if lift == "W40":
            assert ((x >> np.uint64(40)) != 0).any() and ((x >> np.uint64(40)) == 0).any()
    if lift == "W62":
        assert longest >= 28 + 8 + 7  # a 9-byte index and an 8-byte term at the least


# ---- 6. edges of the contract ---------------------------------------------------------------
def test_contract_edges():
    import torch
    from etcd_amd.hipbatch import HipBatchError
    pair, g = _follower_pair(3, G=300, seed=77)
    eng = pair.eng
    peers = _peers(len(g), 3)
    out = {name: torch.zeros(8, dtype=getattr(torch, _TDT[dt]), device="cuda") for name, dt in abi.OUT_BATCH_FIELDS}
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(HipBatchError) as e:  # before hb_set_egress
        eng.egress(SELF, out, 8, count)
    assert e.value.code == abi.HB_EINVAL
    eng.set_egress(True)
    res = _egress(eng, 16)  # no step since hb_set_egress
    assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
    # a step with no encodable event
    z32, z64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    pair.step(dict(group=z32, info=z32, term=z64, index=z64, hint=z64, props=None), ctx="egress empty")
    res = _egress(eng, 16)
    assert (res["count"], res["total"], int(res["off"][0])) == (0, 0, 0)
    assert (res["status"] == 0xEE).all() and (res["data"] == 0xAA).all()
    k, before = next(_follower_steps(pair, g, 78, steps=1))
    want = _expect(pair, before, peers)
    n = len(want)
    full = _egress(eng, n)
    _check(full, want, "edges")
    # cap smaller than the record count: the count, and the first cap records; then a retry
    small = _egress(eng, 100)
    assert small["count"] == n and small["off"][100] == full["off"][100] == small["total"]
    for name, _ in abi.OUT_BATCH_FIELDS:
        assert np.array_equal(small[name][:100], full[name][:100]), name
    assert small["data"][:small["total"]].tobytes() == full["data"][:small["total"]].tobytes()
    _check(_egress(eng, n + 7), want, "edges retry")
    # bytes_cap too small: off, status and total, and not one byte; then a retry
    short = _egress(eng, n, bytes_cap=full["total"] - 1)
    assert short["total"] == full["total"] and np.array_equal(short["off"], full["off"])
    assert np.array_equal(short["status"], full["status"]) and (short["data"] == 0xAA).all()
    exact = _egress(eng, n, bytes_cap=full["total"])
    assert exact["data"].tobytes() == full["data"][:full["total"]].tobytes()
    # a pinned count / total (hb_alloc_pinned) is read and written by the device as well
    import ctypes as C
    from etcd_amd.hipbatch import lib
    p = C.c_void_p()
    assert lib().hb_alloc_pinned(64, C.byref(p)) == 0
    try:
        arrays = {name: torch.zeros(n, dtype=getattr(torch, _TDT[dt]), device="cuda")
                  for name, dt in abi.OUT_BATCH_FIELDS}
        b = eng._out_batch(arrays)
        data = torch.zeros(91 * n, dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        assert lib().hb_egress(eng.h, SELF, C.byref(b), n, p.value) == 0
        assert lib().hb_encode(eng.h, C.byref(b), n, p.value, SELF, data.data_ptr(), 91 * n, off.data_ptr(),
                               status.data_ptr(), p.value + 8) == 0
        eng.sync()
        assert C.c_uint64.from_address(p.value).value == n
        assert C.c_uint64.from_address(p.value + 8).value == full["total"]
        assert data.cpu().numpy()[:full["total"]].tobytes() == full["data"][:full["total"]].tobytes()
    finally:
        lib().hb_free_pinned(p)
    eng.set_egress(False)
    with pytest.raises(HipBatchError):
        eng.egress(SELF, out, 8, count)


# ---- 7. egress off changes nothing ----------------------------------------------------------
def test_egress_off_changes_nothing():
    got = []
    for on in (True, False):
        pair, g = _follower_pair(3)
        if on:
            pair.eng.set_egress(True)
        steps = []
        for k, _ in _follower_steps(pair, g, 74):
            steps.append((pair.eng.events(), pair.eng.stats(), pair.eng.get_groups(), pair.eng.step_kernels()))
        got.append(steps)
    for k, (a, b) in enumerate(zip(*got)):
        assert_events_equal(a[0], b[0], f"egress on/off step {k}")
        assert np.array_equal(a[1], b[1])
        assert_groups_equal(a[2], b[2], f"egress on/off step {k}")
        assert a[3] == b[3]
