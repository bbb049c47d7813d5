#!/usr/bin/env python3
"""Micro-benchmark of the follower side's wire ingestion: hb_decode_follow (not product code).

On a handle of 1,048,576 groups x 3 that this node follows (synth.follow_groups), the
follow workload of bench.py as wire bytes: synth.follow_batch encoded once as
Message.MarshalTo writes it, 1M MsgApp with one entry of 16 B Data plus 1M MsgHeartbeat.

  decode_follow        hb_decode_follow alone
  decode_follow+step   hb_decode_follow, then hb_step over the decoded arrays with the
                       sentinel (b.n = n + 1, n_edesc = ent_cap: no host read between);
                       the groups are reloaded before every repetition, outside the timed
                       region, so every step is the first one (it appends and commits)
  decode (yardstick)   hb_decode on cfg2's 2M MsgAppResp (synth.encode_responses), the same
                       handle, interleaved with the two above repetition by repetition

25 repetitions after 3 warm-ups, each bracketed by HIP events on the handle's stream:
median [min, max] in microseconds, and the bytes of a model with the rate it implies at
the median: the record bytes + 16 B off / len / group + the 64 B peer row + the batch
record written (48 B; hb_decode: 32 B) + the status byte, and for hb_decode_follow 20 B
per entry (eterm, edesc, edata) + 8 B eoff.  (The model counts the record bytes once;
the second walk reads the records with entries again.)

  python tools/microbench/ingest_bench.py [--out profiles/ingest_bench.json]

--workload prop: a step's worth of forwarded proposals on a handle that leads
1,048,576 groups x 3, one MsgProp per group with one entry of 16 B and of 1 KiB Data, through
hb_decode_follow with hb_set_wire_props(HB_WIRE_PROPS_IN) (every record an HB_WIRE_OK batch
record with its entry run) beside the same bytes through hb_decode (every record
HB_WIRE_HOST: what the host unmarshals today), interleaved repetition by repetition.  The byte
model is the one above; the payload bytes are counted, though the parser reads only the
window lines that hold them.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from etcd_amd import abi, synth  # noqa: E402
from etcd_amd.hipbatch import Engine  # noqa: E402

N, W, DATA = 3, 256, 16
SNAP = bytes([0x4A, 0x08, 0x12, 0x06, 0x0A, 0x00, 0x10, 0x00, 0x18, 0x00])


def dv(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])).cuda()


def encode_follow(b, to=1):
    """Vectorized Message.MarshalTo of a synth.follow_batch with one entry per MsgApp: the entry is
    Type 0, the message's Term, Index + 1, DATA bytes of payload.  Returns (bytes u8, off u64, len u32)."""
    n = len(b["group"])
    t = (b["info"] & np.uint32(0xF)).astype(np.uint64)
    frm = ((b["info"] >> np.uint32(4)) & np.uint32(0xF)).astype(np.uint64) + np.uint64(1)
    app = t == abi.HB_MSG_APP
    vl = synth._varint_len
    head = [(0x08, t), (0x10, np.full(n, to, np.uint64)), (0x18, frm), (0x20, b["term"]), (0x28, b["hint"]),
            (0x30, b["index"])]
    eidx = b["index"] + np.uint64(1)
    elen = 2 + 1 + vl(b["term"]) + 1 + vl(eidx) + 2 + DATA  # 08 00 | 10 term | 18 index | 22 10 data
    assert int(elen.max()) < 128
    rec_len = sum(1 + vl(c) for _, c in head) + np.where(app, 2 + elen, 0) + 1 + vl(b["commit"]) + len(SNAP) + 4
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(rec_len[:-1]).astype(np.uint64)
    out = np.zeros(int(rec_len.sum()), np.uint8)
    pos = off.astype(np.int64)

    def put(pos, key, c, rows=None):
        r = np.arange(n) if rows is None else rows
        p, v, l = pos[r], np.asarray(c, np.uint64)[r].copy(), vl(np.asarray(c, np.uint64)[r])
        out[p] = key
        for k in range(int(l.max())):
            live = k < l
            byte = (v & np.uint64(0x7F)).astype(np.uint8) | np.where(k + 1 < l, 0x80, 0).astype(np.uint8)
            out[p[live] + 1 + k] = byte[live]
            v >>= np.uint64(7)
        pos[r] = p + 1 + l
    for key, c in head:
        put(pos, key, c)
    rows = np.nonzero(app)[0]
    p = pos[rows]
    out[p], out[p + 1], out[p + 2], out[p + 3] = 0x3A, elen[rows].astype(np.uint8), 0x08, 0x00
    pos[rows] = p + 4
    put(pos, 0x10, b["term"], rows)
    put(pos, 0x18, eidx, rows)
    p = pos[rows]
    out[p], out[p + 1] = 0x22, DATA
    for j in range(DATA):
        out[p + 2 + j] = (rows + j) & 0xFF
    pos[rows] = p + 2 + DATA
    put(pos, 0x40, b["commit"])
    for j, x in enumerate(SNAP):
        out[pos + j] = x
    pos += len(SNAP)
    out[pos], out[pos + 1], out[pos + 2], out[pos + 3] = 0x50, 0, 0x58, 0
    assert np.array_equal(pos + 4, off.astype(np.int64) + rec_len)
    return out, off, rec_len.astype(np.uint32)


def self_check(b, data, off, ln, k=512):
    """The first k records against the test suite's restatement of Message.MarshalTo."""
    from tests.wire_util import gogo_marshal
    for i in range(min(k, len(off))):
        t, idx = int(b["info"][i]) & 0xF, int(b["index"][i])
        ents = [(0, int(b["term"][i]), idx + 1, bytes((i + j) & 0xFF for j in range(DATA)))] if t == abi.HB_MSG_APP else []
        want = gogo_marshal(t, to=1, frm=((int(b["info"][i]) >> 4) & 0xF) + 1, term=int(b["term"][i]),
                            log_term=int(b["hint"][i]), index=idx, entries=ents, commit=int(b["commit"][i]))
        assert data[int(off[i]):int(off[i]) + int(ln[i])].tobytes() == want, i


def encode_props(G, data_len, to=1, frm=2):
    """One forwarded MsgProp per group as Message.MarshalTo writes it: one entry of data_len bytes."""
    from etcd_amd.splice import varint
    ent = bytes([0x08, 0, 0x10, 0, 0x18, 0, 0x22]) + varint(data_len)
    head = bytes([0x08, abi.HB_MSG_PROP, 0x10, to, 0x18, frm, 0x20, 0, 0x28, 0, 0x30, 0, 0x3A]) + \
        varint(len(ent) + data_len) + ent
    tail = bytes([0x40, 0]) + SNAP + bytes([0x50, 0, 0x58, 0])
    L = len(head) + data_len + len(tail)
    out = np.zeros((G, L), np.uint8)
    out[:, :len(head)] = np.frombuffer(head, np.uint8)
    out[:, len(head):len(head) + data_len] = (np.arange(G)[:, None] + np.arange(data_len)[None, :]) & 0xFF
    out[:, len(head) + data_len:] = np.frombuffer(tail, np.uint8)
    return out.reshape(-1), np.arange(G, dtype=np.uint64) * np.uint64(L), np.full(G, L, np.uint32), len(head)


def main_prop(args):
    import torch
    from tests.wire_util import gogo_marshal
    G = args.groups
    stream = torch.cuda.Stream()
    g, _ = synth.steady_groups(G, N, seed=0x5EED0002, with_runs=False)
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G + 1, stream=stream)
    eng.load_groups(g)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    peers[:, :N] = np.arange(1, N + 1, dtype=np.uint64)
    eng.load_peers(peers)
    eng.set_wire_props(decode=True)
    grp = np.arange(G, dtype=np.uint32)
    res = []
    for data_len in (16, 1024):
        data, off, ln, at = encode_props(G, data_len)
        for i in (0, 1, G - 1):
            want = gogo_marshal(abi.HB_MSG_PROP, to=1, frm=2, entries=[(0, 0, 0, bytes((i + j) & 0xFF for j in range(data_len)))])
            assert data[int(off[i]):int(off[i]) + int(ln[i])].tobytes() == want, i
        ent_cap = G
        with torch.cuda.stream(stream):
            d = [dv(torch, x) for x in (data, off, ln, grp)]
            z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")  # noqa: E731
            out = dict(group=z(G + 1, torch.int32), info=z(G + 1, torch.int32), term=z(G + 1, torch.int64),
                       index=z(G + 1, torch.int64), hint=z(G + 1, torch.int64), commit=z(G + 1, torch.int64),
                       eoff=z(G + 1, torch.int64), eterm=z(ent_cap, torch.int64), edesc=z(ent_cap, torch.int32))
            edata, n_ent, status, hstatus = z(ent_cap, torch.int64), z(1, torch.int64), z(G, torch.uint8), z(G, torch.uint8)
        torch.cuda.synchronize()
        fns = (("decode_follow props", lambda: eng.decode_follow(d[0], d[1], d[2], d[3], out, status, ent_cap, edata, n_ent)),
               ("decode (host's today)", lambda: eng.decode(d[0], d[1], d[2], d[3], out, hstatus)))
        us = {name: [] for name, _ in fns}
        for rep in range(3 + args.reps):
            for name, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= 3:
                    us[name].append(e0.elapsed_time(e1) * 1e3)
        eng.decode_follow(d[0], d[1], d[2], d[3], out, status, ent_cap, edata, n_ent)
        eng.sync()
        assert int(n_ent.item()) == G and bool((status == abi.HB_WIRE_OK).all().item())
        assert bool((hstatus == abi.HB_WIRE_HOST).all().item())
        assert bool((edata == torch.from_numpy((off + np.uint64(at)).view(np.int64)).cuda()).all().item())
        for name, model in (("decode_follow props", len(data) + G * (16 + 64 + 48 + 1 + 8 + 20)),
                            ("decode (host's today)", len(data) + G * (16 + 64 + 32 + 1))):
            r = dict(case=name, workload="prop", data_len=data_len, groups=G, replicas=N, reps=args.reps, records=G,
                     wire_bytes=int(len(data)), entries=G if "props" in name else 0, event_us=stat(us[name]),
                     model_bytes=int(model))
            med = r["event_us"]["median"]
            r.update(model_GBps_at_median=float(model / med / 1e3), ns_per_record_at_median=float(med * 1e3 / G))
            print(json.dumps(r), flush=True)
            res.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


def stat(us):
    return dict(median=float(np.median(us)), min=float(np.min(us)), max=float(np.max(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", choices=("follow", "prop"), default="follow")
    args = ap.parse_args()
    if args.workload == "prop":
        return main_prop(args)
    import torch
    G = args.groups
    stream = torch.cuda.Stream()
    g, _ = synth.follow_groups(G, N, seed=0x5EED0006, with_runs=False)
    b = synth.follow_batch(g, 0, seed=0x5EED0006)
    n = len(b["group"])
    data, off, ln = encode_follow(b)
    self_check(b, data, off, ln)
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=n + 1, stream=stream)
    eng.load_groups(g)
    peers = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    peers[:, :N] = np.arange(1, N + 1, dtype=np.uint64)
    eng.load_peers(peers)
    # the yardstick's records: cfg2's acks
    lg, _ = synth.steady_groups(G, N, seed=0x5EED0002, with_runs=False)
    cb = synth.cfg2_batch(lg, 0, seed=0x5EED0002)
    cfrm = ((cb["info"] >> np.uint32(4)) & np.uint32(0xF)).astype(np.uint64) + np.uint64(1)
    cdata, coff, cln = synth.encode_responses(abi.HB_MSG_APP_RESP, np.ones(len(cfrm), np.uint64), cfrm, cb["term"],
                                              cb["index"])
    nc = len(coff)
    ent_cap = int(ln.astype(np.uint64).sum()) // 8
    with torch.cuda.stream(stream):
        d = [dv(torch, x) for x in (data, off, ln, b["group"])]
        c = [dv(torch, x) for x in (cdata, coff, cln, cb["group"])]
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")  # noqa: E731
        out = dict(group=z(n + 1, torch.int32), info=z(n + 1, torch.int32), term=z(n + 1, torch.int64),
                   index=z(n + 1, torch.int64), hint=z(n + 1, torch.int64), commit=z(n + 1, torch.int64),
                   eoff=z(n + 1, torch.int64), eterm=z(ent_cap, torch.int64), edesc=z(ent_cap, torch.int32))
        edata, n_ent, status = z(ent_cap, torch.int64), z(1, torch.int64), z(n, torch.uint8)
        cout = dict(group=z(nc, torch.int32), info=z(nc, torch.int32), term=z(nc, torch.int64),
                    index=z(nc, torch.int64), hint=z(nc, torch.int64))
        cstatus = z(nc, torch.uint8)
    torch.cuda.synchronize()

    def follow():
        eng.decode_follow(d[0], d[1], d[2], d[3], out, status, ent_cap, edata, n_ent)

    def follow_step():
        follow()
        eng.step_decoded(out, ent_cap)

    def yard():
        eng.decode(c[0], c[1], c[2], c[3], cout, cstatus)

    us = {"decode_follow": [], "decode_follow+step": [], "decode": []}
    for rep in range(3 + args.reps):
        for name, fn in (("decode_follow", follow), ("decode", yard), ("decode_follow+step", follow_step)):
            if name == "decode_follow+step":
                eng.load_groups(g)  # every timed step is the first: it appends and commits
                eng.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if rep >= 3:
                us[name].append(e0.elapsed_time(e1) * 1e3)
    st = eng.stats()
    ents = int(n_ent.item())
    assert ents == G and bool((status == abi.HB_WIRE_OK).all().item()) and bool((cstatus == abi.HB_WIRE_OK).all().item())
    assert st[abi.HB_STAT_ENTRIES] == G and st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_FAULTS] == 0
    model_f = len(data) + n * (16 + 64 + 48 + 1 + 8) + 20 * ents
    model_d = len(cdata) + nc * (16 + 64 + 32 + 1)
    res = []
    for name, model, recs, wire in (("decode_follow", model_f, n, len(data)), ("decode_follow+step", None, n, len(data)),
                                    ("decode", model_d, nc, len(cdata))):
        r = dict(case=name, groups=G, replicas=N, reps=args.reps, records=recs, wire_bytes=int(wire),
                 entries=ents if name != "decode" else 0, event_us=stat(us[name]))
        if model is not None:
            med = r["event_us"]["median"]
            r.update(model_bytes=int(model), model_GBps_at_median=float(model / med / 1e3),
                     records_per_s_at_median=float(recs / med * 1e6))
        print(json.dumps(r), flush=True)
        res.append(r)
    ratio = dict(case="ratio", decode_follow_over_decode=res[0]["event_us"]["median"] / res[2]["event_us"]["median"],
                 per_wire_byte=(res[0]["event_us"]["median"] / len(data)) / (res[2]["event_us"]["median"] / len(cdata)))
    print(json.dumps(ratio), flush=True)
    res.append(ratio)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
