#!/usr/bin/env python3
"""Micro-benchmark of per-peer egress: hb_egress_bin in the egress chain (not product code).

The two workloads of egress_bench.py on a handle of 1,048,576 groups x 3
(follow: one MsgAppResp and one MsgHeartbeatResp per group; tick: half the
groups leaders, two MsgHeartbeat each), each with the groups' peer rows drawn
from a pool of 3 and of 64 node ids, the whole pool in the node table.

Per case the step (or tick) runs once with egress on; then, over that step's
events, 3 warm-up and 25 timed repetitions each, bracketed by HIP events on the
handle's stream, of

  pair   hb_egress + hb_encode                                   (before this call existed)
  chain  hb_egress + hb_egress_bin + hb_encode + hb_peer_spans   (per-peer streams)
  bin    hb_egress_bin alone, on the records of the last hb_egress
  encode hb_encode alone, on the binned records

in one process, interleaved per repetition (pair, chain, bin, encode, pair, ...)
so that clock and cache state drift over all four alike.  Reported: median
[min, max] in microseconds, and for `bin` the bytes of its model and the rate
they imply at the median:

  12 B read to classify (to, info) + 56 B read and 56 B written to move the
  record + 4 B for src                                   = 128 B per record.

(The tiled path also writes and reads one key byte per record and the tile
histograms; the model leaves them out, so the rate is a lower bound on what the
memory system moved.)

  python tools/microbench/egress_bin_bench.py [--out profiles/egress_bin_bench.json]
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

G, N, W, SELF = 1 << 20, 3, 256, 1 << 40
BIN_MODEL = 12 + 56 + 56 + 4


def dv(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])).cuda()


def pool_ids(p):
    """p node ids with bits in both halves (so every compare of the lookup matters)."""
    return (np.arange(1, p + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)


def peer_rows(ids, seed):
    """Per group three distinct ids of the pool."""
    rng = np.random.default_rng(seed)
    p = len(ids)
    a = rng.integers(0, p, G)
    d1 = rng.integers(1, p - 1, G)
    d2 = d1 + 1 + rng.integers(0, 1 << 30, G) % (p - 1 - d1)
    rows = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    for s, d in enumerate((0, d1, d2)):
        rows[:, s] = ids[(a + d) % p]
    return rows


class Sink:
    """Device buffers of one chain."""

    def __init__(self, torch, cap, nb):
        mk = lambda: {name: torch.zeros(cap, dtype=torch.int32 if dt == "<u4" else torch.int64, device="cuda")  # noqa: E731
                      for name, dt in abi.OUT_BATCH_FIELDS}
        self.cap, self.raw, self.out = cap, mk(), mk()
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.total = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.data = torch.zeros(91 * cap, dtype=torch.uint8, device="cuda")
        self.off = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        self.status = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        self.src = torch.zeros(cap, dtype=torch.int32, device="cuda")
        self.bin_off = torch.zeros(nb + 2, dtype=torch.int64, device="cuda")
        self.span = torch.zeros(nb + 2, dtype=torch.int64, device="cuda")

    def pair(self, eng):
        eng.egress(SELF, self.raw, self.cap, self.count)
        eng.encode(SELF, self.raw, self.cap, self.data, self.off, self.status, self.total, n_dev=self.count)

    def bin(self, eng):
        eng.egress_bin(self.raw, self.cap, self.out, self.bin_off, src=self.src, n_dev=self.count)

    def encode(self, eng):
        eng.encode(SELF, self.out, self.cap, self.data, self.off, self.status, self.total, n_dev=self.count)

    def chain(self, eng):
        eng.egress(SELF, self.raw, self.cap, self.count)
        self.bin(eng)
        self.encode(eng)
        eng.peer_spans(self.off, self.bin_off, self.span)


def timed(torch, stream, eng, sink, reps):
    what = ("pair", "chain", "bin", "encode")
    us = {w: [] for w in what}
    for rep in range(3 + reps):
        for w in what:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            getattr(sink, w)(eng)
            e1.record(stream)
            e1.synchronize()
            if rep >= 3:
                us[w].append(e0.elapsed_time(e1) * 1e3)
    return us


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def report(name, pool, sink, us, reps):
    records, wire = int(sink.count.item()), int(sink.total.item())
    boff = sink.bin_off.cpu().numpy().view(np.uint64)
    span = sink.span.cpu().numpy().view(np.uint64)
    assert int(boff[-1]) == records and int(span[-1]) == wire and int(boff[pool]) == records  # "other" is empty
    cnt = np.diff(boff[:pool + 1].astype(np.int64))
    model = BIN_MODEL * records
    med = {w: float(np.median(v)) for w, v in us.items()}
    r = dict(case=name, pool=pool, groups=G, replicas=N, reps=reps, records=records, wire_bytes=wire,
             records_per_peer=dict(min=int(cnt.min()), max=int(cnt.max())),
             pair_us=stat(us["pair"]), chain_us=stat(us["chain"]), bin_us=stat(us["bin"]), encode_us=stat(us["encode"]),
             chain_over_pair=med["chain"] / med["pair"], bin_over_encode=med["bin"] / med["encode"],
             bin_model_bytes=int(model), bin_model_GBps_at_median=float(model / med["bin"] / 1e3))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(stream):
        # ---- follow ---------------------------------------------------------------------
        seed = 0x5EED0006
        g, _ = synth.follow_groups(G, N, seed=seed, with_runs=False)
        b = synth.follow_batch(g, 0, seed=seed)
        nmsg = len(b["group"])
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=nmsg, stream=stream)
        eng.load_groups(g)
        eng.set_egress(True)
        d = {k: dv(torch, b[k]) for k in ("group", "info", "term", "hint", "eoff", "eterm", "index", "commit")}
        eng.step(d["group"], d["info"], d["term"], d["index"], d["hint"], None, host=False, eoff=d["eoff"],
                 commit=d["commit"], eterm=d["eterm"])
        for pool in (3, 64):
            ids = pool_ids(pool)
            eng.load_peers(peer_rows(ids, seed + pool))
            eng.set_egress_peers(ids)
            sink = Sink(torch, nmsg, pool)
            us = timed(torch, stream, eng, sink, args.reps)
            results.append(report("follow: MsgAppResp + MsgHeartbeatResp per group", pool, sink, us, args.reps))
            assert int(sink.count.item()) == nmsg
            del sink
        eng.close()
        del d
        # ---- tick: half the groups leaders beating ------------------------------------
        seed = 0x5EED0002
        g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
        g["state"][1::2] = abi.HB_STATE_FOLLOWER
        g["lead"][1::2] = 1
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G, stream=stream)
        eng.load_groups(g)
        t = synth.random_timers(G, seed=seed, et_hi=10, ht_hi=1, pos_hi=0)
        t["election_tick"] = 10
        t["elapsed"] = 0
        eng.load_timers(t)
        eng.set_rand(np.random.default_rng(seed).integers(0, 1 << 63, 64, dtype=np.uint64))
        eng.load_peers(peer_rows(pool_ids(3), seed))  # (hb_egress needs a peer row; each case loads its own)
        eng.set_egress(True)
        eng.tick()
        for pool in (3, 64):
            ids = pool_ids(pool)
            eng.load_peers(peer_rows(ids, seed + pool))
            eng.set_egress_peers(ids)
            sink = Sink(torch, 2 * G, pool)
            us = timed(torch, stream, eng, sink, args.reps)
            results.append(report("tick: half the groups leaders, two MsgHeartbeat each", pool, sink, us, args.reps))
            assert int(sink.count.item()) == (N - 1) * (G // 2)
            del sink
        eng.close()
    out = dict(bench="hb_egress + hb_egress_bin + hb_encode + hb_peer_spans", results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
