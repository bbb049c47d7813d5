#!/usr/bin/env python3
"""Micro-benchmark of wire egress: hb_egress + hb_encode (not product code).

Workloads on a handle of 1,048,576 groups x 3:

  follow  the follow workload of bench.py (synth.follow_groups / follow_batch:
          every group receives its leader's MsgApp and MsgHeartbeat), so a step
          leaves one MsgAppResp and one MsgHeartbeatResp per group to send;
  tick    one MultiNode.Tick with half the groups leaders beating
          (HeartbeatTick 1): two MsgHeartbeat per leader;
  campaign  (--workload campaign, after the two above in the same process) one
          MultiNode.Tick in which every group's election timeout fires, vote
          mode on (hb_set_egress bit HB_EGRESS_VOTES): two MsgVote per group,
          every group one EVC_VBCAST word.

  cfg2    (--workload cfg2, a run of its own) the headline step of bench.py in
          append mode (hb_set_egress bit HB_EGRESS_APPS, mode 5): one dense
          proposal and two acks per group, so every group sends four MsgApp,
          two with the new entry (spliced by the host) and two with only the
          new Commit; every group's older term run is loaded, as a node's are.
          With --max-msg-size N the handle has that finite MaxSizePerMsg and
          hb_set_egress_limit is on: every group's last entry
          has a size loaded and every proposed entry a random descriptor, as
          synth.window_sizes / attach_entry_descs make them, and each MsgApp
          with entries takes limitSize's cut from the group's size ring.

  forward (--workload forward, a run of its own) a follower node's step of one
          proposal per group (synth.follow_groups: every group has a lead), mode 1: every
          group's HB_EV_PROP_FWD word.  hb_egress + hb_encode over that one step's events with
          hb_set_wire_props(HB_WIRE_PROPS_OUT) off (no record: the host replays the events and
          marshals every MsgProp) and on (one split MsgProp record per group), interleaved
          repetition by repetition.

  catchup (--workload catchup, a run of its own) the catch-up after an election:
          every group a leader whose follower 2 is in Probe at the boundary (Next = the first
          index of the current-term run) and rejects that probe with a hint two entries lower,
          so the step resends below the boundary: one MsgApp per group whose LogTerm is in no
          event.  --logterm 0: every record is HB_OUT_HOST; --logterm 1
          (hb_set_egress_logterm): every record carries the term read from the group's run
          ring.  One knob value per process, so that the two can be interleaved process by
          process; --workload cfg2 takes --logterm too (no send there is below the boundary).

Per workload: the step (or tick) runs once with egress on, then hb_egress +
hb_encode (chained through the device-resident count, no host sync between
them) run 3 warm-up and 25 timed times over that step's events, each pair
bracketed by HIP events on the handle's stream.  Reported: median [min, max]
in microseconds, the records and wire bytes, and the bytes of a model with the
rate it implies at the median:

  events read (8 B per word) + the snapshot (16 B per group, 24 B in vote
  mode: lterm0, 48 B in append mode: lterm0, commit0, bl0, blt0) + the peer id (8 B per record) + the record written and read
  back (56 + 52 B) + the wire bytes written.

(The model counts the event words once; hb_egress's count pass reads them a
second time.)  The cost of the pre-step snapshot is measured beside it: K
back-to-back steps of the follow and the cfg2 workload with egress off, on
(mode 1) and on with votes (mode 3: the third column), in the same run.

  python tools/microbench/egress_bench.py [--out profiles/egress_bench.json]
  python tools/microbench/egress_bench.py --workload campaign [--out profiles/egress_vote_bench.json]
  python tools/microbench/egress_bench.py --workload cfg2 [--out profiles/egress_app_bench.json]
  python tools/microbench/egress_bench.py --workload cfg2 --max-msg-size 1048576
  python tools/microbench/egress_bench.py --workload forward [--out profiles/wire_props_forward.json]
  python tools/microbench/egress_bench.py --workload catchup --logterm 1
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

G, N, W, SELF = 1 << 20, 3, 256, 1
REC_WRITE, REC_READ = 2 * 4 + 6 * 8, 4 + 6 * 8


def dv(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])).cuda()


def peers():
    p = np.zeros((G, abi.HB_MAX_REPLICAS), np.uint64)
    p[:, :N] = np.arange(1, N + 1, dtype=np.uint64)
    return p


class Sink:
    """Device buffers of one hb_egress + hb_encode pair."""

    def __init__(self, torch, cap):
        self.cap = cap
        self.out = {name: torch.zeros(cap, dtype=torch.int32 if dt == "<u4" else torch.int64, device="cuda")
                    for name, dt in abi.OUT_BATCH_FIELDS}
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.total = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.data = torch.zeros(91 * cap, dtype=torch.uint8, device="cuda")
        self.off = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        self.status = torch.zeros(cap, dtype=torch.uint8, device="cuda")

    def run(self, eng):
        eng.egress(SELF, self.out, self.cap, self.count)
        eng.encode(SELF, self.out, self.cap, self.data, self.off, self.status, self.total, n_dev=self.count)


def timed(torch, stream, eng, sink, reps):
    us = []
    for rep in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        sink.run(eng)
        e1.record(stream)
        e1.synchronize()
        if rep >= 3:
            us.append(e0.elapsed_time(e1) * 1e3)
    return us


def report(name, eng, sink, us, reps, snap=16):
    _, counts = eng.event_words()
    words = int(counts.sum())
    records, wire = int(sink.count.item()), int(sink.total.item())
    model = 8 * words + snap * G + 8 * records + (REC_WRITE + REC_READ) * records + wire
    r = dict(case=name, groups=G, replicas=N, reps=reps, event_words=words, records=records, wire_bytes=wire,
             event_us=dict(median=float(np.median(us)), min=float(np.min(us)), max=float(np.max(us))),
             model_bytes=int(model), model_GBps_at_median=float(model / np.median(us) / 1e3),
             records_per_s_at_median=float(records / np.median(us) * 1e6))
    print(json.dumps(r), flush=True)
    return r


def steps_ms(torch, stream, one, steps, warmup=5):
    for k in range(warmup):
        one(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for k in range(warmup, warmup + steps):
        one(k)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def load_one_older_run(eng, g):
    """hb_load_term_runs for every group at once: the run below the current-term run of
    synth.steady_groups logs, (0, Term - 1)."""
    from etcd_amd import hipbatch
    n = len(g)
    gs, ns = np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.uint32)
    flat = np.zeros((n, 2), dtype=np.uint64)
    flat[:, 1] = np.maximum(g["term"].astype(np.int64) - 1, 0).astype(np.uint64)
    rc = hipbatch.lib().hb_load_term_runs(eng.h, n, gs.ctypes.data, ns.ctypes.data, flat.ctypes.data)
    assert rc == abi.HB_OK, rc


def load_last_sizes(eng, g, seed, max_len=64):
    """hb_load_entry_sizes for every group at once: Entry.Size() of its last entry, a random
    payload as synth.window_sizes draws them (the ring then keeps its minimum capacity; a cfg2
    step sends from the last index, which the ring always holds)."""
    from etcd_amd import hipbatch
    n = len(g)
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, max_len + 1, n).astype(np.uint64)
    has = rng.random(n) >= 0.2
    z = 4 + synth._sov(g["term"]) + synth._sov(g["last_index"]) + np.where(has, 1 + ln + synth._sov(ln), 0)
    gs, ns, z = np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.uint32), z.astype(np.uint32)
    rc = hipbatch.lib().hb_load_entry_sizes(eng.h, n, gs.ctypes.data, ns.ctypes.data, z.ctypes.data)
    assert rc == abi.HB_OK, rc


def snapshot_modes(torch, stream, eng, one, steps, name):
    """ms per step of `one` with egress off, then mode 1, then mode 5 (K back-to-back steps each)."""
    span = 5 + steps
    off_ms = steps_ms(torch, stream, one, steps)
    eng.set_egress(True)
    on_ms = steps_ms(torch, stream, lambda k: one(span + k), steps)
    eng.set_egress(True, apps=True)
    apps_ms = steps_ms(torch, stream, lambda k: one(2 * span + k), steps)
    return dict(workload=name, steps=steps, ms_per_step_egress_off=off_ms, ms_per_step_egress_on=on_ms,
                ms_per_step_egress_apps=apps_ms)


def cfg2_main(args, torch, stream):
    results, snapshot = [], []
    # ---- follow steps: egress off / mode 1 / mode 5 ------------------------------------------
    seed = 0x5EED0006
    g, _ = synth.follow_groups(G, N, seed=seed, with_runs=False)
    b = synth.follow_batch(g, 0, seed=seed)
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=len(b["group"]), stream=stream)
    eng.load_groups(g)
    eng.load_peers(peers())
    d = {k: dv(torch, b[k]) for k in ("group", "info", "term", "hint", "eoff", "eterm", "index", "commit")}
    i_inc = dv(torch, ((b["info"] & 0xF) == abi.HB_MSG_APP).astype(np.uint64))

    def follow(k):
        eng.step(d["group"], d["info"], d["term"], d["index"] + i_inc * k, d["hint"], None, host=False,
                 eoff=d["eoff"], commit=d["commit"] + k, eterm=d["eterm"])
    snapshot.append(snapshot_modes(torch, stream, eng, follow, args.steps, "follow"))
    eng.close()
    del d
    # ---- cfg2 steps: egress off / mode 1 / mode 5, then one step's hb_egress + hb_encode -------
    seed = 0x5EED0002
    g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
    limit = args.max_msg_size
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=2 * G, stream=stream,
                 **(dict(max_msg_size=limit) if limit else {}))
    eng.load_groups(g)
    eng.load_peers(peers())
    load_one_older_run(eng, g)
    b0 = synth.cfg2_batch(g, 0, seed=seed)  # step k acks last + k + 1 (the same arrival order every step)
    x = {k: dv(torch, b0[k]) for k in ("group", "info", "term", "index", "props")}
    sized = {}
    if limit:  # the same descriptors every step: one proposed entry per group
        load_last_sizes(eng, g, seed + 1)
        bd = synth.attach_entry_descs(b0, G, seed=seed + 2)
        sized = {k: dv(torch, bd[k]) for k in ("edesc", "eoff", "peoff")}
        eng.set_egress_limit(True)
    eng.set_egress_logterm(bool(args.logterm))

    def cfg2(k):
        eng.step(x["group"], x["info"], x["term"], x["index"] + k, None, x["props"], host=False, **sized)
    snapshot.append(snapshot_modes(torch, stream, eng, cfg2, args.steps, "cfg2"))
    print(json.dumps(snapshot), flush=True)
    assert eng.egress_mode() == abi.HB_EGRESS_ON | abi.HB_EGRESS_APPS and eng.egress_limit() == bool(limit)
    cfg2(3 * (5 + args.steps))
    sink = Sink(torch, 4 * G)
    us = timed(torch, stream, eng, sink, args.reps)
    r = report("cfg2: one proposal and two acks per group, four MsgApp each (append mode)", eng, sink, us, args.reps,
               snap=48)
    info = sink.out["info"].cpu().numpy().view(np.uint32)
    status = sink.status.cpu().numpy()
    r["records_spliced"] = int((status & abi.HB_WIRE_SPLICE != 0).sum())
    r["records_flagged"] = int((info & abi.HB_OUT_HOST != 0).sum())
    r["records_entries_flag"] = int((info & abi.HB_OUT_ENTS != 0).sum())
    print(json.dumps({k: r[k] for k in ("records", "records_spliced", "records_flagged")}), flush=True)
    assert r["records"] == 4 * G and ((info & 0xF) == abi.HB_MSG_APP).all()
    assert r["records_spliced"] == r["records_entries_flag"] == 2 * G and r["records_flagged"] == 0
    assert (status[info & abi.HB_OUT_ENTS == 0] == abi.HB_WIRE_OK).all()
    r["max_msg_size"] = limit
    r["logterm"] = bool(args.logterm)
    results.append(r)
    eng.close()
    return dict(bench="hb_egress + hb_encode, append mode", results=results, snapshot_cost=snapshot)


def catchup_main(args, torch, stream):
    seed = 0x5EED0025
    g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
    # the current-term run starts at 4 or later, the Term is 2 or more: the index two below the
    # boundary exists and lies in the older run (0, Term - 1) that load_one_older_run loads
    tf = np.maximum(g["term_first"], 4).astype(np.uint64)
    last = np.maximum(g["last_index"], tf).astype(np.uint64)
    g["term"] = np.maximum(g["term"], 2)
    g["term_first"] = tf
    for f in ("last_index", "committed", "term_last"):
        g[f] = last
    pr = g["pr"]
    for s in range(N):
        pr[:, s]["match"] = last
        pr[:, s]["next"] = last + np.uint64(1)
    pr[:, 1]["state"], pr[:, 1]["match"], pr[:, 1]["next"] = abi.HB_PR_PROBE, 0, tf
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G, stream=stream)
    eng.load_groups(g)
    eng.load_peers(peers())
    load_one_older_run(eng, g)
    eng.set_egress(True, apps=True)
    eng.set_egress_logterm(bool(args.logterm))
    grp = np.random.default_rng(seed).permutation(G).astype(np.uint32)
    rej = abi.hb_info(abi.HB_MSG_APP_RESP, 1) | (1 << 8)
    d = dict(group=dv(torch, grp), info=dv(torch, np.full(G, rej, np.uint32)), term=dv(torch, g["term"][grp]),
             index=dv(torch, tf[grp] - np.uint64(1)), hint=dv(torch, tf[grp] - np.uint64(3)))
    eng.step(d["group"], d["info"], d["term"], d["index"], d["hint"], None, host=False)
    sink = Sink(torch, G)
    us = timed(torch, stream, eng, sink, args.reps)
    r = report(f"catchup: one resend two below the boundary per group, logterm {'on' if args.logterm else 'off'}", eng,
               sink, us, args.reps, snap=48)
    info = sink.out["info"].cpu().numpy().view(np.uint32)
    status = sink.status.cpu().numpy()
    r["records_flagged"] = int((info & abi.HB_OUT_HOST != 0).sum())
    r["records_spliced"] = int((status & abi.HB_WIRE_SPLICE != 0).sum())
    r["logterm"] = bool(args.logterm)
    assert r["records"] == G and ((info & 0xF) == abi.HB_MSG_APP).all()
    order = sink.out["group"].cpu().numpy().view(np.uint32)
    assert np.array_equal(sink.out["index"].cpu().numpy().view(np.uint64), tf[order] - np.uint64(3))
    if args.logterm:
        assert r["records_flagged"] == 0 and r["records_spliced"] == G
        assert np.array_equal(sink.out["log_term"].cpu().numpy().view(np.uint64), g["term"][order] - np.uint64(1))
        assert np.array_equal(sink.out["hint"].cpu().numpy().view(np.uint64), last[order])
    else:
        assert r["records_flagged"] == G and r["wire_bytes"] == 0
    print(json.dumps({k: r[k] for k in ("records", "records_spliced", "records_flagged")}), flush=True)
    eng.close()
    return dict(bench="hb_egress + hb_encode, catch-up below the boundary", results=[r])


def forward_main(args, torch, stream):
    seed = 0x5EED0006
    g, _ = synth.follow_groups(G, N, seed=seed, with_runs=False)
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G, stream=stream)
    eng.load_groups(g)
    eng.load_peers(peers())
    eng.set_egress(True)
    grp = np.random.default_rng(seed).permutation(G).astype(np.uint32)
    d = dict(group=dv(torch, grp), info=dv(torch, np.full(G, abi.hb_info(abi.HB_MSG_PROP, 0), np.uint32)),
             zero=dv(torch, np.zeros(G, np.uint64)), one=dv(torch, np.ones(G, np.uint64)))
    eng.step(d["group"], d["info"], d["zero"], d["one"], d["zero"], None, host=False, msg_props=True)
    sink = Sink(torch, G)
    us = {False: [], True: []}
    for rep in range(3 + args.reps):
        for on in (False, True):
            eng.set_wire_props(egress=on)  # (waits for the stream; the step's events stay good)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sink.run(eng)
            e1.record(stream)
            e1.synchronize()
            if rep >= 3:
                us[on].append(e0.elapsed_time(e1) * 1e3)
    results = []
    for on in (False, True):
        eng.set_wire_props(egress=on)
        sink.run(eng)
        eng.sync()
        r = report(f"forward: one proposal per group at a follower, wire_props egress {'on' if on else 'off'}", eng, sink,
                   us[on], args.reps)
        n = r["records"]
        assert n == (G if on else 0)
        if on:
            info = sink.out["info"].cpu().numpy().view(np.uint32)
            status = sink.status.cpu().numpy()
            assert (info == (abi.hb_info(abi.HB_MSG_PROP, 1) | abi.HB_OUT_ENTS)).all()
            assert (status & abi.HB_WIRE_SPLICE != 0).all()
            hint = np.sort(sink.out["hint"].cpu().numpy().view(np.uint64))
            assert np.array_equal(hint, np.arange(G, dtype=np.uint64))
        r["wire_props_egress"] = on
        results.append(r)
    eng.close()
    return dict(bench="hb_egress + hb_encode, forwarded proposals", results=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--workload", choices=("egress", "campaign", "cfg2", "forward", "catchup"), default="egress")
    ap.add_argument("--max-msg-size", type=int, default=0,
                    help="cfg2 only: a finite MaxSizePerMsg, with hb_set_egress_limit on (0: no limit, the default)")
    ap.add_argument("--logterm", type=int, choices=(0, 1), default=0,
                    help="cfg2 and catchup: hb_set_egress_logterm on (DESIGN.md 3.25; 0: off, the default)")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    results, snapshot = [], []
    if args.workload in ("cfg2", "forward", "catchup"):
        with torch.cuda.stream(stream):
            out = dict(cfg2=cfg2_main, forward=forward_main, catchup=catchup_main)[args.workload](args, torch, stream)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    with torch.cuda.stream(stream):
        # ---- follow ---------------------------------------------------------------------
        seed = 0x5EED0006
        g, _ = synth.follow_groups(G, N, seed=seed, with_runs=False)
        b = synth.follow_batch(g, 0, seed=seed)
        nmsg = len(b["group"])
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=nmsg, stream=stream)
        eng.load_groups(g)
        eng.load_peers(peers())
        d = {k: dv(torch, b[k]) for k in ("group", "info", "term", "hint", "eoff", "eterm", "index", "commit")}
        i_inc = dv(torch, ((b["info"] & 0xF) == abi.HB_MSG_APP).astype(np.uint64))
        total_steps = 3 * (5 + args.steps) + 1

        def follow(k):
            eng.step(d["group"], d["info"], d["term"], d["index"] + i_inc * k, d["hint"], None, host=False,
                     eoff=d["eoff"], commit=d["commit"] + k, eterm=d["eterm"])
        off_ms = steps_ms(torch, stream, follow, args.steps)
        eng.set_egress(True)
        on_ms = steps_ms(torch, stream, lambda k: follow(5 + args.steps + k), args.steps)
        eng.set_egress(True, votes=True)
        votes_ms = steps_ms(torch, stream, lambda k: follow(2 * (5 + args.steps) + k), args.steps)
        eng.set_egress(True)
        snapshot.append(dict(workload="follow", steps=args.steps, ms_per_step_egress_off=off_ms,
                             ms_per_step_egress_on=on_ms, ms_per_step_egress_votes=votes_ms))
        follow(total_steps - 1)
        sink = Sink(torch, nmsg)
        us = timed(torch, stream, eng, sink, args.reps)
        results.append(report("follow: MsgAppResp + MsgHeartbeatResp per group", eng, sink, us, args.reps))
        assert int(sink.count.item()) == nmsg and (sink.status.cpu().numpy() == abi.HB_WIRE_OK).all()
        eng.close()
        del sink
        # ---- cfg2 steps, egress off / on (the snapshot's cost on the headline step) -----
        seed = 0x5EED0002
        g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=2 * G, stream=stream)
        eng.load_groups(g)
        b0 = synth.cfg2_batch(g, 0, seed=seed)  # step k acks last + k + 1 (the same arrival order every step)
        x = {k: dv(torch, b0[k]) for k in ("group", "info", "term", "index", "props")}

        def cfg2(k):
            eng.step(x["group"], x["info"], x["term"], x["index"] + k, None, x["props"], host=False)
        off_ms = steps_ms(torch, stream, cfg2, args.steps)
        eng.set_egress(True)
        on_ms = steps_ms(torch, stream, lambda k: cfg2(5 + args.steps + k), args.steps)
        eng.set_egress(True, votes=True)
        votes_ms = steps_ms(torch, stream, lambda k: cfg2(2 * (5 + args.steps) + k), args.steps)
        snapshot.append(dict(workload="cfg2", steps=args.steps, ms_per_step_egress_off=off_ms,
                             ms_per_step_egress_on=on_ms, ms_per_step_egress_votes=votes_ms))
        print(json.dumps(snapshot), flush=True)
        eng.close()
        del x
        # ---- tick: half the groups leaders beating ------------------------------------
        g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
        g["state"][1::2] = abi.HB_STATE_FOLLOWER
        g["lead"][1::2] = 1
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G, stream=stream)  # (hb_encode: cap <= max_batch x (n + 4))
        eng.load_groups(g)
        eng.load_peers(peers())
        t = synth.random_timers(G, seed=seed, et_hi=10, ht_hi=1, pos_hi=0)
        t["election_tick"] = 10
        t["elapsed"] = 0
        eng.load_timers(t)
        eng.set_rand(np.random.default_rng(seed).integers(0, 1 << 63, 64, dtype=np.uint64))
        eng.set_egress(True)
        eng.tick()
        sink = Sink(torch, 2 * G)
        us = timed(torch, stream, eng, sink, args.reps)
        results.append(report("tick: half the groups leaders, two MsgHeartbeat each", eng, sink, us, args.reps))
        assert int(sink.count.item()) == (N - 1) * (G // 2)
        eng.close()
        del sink
        # ---- campaign: every group's election timeout fires, vote mode ----------------
        if args.workload == "campaign":
            g, _ = synth.follow_groups(G, N, seed=0x5EED0006, with_runs=False)
            eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=G, stream=stream)
            eng.load_groups(g)
            eng.load_peers(peers())
            t["elapsed"] = 20  # past every randomized timeout (ElectionTick 10)
            eng.load_timers(t)
            eng.set_rand(np.random.default_rng(seed).integers(0, 1 << 63, 64, dtype=np.uint64))
            eng.set_egress(True, votes=True)
            eng.tick()
            sink = Sink(torch, 2 * G)
            us = timed(torch, stream, eng, sink, args.reps)
            results.append(report("campaign: every group times out, two MsgVote each (vote mode)", eng, sink, us,
                                  args.reps, snap=24))
            info = sink.out["info"].cpu().numpy().view(np.uint32)
            assert int(sink.count.item()) == (N - 1) * G and ((info & 0xF) == abi.HB_MSG_VOTE).all()
            assert not (info & abi.HB_OUT_HOST).any() and (sink.status.cpu().numpy() == abi.HB_WIRE_OK).all()
            words, _ = eng.event_words()
            assert int(((words & np.uint64(0xF)) == abi.HB_EVW_VBCAST).sum()) == G
            eng.close()
    out = dict(bench="hb_egress + hb_encode", results=results, snapshot_cost=snapshot)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
