#!/usr/bin/env python3
"""Micro-benchmark of hb_encode_ents (not product code).

On a handle of 1,048,576 groups x 3 in append mode (mode 5), one cfg2 step (one
dense proposal and two acks per group: four MsgApp per group, two of them with
the new entry), 25 runs after 3 warm-ups between HIP events on the handle's
stream, median [min, max] in microseconds:

  (a) hb_egress + hb_encode_ents with 16-byte payloads (synth.cfg2_entry_source)
      and, interleaved in the same process, hb_egress + hb_encode on the same
      records (the host would still splice 2M entries into that one's output);
  (b) hb_encode_ents alone on the step's records: 1 KiB payloads at 1M groups,
      and 64 KiB payloads on the 65,536 records of the first 16,384 groups (the
      cooperative copy).

The byte model of hb_encode_ents: the record columns read (52 B a record, + 4 B
of `group` for a record with entries), 20 B of window per record with entries,
20 B per entry, the payload read, and the bytes, off (8 B) and status (1 B)
written.  For (a) the hb_egress side is egress_bench.py's model.

  python tools/microbench/encode_ents_bench.py [--out profiles/encode_ents_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from etcd_amd import abi, synth  # noqa: E402
from etcd_amd.hipbatch import Engine, EntSource  # noqa: E402
from tools.microbench.egress_bench import REC_READ, REC_WRITE, dv, load_one_older_run, peers  # noqa: E402

G, N, W, SELF = 1 << 20, 3, 256, 1


def stats(us):
    return dict(median=float(np.median(us)), min=float(np.min(us)), max=float(np.max(us)))


def source(torch, src):
    t = {k: dv(torch, v) for k, v in src.items()}
    return EntSource(t["first"], t["count"], t["start"], t["eterm"], t["edesc"], t["edata"], t["data"])


def ents_model(records, with_ents, entries, payload, wire):
    return REC_READ * records + 4 * with_ents + 20 * with_ents + 20 * entries + payload + wire + 9 * records


def timed(torch, stream, runs, reps):
    """runs: callables timed in turn inside every repetition (interleaved); us per callable."""
    us = [[] for _ in runs]
    for rep in range(3 + reps):
        for k, run in enumerate(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            if rep >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(stream):
        seed = 0x5EED0002
        g, _ = synth.steady_groups(G, N, seed=seed, with_runs=False)
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=2 * G, stream=stream)
        eng.load_groups(g)
        eng.load_peers(peers())
        load_one_older_run(eng, g)
        eng.set_egress(True, apps=True)
        b0 = synth.cfg2_batch(g, 0, seed=seed)
        x = {k: dv(torch, b0[k]) for k in ("group", "info", "term", "index", "props")}
        eng.step(x["group"], x["info"], x["term"], x["index"], None, x["props"], host=False)
        cap = 4 * G
        z = lambda dt, k: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
        out = {name: z(torch.int32 if dt == "<u4" else torch.int64, cap) for name, dt in abi.OUT_BATCH_FIELDS}
        count, total = z(torch.int64, 1), z(torch.int64, 1)
        off, status = z(torch.int64, cap + 1), z(torch.uint8, cap)
        # ---- (a) 16-byte payloads, against hb_encode on the same records ----------------------
        PL = 16
        src = source(torch, synth.cfg2_entry_source(g, 0, PL))
        data = z(torch.uint8, (91 + 40 + PL) * cap)
        data0, off0, status0, total0 = z(torch.uint8, 91 * cap), z(torch.int64, cap + 1), z(torch.uint8, cap), z(torch.int64, 1)

        def with_ents():
            eng.egress(SELF, out, cap, count)
            eng.encode_ents(SELF, out, cap, src, data, off, status, total, n_dev=count)

        def plain():
            eng.egress(SELF, out, cap, count)
            eng.encode(SELF, out, cap, data0, off0, status0, total0, n_dev=count)

        def ents_only():
            eng.encode_ents(SELF, out, cap, src, data, off, status, total, n_dev=count)

        def plain_only():
            eng.encode(SELF, out, cap, data0, off0, status0, total0, n_dev=count)
        us = timed(torch, stream, (with_ents, plain, ents_only, plain_only), args.reps)
        records, wire, wire0 = int(count.item()), int(total.item()), int(total0.item())
        st = status.cpu().numpy()
        assert records == 4 * G and (st == abi.HB_WIRE_OK).all()
        assert int((status0.cpu().numpy() & abi.HB_WIRE_SPLICE != 0).sum()) == 2 * G
        _, counts = eng.event_words()
        egress_model = 8 * int(counts.sum()) + 48 * G + 8 * records + REC_WRITE * records
        m = ents_model(records, 2 * G, 2 * G, 2 * G * PL, wire)
        m0 = REC_READ * records + wire0 + 9 * records
        for name, u, model, w in (("(a) hb_egress + hb_encode_ents, 16 B payloads", us[0], egress_model + m, wire),
                                  ("(a) hb_egress + hb_encode, the same records (entries left to the host)", us[1],
                                   egress_model + m0, wire0),
                                  ("(a) hb_encode_ents alone, 16 B payloads", us[2], m, wire),
                                  ("(a) hb_encode alone", us[3], m0, wire0)):
            r = dict(case=name, groups=G, records=records, wire_bytes=w, event_us=stats(u), model_bytes=int(model),
                     model_GBps_at_median=float(model / np.median(u) / 1e3))
            print(json.dumps(r), flush=True)
            results.append(r)
        del data, data0, src
        # ---- (b) the cooperative copy ---------------------------------------------------------
        for PL, groups in ((1024, G), (65536, 16384)):
            s = synth.cfg2_entry_source(g[:groups], 0, PL)
            if groups < G:  # the windows of the other groups are empty
                pad = G - groups
                s["first"] = np.concatenate([s["first"], np.zeros(pad, np.uint64)])
                s["count"] = np.concatenate([s["count"], np.zeros(pad, np.uint32)])
                s["start"] = np.concatenate([s["start"], np.zeros(pad, np.uint64)])
            src = source(torch, s)
            grp = out["group"].cpu().numpy().view(np.uint32)[:records]
            if groups < G:  # the records of the first `groups` groups, in the step's order
                keep = np.nonzero(grp < groups)[0]
                sub = {name: dv(torch, out[name].cpu().numpy()[keep]) for name, _ in abi.OUT_BATCH_FIELDS}
            else:
                sub = out
            n = 4 * groups
            data = z(torch.uint8, (91 + 40 + PL) * 2 * groups + 91 * 2 * groups)
            off_b, status_b = z(torch.int64, n + 1), z(torch.uint8, n)

            def run():
                eng.encode_ents(SELF, sub, n, src, data, off_b, status_b, total)
            (u,) = timed(torch, stream, (run,), args.reps)
            wire = int(total.item())
            assert (status_b.cpu().numpy() == abi.HB_WIRE_OK).all() and wire > 2 * groups * PL
            model = ents_model(n, 2 * groups, 2 * groups, 2 * groups * PL, wire)
            r = dict(case=f"(b) hb_encode_ents alone, {PL} B payloads, {groups} groups", groups=groups, records=n,
                     wire_bytes=wire, payload_bytes=2 * groups * PL, event_us=stats(u), model_bytes=int(model),
                     model_GBps_at_median=float(model / np.median(u) / 1e3),
                     payload_copy_GBps_at_median=float(2 * 2 * groups * PL / np.median(u) / 1e3))
            print(json.dumps(r), flush=True)
            results.append(r)
            del data, src
        eng.close()
    res = dict(bench="hb_encode_ents", results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
