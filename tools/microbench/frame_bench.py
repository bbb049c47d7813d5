#!/usr/bin/env python3
"""Micro-benchmark of framed peer streams (not product code).

On a handle of 1,048,576 groups x 3 in append mode (mode 5) with two peers in the node
table, one cfg2 step (one dense proposal and two acks per group: four MsgApp per group,
two for each peer, one of the two with the new 16-byte entry), 25 runs after 3 warm-ups
between HIP events on the handle's stream, interleaved per repetition, median [min, max]
in microseconds:

  chain        hb_egress + hb_egress_bin + hb_encode_ents + hb_peer_spans
  chain+frame  the same and hb_frame: the six-call send chain
  frame        hb_frame alone on the binned records
  dir          hb_gid_dir_build over the 1,048,576 ids (cap 2^21)
  unframe      hb_unframe of the two resulting frames (4,194,304 rows) in one call
  unframe+dec  hb_unframe + hb_decode_follow of the same rows
  holes        hb_unframe of the same frames with every row's hole bit set: no probe

The two frames go to different nodes; so that one receiver can take both in one call, the
second frame's `to` word is rewritten to the first's before the receive side is timed.
The receive side runs on the same handle (a directory over the same id column: the
lookups are the same random probes whatever the slot order).

Byte models.  hb_frame: per row group (4 B), status (1 B) and two off words (16 B) read
and 12 B written = 33 B, beside one gid word gathered from the [capacity] column (8 B useful
of a random 64 B line).  hb_unframe: 12 B per row read, a probe (one key and one slot
word, 12 B useful of two random lines), 16 B per row written = 40 B.  hb_gid_dir_build: 8 B
per key cleared, 8 B per id read, a compare-and-swap of 8 B and a 4 B slot per id.  The
rates are the model over the median, lower bounds on what the memory system moved.

  python tools/microbench/frame_bench.py [--out profiles/frame_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from etcd_amd import abi, frame, synth  # noqa: E402
from etcd_amd.hipbatch import Engine, GidDir  # noqa: E402
from tools.microbench.egress_bench import dv, load_one_older_run, peers  # noqa: E402
from tools.microbench.encode_ents_bench import source, stats, timed  # noqa: E402

G, N, W, SELF, PL = 1 << 20, 3, 256, 1, 16
FRAME_MODEL, UNFRAME_MODEL = 4 + 1 + 16 + 12, 12 + 12 + 16


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
        cap = 4 * G
        eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=cap + 8, stream=stream)
        eng.load_groups(g)
        eng.load_peers(peers())
        load_one_older_run(eng, g)
        eng.set_egress(True, apps=True)
        eng.set_egress_peers(np.array([2, 3], np.uint64))
        b0 = synth.cfg2_batch(g, 0, seed=seed)
        x = {k: dv(torch, b0[k]) for k in ("group", "info", "term", "index", "props")}
        eng.step(x["group"], x["info"], x["term"], x["index"], None, x["props"], host=False)
        z = lambda dt, k: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
        mk = lambda: {name: z(torch.int32 if dt == "<u4" else torch.int64, cap) for name, dt in abi.OUT_BATCH_FIELDS}  # noqa: E731
        raw, out = mk(), mk()
        count, total = z(torch.int64, 1), z(torch.int64, 1)
        off, status = z(torch.int64, cap + 1), z(torch.uint8, cap)
        bin_off, span, ispan, fstat = z(torch.int64, 4), z(torch.int64, 4), z(torch.int64, 4), z(torch.int32, 3)
        src = source(torch, synth.cfg2_entry_source(g, 0, PL))
        data = z(torch.uint8, (91 + 40 + PL) * cap)
        index = z(torch.uint8, frame.isize(cap) + 128)
        ids = (np.arange(1, G + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1 << 63)
        gid = dv(torch, ids)
        dcap = frame.dir_cap(G)
        d = GidDir(z(torch.int64, dcap), z(torch.int32, dcap), dcap)
        dups = z(torch.int32, 1)

        def chain():
            eng.egress(SELF, raw, cap, count)
            eng.egress_bin(raw, cap, out, bin_off, n_dev=count)
            eng.encode_ents(SELF, out, cap, src, data, off, status, total, n_dev=count)
            eng.peer_spans(off, bin_off, span)

        def frame_only():
            eng.frame(SELF, 7, out, off, status, bin_off, span, gid, index, ispan, fstat)

        def chain_frame():
            chain()
            frame_only()

        def dir_build():
            eng.gid_dir_build(gid, d, dups)

        us = timed(torch, stream, (chain, chain_frame, frame_only, dir_build), args.reps)
        records, wire = int(count.item()), int(total.item())
        isp = ispan.cpu().numpy().view(np.uint64)
        sp = span.cpu().numpy().view(np.uint64)
        boff = bin_off.cpu().numpy().view(np.uint64)
        rows = int(boff[2])
        assert records == cap and rows == cap and int(boff[1]) == 2 * G and int(dups.item()) == 0
        assert fstat.cpu().numpy().tolist() == [0, 0, 0] and int(isp[2]) == 2 * frame.isize(2 * G)
        # ---- the receive side: both frames in one call ------------------------------------------
        to2 = torch.tensor([2, 0, 0, 0, 0, 0, 0, 0], dtype=torch.uint8, device="cuda")
        index[int(isp[1]) + 16:int(isp[1]) + 24] = to2
        frames = [(int(isp[k]), int(isp[k + 1] - isp[k]), int(sp[k]), int(sp[k + 1] - sp[k]), SELF) for k in (0, 1)]
        u_off, u_len, u_grp = z(torch.int64, rows), z(torch.int32, rows), z(torch.int32, rows)
        fst, unk = z(torch.int32, 2), z(torch.int64, 1)
        ent_cap = 2 * G
        fout = {k: z(torch.int32 if k in ("group", "info") else torch.int64, rows + 1)
                for k in ("group", "info", "term", "index", "hint", "commit", "eoff")}
        fout["eterm"], fout["edesc"] = z(torch.int64, ent_cap), z(torch.int32, ent_cap)
        edata, n_ent, dstatus = z(torch.int64, ent_cap), z(torch.int64, 1), z(torch.uint8, rows)

        def unframe():
            eng.unframe(2, index, frames, d, len(data), u_off, u_len, u_grp, fst, unk)

        def unframe_decode():
            unframe()
            eng.decode_follow(data, u_off, u_len, u_grp, fout, dstatus, ent_cap, edata, n_ent)

        # the same two frames with every row a hole: no row probes the directory
        holes = index.clone()
        for k in (0, 1):
            c = frame.rows(frames[k][1])
            lo = frames[k][0] + frame.HEADER + 8 * c
            holes[lo:lo + 4 * c].view(torch.int32).bitwise_or_(-0x80000000)
        h_off, h_len, h_grp, h_fst, h_unk = z(torch.int64, rows), z(torch.int32, rows), z(torch.int32, rows), \
            z(torch.int32, 2), z(torch.int64, 1)

        def unframe_holes():
            eng.unframe(2, holes, frames, d, len(data), h_off, h_len, h_grp, h_fst, h_unk)

        us += timed(torch, stream, (unframe, unframe_decode, unframe_holes), args.reps)
        assert h_fst.cpu().numpy().tolist() == [0, 0] and int(h_unk.item()) == 0 and not h_len.any()
        assert np.array_equal(h_off.cpu().numpy(), off.cpu().numpy()[:rows])
        assert fst.cpu().numpy().tolist() == [0, 0] and int(unk.item()) == 0
        assert (dstatus.cpu().numpy() == abi.HB_WIRE_OK).all() and int(n_ent.item()) == ent_cap
        want = out["group"].cpu().numpy().view(np.uint32)
        assert np.array_equal(u_grp.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(u_off.cpu().numpy(), off.cpu().numpy()[:rows])
        dir_model = 8 * dcap + (8 + 8 + 4) * G
        for name, u, model in (("chain: hb_egress + hb_egress_bin + hb_encode_ents + hb_peer_spans", us[0], None),
                               ("chain + hb_frame", us[1], None),
                               ("hb_frame alone", us[2], FRAME_MODEL * rows),
                               ("hb_gid_dir_build, 1,048,576 ids, cap 2^21", us[3], dir_model),
                               ("hb_unframe, two frames", us[4], UNFRAME_MODEL * rows),
                               ("hb_unframe + hb_decode_follow", us[5], None),
                               ("hb_unframe, every row a hole (no probe)", us[6], (12 + 16) * rows)):
            r = dict(case=name, groups=G, rows=rows, wire_bytes=wire, index_bytes=int(isp[2]), event_us=stats(u))
            if model is not None:
                r.update(model_bytes=int(model), model_GBps_at_median=float(model / np.median(u) / 1e3))
            print(json.dumps(r), flush=True)
            results.append(r)
        eng.close()
    res = dict(bench="hb_frame / hb_unframe / hb_gid_dir_build", results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
