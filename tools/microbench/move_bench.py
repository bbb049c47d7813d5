#!/usr/bin/env python3
"""Micro-benchmark of hb_move_groups (not product code).

A handle of 1,048,576 groups x 3 with MaxInflightMsgs 256; K randomly chosen
groups are permuted among their own slots (every source is a destination, so
nothing is vacated), K in {1 Ki, 64 Ki, 1 Mi} with empty inflight windows, and
64 Ki groups whose two followers each hold a 4-entry window.

Per case: 3 warm-up calls, then 25 timed ones.  A call is bracketed by HIP
events on the handle's apply stream (it uploads the slot lists, runs the
gather, reads the window count back, runs the scatter and synchronizes, so the
event time is the whole call as the stream sees it) and by the host clock.
Reported: median, min and max in microseconds, and the bytes of a line-granular
model (64 B per distinct 64-byte line read at the sources or written at the
destinations of every per-group array, plus the staging buffer written and read
once and the slot lists) with the rate they imply at the median.

  python tools/microbench/move_bench.py [--out profiles/move_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from etcd_amd import synth  # noqa: E402
from etcd_amd.hipbatch import Engine  # noqa: E402

G, N, W = 1 << 20, 3, 256
LINE = 64


def model_bytes(src, dst, windows):
    """64 B per distinct line touched at src (read) and dst (written)."""
    def lines(slots, elem):
        return len(np.unique(slots // (LINE // elem)))
    u64_cols = 8 + 3 * N + 2  # the [G] columns, match / next / pending rows, trc / trx
    u32_cols = N + 3          # pm rows, elapsed / rpos / tcfg
    b = 0
    for slots in (src, dst):
        b += LINE * (u64_cols * lines(slots, 8) + u32_cols * lines(slots, 4))
    words = 8 + 4 * N + 2 + 2
    b += 2 * 8 * words * len(src)        # the staging buffer, written then read
    b += 2 * 2 * 4 * len(src)            # src / dst lists, read by both kernels
    if windows:                          # [N][W][G]: every window entry is a line of its own
        b += 2 * LINE * windows * (N - 1) * len(src) + 2 * 8 * windows * (N - 1) * len(src)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    g, _ = synth.steady_groups(G, N, seed=3, with_runs=False)
    win_groups = rng.choice(G, 1 << 16, replace=False)
    for s in (1, 2):  # 4-entry windows for the last case (the ring words themselves are whatever they are)
        g["pr"]["ins_count"][win_groups, s] = 4
        g["pr"]["ins_start"][win_groups, s] = 254  # wraps at W
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=1 << 10)
    eng.set_stream(stream)
    eng.load_groups(g)
    plain = np.setdiff1d(np.arange(G), win_groups)
    cases = [("1Ki empty windows", rng.choice(plain, 1 << 10, replace=False), 0),
             ("64Ki empty windows", rng.choice(plain, 1 << 16, replace=False), 0),
             ("64Ki 4-entry windows", win_groups, 4),
             ("1Mi (64Ki of them with 4-entry windows)", np.arange(G), 0)]
    results = []
    for name, slots, windows in cases:
        src = np.ascontiguousarray(slots, dtype=np.uint32)
        dev, host = [], []
        for rep in range(3 + args.reps):
            dst = np.ascontiguousarray(rng.permutation(src), dtype=np.uint32)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            eng.move_groups(src, dst)
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if rep >= 3:
                dev.append(e0.elapsed_time(e1) * 1e3)
                host.append((t1 - t0) * 1e6)
        b = model_bytes(src.astype(np.int64), dst.astype(np.int64), windows)
        if name.startswith("1Mi"):
            b += 2 * LINE * 4 * 2 * len(win_groups) + 2 * 8 * 4 * 2 * len(win_groups)
        r = dict(case=name, moves=int(len(src)), reps=args.reps,
                 event_us=dict(median=float(np.median(dev)), min=float(np.min(dev)), max=float(np.max(dev))),
                 host_us=dict(median=float(np.median(host)), min=float(np.min(host)), max=float(np.max(host))),
                 model_bytes=int(b), model_GBps_at_median=float(b / np.median(dev) / 1e3))
        results.append(r)
        print(json.dumps(r), flush=True)
    after = eng.get_groups()
    assert int((after["n"] == N).sum()) == G, "a group was lost"
    out = dict(bench="hb_move_groups", groups=G, replicas=N, max_inflight=W, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
