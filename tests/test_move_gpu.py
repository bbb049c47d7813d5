"""GPU tests of hb_move_groups (the batched device move of whole groups).

test_move_keeps_every_word: every word the handle keeps for a slot arrives at
its destination as it was, vacated slots are empty, untouched slots do not
change, the log-ring extents travel and none is leaked, bad arguments are
refused.  test_steps_after_moves_match_oracle: groups that keep being moved
step and tick exactly as the oracle's (which never moves anything), through
the permutation kept by tests/move_util.py.
"""
import numpy as np
import pytest

from etcd_amd import abi, synth
from oracle.pyoracle import OracleGroups

from . import wire_util as WU
from .lift_util import lifted
from .move_util import MovedPair
from .test_wire_gpu import _decode_dev

pytestmark = pytest.mark.gpu

DRAWS = np.random.default_rng(77).integers(0, 1 << 63, 4096, dtype=np.uint64)

CAP, LIVE, W8 = 200, 150, 8


def _mapping(rng):
    """150 pairs over 200 slots (0..149 live): in this order a swap, a 3-cycle,
    a chain into an empty slot, a live dst that is not a src (overwritten), an
    identity pair, an empty src, then every other live slot to a random
    arrangement of their own slots and free ones.  Any prefix is a valid mapping."""
    pairs = [(0, 1), (1, 0),            # swap
             (2, 3), (3, 4), (4, 2),    # 3-cycle
             (20, 150), (21, 20),       # chain: 21 -> 20 -> 150 (150 empty), 21 vacated
             (30, 31),                  # 31 is live and not a source: overwritten
             (5, 5),                    # identity
             (199, 198)]                # an empty slot moves too
    used = {0, 1, 2, 3, 4, 5, 20, 21, 30, 31}
    rest = np.array([s for s in range(LIVE) if s not in used])
    pool = np.concatenate([rest, np.arange(151, 198)])
    dst = rng.choice(pool, len(rest), replace=False)
    pairs += list(zip(rest.tolist(), dst.tolist()))
    assert len(pairs) == 150
    src, dst = np.array(pairs, dtype=np.uint32).T
    assert len(set(src.tolist())) == 150 and len(set(dst.tolist())) == 150
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def _snapshot(eng, nmax):
    """Everything the public getters show, per slot."""
    ins = {}
    for g in range(eng.capacity):
        for s in range(nmax):
            st, vals = eng.get_inflights(g, s)
            ins[(g, s)] = (st, vals.tolist())
    return dict(groups=eng.get_groups(), timers=eng.get_timers(), ins=ins,
                caps=[eng.log_capacity(g) for g in range(eng.capacity)])


@pytest.mark.parametrize("count", [1, 64, 65, 150])
@pytest.mark.parametrize("nmax", [3, 5, 7])
def test_move_keeps_every_word(nmax, count):
    """Capacity 200 (no multiple of 64) with 150 live groups of n = 1..nmax,
    W = 8, finite max_msg_size 40 (both log rings in use, grown to different
    capacities), random timers with rand_pos up to 50, peer ids loaded;
    windows set with hb_set_inflights: wrapping (start 6, count 5), full
    (start 3, count 8), empty (start 2, count 0), besides the random ones.
    The first `count` pairs of the 150-pair mapping of _mapping()."""
    import torch
    from etcd_amd.hipbatch import Engine, lib
    rng = np.random.default_rng(1000 * nmax + count)
    g, runs, ins = synth.random_groups(LIVE, nmax, seed=7 + nmax, W=W8)
    g = OracleGroups(g, runs, W8, 40, ins).groups()  # the canonical records (term run derived from the log)
    eng = Engine(CAP, max_replicas=nmax, max_inflight=W8, max_msg_size=40, max_batch=1 << 12)
    eng.load_groups(g)
    for (gi, s), vals in ins.items():
        eng.set_inflights(gi, s, int(g[gi]["pr"][s]["ins_start"]), vals)
    eng.set_inflights(0, 0, 6, np.arange(100, 105, dtype=np.uint64))   # wraps: 6 + 5 > 8
    eng.set_inflights(1, 0, 3, np.arange(200, 208, dtype=np.uint64))   # full
    eng.set_inflights(2, 0, 2, np.zeros(0, dtype=np.uint64))           # empty, start kept
    eng.load_entry_sizes(synth.window_sizes(g, runs, seed=3))
    eng.load_term_runs(synth.older_runs(g, runs))
    eng.reserve_log(np.arange(0, LIVE, 3, dtype=np.uint32), 64, 32)    # some larger extents
    eng.load_timers(synth.random_timers(CAP, seed=nmax))
    ids = (1000 * (np.arange(CAP, dtype=np.uint64)[:, None] + 1) + np.arange(abi.HB_MAX_REPLICAS, dtype=np.uint64))
    eng.load_peers(ids)

    src, dst = _mapping(rng)
    src, dst = src[:count].copy(), dst[:count].copy()
    before = _snapshot(eng, nmax)
    eng.move_groups(src, dst)
    after = _snapshot(eng, nmax)

    sset, dset = set(src.tolist()), set(dst.tolist())
    for s, d in zip(src.tolist(), dst.tolist()):
        assert after["groups"][d].tobytes() == before["groups"][s].tobytes(), f"group record {s} -> {d}"
        assert after["timers"][d].tobytes() == before["timers"][s].tobytes(), f"timers {s} -> {d}"
        assert after["caps"][d] == before["caps"][s], f"log capacity {s} -> {d}"
        for k in range(nmax):
            assert after["ins"][(d, k)] == before["ins"][(s, k)], f"inflights {s} -> {d} slot {k}"
    for v in sset - dset:
        assert after["groups"]["n"][v] == 0, f"vacated slot {v} is not empty"
    for u in set(range(CAP)) - sset - dset:
        assert after["groups"][u].tobytes() == before["groups"][u].tobytes(), f"untouched slot {u}"
        assert after["timers"][u].tobytes() == before["timers"][u].tobytes(), f"untouched slot {u} timers"
        assert after["caps"][u] == before["caps"][u]
        for k in range(nmax):
            assert after["ins"][(u, k)] == before["ins"][(u, k)]
    # every slot still owns one extent of each kind and the pool did not change
    assert sorted(after["caps"]) == sorted(before["caps"])
    if count >= 3:
        assert after["ins"][(1, 0)] == (6, list(range(100, 105))) and after["ins"][(0, 0)] == (3, list(range(200, 208)))
    if count >= 5:
        assert after["ins"][(3, 0)][0] == 2 and after["ins"][(3, 0)][1] == []

    # the peer row travelled: a MsgAppResp to a moved slot from the last peer of the group now there
    live = [(s, d) for s, d in zip(src.tolist(), dst.tolist()) if s < LIVE]
    recs, grp, want = [], [], []
    for s, d in live:
        k = int(g[s]["n"]) - 1
        recs.append(WU.gogo_marshal(abi.HB_MSG_APP_RESP, to=1, frm=int(ids[s, k]), term=int(g[s]["term"]), index=1))
        grp.append(d)
        want.append(k)
    data, off, ln = WU.pack(recs)
    out, status = _decode_dev(eng, torch, data, off, ln, np.array(grp, dtype=np.uint32))
    assert (status.cpu().numpy() == abi.HB_WIRE_OK).all()
    info = out["info"].cpu().numpy().view(np.uint32)
    assert np.array_equal((info >> 4) & 0xF, np.array(want, dtype=np.uint32)), "From resolves through the moved peer row"

    # refused before any device work
    L = lib()
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
    for bs, bd in [([1, 1], [2, 3]), ([1, 2], [3, 3]), ([CAP], [0]), ([0], [CAP])]:
        a, b = u32(bs), u32(bd)
        assert L.hb_move_groups(eng.h, len(a), a.ctypes.data, b.ctypes.data) == abi.HB_EINVAL
    assert L.hb_move_groups(eng.h, 2, None, None) == abi.HB_EINVAL
    assert L.hb_move_groups(eng.h, 0, None, None) == abi.HB_OK
    again = eng.get_groups()
    assert again.tobytes() == after["groups"].tobytes(), "a refused call changed the state"
    eng.close()


def _case(name):
    """(groups, runs, nmax, extra MovedPair arguments, batch(k, now, rng))"""
    G = 300
    if name == "n3_lagging":
        g, runs = synth.lagging_groups(G, 3, seed=0x5EED0003, W=W8)
        return g, runs, 3, {}, lambda k, now, rng: synth.cfg3_open_batch(now, rng)
    if name == "n5_fuzz":
        g, runs, ins = synth.random_groups(G, 5, seed=12, W=W8)
        return g, runs, 5, dict(ins=ins), lambda k, now, rng: synth.random_batch(g, 1200, seed=120 + k)
    if name == "n5_fuzz_W40":  # the same at the record and event-word boundary (tests/lift_util.py)
        g, runs, ins = lifted("W40", *synth.random_groups(G, 5, seed=12, W=W8), delta=24, eps=20)
        return g, runs, 5, dict(ins=ins), lambda k, now, rng: synth.random_batch(g, 1200, seed=120 + k)
    if name == "sized":
        g, runs, ins = synth.random_groups(G, 3, seed=13, W=W8)
        sizes = synth.window_sizes(g, runs, seed=14)
        return g, runs, 3, dict(ins=ins, max_msg_size=40, sizes=sizes), \
            lambda k, now, rng: synth.attach_entry_descs(synth.random_batch(g, 1200, seed=130 + k), G, seed=140 + k)
    if name == "mixed_term_runs":
        g, runs = synth.mixed_groups(G, 3, seed=0x5EED0007, last_hi=1 << 12, with_runs=True)
        return g, runs, 3, dict(term_runs=True), lambda k, now, rng: synth.mixed_batch(g, k, seed=0x5EED0007)[0]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["n3_lagging", "n5_fuzz", "sized", "mixed_term_runs", "n5_fuzz_W40"])
def test_steps_after_moves_match_oracle(name):
    """300 groups in capacity 320, W = 8: n = 3 leaders with lagging followers
    (cfg3 open loop), n = 5 fuzz with inflight windows, n = 3 with
    max_msg_size 40 and sizes loaded (the size ring is read after the move and
    hb_reserve_log grows moved slots), and synth.mixed_groups with its term
    runs loaded (the term-run ring is read after the move).  6 steps with one
    tick after the third; before every step and the tick a random third of the
    groups moves to a random arrangement of their own and the free slots
    (swaps, cycles, chains).  Full parity each time: events, statistics, every
    group record, inflight windows, timers."""
    g, runs, nmax, kw, batch = _case(name)
    pair = MovedPair(g, runs, nmax, W8, 320, max_batch=1 << 14, **kw)
    pair.set_timers(synth.random_timers(len(g), seed=5, et_hi=6, ht_hi=3), DRAWS)
    rng = np.random.default_rng(99)
    mrng = np.random.default_rng(7)
    now = pair.og.groups()
    moved = 0
    for k in range(6):
        src, dst = pair.view.random_move(mrng)
        moved += int((src != dst).sum())
        _, _, now = pair.step(batch(k, now, rng), ctx=f"{name} step {k}")
        if k == 2:
            pair.view.random_move(mrng)
            _, _, now = pair.tick(ctx=f"{name} tick", check_inflights=True)
    assert moved > 300 and not np.array_equal(pair.view.slot, np.arange(len(g)))
    pair.eng.real.close()
