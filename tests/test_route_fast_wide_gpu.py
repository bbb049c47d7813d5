"""k_route_fast's wide form: 1024 lanes and, with two leader-side
slots, 4096 groups per workgroup, so that one workgroup owns a 4096-group
bucket that two 2048-group sisters shared; its partitions' M event chunks are
then placed by a prefix in LDS instead of the bucket's global cursor.

Wave v of workgroup b owns the four group-waves k = 0..3 at groups
b * 4096 + k * 1024 + v * 64 + [0, 64).

Every handle is created with HB_SIS_LOG=4 (4096-group buckets at any size),
HB_RF_WIDE=1 and HB_FAST_STEADY_COUNT=1, stepped against the oracle
(tests.parity_util.Pair) and beside a second handle created with HB_RF_WIDE=0
that takes the same batches: sorted events, statistics, groups and the count
of steady group-waves are equal, and hb_step_kernels shows the wide bit on the
first handle only."""
import ctypes as C

import numpy as np
import pytest

from etcd_amd import abi, synth
from tests.parity_util import Pair, sort_events

gpu = pytest.mark.gpu

N, W = 3, 8
BK, RG, LANES, WAVE, PART = 4096, 4096, 1024, 64, 256
KEYS = ("group", "info", "term", "index", "hint")


def _waves(G):
    return (G + WAVE - 1) // WAVE


class Both:
    """A wide handle with its oracle, and a narrow handle on the same groups."""

    def __init__(self, monkeypatch, g, runs, term_runs=None, inflight=W):
        from etcd_amd.hipbatch import Engine
        monkeypatch.delenv("HB_ROUTE_FUSE", raising=False)
        monkeypatch.delenv("HB_FAST_STEADY", raising=False)
        monkeypatch.setenv("HB_SIS_LOG", "4")
        monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
        monkeypatch.setenv("HB_RF_WIDE", "1")
        G = len(g)
        mb = max(4 * G, 64)
        self.pair = Pair(g, runs, N, inflight, max_batch=mb, term_runs=term_runs)
        monkeypatch.setenv("HB_RF_WIDE", "0")
        self.narrow = Engine(G, max_replicas=N, max_inflight=inflight, max_batch=mb)
        monkeypatch.setenv("HB_RF_WIDE", "1")
        init = self.pair.og.groups()
        self.narrow.load_groups(init)
        if term_runs:
            self.narrow.load_term_runs(synth.older_runs(init, runs))

    def step(self, b, ctx, **kw):
        pair, narrow = self.pair, self.narrow
        wide, pair.eng = pair.eng, narrow  # (the narrow handle's log rings, from the oracle's state before the step)
        try:
            pair.reserve(b)
        finally:
            pair.eng = wide
        ev, st, now = pair.step(b, ctx=ctx, **kw)
        narrow.step_batch(b, host=True)
        kw_, kn = wide.step_kernels(), narrow.step_kernels()
        assert kw_ & abi.HB_KERN_ROUTE_FAST and kw_ & abi.HB_KERN_ROUTE_FAST_WIDE, f"{ctx}: wide handle ran {kw_}"
        assert kn & abi.HB_KERN_ROUTE_FAST and not kn & abi.HB_KERN_ROUTE_FAST_WIDE, f"{ctx}: narrow handle ran {kn}"
        assert np.array_equal(sort_events(narrow.events()), sort_events(ev)), f"{ctx}: events differ from HB_RF_WIDE=0"
        assert np.array_equal(narrow.stats(), st), f"{ctx}: statistics differ from HB_RF_WIDE=0"
        assert np.array_equal(narrow.get_groups(), wide.get_groups()), f"{ctx}: groups differ from HB_RF_WIDE=0"
        assert narrow.steady_waves() == wide.steady_waves(), f"{ctx}: steady group-waves differ from HB_RF_WIDE=0"
        return ev, st, now


def _batch(g, step, seed):
    b = synth.cfg2_batch(g, step, seed=seed)
    b["hint"] = np.zeros(len(b["group"]), dtype=np.uint64)
    return b


def _msgs(b, i):
    return np.nonzero(b["group"] == i)[0]


def _append(b, i, info, term, index):
    for k, v in (("group", i), ("info", info), ("term", term), ("index", index), ("hint", 0)):
        b[k] = np.append(b[k], np.array([v], dtype=b[k].dtype))


def _keep(b, keep):
    for k in KEYS:
        b[k] = b[k][keep]


# ---------------------------------------------------------------------------
# Handle edges: a part-filled single workgroup, exactly one bucket, one group
# in a second bucket, and the grid padding (the grid is whole groups of 8
# buckets: every handle here has blocks that return at once).
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G", [1, 4095, 4096, 4097, 8191, 8193])
def test_handle_edges(G, monkeypatch):
    g, runs = synth.steady_groups(G, N, seed=1001, last_hi=1 << 16)
    both = Both(monkeypatch, g, runs)
    for t in range(2):
        _, st, _ = both.step(_batch(g, t, seed=1002), ctx=f"edges G={G}, step {t}")
        assert st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_APPRESP] == 2 * G
        assert both.pair.eng.steady_waves() == _waves(G)


# ---------------------------------------------------------------------------
# Every pending set.  G = 4096 + 1024 + 65: two buckets, two workgroups, the
# second part-filled, its second group-wave cut at G (one group).  The 16 waves
# of the first workgroup: wave p gets pattern p (bit k: its group-wave k is not
# steady) at step 0, by one odd lane per such group-wave.
# ---------------------------------------------------------------------------
G_ALL = RG + LANES + WAVE + 1
KINDS = ("probe", "reject", "third", "follower")


def _group(p, k, shift):
    return k * LANES + p * WAVE + (7 * p + 13 * k + shift) % WAVE


def _schedule():
    """odd[t]: the (group, kind) changes of step t; off[t]: the group-waves
    (group // 64) that are not steady at step t.  A Probe follower is healed by
    its ack in the step (steady afterwards); a rejected ack leaves its follower
    in Probe, paused, for the next step too, whose ack heals it; a third
    message lasts its step; a follower-state group has work at every step."""
    odd = [[], [], []]
    for p in range(16):
        for k in range(4):
            if (p >> k) & 1:  # step 0: pattern p, the four kinds in turn
                odd[0].append((_group(p, k, 0), KINDS[(p + k) % 4]))
            else:  # step 1: the complement, on other groups
                odd[1].append((_group(p, k, 1), ("third", "reject")[(p + k) % 2]))
                if (p + k) % 2 == 0:  # step 2: again where step 1 had a third message, on other groups
                    odd[2].append((_group(p, k, 2), "third"))
    off = []
    for t in range(3):
        s = {g // WAVE for g, _ in odd[t]}
        s |= {g // WAVE for g, kind in odd[0] if kind == "follower"}
        if t:
            s |= {g // WAVE for g, kind in odd[t - 1] if kind == "reject"}
        off.append(s)
    return odd, off


def _patterns(off_t):
    """Wave p's pending set, as the group-waves in off_t give it."""
    return [sum(1 << k for k in range(4) if (k * LANES + p * WAVE) // WAVE in off_t) for p in range(16)]


def test_schedule_covers_every_pending_set():  # (no GPU: the schedule alone)
    odd, off = _schedule()
    assert _patterns(off[0]) == list(range(16))
    assert {kind for _, kind in odd[0]} == set(KINDS)
    # each of the workgroup's 64 group-waves is steady at some step and not steady at another
    gws = {(k * LANES + p * WAVE) // WAVE for p in range(16) for k in range(4)}
    assert gws == set(range(RG // WAVE))
    always = off[0] & off[1] & off[2]
    never = gws - (off[0] | off[1] | off[2])
    follower = {g // WAVE for g, kind in odd[0] if kind == "follower"}
    assert always == follower and not never
    assert len({g for t in range(3) for g, _ in odd[t]}) == sum(len(o) for o in odd)  # (distinct groups)


@gpu
def test_every_pending_set(monkeypatch):
    odd, off = _schedule()
    g, runs = synth.steady_groups(G_ALL, N, seed=1011, last_hi=1 << 16)
    for i, kind in odd[0]:
        if kind == "probe":
            g["pr"][i][1]["state"] = abi.HB_PR_PROBE
        elif kind == "follower":
            g["state"][i], g["lead"][i] = abi.HB_STATE_FOLLOWER, 1
    both = Both(monkeypatch, g, runs)
    seen = set()
    for t in range(3):
        b = _batch(g, t, seed=1012)
        for i, kind in odd[t]:
            if kind == "reject":
                b["info"][_msgs(b, i)[0]] |= 1 << 8
            elif kind == "third":
                _append(b, i, abi.HB_MSG_APP_RESP | (1 << 4), g["term"][i], g["last_index"][i] + t + 1)
        both.step(b, ctx=f"pending sets, step {t}")
        assert both.pair.eng.steady_waves() == _waves(G_ALL) - len(off[t]), f"step {t}"
        seen |= set(_patterns(off[t]))
    assert seen == set(range(16))


# ---------------------------------------------------------------------------
# Both halves of a bucket: the groups two sisters owned.  Idle and steady
# stripes alternate every 1024 groups (a lane's consecutive groups alternate);
# a batch addresses the lower halves of the buckets, the upper halves, or both.
# ---------------------------------------------------------------------------
G_HALF = 2 * BK + WAVE + 1


@gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_both_halves_of_a_bucket(flip, monkeypatch):
    g, runs = synth.steady_groups(G_HALF, N, seed=1021 + flip, last_hi=1 << 16)
    both = Both(monkeypatch, g, runs)
    idx = np.arange(G_HALF)
    stripe = (idx // LANES + flip) % 2 == 1
    low = idx % BK < BK // 2
    acked = np.zeros(G_HALF, dtype=np.int64)  # steps taken per group: the index its next ack carries
    for t, half in enumerate((low, ~low, np.ones(G_HALF, dtype=bool))):
        busy = stripe & half
        b = _batch(g, 0, seed=1023 + t)
        b["index"] = (g["last_index"][b["group"]] + (acked[b["group"]] + 1).astype(np.uint64)).astype(np.uint64)
        _keep(b, busy[b["group"]])
        b["props"][~busy] = 0
        _, st, _ = both.step(b, ctx=f"halves flip {flip}, step {t}")
        n = int(busy.sum())
        assert st[abi.HB_STAT_COMMITS] == n and st[abi.HB_STAT_APPRESP] == 2 * n
        assert both.pair.eng.steady_waves() == _waves(G_HALF)
        acked += busy


# ---------------------------------------------------------------------------
# Hand-over and the bucket walk: groups with 0, 1, 2, 3 and 5 messages on both
# sides of every partition boundary of two buckets (more messages than slots
# are handed to k_apply, which reads the count, the slots and, above the slots,
# walks the bucket by the key bytes this kernel wrote).
# ---------------------------------------------------------------------------
COUNTS = (0, 1, 2, 3, 5)


@gpu
def test_hand_over_at_partition_boundaries(monkeypatch):
    G = G_HALF
    g, runs = synth.steady_groups(G, N, seed=1031, last_hi=1 << 16)
    both = Both(monkeypatch, g, runs)
    want = {}
    for edge in range(PART, G, PART):
        for j, c in enumerate(COUNTS):
            want[edge - 1 - j] = c
            want[edge + j] = COUNTS[len(COUNTS) - 1 - j]
    want = {i: c for i, c in want.items() if i < G}
    special = np.zeros(G, dtype=bool)
    special[list(want)] = True
    for t in range(2):
        b = _batch(g, t, seed=1032)
        _keep(b, ~special[b["group"]])
        for i, c in sorted(want.items()):
            for m in range(c):
                _append(b, i, abi.HB_MSG_APP_RESP | ((1 + m % 2) << 4), g["term"][i], g["last_index"][i] + t + 1)
        perm = np.random.default_rng(1033 + t).permutation(len(b["group"]))
        _keep(b, perm)
        _, st, _ = both.step(b, ctx=f"hand-over, step {t}")
        assert st[abi.HB_STAT_MSGS] == len(perm) and st[abi.HB_STAT_FAULTS] == 0


# ---------------------------------------------------------------------------
# Event chunks: with one workgroup per bucket the M chunks of the bucket's
# partitions are an exclusive prefix of their reservations from the region's
# base.  Bucket bk's region starts at epm * (NB * 256 + lo + bk * 4096 * props)
# words, lo = the records of the buckets below, props = 1 with dense proposals,
# and a partition reserves epm * (its messages + 256 * props) words.
# ---------------------------------------------------------------------------
class _Dev:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _chunks(eng):
    import torch
    from etcd_amd import hipbatch
    base, off, cnt, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
    eng.sync()
    assert hipbatch.lib().hb_events_device(eng.h, C.byref(base), C.byref(off), C.byref(cnt), C.byref(n)) == abi.HB_OK
    assert n.value == eng.n_chunks()[0]
    o = torch.as_tensor(_Dev(off.value, n.value, "<i8"), device="cuda").cpu().numpy().astype(np.int64)
    c = torch.as_tensor(_Dev(cnt.value, n.value, "<i4"), device="cuda").cpu().numpy().astype(np.int64)
    return o, c


@gpu
def test_event_chunks_in_the_bucket_region(monkeypatch):
    G = G_HALF
    NB, NBK = (G + PART - 1) // PART, (G + BK - 1) // BK
    g, runs = synth.steady_groups(G, N, seed=1041, last_hi=1 << 16)
    both = Both(monkeypatch, g, runs)
    epm = None
    for t, dense in enumerate((True, False)):
        b = _batch(g, t, seed=1042)
        if t == 1:  # no proposals: the acks of step 0 again, fewer in the odd partitions
            b = _batch(g, 0, seed=1043)
            _keep(b, ((b["group"] // PART) % 2 == 0) | (b["info"] >> 4 == 1))
            b["props"] = None
        both.step(b, ctx=f"event chunks, dense {dense}")
        off, cnt = _chunks(both.pair.eng)
        per_part = np.bincount(b["group"] // PART, minlength=NB).astype(np.int64)
        props = 1 if dense else 0
        if epm is None:
            epm = off[1] // (NB * PART)  # (bucket 0's region starts right after the P chunks)
            assert epm > 0 and off[1] == epm * NB * PART
        lo = 0
        for bk in range(NBK):
            parts = range(bk * 16, min(bk * 16 + 16, NB))
            start = epm * (NB * PART + lo + bk * BK * props)
            end = start + epm * (int(per_part[parts.start:parts.stop].sum()) + BK * props)
            at = start
            for p in parts:
                o, n = int(off[2 * p + 1]), int(cnt[2 * p + 1])
                assert at <= o, f"dense {dense}: partition {p}'s M chunk overlaps its lower sister or starts below the region"
                assert n <= epm * (int(per_part[p]) + PART * props), f"dense {dense}: partition {p} overran its reservation"
                at = o + epm * (int(per_part[p]) + PART * props)
                assert at <= end, f"dense {dense}: partition {p}'s M chunk leaves bucket {bk}'s region"
            lo += int(per_part[parts.start:parts.stop].sum())


# ---------------------------------------------------------------------------
# The other forms, wide: a follower-side batch (X mode: MsgApp + MsgHeartbeat,
# 2048 groups per workgroup) and a batch with MsgProp rows (three slots, 2048
# groups per workgroup).  Both still have two sisters per bucket.
# ---------------------------------------------------------------------------
def _leader_cycle(g, rng, last, ents):
    """Both followers ack the last index, then a MsgProp of ents[g] entries
    (Term 0), all groups interleaved in one random arrival order."""
    G = len(g)
    grp = np.repeat(np.arange(G), 3)[rng.permutation(3 * G)].astype(np.uint32)
    order = np.argsort(grp, kind="stable")
    kind = np.zeros(3 * G, np.int64)
    kind[order] = np.tile(np.arange(3), G)  # the group's 0th, 1st, 2nd message in arrival order
    t = np.where(kind == 2, abi.HB_MSG_PROP, abi.HB_MSG_APP_RESP).astype(np.uint32)
    slot = np.where(kind == 2, 0, kind + 1).astype(np.uint32)
    return dict(group=grp, info=(t | (slot << np.uint32(4))).astype(np.uint32),
                term=np.where(kind == 2, 0, g["term"][grp].astype(np.int64)).astype(np.uint64),
                index=np.where(kind == 2, ents[grp], last[grp]).astype(np.uint64), hint=None, props=None, msg_props=True)


@gpu
@pytest.mark.parametrize("G", [BK + 1, 2 * BK + WAVE + 1])
def test_follower_side_batch_wide(G, monkeypatch):
    g, runs = synth.follow_groups(G, N, seed=1051, last_hi=1 << 14, with_runs=True)
    both = Both(monkeypatch, g, runs, term_runs=True, inflight=256)
    for t in range(2):
        _, st, now = both.step(synth.follow_batch(g, t, seed=1052, ents=2), ctx=f"follow G={G}, step {t}",
                               check_inflights=False)
        assert st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_ENTRIES] == 2 * G
        assert st[abi.HB_STAT_MSGS] == 2 * G and st[abi.HB_STAT_FAULTS] == 0


@gpu
@pytest.mark.parametrize("G", [BK + 1, 2 * BK + WAVE + 1])
def test_msgprop_batch_wide(G, monkeypatch):
    g, runs = synth.steady_groups(G, N, seed=1061, last_hi=1 << 12)
    both = Both(monkeypatch, g, runs, inflight=256)
    rng = np.random.default_rng(1062)
    last = g["last_index"].astype(np.int64).copy()
    for t in range(2):
        ents = rng.integers(1, 4, G).astype(np.int64)
        _, st, _ = both.step(_leader_cycle(g, rng, last, ents), ctx=f"msgprop G={G}, step {t}")
        assert st[abi.HB_STAT_FAULTS] == 0 and st[abi.HB_STAT_ENTRIES] == int(ents.sum())
        last = last + ents
