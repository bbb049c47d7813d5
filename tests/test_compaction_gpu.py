"""Parity under log compaction with the log-index rings at fixed size.

The application compacts as the log grows (tests/compact_util.py), so each
group's size ring (HB_SIZE_RING_MIN = 16) and term-run ring (HB_TERM_RING_MIN
= 8) wrap and drop what lies below firstIndex - 1, and hb_set_log_bounds moves
firstIndex mid-stream: sendAppend's needSnapshot branch, limitSize over a
wrapped ring and raftLog.term through a ring whose head is not 0 are compared
with the oracle on every step.  The scenario bodies are run_*(make=...): under
CompactPair on the GPU here, under OracleCompactPair on the CPU in
tests/test_compaction_ref.py, which checks that the streams reach what they
are meant to reach."""
import numpy as np
import pytest

from etcd_amd import abi, synth

from .compact_util import CompactPair, MovedCompactPair, trim_runs
from .lift_util import lifted

W = 8
NOSNAP = (3, 85, 167, 249, 331, 413, 495, 577)  # groups whose application compacts without a snapshot


def append_msgs(b, group, info, term, index, hint):
    """Messages added at the end of a batch's arrival order."""
    group = np.atleast_1d(group)
    for k, v in (("group", group), ("info", info), ("term", term), ("index", index), ("hint", hint)):
        b[k] = np.concatenate([b[k], np.broadcast_to(np.asarray(v), group.shape).astype(b[k].dtype)])
    return b


def keep_msgs(b, keep):
    for k in ("group", "info", "term", "index", "hint"):
        b[k] = b[k][keep]
    return b


def thin(b, kmax):
    """At most kmax messages per group, the first in arrival order (each message
    counts as one possible noop or term run in the reservation rule, so a step
    of n - 1 acks and more would by itself ask for a larger term-run ring)."""
    grp = b["group"].astype(np.int64)
    order = np.argsort(grp, kind="stable")
    start = np.searchsorted(grp[order], grp[order], side="left")
    rank = np.empty(len(grp), np.int64)
    rank[order] = np.arange(len(grp)) - start
    return keep_msgs(b, rank < kmax)


# ---------------------------------------------------------------- 1. leader stream
def leader_state(G, n, seed, sized, lift=None):
    """synth.lagging_groups-style leaders whose log is already compacted: every
    follower within 4 entries of lastIndex, firstIndex at most 2 below the
    slowest follower's Next, a snapshot at firstIndex - 1 (none in NOSNAP)."""
    g, runs = synth.lagging_groups(G, n, seed=seed, W=W)
    rng = np.random.default_rng(seed + 2)
    last = g["last_index"].astype(np.int64)
    for s in range(1, n):
        m = np.maximum(last - rng.integers(0, 5, G), 0)
        g["pr"][:, s]["match"] = m
        g["pr"][:, s]["next"] = m + 1
    mt = np.sort(np.stack([g["pr"][:, s]["match"] for s in range(n)], 1).astype(np.int64), axis=1)[:, ::-1]
    g["committed"] = mt[:, n // 2]
    first = np.maximum(mt[:, -1] + 1 - rng.integers(0, 3, G), 1)
    g["first_index"] = first
    g["snap_index"] = first - 1
    g["snap_index"][list(NOSNAP)] = 0
    runs = [trim_runs(runs[i], int(first[i]) - 1) for i in range(G)]
    g, runs, _ = lifted(lift, g, runs, None, delta=2048, eps=50)  # (lastIndex 1..4096, Term 1..100: both straddle)
    g["snap_index"][list(NOSNAP)] = 0
    sizes = synth.window_sizes(g, runs, seed=seed + 3, frac_full=1.0) if sized else None
    return g, runs, sizes


def compact_some(pair, now, k, rng, ctx, every=2):
    """The application: every `every`-th group (another one each step) compacts at
    committed - keep, keep in 0..3."""
    G = len(now)
    keep = rng.integers(0, 4, G)
    idx = now["committed"].astype(np.int64) - keep
    sel = ((np.arange(G) + k) % every == 0) & (now["fault"] == 0) & (now["n"] != 0) & (idx > now["first_index"].astype(np.int64) - 1)
    gs = np.nonzero(sel)[0]
    snap = np.ones(len(gs), np.uint8)
    snap[np.isin(gs, NOSNAP)] = 0
    rc, now = pair.compact(gs, idx[gs], snap, ctx)
    assert (rc == 0).all(), f"{ctx}: compaction refused {rc[rc != 0][:4]}"
    return now


def run_leader_stream(n, size, make=CompactPair, G=640 + 17, steps=72, seed=1100, lift=None):
    """Scenario 1: cfg3 open-loop traffic built from the oracle's records, 1-2
    proposals per group, then compaction.  From step 6 on one follower of each
    NOSNAP group and of every tenth group rejects with RejectHint 0 (Next falls
    to 1, below firstIndex): MsgSnap where the application made a snapshot,
    HB_FAULT_EMPTY_SNAPSHOT (raft/raft.go:252-254) where it did not."""
    sized = size is not None
    g, runs, sizes = leader_state(G, n, seed + n, sized, lift)
    kw = dict(max_msg_size=size, sizes=sizes) if sized else {}
    pair = make(g, runs, n, W, max_batch=8 * G, **kw)
    rng = np.random.default_rng(seed + 7)
    back = np.zeros(G, bool)
    back[list(NOSNAP)] = True
    back[5::10] = True
    now = pair.og.groups()
    fast = 0
    for k in range(steps):
        b = thin(synth.cfg3_open_batch(now, rng, max_props=2), 3)
        if k >= 6:  # follower s of the chosen groups sends nothing but a reject that the leader accepts
            gs = np.nonzero(back & (now["fault"] == 0) & (rng.random(G) < 0.5))[0]
            s = 1 + (k % (n - 1))
            chosen = np.zeros(G, bool)
            chosen[gs] = True
            b = keep_msgs(b, ~(chosen[b["group"]] & (((b["info"] >> 4) & 0xF) == s)))
            p = now["pr"][gs, s]
            rejected = np.where(p["state"] == abi.HB_PR_REPLICATE, now["last_index"][gs] + b["props"][gs], p["next"] - 1)
            b = append_msgs(b, gs, abi.HB_MSG_APP_RESP | (s << 4) | (1 << 8), now["term"][gs], rejected,
                            np.zeros(len(gs)))
        if sized:
            b = synth.attach_entry_descs(b, G, seed=seed + 31 * k)
        _, _, now = pair.step(b, ctx=f"leader stream n={n} size={size} step {k}",
                              check_inflights=(k % 8 == 7 or k == steps - 1))
        if pair.gpu and n == 3:
            fast += bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        now = compact_some(pair, now, k, rng, f"leader stream compact {k}")
    pair.check_capacity("leader stream end")
    assert not (pair.gpu and n == 3) or fast == steps
    return pair


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(3, None), (3, 150), (5, 150), (7, 40)])
def test_leader_stream(n, size, monkeypatch):
    if n == 3:
        monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    run_leader_stream(n, size)


# ---------------------------------------------------------------- 3. boundary known-answers
def _boundary_state(n, G=64):
    """Case c = g % 8 (leaders 0..4, followers 5..7); lastIndex 50 + g, Term 6,
    two term runs: [0, last - 10) at 5 and [last - 10, last] at 6, except every
    group with g % 16 >= 8, whose current-term run starts at last - 1."""
    g = np.zeros(G, dtype=abi.GROUP_DTYPE)
    runs = []
    for i in range(G):
        r, c = g[i], i % 8
        last = 50 + i
        tf = last - 1 if i % 16 >= 8 else last - 10
        runs.append([(0, 5), (tf, 6)])
        r["term"], r["first_index"], r["last_index"], r["committed"] = 6, 1, last, last - 2
        r["n"], r["self_slot"] = n, 0
        if c < 5:
            r["state"], r["lead"], r["vote"] = abi.HB_STATE_LEADER, 0, 0
            for s in range(n):
                p = r["pr"][s]
                p["match"], p["next"], p["state"] = last, last + 1, abi.HB_PR_PROBE if s == 0 else abi.HB_PR_REPLICATE
            comp = last - 4  # the index the case compacts at
            p = r["pr"][1]
            if c == 0:    # Next == first
                p["match"], p["next"], p["state"] = comp, comp + 1, abi.HB_PR_PROBE
            elif c in (1, 2):  # Next == first - 1 (2: no snapshot was made)
                p["match"], p["next"], p["state"] = comp - 1, comp, abi.HB_PR_PROBE
            elif c == 3:  # compacted at last: everything acked and committed
                r["committed"] = last
            elif c == 4:  # the quorum index falls below first - 1 (an application that compacts past committed)
                r["committed"] = last - 8
                for s in range(1, n):
                    r["pr"][s]["match"], r["pr"][s]["next"], r["pr"][s]["state"] = last - 8, last - 7, abi.HB_PR_PROBE
        else:
            r["state"], r["lead"], r["vote"] = abi.HB_STATE_FOLLOWER, 1, 1
            for s in range(n):
                r["pr"][s]["match"], r["pr"][s]["next"] = (last if s == 0 else 0), last + 1
            if c == 6:
                r["commit_zero"] = 1  # r.Commit is still 0: m.Index < r.Commit never holds (raft/raft.go:652)
            if c == 7:
                r["committed"], r["vote"] = last, abi.HB_REF_NONE
    return g, runs


def run_boundaries(n, make=CompactPair):
    """Scenario 3.  Returns the pair and the events per step."""
    G = 64
    g, runs = _boundary_state(n, G)
    pair = make(g, runs, n, W, max_batch=1 << 12, term_runs=True)
    ids = np.arange(G)
    case = ids % 8
    last = g["last_index"].astype(np.int64)
    comp = np.where(case == 3, last, np.where(case == 4, last - 5, np.where(case < 5, last - 4, np.where(case == 7, last, last - 2))))
    rc, now = pair.compact(ids, comp, case != 2, "boundaries compact")
    assert (rc == 0).all()
    assert np.array_equal(now["first_index"], (comp + 1).astype(np.uint64))
    assert np.array_equal(now["snap_index"], np.where(case != 2, comp, 0).astype(np.uint64))
    # step 1: the probes
    term = np.full(G, 6, np.int64)
    z = np.zeros(0, np.int64)
    b = dict(group=z.astype(np.uint32), info=z.astype(np.uint32), term=z.astype(np.uint64), index=z.astype(np.uint64),
             hint=z.astype(np.uint64))
    commit, eterm, ne = [], [], []

    def add(gs, info, index=0, hint=0, com=0, ents=()):
        gs = np.atleast_1d(gs)
        append_msgs(b, gs, info, term[gs], index, hint)
        for k in range(len(gs)):
            commit.append(int(np.broadcast_to(com, gs.shape)[k]))
            ne.append(len(ents))
            eterm.extend(ents)

    hbresp = abi.HB_MSG_HEARTBEAT_RESP | (1 << 4)
    add(ids[case <= 2], hbresp)  # Next == first: MsgApp at first - 1; Next == first - 1: MsgSnap / the fault
    c4 = ids[case == 4]
    add(c4, abi.HB_MSG_APP_RESP | (1 << 4), index=last[c4] - 6)  # quorum index last - 6 = first - 2: term() is 0, no commit
    add(c4, abi.HB_MSG_APP_RESP | (2 << 4), index=last[c4] - 6)
    f = ids[case == 5]
    fa = abi.HB_MSG_APP | (1 << 4)
    t_dummy = np.array([pair.og.term(int(i), int(comp[i])) for i in ids], np.int64)
    add(f[0::4], fa, index=comp[f[0::4]], hint=t_dummy[f[0::4]], com=last[f[0::4]], ents=(6, 6))   # first - 1, the right LogTerm
    add(f[1::4], fa, index=comp[f[1::4]], hint=t_dummy[f[1::4]] - 1, com=last[f[1::4]])            # first - 1, a wrong one
    add(f[2::4], fa, index=comp[f[2::4]] - 1, hint=5, com=last[f[2::4]])                           # index < committed
    add(f[3::4], fa, index=comp[f[3::4]] + 1, hint=6, com=last[f[3::4]], ents=(6, 6, 6))           # first: replaces nothing, appends one
    f = ids[case == 6]
    add(f, fa, index=comp[f] - 1, hint=5, com=last[f])  # first - 2 with r.Commit = 0: term() == 0, a reject
    f = ids[case == 7]  # MsgVote at Term 7 against a log that is all dummy
    term[f] = 7
    vt = abi.HB_MSG_VOTE | (2 << 4)
    add(f[0::3], vt, index=last[f[0::3]], hint=t_dummy[f[0::3]])          # as up to date: granted
    add(f[1::3], vt, index=last[f[1::3]] - 1, hint=t_dummy[f[1::3]])      # a shorter log: rejected
    add(f[2::3], vt, index=last[f[2::3]] - 5, hint=t_dummy[f[2::3]] + 1)  # a higher last term: granted
    ne = np.array(ne, np.int64)
    b.update(commit=np.array(commit, np.uint64), eoff=np.concatenate([[0], np.cumsum(ne)[:-1]]).astype(np.uint64),
             eterm=np.array(eterm, np.uint64), props=None)
    ev1, _, now = pair.step(b, ctx=f"boundaries n={n} probes")
    # step 2: the log compacted at last takes a proposal and sends it from the dummy entry
    props = (case == 3).astype(np.uint32)
    b2 = dict(group=z.astype(np.uint32), info=z.astype(np.uint32), term=z.astype(np.uint64), index=z.astype(np.uint64),
              hint=z.astype(np.uint64), props=props)
    ev2, _, now = pair.step(b2, ctx=f"boundaries n={n} proposal")
    pair.check_capacity("boundaries end")
    return pair, ev1, ev2, now, comp


def check_boundaries(n, pair, ev1, ev2, now, comp):
    """The known answers (on whichever side produced the events)."""
    G = 64
    ids = np.arange(G)
    case = ids % 8
    last0 = 50 + ids

    def evs(ev, i, t):
        e = ev[(ev["group"] == i) & (ev["type"] == t)]
        return [(int(x["to"]), int(x["x"]), int(x["aux"])) for x in e]

    for i in ids:
        c = case[i]
        late = i % 16 >= 8  # the current-term run starts at last - 1: above every compaction index but `last`
        if c == 0:
            assert evs(ev1, i, abi.HB_EV_APP) == [(1, comp[i], 0 if late else 1)], i
        elif c == 1:
            assert evs(ev1, i, abi.HB_EV_SNAP) == [(1, comp[i], 0)] and evs(ev1, i, abi.HB_EV_APP) == [], i
            p = now[i]["pr"][1]
            assert (p["state"], p["pending_snapshot"]) == (abi.HB_PR_SNAPSHOT, comp[i]), i
        elif c == 2:
            assert now[i]["fault"] == abi.HB_FAULT_EMPTY_SNAPSHOT and evs(ev1, i, abi.HB_EV_SNAP) == [], i
        elif c == 3:
            assert now[i]["first_index"] == last0[i] + 1 and now[i]["last_index"] == last0[i] + 1, i
            assert evs(ev2, i, abi.HB_EV_APP) == [(s, last0[i], 1) for s in range(1, n)], i
            assert evs(ev2, i, abi.HB_EV_LAST) == [(0, last0[i] + 1, 0)], i
        elif c == 4:
            assert evs(ev1, i, abi.HB_EV_COMMIT) == [] and now[i]["committed"] == last0[i] - 8, i
        elif c == 5:
            k = (i // 8) % 4
            resp = evs(ev1, i, abi.HB_EV_RESP)
            want = [(1, comp[i] + 2, abi.HB_RESP_APP), (1, comp[i], abi.HB_RESP_APP | abi.HB_RESP_REJECT),
                    (1, now[i]["committed"], abi.HB_RESP_APP), (1, comp[i] + 4, abi.HB_RESP_APP)][k]
            assert resp == [want], (i, resp)
            assert now[i]["last_index"] == last0[i] + (2 if k == 3 else 0), i
        elif c == 6:
            assert evs(ev1, i, abi.HB_EV_RESP) == [(1, comp[i] - 1, abi.HB_RESP_APP | abi.HB_RESP_REJECT)], i
        else:
            k = (i // 8) % 3
            rej = abi.HB_RESP_REJECT if k == 1 else 0
            assert evs(ev1, i, abi.HB_EV_RESP) == [(2, 0, abi.HB_RESP_VOTE | rej)], i
    assert (now["fault"][case != 2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 5])
def test_boundaries(n):
    check_boundaries(n, *run_boundaries(n))


# ---------------------------------------------------------------- 6. the drop rule of a caller that under-reserves
def run_drop_rule(make=CompactPair, G=64, seed=1600):
    """Scenario 6 (size ring only): capacity stays 16, the log grows past it.
    Every follower is a paused Probe, so the append steps send nothing; after
    each the oracle's sz_lo follows the header's rule, max(sz_lo, last - 15).
    The probe step: follower 1 acks sz_lo (it turns Replicate and is sent
    entries(sz_lo + 1, 150): the oldest cumulative size the ring still holds is
    the base of the cut), then answers two heartbeats (further cuts over the
    wrapped ring); in every other group follower 2 then acks sz_lo - 1, and the
    append it is owed needs a size the ring dropped: HB_FAULT_SIZE_WINDOW.
    (A heartbeat response alone cannot be the boundary probe: no state the
    reference can reach has a follower's Next beyond the lastIndex the group
    was loaded with, and sz_lo ends above it.)"""
    n, size, cap = 3, 150, abi.HB_SIZE_RING_MIN
    g, runs = synth.steady_groups(G, n, seed=seed, last_hi=1 << 10)
    g["last_index"] += 8
    g["term_last"] = g["last_index"]
    last0 = g["last_index"].astype(np.int64)
    for s in range(1, n):
        p = g["pr"][:, s]
        p["match"], p["next"], p["state"], p["paused"] = last0 - 2, last0 - 1, abi.HB_PR_PROBE, 1
    g["pr"][:, 0]["match"], g["pr"][:, 0]["next"] = last0, last0 + 1
    g["committed"] = last0 - 2
    part = g.copy()
    part["first_index"] = last0 - 4  # the caller loads the last 5 sizes only
    sizes = synth.window_sizes(part, runs, seed=seed + 1, frac_full=1.0)
    pair = make(g, runs, n, W, hold=True, max_msg_size=size, sizes=sizes, max_batch=1 << 12)
    rng = np.random.default_rng(seed + 2)
    z = np.zeros(0, np.int64)

    def follow_rule():
        info = pair.og.log_info().astype(np.int64)
        for i in range(G):
            r = pair.og.raft(i)
            r.sz_lo = max(int(r.sz_lo), int(info[i, 3]) - (cap - 1))

    for k in range(9):
        b = dict(group=z.astype(np.uint32), info=z.astype(np.uint32), term=z.astype(np.uint64), index=z.astype(np.uint64),
                 hint=z.astype(np.uint64), props=rng.integers(1, 4, G).astype(np.uint32))
        ev, _, now = pair.step(synth.attach_entry_descs(b, G, seed=seed + 10 + k), ctx=f"drop rule append {k}")
        assert not np.isin(ev["type"], (abi.HB_EV_APP, abi.HB_EV_SNAP)).any()  # no step both drops and sends
        follow_rule()
    ids = np.arange(G)
    b = dict(group=ids.astype(np.uint32), info=np.full(G, abi.HB_MSG_PROP, np.uint32), term=np.zeros(G, np.uint64),
             index=np.full(G, 40, np.uint64), hint=np.zeros(G, np.uint64), props=None, msg_props=True)
    ev, _, now = pair.step(synth.attach_entry_descs(b, G, seed=seed + 30), ctx="drop rule MsgProp of 40")
    assert not np.isin(ev["type"], (abi.HB_EV_APP, abi.HB_EV_SNAP)).any()
    follow_rule()
    last = now["last_index"].astype(np.int64)
    assert (last - last0 >= 40 + 9).all()
    szlo = last - (cap - 1)
    both = ids[ids % 2 == 1]
    ack1, ack2, hb1 = abi.HB_MSG_APP_RESP | (1 << 4), abi.HB_MSG_APP_RESP | (2 << 4), abi.HB_MSG_HEARTBEAT_RESP | (1 << 4)
    b = dict(group=z.astype(np.uint32), info=z.astype(np.uint32), term=z.astype(np.uint64), index=z.astype(np.uint64),
             hint=z.astype(np.uint64))
    append_msgs(b, ids, ack1, now["term"], szlo, 0)
    append_msgs(b, ids, hb1, now["term"], 0, 0)
    append_msgs(b, ids, hb1, now["term"], 0, 0)
    append_msgs(b, both, ack2, now["term"][both], szlo[both] - 1, 0)
    b["props"] = None
    b = synth.attach_entry_descs(b, G, seed=seed + 40)  # (no entries: a sized step still takes the offsets)
    ev, _, now = pair.step(b, ctx="drop rule probes")
    pair.check_capacity("drop rule end")
    return pair, ev, now, szlo


def check_drop_rule(pair, ev, now, szlo):
    G = len(now)
    ids = np.arange(G)
    both = ids % 2 == 1
    assert (now["fault"][both] == abi.HB_FAULT_SIZE_WINDOW).all() and (now["fault"][~both] == 0).all()
    for i in ids:
        e = ev[(ev["group"] == i) & (ev["type"] == abi.HB_EV_APP)]
        assert len(e) == 3 and (e["to"] == 1).all() and e["x"][0] == szlo[i], (i, e)  # the ack's send, then the two heartbeats'
        assert e["x"][0] < e["x"][1] < e["x"][2] <= now["last_index"][i]               # each cut short of the log's end
    assert (pair.cap_sz == abi.HB_SIZE_RING_MIN).all()


@pytest.mark.gpu
def test_drop_rule_size_ring():
    check_drop_rule(*run_drop_rule())


# ---------------------------------------------------------------- hb_set_log_bounds argument checks
@pytest.mark.gpu
def test_set_log_bounds_arguments():
    from etcd_amd.hipbatch import Engine, lib
    G = 16
    g, _ = synth.steady_groups(G, 3, seed=1700, last_hi=1 << 10)
    g["last_index"] += 8
    g["term_last"] = g["last_index"]
    eng = Engine(G, max_replicas=3, max_inflight=W, max_batch=64)
    eng.load_groups(g)
    before = eng.get_groups()
    h, u32, u64 = eng.h, np.array([1, 2], np.uint32), np.array([5, 6], np.uint64)
    call = lib().hb_set_log_bounds
    assert call(h, 2, u32.ctypes.data, np.array([5, 0], np.uint64).ctypes.data, u64.ctypes.data) == abi.HB_EINVAL  # first_index 0
    assert call(h, 2, np.array([1, G], np.uint32).ctypes.data, u64.ctypes.data, u64.ctypes.data) == abi.HB_EINVAL   # group >= capacity
    assert call(h, 0, None, None, None) == abi.HB_OK
    for args in ((None, u64.ctypes.data, u64.ctypes.data), (u32.ctypes.data, None, u64.ctypes.data),
                 (u32.ctypes.data, u64.ctypes.data, None)):
        assert call(h, 2, *args) == abi.HB_EINVAL
    assert np.array_equal(eng.get_groups(), before)  # an error leaves the state untouched
    eng.set_log_bounds(u32, u64, u64 - 1)
    after = eng.get_groups()
    assert np.array_equal(after["first_index"][u32], u64) and np.array_equal(after["snap_index"][u32], u64 - 1)
    rest = np.ones(G, bool)
    rest[u32] = False
    assert np.array_equal(after[rest], before[rest])


# ---------------------------------------------------------------- 2. follower and role-churn stream
class Batch:
    """A batch built message by message; MsgApp entries (terms) and MsgProp
    entries share one entry array, each entry with a random descriptor."""

    def __init__(self, rng, sized):
        self.rng, self.sized = rng, sized
        self.rows, self.eterm = [], []

    def add(self, g, typ, slot, term=0, index=0, hint=0, commit=0, ents=(), reject=0):
        nprop = int(index) if typ == abi.HB_MSG_PROP else 0
        self.rows.append((g, typ | (slot << 4) | (reject << 8), term, index, hint, commit, len(self.eterm)))
        self.eterm.extend(list(ents) + [0] * nprop)

    def arrays(self):
        rows = np.array(self.rows, dtype=np.int64).reshape(-1, 7)
        n = len(rows)
        # a random arrival order in which each group's own messages keep the order they were added in
        by_group = np.argsort(rows[:, 0], kind="stable")
        seq = rows[by_group, 0][self.rng.permutation(n)]  # the group of each arrival position
        order = np.empty(n, np.int64)
        order[np.argsort(seq, kind="stable")] = by_group
        bounds = np.append(rows[:, 6], len(self.eterm))
        et, eoff = [], []
        for i in order.tolist():
            eoff.append(len(et))
            et.extend(self.eterm[bounds[i]:bounds[i + 1]])
        r, E = rows[order], len(et)
        b = dict(group=r[:, 0].astype(np.uint32), info=r[:, 1].astype(np.uint32), term=r[:, 2].astype(np.uint64),
                 index=r[:, 3].astype(np.uint64), hint=r[:, 4].astype(np.uint64), commit=r[:, 5].astype(np.uint64),
                 eoff=np.array(eoff, np.uint64), eterm=np.array(et, np.uint64).reshape(-1), props=None, msg_props=True)
        if self.sized:
            ln = self.rng.integers(0, 65, E).astype(np.uint32)
            has = (self.rng.random(E) >= 0.2).astype(np.uint32)
            b["edesc"] = (np.where(has == 1, ln, 0).astype(np.uint32) | (has << np.uint32(31))).astype(np.uint32)
        return b


EVERY = 1  # every group compacts after every step (at every second one, as in scenario 1, a new term run
# per step plus the rule's one run per message asks most groups for a 16-run ring: test_compaction_ref.py)
# the role a cycling group must be in for stages 2 .. 6 (MsgHup, votes, reject + proposal, acks, the next Term)
STAGE_STATE = {2: abi.HB_STATE_FOLLOWER, 3: abi.HB_STATE_CANDIDATE, 4: abi.HB_STATE_LEADER, 5: abi.HB_STATE_LEADER,
               6: abi.HB_STATE_LEADER}


def follow_state(G, n, seed, sized, lift=None):
    """Followers of slot 1 whose log is already compacted to six entries in two
    term runs above the dummy entry's: [last - 5, last - 3] at Term - 1,
    [last - 2, last] at Term; everything but the last entry committed."""
    rng = np.random.default_rng(seed)
    g = np.zeros(G, dtype=abi.GROUP_DTYPE)
    last = 40 + rng.integers(0, 200, G)
    T = 10 + rng.integers(0, 50, G)
    g["term"], g["first_index"], g["last_index"], g["committed"] = T, last - 5, last, last - 1
    g["term_first"], g["term_last"], g["snap_index"] = last - 2, last, last - 6
    g["state"], g["n"], g["self_slot"], g["lead"], g["vote"] = abi.HB_STATE_FOLLOWER, n, 0, 1, 1
    for s in range(n):
        g["pr"][:, s]["match"] = last if s == 0 else 0
        g["pr"][:, s]["next"] = last + 1
    runs = [[(int(last[i]) - 6, int(T[i]) - 2), (int(last[i]) - 5, int(T[i]) - 1), (int(last[i]) - 2, int(T[i]))]
            for i in range(G)]
    g, runs, _ = lifted(lift, g, runs, None, delta=200, eps=60)
    sizes = synth.window_sizes(g, runs, seed=seed + 1, frac_full=1.0) if sized else None
    return g, runs, sizes


def run_follow_stream(n, size, make=CompactPair, G=600, steps=72, seed=1200, lift=None, hook=None):
    """Scenario 2.  Every group takes one follower-side message per step: mostly
    its leader's MsgApp at the next Term with 1-3 entries (a new term run each)
    and an advancing Commit; else a heartbeat, a MsgVote, an empty MsgApp probe
    at first - 1, first or last with the right or a wrong LogTerm, or a MsgSnap
    ahead of the log.  Every third group cycles through the roles, one stage a
    step: follower (two steps of that traffic), MsgHup, granted votes (leader:
    the noop), a reject from follower 1 that takes its Next a few entries back
    (the leader serves entries it received as a follower: the sizes
    follower_append wrote are read by limitSize) and a proposal, acks from a
    quorum, then a MsgApp of the next Term (follower again).  After every step
    the application compacts as in scenario 1.  hook(pair, k, now) runs after
    step k's compaction and returns the records it left."""
    sized = size is not None
    g, runs, sizes = follow_state(G, n, seed + n, sized, lift)
    kw = dict(max_msg_size=size, sizes=sizes) if sized else {}
    pair = make(g, runs, n, W, max_batch=8 * G, term_runs=True, **kw)
    rng = np.random.default_rng(seed + 9)
    stage = np.where(np.arange(G) % 3 == 0, (np.arange(G) // 3) % 7, -1)  # -1: a plain follower
    pair.cycles = np.zeros(G, dtype=np.int64)  # completed role cycles
    q = n // 2 + 1
    now = pair.og.groups()
    for k in range(steps):
        B = Batch(rng, sized)
        was_leader = now["state"] == abi.HB_STATE_LEADER
        for i in range(len(now)):
            r = now[i]
            if r["fault"] or r["n"] == 0:
                continue
            T, first, last, com = int(r["term"]), int(r["first_index"]), int(r["last_index"]), int(r["committed"])
            st = int(stage[i])
            if st >= 2 and r["state"] != STAGE_STATE[st]:
                st = stage[i] = 0  # the cycle was cut short (a MsgSnap, a lost vote): start over as it is
            if st == 2:
                B.add(i, abi.HB_MSG_HUP, abi.HB_SLOT_NONE)
            elif st == 3:
                for s in range(1, q):
                    B.add(i, abi.HB_MSG_VOTE_RESP, s, term=T)
            elif st == 4:
                nx = int(r["pr"][1]["next"])
                B.add(i, abi.HB_MSG_APP_RESP, 1, term=T, index=nx - 1, hint=max(nx - 2 - int(rng.integers(1, 4)), 0), reject=1)
                B.add(i, abi.HB_MSG_PROP, abi.HB_SLOT_NONE, index=int(rng.integers(1, 3)))
            elif st == 5:
                for s in range(1, q):
                    B.add(i, abi.HB_MSG_APP_RESP, s, term=T, index=last)
            elif st == 6 or r["state"] != abi.HB_STATE_FOLLOWER:
                B.add(i, abi.HB_MSG_APP, 1, term=T + 1, index=last, hint=pair.og.term(i, last), commit=last, ents=[T + 1])
            else:
                u = rng.random()
                if u < 0.80:
                    ne = int(rng.choice(3, p=[0.5, 0.35, 0.15])) + 1
                    B.add(i, abi.HB_MSG_APP, 1, term=T + 1, index=last, hint=pair.og.term(i, last),
                          commit=last + ne - int(rng.random() < 0.3), ents=[T + 1] * ne)
                elif u < 0.86:
                    B.add(i, abi.HB_MSG_HEARTBEAT, 1, term=T, commit=min(com + 1, last))
                elif u < 0.91:
                    v = int(rng.integers(0, 3))
                    lt = pair.og.term(i, last)
                    B.add(i, abi.HB_MSG_VOTE, 2, term=T + 1, index=last - (v == 1), hint=lt + (v == 2))
                elif u < 0.97:
                    x = max((first - 1, first, last)[int(rng.integers(0, 3))], 0)
                    lt = pair.og.term(i, x)
                    B.add(i, abi.HB_MSG_APP, 1, term=T, index=x, hint=lt if rng.random() < 0.6 else lt + 1, commit=com)
                else:
                    B.add(i, abi.HB_MSG_SNAP, 1, term=T + 1, index=last + int(rng.integers(3, 9)), hint=T + 1)
            if stage[i] >= 0:
                stage[i] = (st + 1) % 7
        _, _, now = pair.step(B.arrays(), ctx=f"follow stream n={n} size={size} step {k}",
                              check_inflights=(k % 8 == 7 or k == steps - 1))
        pair.cycles += was_leader & (now["state"] == abi.HB_STATE_FOLLOWER) & (stage == 0)
        now = compact_some(pair, now, k, rng, f"follow stream compact {k}", every=EVERY)
        if hook:
            now = hook(pair, k, now)
    pair.check_capacity("follow stream end")
    return pair


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(3, 150), (5, None)])
def test_follow_stream(n, size):
    run_follow_stream(n, size)


# ---------------------------------------------------------------- 4. wrapped rings through k_regrow, hb_move_groups, reload
RELOADED = (7, 80, 153, 226, 299, 372, 445, 518)
K_MOVE = 40  # the step after which the rings are regrown, moved and reloaded


def run_wrapped_rings_moved(make=MovedCompactPair, steps=84):
    """Scenario 4: scenario 2's stream at n = 3, size 150.  After step K_MOVE
    (every ring has wrapped by then: tests/test_compaction_ref.py) every third
    group's rings are raised to 64 / 32 (k_regrow copies a run ring whose head
    is not 0 and a size ring whose positions wrapped), the first 100 grown
    groups trade slots with ungrown ones (hb_move_groups), and eight groups'
    slots are removed and loaded with fresh groups.  Then the stream runs on."""
    seen = {}

    def hook(pair, k, now):
        if k != K_MOVE:
            return now
        G = len(now)
        seen.update(appended=pair.appended.copy(), runs_started=pair.runs_started.copy(),
                    cap_sz=pair.cap_sz.copy(), cap_tr=pair.cap_tr.copy())
        grown = np.arange(1, G, 3)
        pair.raise_capacity(grown, 64, 32)
        pair.check_capacity("regrown")
        pair.swap(grown[:100], grown[:100] + 1)
        pair.check_capacity("moved")
        fresh, fruns, fsizes = follow_state(len(RELOADED), 3, 1290, True)
        for j, i in enumerate(RELOADED):
            pair.reload(i, fresh[j], fruns[j], fsizes[j], fruns[j][:2])
        pair.check_capacity("reloaded")
        now = pair.og.groups()
        if pair.gpu:
            from .parity_util import assert_groups_equal
            assert_groups_equal(pair.eng.get_groups(), now, "moved and reloaded")
        return now

    pair = run_follow_stream(3, 150, make=make, steps=steps, seed=1400, hook=hook)
    return pair, seen


@pytest.mark.gpu
def test_wrapped_rings_moved():
    pair, _ = run_wrapped_rings_moved()
    grown = np.arange(1, pair.G, 3)
    assert (pair.cap_sz[grown] >= 64).all() and (pair.cap_tr[grown] >= 32).all()


# ---------------------------------------------------------------- 5. steady lane x compaction
SG = 4096 + 17  # the geometry and the odd lanes of tests/test_steady_lane_gpu.py
SWAVES = (SG + 63) // 64
ODD = (0, 2047, 2048 + 64 + 31, 4096 + 5)


LAG = (200, 1033, 3000, 3500)  # lanes of four other waves: both followers Replicate at the same Next, far behind


def run_steady_compaction(make=CompactPair):
    """Scenario 5: four cfg2 steps on the n = 3 steady path, each followed by
    compaction at committed - 1 on every group (SteadyLane::send's Next >= first
    holds: every wave stays steady).  In the fifth step follower 1 of each ODD
    group rejects the proposal's MsgApp (Probe at Match + 1) and the group is
    compacted at committed, past that Next; in the sixth it rejects again, and
    sendAppend finds Next < firstIndex: MsgSnap.
    The LAG groups are the case only SteadyLane::send's own test catches: both
    followers Replicate with empty windows at Match = last - 4, Next = last - 3
    (a new leader's followers after a heartbeat round and an ack each, its
    committed index ahead of them).  They stay idle until the fifth step's
    compaction at committed - 1 moves firstIndex past that Next; the sixth
    step's proposal then sends both the same Index, every other steady
    condition holds, and only Next >= first keeps the wave off the path:
    MsgSnap to both followers."""
    G, n = SG, 3
    g, runs = synth.steady_groups(G, n, seed=1500, last_hi=1 << 16)
    g["last_index"] += 8
    g["term_last"] = g["last_index"]
    g["committed"] = g["last_index"]
    L0 = g["last_index"].astype(np.int64)
    lag = np.array(LAG)
    for s in range(n):
        g["pr"][:, s]["match"], g["pr"][:, s]["next"] = L0, L0 + 1
    for s in (1, 2):
        g["pr"]["match"][lag, s], g["pr"]["next"][lag, s] = L0[lag] - 4, L0[lag] - 3
    pair = make(g, runs, n, W, max_batch=4 * G)
    ids = np.arange(G)
    odd = np.array(ODD)
    idle = np.zeros(G, bool)
    idle[lag] = True
    out = []

    def f1_rejects(b, index, hint):
        b["hint"] = np.zeros(len(b["group"]), np.uint64)
        for i in ODD:
            m = np.nonzero((b["group"] == i) & (((b["info"] >> 4) & 0xF) == 1))[0]
            b["info"][m] |= np.uint32(1 << 8)
            b["index"][m], b["hint"][m] = index[i], hint[i]
        return b

    for step in range(6):
        b = synth.cfg2_batch(g, step, seed=1501)
        if step < 5:  # the LAG groups wait
            b["props"][lag] = 0
            keep = ~idle[b["group"]]
            for k in ("group", "info", "term", "index"):
                b[k] = b[k][keep]
        else:         # ... and join as if it were their first step
            m = idle[b["group"]]
            b["index"][m] = (L0[b["group"][m]] + 1).astype(np.uint64)
        if step == 4:
            b = f1_rejects(b, L0 + 5, np.zeros(G, np.int64))       # Replicate: any Index above Match
        if step == 5:
            b = f1_rejects(b, L0 + 4, L0 + 4)                      # Probe: Index = Next - 1, hint = Match
        ev, st, now = pair.step(b, ctx=f"steady compaction {step}")
        out.append((ev, pair.eng.steady_waves() if pair.gpu else None, pair.eng.lazy_next_groups() if pair.gpu else None,
                    bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST) if pair.gpu else None, now))
        idx = now["committed"].astype(np.int64) - 1
        if step == 4:
            idx[odd] += 1
        who = ~idle if step < 4 else np.ones(G, bool)
        if step == 5:
            who[odd] = False  # (their committed - 1 is compacted already)
        rc, now = pair.compact(ids[who], idx[who], True, f"steady compaction compact {step}")
        assert (rc == 0).all()
    return pair, out, now


def check_steady_compaction(pair, out, now):
    for step in range(4):
        assert not np.isin(out[step][0]["type"], (abi.HB_EV_SNAP, abi.HB_EV_FAULT)).any()
    snap = out[5][0][out[5][0]["type"] == abi.HB_EV_SNAP]
    snap = snap[np.lexsort((snap["to"], snap["group"]))]
    want = sorted([(i, 1) for i in ODD] + [(i, s) for i in LAG for s in (1, 2)])
    assert list(zip(snap["group"].tolist(), snap["to"].tolist())) == want
    assert np.array_equal(snap["x"], out[5][4]["snap_index"][snap["group"]])  # the snapshot of the fifth step's compaction
    assert (now["pr"]["state"][list(ODD), 1] == abi.HB_PR_SNAPSHOT).all() and (now["fault"] == 0).all()
    if pair.gpu:
        for step in range(4):  # (the LAG groups keep their Next arrays: Next != last + 1)
            assert out[step][1:4] == (SWAVES, SG - len(LAG), True), (step, out[step][1:4])
        assert out[5][1] == SWAVES - len({i // 64 for i in ODD + LAG}) and out[5][3]


@pytest.mark.gpu
def test_steady_lane_compaction(monkeypatch):
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    check_steady_compaction(*run_steady_compaction())


# ---------------------------------------------------------------- 7. wide values
@pytest.mark.gpu
def test_leader_stream_w40(monkeypatch):
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    run_leader_stream(3, 150, lift="W40")


@pytest.mark.gpu
def test_follow_stream_w40():
    run_follow_stream(3, 150, lift="W40")
