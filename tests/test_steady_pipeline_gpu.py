"""k_route_fast<2, false>'s two passes over a lane's groups: the
steady group-waves stepped first on the lean lane, with the next group's first
round trip in flight, the others afterwards by the general fast lane.

A workgroup steps 2048 groups with 512 lanes: wave v of workgroup b owns the
four group-waves k = 0..3 at groups b * 2048 + k * 512 + v * 64 + [0, 64).
Parity against the oracle (tests.parity_util.Pair) with the count of steady
group-waves (HB_FAST_STEADY_COUNT=1 at create)."""
import numpy as np
import pytest

from etcd_amd import abi, synth
from tests.parity_util import Pair, sort_events

gpu = pytest.mark.gpu

N, W = 3, 8
RG, LANES, WAVE = 2048, 512, 64


def _waves(G):
    return (G + WAVE - 1) // WAVE


def _pair(monkeypatch, g, runs, **kw):
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    return Pair(g, runs, N, W, max_batch=max(4 * len(g), 64), **kw)


def _batch(g, step, seed):
    b = synth.cfg2_batch(g, step, seed=seed)
    b["hint"] = np.zeros(len(b["group"]), dtype=np.uint64)
    return b


def _msgs(b, i):
    return np.nonzero(b["group"] == i)[0]


def _append(b, i, info, term, index):
    for k, v in (("group", i), ("info", info), ("term", term), ("index", index), ("hint", 0)):
        b[k] = np.append(b[k], np.array([v], dtype=b[k].dtype))


# ---------------------------------------------------------------------------
# Every pending set.  G = 3 * 2048 + 65: two buckets, four workgroups, the last
# one part-filled, its second group-wave cut at G (one group).  The 16 waves
# of the first two workgroups: wave p gets pattern p (bit k: its group-wave k
# is not steady) at step 0, by one odd lane per such group-wave.
# ---------------------------------------------------------------------------
G_ALL = 3 * RG + WAVE + 1
KINDS = ("probe", "reject", "third", "follower")


def _group(p, k, shift):
    b, v = divmod(p, 8)
    return b * RG + k * LANES + v * WAVE + (7 * p + 13 * k + shift) % WAVE


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
    out = []
    for p in range(16):
        b, v = divmod(p, 8)
        out.append(sum(1 << k for k in range(4) if (b * RG + k * LANES + v * WAVE) // WAVE in off_t))
    return out


def test_schedule_covers_every_pending_set():  # (no GPU: the schedule alone)
    odd, off = _schedule()
    assert _patterns(off[0]) == list(range(16))
    assert {kind for _, kind in odd[0]} == set(KINDS)
    # each of the 64 group-waves is steady at some step and not steady at another:
    # state stored by each pass is loaded by the other
    gws = {(b * RG + k * LANES + v * WAVE) // WAVE for b in range(2) for v in range(8) for k in range(4)}
    always = off[0] & off[1] & off[2]
    never = gws - (off[0] | off[1] | off[2])
    follower = {g // WAVE for g, kind in odd[0] if kind == "follower"}
    assert always == follower and not never
    assert len({g for t in range(3) for g, _ in odd[t]}) == sum(len(o) for o in odd)  # (distinct groups)


@gpu
def test_every_pending_set(monkeypatch):
    from etcd_amd.hipbatch import Engine
    odd, off = _schedule()
    g, runs = synth.steady_groups(G_ALL, N, seed=901, last_hi=1 << 16)
    for i, kind in odd[0]:
        if kind == "probe":
            g["pr"][i][1]["state"] = abi.HB_PR_PROBE
        elif kind == "follower":
            g["state"][i], g["lead"][i] = abi.HB_STATE_FOLLOWER, 1
    monkeypatch.delenv("HB_ROUTE_FUSE", raising=False)
    monkeypatch.delenv("HB_FAST_STEADY", raising=False)
    pair = _pair(monkeypatch, g, runs)
    # the same groups on a handle without the steady path: every group-wave is pass 2's
    monkeypatch.setenv("HB_FAST_STEADY", "0")
    plain = Engine(G_ALL, max_replicas=N, max_inflight=W, max_batch=4 * G_ALL)
    monkeypatch.delenv("HB_FAST_STEADY")
    plain.load_groups(pair.og.groups())
    plain.reserve_log(np.arange(G_ALL, dtype=np.uint32), None, np.full(G_ALL, 16, dtype=np.int64))
    seen = set()
    for t in range(3):
        b = _batch(g, t, seed=902)
        for i, kind in odd[t]:
            if kind == "reject":
                b["info"][_msgs(b, i)[0]] |= 1 << 8
            elif kind == "third":
                _append(b, i, abi.HB_MSG_APP_RESP | (1 << 4), g["term"][i], g["last_index"][i] + t + 1)
        ev, st, now = pair.step(b, ctx=f"pending sets, step {t}")
        assert bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        plain.step_batch(b, host=True)
        assert bool(plain.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        assert np.array_equal(sort_events(plain.events()), sort_events(ev)), f"step {t}: events differ from HB_FAST_STEADY=0"
        assert np.array_equal(plain.stats(), st), f"step {t}: statistics differ from HB_FAST_STEADY=0"
        assert np.array_equal(plain.get_groups(), pair.eng.get_groups()), f"step {t}: groups differ from HB_FAST_STEADY=0"
        assert pair.eng.steady_waves() == _waves(G_ALL) - len(off[t]), f"step {t}"
        seen |= set(_patterns(off[t]))
    assert seen == set(range(16))


# ---------------------------------------------------------------------------
# Edges of the look-ahead: the handle ends inside a lane's first, second, third
# or fourth group, at a wave, partition and workgroup boundary and one past it.
# In even stripes of 512 groups the even groups are idle, in odd stripes the
# odd ones, so a lane's consecutive groups alternate: steady then idle (or
# past G), and idle then steady.
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G", [1, 63, 65, 513, 1025, 1537, 2047, 2049, 4097])
def test_look_ahead_edges(G, monkeypatch):
    g, runs = synth.steady_groups(G, N, seed=911, last_hi=1 << 16)
    idx = np.arange(G)
    idle = (idx // LANES + idx) % 2 == 0
    if G == 1:
        idle[:] = False
    pair = _pair(monkeypatch, g, runs)
    for t in range(2):
        b = _batch(g, t, seed=912)
        keep = ~idle[b["group"]]
        for k in ("group", "info", "term", "index", "hint"):
            b[k] = b[k][keep]
        b["props"][idle] = 0
        _, st, _ = pair.step(b, ctx=f"edges G={G}, step {t}")
        busy = int((~idle).sum())
        assert st[abi.HB_STAT_COMMITS] == busy and st[abi.HB_STAT_APPRESP] == 2 * busy
        assert bool(pair.eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        assert pair.eng.steady_waves() == _waves(G)


# ---------------------------------------------------------------------------
# Second-round loads that the all-lazy steady state never issues.
# ---------------------------------------------------------------------------
G2 = RG + WAVE + 1


@gpu
def test_tlast_and_self_words_loaded(monkeypatch):
    """M_TL clear (no entry of the leader's term yet: the current-term run is
    empty, tlast != last) and M_SM clear (the self slot's Match behind last):
    tlast and the self Match / Next words are read, and written back."""
    g, runs = synth.steady_groups(G2, N, seed=921, last_hi=1 << 16)
    idx = np.arange(G2)
    for i in np.nonzero((idx % 2 == 0) & (g["term"] > 1))[0]:
        runs[i] = [(0, int(g["term"][i]) - 1)]
        g["term_first"][i], g["term_last"][i] = abi.HB_NO_INDEX, 0
    sm = (idx % 3 == 0) & (g["last_index"] >= 2)
    g["pr"]["match"][sm, 0] = g["last_index"][sm] - np.uint64(1)
    pair = _pair(monkeypatch, g, runs)
    for t in range(3):
        _, st, _ = pair.step(_batch(g, t, seed=922), ctx=f"M_TL / M_SM clear, step {t}")
        assert st[abi.HB_STAT_COMMITS] == G2
        assert pair.eng.steady_waves() == _waves(G2)


@gpu
def test_next_words_loaded(monkeypatch):
    """HB_LAZY_NEXT=0: no group is held in the lazy form, so every step reads
    and writes the Next words."""
    monkeypatch.setenv("HB_LAZY_NEXT", "0")
    g, runs = synth.steady_groups(G2, N, seed=931, last_hi=1 << 16)
    pair = _pair(monkeypatch, g, runs)
    assert pair.eng.lazy_next_groups() == 0
    for t in range(3):
        _, st, _ = pair.step(_batch(g, t, seed=932), ctx=f"HB_LAZY_NEXT=0, step {t}")
        assert st[abi.HB_STAT_COMMITS] == G2
        assert pair.eng.steady_waves() == _waves(G2)
        assert pair.eng.lazy_next_groups() == 0


@gpu
def test_acks_trail_by_one_step(monkeypatch):
    """Open loop: step t proposes, and acks the proposal of step t - 1.  Step 0
    (proposals only) is steady: pass 1 steps it and stores the inflights.add
    words.  From step 1 on every window is non-empty at the start of the step
    and the ack (index last - 1 after the step's proposal) lies below Next - 1,
    so plan turns every group down: pass 1 defers every group-wave and pass 2
    steps it, reading the ring heads pass 1 (then pass 2) stored and storing
    its own adds (Pair.step compares the live windows)."""
    g, runs = synth.steady_groups(G2, N, seed=941, last_hi=1 << 16)
    pair = _pair(monkeypatch, g, runs)
    for t in range(5):
        b = _batch(g, max(t - 1, 0), seed=942)  # (acks of last0 + t)
        if t == 0:
            for k in ("group", "info", "term", "index", "hint"):
                b[k] = b[k][:0]
        _, st, now = pair.step(b, ctx=f"trailing acks, step {t}")
        assert st[abi.HB_STAT_ENTRIES] == G2 and st[abi.HB_STAT_FAULTS] == 0
        assert st[abi.HB_STAT_COMMITS] == (G2 if t else 0)
        assert pair.eng.steady_waves() == (0 if t else _waves(G2))
        if t:
            assert (now["pr"]["ins_count"][:, 1:N] == 1).all()
