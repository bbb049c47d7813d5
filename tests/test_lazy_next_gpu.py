"""The lazily kept Next array (M_NX) and SteadyLane's dropped
ring stores: a leader whose every slot has Next == lastIndex + 1 keeps no next
words, every reader derives them, and an inflights.add that the same step
frees is not stored.  Parity against the oracle (events, statistics,
hb_get_groups — so Next as the oracle has it — and the live windows) with the
form in use, lost and regained, switched off, moved, ticked and stepped down;
hb_lazy_next_groups counts the groups held in the form.

The geometry of tests/test_steady_lane_gpu.py: G = 4096 + 17 at n = 3, W = 8
(two buckets, three k_route_fast workgroups, a ragged last wave and partition)."""
import numpy as np
import pytest

from etcd_amd import abi, synth
from oracle.pyoracle import OracleGroups
from tests.lift_util import lifted
from tests.move_util import MovedPair
from tests.parity_util import Pair, assert_groups_equal, sort_events

gpu = pytest.mark.gpu

G, N, W = 4096 + 17, 3, 8
WAVES = (G + 63) // 64
ODD = (0, 2047, 2048 + 64 + 31, 4096 + 5)
DRAWS = np.random.default_rng(77).integers(0, 1 << 63, 4096, dtype=np.uint64)


def _state():
    return synth.steady_groups(G, N, seed=701, last_hi=1 << 16)


def _pair(monkeypatch, g, runs, ins=None, **kw):
    monkeypatch.setenv("HB_FAST_STEADY_COUNT", "1")
    monkeypatch.delenv("HB_LAZY_NEXT", raising=False)
    return Pair(g, runs, N, W, ins=ins, max_batch=4 * G, **kw)


def lazy_want(now):
    """The groups the engine holds in the lazy form: live leaders whose every
    slot < n has Next == lastIndex + 1 (from the oracle's records)."""
    slots = np.arange(now["pr"].shape[1])[None, :] < now["n"][:, None]
    at = now["pr"]["next"] == (now["last_index"] + np.uint64(1))[:, None]
    return (now["state"] == abi.HB_STATE_LEADER) & (now["n"] != 0) & (at | ~slots).all(axis=1)


# ---- 1 / 6: the form in use, also at wide values
@gpu
@pytest.mark.parametrize("lift", [None, "W40", "W62"])
def test_lazy_form_in_use(lift, monkeypatch):
    g, runs = _state()
    g, runs, _ = lifted(lift, g, runs, delta=1 << 15, eps=500)  # (W40: indices and terms on both sides of the bounds)
    pair = _pair(monkeypatch, g, runs)
    assert pair.eng.lazy_next_groups() == G
    for step in range(3):
        _, st, now = pair.step(synth.cfg2_batch(g, step, seed=702), ctx=f"lazy in use {lift}/{step}")
        assert st[abi.HB_STAT_COMMITS] == G and st[abi.HB_STAT_APPRESP] == 2 * G
        assert lazy_want(now).all()
        assert pair.eng.lazy_next_groups() == G
        if lift is None:
            assert pair.eng.steady_waves() == WAVES
        elif lift == "W62":  # (every event value takes a second word: no wave is steady)
            assert pair.eng.steady_waves() == 0


# ---- 2: lost by a rejected ack, regained by the acks that follow
OPEN = dict(lag_p=0.1, stale_p=0.02, reject_p=0.02)  # (cfg3_open_batch, gentler: four groups recover together)
BOUND = 6


def _reject_batch(g):
    b = synth.cfg2_batch(g, 0, seed=703)
    b["hint"] = np.zeros(len(b["group"]), dtype=np.uint64)
    for i in ODD:
        b["info"][np.nonzero(b["group"] == i)[0][0]] |= 1 << 8
    return b


def _odd_lazy(now):
    return bool(lazy_want(now)[list(ODD)].all())


def test_regain_stream_on_oracle():
    """The stream of test_lost_and_regained, on the oracle alone: the rejected
    groups are back at Next == last + 1 on every slot within the bound."""
    g, runs = _state()
    og = OracleGroups(g, runs, W, abi.HB_NO_LIMIT, None)
    og.step(_reject_batch(g))
    now = og.groups()
    assert not lazy_want(now)[list(ODD)].any()
    rng = np.random.default_rng(741)
    for k in range(BOUND):
        og.step(synth.cfg3_open_batch(now, rng, **OPEN))
        now = og.groups()
        assert (now["fault"] == 0).all()
        if _odd_lazy(now):
            return
    raise AssertionError("the stream does not bring the rejected groups back within the bound")


@gpu
def test_lost_and_regained(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs)
    _, _, now = pair.step(_reject_batch(g), ctx="rejected acks")
    assert not lazy_want(now)[list(ODD)].any()
    assert pair.eng.lazy_next_groups() <= G - len(ODD)
    assert pair.eng.lazy_next_groups() == int(lazy_want(now).sum())
    rng = np.random.default_rng(741)
    back = None
    for k in range(BOUND + 2):
        _, _, now = pair.step(synth.cfg3_open_batch(now, rng, **OPEN), ctx=f"regain {k}")
        if back is None and _odd_lazy(now):
            back = k
        # (the flag is derived at every store, so the count follows the oracle before the groups are back, too)
        assert pair.eng.lazy_next_groups() == int(lazy_want(now).sum()), f"step {k}"
        if back is not None and k >= back + 1:
            break
    assert back is not None and back < BOUND


# ---- 3: one-sided acks, ring positions wrapping twice
@gpu
def test_one_sided_acks_and_wrap(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs)
    term = g["term"].astype(np.uint64)
    rng = np.random.default_rng(751)
    for step in range(2 * W + 3):
        last = g["last_index"] + np.uint64(step + 1)
        frm = (1,) if step % 2 else (1, 2)  # odd steps: follower 2's add stays live; even: its ack covers both
        grp = np.concatenate([np.arange(G, dtype=np.uint32)] * len(frm))
        slot = np.repeat(np.array(frm, dtype=np.uint32), G)
        perm = rng.permutation(len(grp))
        grp, slot = grp[perm], slot[perm]
        b = dict(group=grp, info=(abi.HB_MSG_APP_RESP | (slot << np.uint32(4))).astype(np.uint32), term=term[grp],
                 index=last[grp], hint=None, props=np.ones(G, dtype=np.uint32))
        _, st, now = pair.step(b, ctx=f"one-sided {step}")  # (compares every live window)
        assert st[abi.HB_STAT_COMMITS] == G
        cnt = now["pr"]["ins_count"]
        assert (cnt[:, 1] == 0).all() and (cnt[:, 2] == step % 2).all()
        assert pair.eng.steady_waves() == WAVES
        assert pair.eng.lazy_next_groups() == G


# ---- 4: the switch
def _stream(monkeypatch, env):
    from etcd_amd.hipbatch import Engine
    for k in ("HB_FAST_STEADY", "HB_ROUTE_FUSE", "HB_LAZY_NEXT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, _ = _state()
    rng = np.random.default_rng(721)
    g["pr"]["state"][rng.random(G) < 0.01, 1] = abi.HB_PR_PROBE
    eng = Engine(G, max_replicas=N, max_inflight=W, max_batch=4 * G)
    eng.load_groups(g)
    eng.reserve_log(np.arange(G, dtype=np.uint32), None, np.full(G, 8, dtype=np.int64))
    out = []
    for step in range(3):
        eng.step_batch(synth.cfg2_batch(g, step, seed=722), host=True)
        fast = bool(eng.step_kernels() & abi.HB_KERN_ROUTE_FAST)
        out.append((sort_events(eng.events()), eng.stats(), eng.get_groups(), fast, eng.lazy_next_groups()))
    return out


@gpu
@pytest.mark.parametrize("fuse", [None, "0"])
def test_switch_off_vs_on(fuse, monkeypatch):
    env = {} if fuse is None else {"HB_ROUTE_FUSE": fuse}
    on = _stream(monkeypatch, env)
    off = _stream(monkeypatch, dict(env, HB_LAZY_NEXT="0"))
    for step, (a, b) in enumerate(zip(on, off)):
        assert a[3] == b[3] == (fuse is None)
        assert np.array_equal(a[0], b[0]), f"step {step}: events differ"
        assert np.array_equal(a[1], b[1]), f"step {step}: statistics differ"
        assert np.array_equal(a[2], b[2]), f"step {step}: groups differ"
        assert a[1][abi.HB_STAT_COMMITS] > G // 4
        assert b[4] == 0
        assert a[4] == int(lazy_want(a[2]).sum()) and a[4] > G // 2


# ---- 5: every other reader materializes
@gpu
def test_move_swaps_lazy_and_kept(monkeypatch):
    monkeypatch.delenv("HB_LAZY_NEXT", raising=False)
    g, runs = _state()
    part = [i + 1 for i in ODD]
    for j in part:  # a Probe follower one entry behind: its Next is kept
        p = g["pr"][j][1]
        p["state"], p["match"], p["next"] = abi.HB_PR_PROBE, g["last_index"][j] - 1, g["last_index"][j]
    pair = MovedPair(g, runs, N, W, capacity=G, max_batch=4 * G)
    real = pair.view.real
    assert real.lazy_next_groups() == G - len(part)
    pair.view.move_slots(list(ODD) + part, part + list(ODD))
    assert_groups_equal(pair.eng.get_groups(), pair.og.groups(), "swapped")
    assert real.lazy_next_groups() == G - len(part)
    raw = real.get_groups()
    assert lazy_want(raw)[part].all() and not lazy_want(raw)[list(ODD)].any()
    _, _, now = pair.step(synth.cfg2_batch(g, 0, seed=761), ctx="step after the swap")
    assert real.lazy_next_groups() == int(lazy_want(now).sum())


@gpu
def test_set_inflights_on_a_lazy_group(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs)
    want = pair.eng.get_groups()
    for i in ODD:
        last = int(g["last_index"][i])
        vals = np.array([last - 1, last], dtype=np.uint64)
        pair.eng.set_inflights(i, 2, W - 1, vals)  # (wraps)
        want["pr"][i][2]["ins_start"], want["pr"][i][2]["ins_count"] = W - 1, 2
        start, got = pair.eng.get_inflights(i, 2)
        assert start == W - 1 and np.array_equal(got, vals)
    assert np.array_equal(pair.eng.get_groups(), want)
    assert pair.eng.lazy_next_groups() == G


@gpu
def test_tick_over_lazy_leaders(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs)
    t = np.zeros(G, abi.TIMER_DTYPE)
    t["election_tick"], t["heartbeat_tick"] = 10, 2
    pair.set_timers(t, DRAWS)
    beats = 0
    for k in range(4):
        _, st, _ = pair.tick(ctx=f"tick {k}")
        beats += int(st[abi.HB_STAT_MSGS])
        assert pair.eng.lazy_next_groups() == G
    assert beats == 2 * G
    pair.step(synth.cfg2_batch(g, 0, seed=771), ctx="step after the ticks")
    assert pair.eng.lazy_next_groups() == G


def _app(g0, term_up, ents):
    """A MsgApp to each ODD group from slot 1 at Term + term_up: Index / LogTerm =
    the group's last entry, `ents` entries at that Term, Commit = what it has."""
    i = np.array(ODD)
    term = g0["term"][i] + np.uint64(term_up)
    return dict(group=i.astype(np.uint32), info=np.full(len(i), abi.HB_MSG_APP | (1 << 4), dtype=np.uint32), term=term,
                index=g0["last_index"][i].astype(np.uint64), hint=g0["term"][i].astype(np.uint64),
                commit=g0["committed"][i].astype(np.uint64), eoff=(np.arange(len(i)) * ents).astype(np.uint64),
                eterm=np.repeat(term, ents).astype(np.uint64), props=None)


@gpu
def test_step_down_then_append(monkeypatch):
    g, runs = _state()
    pair = _pair(monkeypatch, g, runs, term_runs=True)
    g0 = pair.og.groups()
    i = list(ODD)
    _, _, now = pair.step(_app(g0, 1, 0), ctx="higher-term MsgApp")
    assert (now["state"][i] == abi.HB_STATE_FOLLOWER).all() and (now["term"][i] == g0["term"][i] + 1).all()
    assert pair.eng.lazy_next_groups() == G - len(ODD)
    _, _, now = pair.step(_app(g0, 1, 2), ctx="append as a follower")
    assert (now["last_index"][i] == g0["last_index"][i] + 2).all()
    assert (now["pr"]["next"][i, :N] == (g0["last_index"][i] + 1)[:, None]).all()  # frozen where reset left them
    assert pair.eng.lazy_next_groups() == G - len(ODD) == int(lazy_want(now).sum())
    _, _, now = pair.step(synth.cfg2_batch(g, 0, seed=781), ctx="the leaders go on")
    assert pair.eng.lazy_next_groups() == G - len(ODD) == int(lazy_want(now).sum())
